"""Host side of banded Jacobian storage (`IVP_RHS_BANDED`, `jac_storage="banded"`; no GPU): the bandwidths of a pattern
from ivp_jac_sparsity_bandwidth and api.jac_bandwidth against known answers, its validation against
ivp_jac_sparsity_groups on the same malformed input, the argument checks of DeviceIVP / pyfront.solve_ivp (which must come
before any device call), and the declarations of the two new entry points in the header and the Rust bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ivp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = -100
I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def csc_of(dense):
    dense = np.asarray(dense)
    col_ptr, row_idx = [0], []
    for c in range(dense.shape[1]):
        row_idx += [r for r in range(dense.shape[0]) if dense[r, c]]
        col_ptr.append(len(row_idx))
    return np.array(col_ptr, dtype=np.int32), np.array(row_idx, dtype=np.int32)


def banded(n, ml, mu):
    i, j = np.indices((n, n))
    return ((i - j <= ml) & (j - i <= mu)).astype(np.int8)


def bandwidth_raw(lib, n, col_ptr, row_idx):
    """The C entry point as it is: (rc, ml, mu)."""
    col_ptr = np.ascontiguousarray(col_ptr, dtype=np.int32)
    row_idx = np.ascontiguousarray(row_idx if len(row_idx) else [0], dtype=np.int32)
    ml, mu = C.c_int32(-7), C.c_int32(-7)
    rc = lib.ivp_jac_sparsity_bandwidth(n, col_ptr.ctypes.data_as(I32P), row_idx.ctypes.data_as(I32P), C.byref(ml), C.byref(mu))
    return rc, ml.value, mu.value


def groups_rc(lib, n, col_ptr, row_idx):
    col_ptr = np.ascontiguousarray(col_ptr, dtype=np.int32)
    row_idx = np.ascontiguousarray(row_idx if len(row_idx) else [0], dtype=np.int32)
    out = np.zeros(max(n, 1), dtype=np.int32)
    ng = C.c_int32()
    return lib.ivp_jac_sparsity_groups(n, col_ptr.ctypes.data_as(I32P), row_idx.ctypes.data_as(I32P), out.ctypes.data_as(I32P), C.byref(ng))


def arrow(n):
    pat = np.eye(n, dtype=np.int8)
    pat[0, :] = 1
    pat[:, 0] = 1
    return pat


def known_patterns():
    n = 20
    empty_col = banded(n, 1, 1)
    empty_col[:, 7] = 0      # column 7 declares nothing: rows 6 and 8 of it are gone, the neighbours still span (1, 1)
    return [
        ("tridiagonal", n, banded(n, 1, 1), (1, 1)),
        ("|i - j| <= 4", n, banded(n, 4, 4), (4, 4)),
        ("lower 2 / upper 1", n, banded(n, 2, 1), (2, 1)),
        ("diagonal", n, np.eye(n, dtype=np.int8), (0, 0)),
        ("an empty column", n, empty_col, (1, 1)),
        ("arrow", n, arrow(n), (n - 1, n - 1)),
        ("tridiagonal 512", 512, banded(512, 1, 1), (1, 1)),
    ]


def test_bandwidth_of_known_patterns(lib):
    for name, n, pat, want in known_patterns():
        rc, ml, mu = bandwidth_raw(lib, n, *csc_of(pat))
        assert (rc, ml, mu) == (0, *want), name
        assert api.jac_bandwidth(pat, n) == want, name
    n = 12
    assert bandwidth_raw(lib, n, np.zeros(n + 1, dtype=np.int32), []) == (0, 0, 0)   # nothing declared at all
    assert api.jac_bandwidth((np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)), n) == (0, 0)
    one = np.zeros((n, n), dtype=np.int8)
    one[9, 2] = 1                                                                    # one entry below the diagonal
    assert api.jac_bandwidth(one, n) == (7, 0)
    assert api.jac_bandwidth(one.T, n) == (0, 7)


def test_bandwidth_of_the_medazko_pattern():
    pytest.importorskip("scipy.sparse")
    from tests.test_gpu_jac_sparsity import medazko_pattern
    assert api.jac_bandwidth(medazko_pattern(200), 400) == (2, 2)
    assert api.jac_bandwidth(medazko_pattern(10), 20) == (2, 2)


def test_malformed_patterns_give_the_error_codes_of_the_grouping(lib):
    n = 12
    col_ptr, row_idx = csc_of(banded(n, 1, 1))
    cases = []
    bad = col_ptr.copy(); bad[0] = 1
    cases.append((n, bad, row_idx))                         # col_ptr[0] != 0
    bad = col_ptr.copy(); bad[5] = bad[4] - 1
    cases.append((n, bad, row_idx))                         # decreasing col_ptr
    bad = row_idx.copy(); bad[7] = n
    cases.append((n, col_ptr, bad))                         # row index == n
    bad = row_idx.copy(); bad[3] = -1
    cases.append((n, col_ptr, bad))                         # negative row index
    for bad_n in (0, 1, 8, 513, -3):                        # 8 < n <= 512
        cases.append((bad_n, np.zeros(max(bad_n, 0) + 1, dtype=np.int32), []))
    cases.append((n, col_ptr, row_idx))                     # and a good one
    cases.append((9, np.zeros(10, dtype=np.int32), []))
    for q, (nn, cp, ri) in enumerate(cases):
        want = groups_rc(lib, nn, cp, ri)
        assert bandwidth_raw(lib, nn, cp, ri)[0] == want, q
        assert want == (0 if q >= len(cases) - 2 else BAD_ARGUMENT), q
    ml, mu = C.c_int32(), C.c_int32()
    assert lib.ivp_jac_sparsity_bandwidth(n, None, None, C.byref(ml), C.byref(mu)) == BAD_ARGUMENT
    assert lib.ivp_jac_sparsity_bandwidth(n, col_ptr.ctypes.data_as(I32P), row_idx.ctypes.data_as(I32P), None, C.byref(mu)) == BAD_ARGUMENT
    assert lib.ivp_jac_sparsity_bandwidth(n, col_ptr.ctypes.data_as(I32P), row_idx.ctypes.data_as(I32P), C.byref(ml), None) == BAD_ARGUMENT
    assert lib.ivp_rhs_jac_layout(None, None, None, None, None, None) == BAD_ARGUMENT
    with pytest.raises(api.ConfigError) as e:
        api.jac_bandwidth((col_ptr, np.where(row_idx == 3, n + 4, row_idx)), n)
    assert e.value.code == BAD_ARGUMENT
    # the compile entry point refuses before it needs a device: no context
    h = C.c_void_p()
    assert lib.ivp_rhs_compile_sparse(None, b"", n, 0, 0, 2, col_ptr.ctypes.data_as(I32P), row_idx.ctypes.data_as(I32P), C.byref(h)) == BAD_ARGUMENT


def test_argument_validation_comes_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made before the arguments were validated")
    monkeypatch.setattr(api, "default_context", no_device)
    n = 12
    src = "__device__ double ode_comp(int i, double t, const double* y, const double* p) { return -y[i]; }"
    with pytest.raises(ValueError, match="jac_storage"):
        api.DeviceIVP(src, n=n, jac_sparsity=banded(n, 1, 1), jac_storage="band")
    with pytest.raises(ValueError, match="jac_storage"):
        api.DeviceIVP(src, n=n, jac_sparsity=banded(n, 1, 1), jac_storage=None)
    with pytest.raises(ValueError, match="jac_sparsity"):
        api.DeviceIVP(src, n=n, jac_storage="banded")
    with pytest.raises(ValueError, match="jac=True"):
        api.DeviceIVP(src, n=n, jac=True, jac_sparsity=banded(n, 1, 1), jac_storage="banded")

    from ivp_amd import pyfront
    monkeypatch.setattr(pyfront, "_device_problem", no_device)
    body = "for (int i = 0; i < 12; ++i) dydx[i] = -y[i];"
    y0 = np.ones(n)
    with pytest.raises(ValueError, match="jac_storage"):
        pyfront.solve_ivp(body, (0.0, 1.0), y0, method="BDF", jac_sparsity=banded(n, 1, 1), jac_storage="sparse")
    with pytest.raises(ValueError, match="jac_storage"):
        pyfront.solve_ivp(body, (0.0, 1.0), y0, method="RK45", jac_storage="sparse")          # the value is checked for every method
    with pytest.raises(ValueError, match="jac_sparsity"):
        pyfront.solve_ivp(body, (0.0, 1.0), y0, method="BDF", jac_storage="banded")


def test_header_rust_and_export_list_declare_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "ivp_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "ivp-hip-sys", "src", "lib.rs")).read()
    assert re.search(r"#define\s+IVP_RHS_BANDED\s+2u", header)
    assert re.search(r"pub const IVP_RHS_BANDED: u32 = 2;", rust)
    assert re.search(r"#define\s+IVP_HIP_ABI_VERSION\s+5\b", header)
    for name in ("ivp_jac_sparsity_bandwidth", "ivp_rhs_jac_layout"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert re.search(r"pub fn " + name + r"\(", rust), name
        assert name in _lib.EXPORTS, name
