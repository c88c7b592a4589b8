"""Host side of `jac_sparsity` (no GPU): the first-fit column grouping of ivp_jac_sparsity_groups against known answers
and against a restatement of the reference's rule (src/python/sparsity.rs:110-154), the validation errors of the
pattern, and the three input forms of the Python layer."""
import ctypes as C

import numpy as np
import pytest

from ivp_amd import _lib, api

BAD_ARGUMENT = -100
I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def csc_of(dense):
    """(col_ptr, row_idx) of a dense 0/1 matrix, rows ascending within a column."""
    dense = np.asarray(dense)
    col_ptr, row_idx = [0], []
    for c in range(dense.shape[1]):
        row_idx += [r for r in range(dense.shape[0]) if dense[r, c]]
        col_ptr.append(len(row_idx))
    return np.array(col_ptr, dtype=np.int32), np.array(row_idx, dtype=np.int32)


def groups_raw(lib, n, col_ptr, row_idx):
    """The C entry point as it is: (rc, groups, n_groups)."""
    col_ptr = np.ascontiguousarray(col_ptr, dtype=np.int32)
    row_idx = np.ascontiguousarray(row_idx if len(row_idx) else [0], dtype=np.int32)
    out = np.full(max(n, 1), -7, dtype=np.int32)
    ng = C.c_int32(-7)
    rc = lib.ivp_jac_sparsity_groups(n, col_ptr.ctypes.data_as(I32P), row_idx.ctypes.data_as(I32P), out.ctypes.data_as(I32P), C.byref(ng))
    return rc, out[:max(n, 0)], ng.value


def first_fit(n, col_ptr, row_idx):
    """sparsity.rs:110-154 restated: columns in index order, the first group none of whose used rows the column touches."""
    groups, used = [], []
    for c in range(n):
        rows = [int(r) for r in row_idx[col_ptr[c]:col_ptr[c + 1]]]
        for g, u in enumerate(used):
            if not any(r in u for r in rows):
                break
        else:
            g = len(used)
            used.append(set())
        used[g].update(rows)
        groups.append(g)
    return groups, len(used)


def banded(n, ml, mu):
    i, j = np.indices((n, n))
    return ((i - j <= ml) & (j - i <= mu)).astype(np.int8)


@pytest.mark.parametrize("n", [9, 12, 65, 256, 512])
def test_tridiagonal_pattern_gives_three_groups(lib, n):
    rc, g, ng = groups_raw(lib, n, *csc_of(banded(n, 1, 1)))
    assert rc == 0 and ng == 3
    assert g.tolist() == [c % 3 for c in range(n)]


def test_known_patterns(lib):
    n = 20
    rc, g, ng = groups_raw(lib, n, *csc_of(np.eye(n)))
    assert (rc, ng, g.tolist()) == (0, 1, [0] * n)                       # diagonal: every column in one group
    rc, g, ng = groups_raw(lib, n, *csc_of(np.ones((n, n))))
    assert (rc, ng, g.tolist()) == (0, n, list(range(n)))                # full: n groups
    arrow = np.eye(n)
    arrow[0, :] = 1
    arrow[:, 0] = 1
    rc, g, ng = groups_raw(lib, n, *csc_of(arrow))
    assert (rc, ng, g.tolist()) == (0, n, list(range(n)))                # dense row 0: every pair of columns shares it
    rc, g, ng = groups_raw(lib, n, *csc_of(banded(n, 4, 4)))
    assert (rc, ng, g.tolist()) == (0, 9, [c % 9 for c in range(n)])     # ml = mu = 4: 9 groups


def test_empty_column_lands_in_group_zero(lib):
    n = 10
    pat = banded(n, 1, 1)
    pat[:, 4] = 0            # column 4 declares nothing
    pat[:, 0] = 0            # ... and neither does the very first column: it OPENS group 0
    rc, g, ng = groups_raw(lib, n, *csc_of(pat))
    assert rc == 0 and g[4] == 0 and g[0] == 0
    assert (g.tolist(), ng) == first_fit(n, *csc_of(pat))
    rc, g, ng = groups_raw(lib, n, np.zeros(n + 1, dtype=np.int32), [])   # nothing declared at all
    assert (rc, ng, g.tolist()) == (0, 1, [0] * n)


def test_duplicate_rows_within_a_column_are_accepted(lib):
    n = 9
    col_ptr, row_idx = csc_of(banded(n, 1, 1))
    dup_ptr, dup_idx = [0], []
    for c in range(n):
        rows = row_idx[col_ptr[c]:col_ptr[c + 1]].tolist()
        dup_idx += rows + rows[::-1]
        dup_ptr.append(len(dup_idx))
    assert groups_raw(lib, n, dup_ptr, dup_idx)[0] == 0
    assert groups_raw(lib, n, dup_ptr, dup_idx)[1].tolist() == groups_raw(lib, n, col_ptr, row_idx)[1].tolist()


def test_random_patterns_equal_the_restated_first_fit(lib):
    rng = np.random.default_rng(20251)
    sizes = [9, 17, 64, 65, 200, 512]
    for case in range(200):
        n = sizes[case % len(sizes)]
        density = [0.5 / n, 2.0 / n, 6.0 / n, 0.2][(case // len(sizes)) % 4]
        col_ptr, row_idx = [0], []
        for c in range(n):
            k = rng.binomial(n, density)
            rows = rng.choice(n, size=k, replace=False)       # unsorted on purpose
            if case % 5 == 0 and k:
                rows = np.concatenate([rows, rows[:1]])       # with a duplicate
            row_idx += rows.tolist()
            col_ptr.append(len(row_idx))
        rc, g, ng = groups_raw(lib, n, col_ptr, row_idx)
        want, want_ng = first_fit(n, col_ptr, row_idx)
        assert rc == 0 and ng == want_ng and g.tolist() == want, (case, n)


def test_validation_errors(lib):
    n = 12
    col_ptr, row_idx = csc_of(banded(n, 1, 1))
    assert groups_raw(lib, n, col_ptr, row_idx)[0] == 0
    bad = col_ptr.copy(); bad[0] = 1
    assert groups_raw(lib, n, bad, row_idx)[0] == BAD_ARGUMENT                 # col_ptr[0] != 0
    bad = col_ptr.copy(); bad[5] = bad[4] - 1
    assert groups_raw(lib, n, bad, row_idx)[0] == BAD_ARGUMENT                 # decreasing col_ptr
    bad = row_idx.copy(); bad[7] = n
    assert groups_raw(lib, n, col_ptr, bad)[0] == BAD_ARGUMENT                 # row index == n
    bad = row_idx.copy(); bad[3] = -1
    assert groups_raw(lib, n, col_ptr, bad)[0] == BAD_ARGUMENT                 # negative row index
    for bad_n in (0, 1, 8, 513, -3):                                           # 8 < n <= 512
        cp = np.zeros(max(bad_n, 0) + 1, dtype=np.int32)
        assert groups_raw(lib, bad_n, cp, [])[0] == BAD_ARGUMENT, bad_n
    assert groups_raw(lib, 9, np.zeros(10, dtype=np.int32), [])[0] == 0
    assert groups_raw(lib, 512, np.zeros(513, dtype=np.int32), [])[0] == 0
    ng = C.c_int32()
    out = np.zeros(n, dtype=np.int32)
    assert lib.ivp_jac_sparsity_groups(n, None, None, out.ctypes.data_as(I32P), C.byref(ng)) == BAD_ARGUMENT
    assert lib.ivp_jac_sparsity_groups(n, col_ptr.ctypes.data_as(I32P), row_idx.ctypes.data_as(I32P), None, C.byref(ng)) == BAD_ARGUMENT
    # the compile entry point refuses before it needs a device: no context
    h = C.c_void_p()
    assert lib.ivp_rhs_compile_sparse(None, b"", n, 0, 0, 0, col_ptr.ctypes.data_as(I32P), row_idx.ctypes.data_as(I32P), C.byref(h)) == BAD_ARGUMENT
    with pytest.raises(api.ConfigError) as e:
        api.jac_sparsity_groups((col_ptr, np.where(row_idx == 3, n + 4, row_idx)), n)
    assert e.value.code == BAD_ARGUMENT


def test_python_input_forms_give_the_same_csc_pattern():
    sp = pytest.importorskip("scipy.sparse")
    n = 25
    rng = np.random.default_rng(7)
    dense = (rng.uniform(size=(n, n)) < 0.15) | np.eye(n, dtype=bool)
    want_ptr, want_idx = csc_of(dense)
    forms = {
        "bool ndarray": dense,
        "float ndarray": np.where(dense, 2.5, 0.0),
        "nested lists": dense.astype(int).tolist(),
        "csr_matrix": sp.csr_matrix(dense.astype(float)),
        "csc_matrix": sp.csc_matrix(dense.astype(float)),
        "coo_matrix": sp.coo_matrix(dense.astype(float)),
        "(col_ptr, row_idx) int32": (want_ptr, want_idx),
        "(col_ptr, row_idx) lists": (want_ptr.tolist(), want_idx.tolist()),
    }
    for name, form in forms.items():
        col_ptr, row_idx = api.sparsity_csc(form, n)
        assert col_ptr.dtype == np.int32 and row_idx.dtype == np.int32, name
        assert col_ptr.tolist() == want_ptr.tolist(), name
        for c in range(n):   # scipy does not promise sorted rows within a column: compare as sets per column
            assert sorted(row_idx[col_ptr[c]:col_ptr[c + 1]].tolist()) == want_idx[want_ptr[c]:want_ptr[c + 1]].tolist(), (name, c)
        g, ng = api.jac_sparsity_groups(form, n)
        assert (g.tolist(), ng) == first_fit(n, want_ptr, want_idx), name
    with pytest.raises(ValueError):
        api.sparsity_csc(np.eye(n + 1), n)
    with pytest.raises(ValueError):
        api.sparsity_csc(sp.eye(n + 1), n)
    with pytest.raises(ValueError):
        api.sparsity_csc((want_ptr, want_idx[:-1]), n)
