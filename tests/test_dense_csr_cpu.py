"""Batch dense output in CSR form, without a GPU:

  * ivp_dense_log_t (include/ivp_hip.h): offsetof / sizeof from gcc equal the ctypes binding, and the #[repr(C)] twin in
    rust/ivp-hip-sys/src/lib.rs lists the same members in the same order;
  * the segment search and per-component interpolation of the device evaluation (ivp_amd/csrc/dense_eval.h, built here
    for the host from the same header, on rk_core.h's interpolate<M, 1>) give the same bits as the host
    ContinuousOutput.evaluate / evaluate_extrapolate (src/solve/cont.rs:104-153) for every method, forward and
    backward runs, queries on and around every boundary (+-0.5e-12 inside the 1e-12 tolerance, +-2e-12 outside it),
    before the start and past the end, an empty run and the constant segment of a zero-length interval.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ivp_amd import _lib
from ivp_amd.api import ContinuousOutput, Method

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivp_amd", "csrc")
MEMBERS = ["offsets", "cont", "xold", "h", "capacity", "owned", "device", "passes", "ncoef_n", "total", "staging_bytes"]


def test_dense_log_struct_layout_matches_ctypes_and_rust(tmp_path):
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ivp_hip.h"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(ivp_dense_log_t));']
    lines += [f'  printf("{m} %zu %zu\\n", offsetof(ivp_dense_log_t, {m}), sizeof(((ivp_dense_log_t *)0)->{m}));' for m in MEMBERS]
    lines += ['  return 0;', '}']
    src = tmp_path / "dl.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "dl"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    assert int(out[0]) == C.sizeof(_lib.DenseLogT)
    assert [f[0] for f in _lib.DenseLogT._fields_] == MEMBERS
    for line in out[1:]:
        if not line:
            continue
        name, off, size = line.split()
        d = getattr(_lib.DenseLogT, name)
        assert (d.offset, d.size) == (int(off), int(size)), name
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivp_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*ivp_dense_log_t\s*;", hdr).group(1)
    assert [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()] == MEMBERS
    rust = open(os.path.join(ROOT, "rust", "ivp-hip-sys", "src", "lib.rs")).read()
    rbody = re.search(r"#\[repr\(C\)\]\s*pub struct ivp_dense_log_t\s*\{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+)\s*:", rbody) == MEMBERS


SHIM = r"""
#include <cstdint>
#include <cstddef>
#define IVP_HD inline
#define IVP_NS ivp_dense_host
#include "rk_core.h"
#include "dense_eval.h"
using namespace ivp_dense_host;
template <int M>
static int eval_one(int n, unsigned long long cnt, const double *cont, const double *xold, const double *h, double t, int ex, double *y)
{
    unsigned long long q = 0;
    const int f = dense_find(xold, h, 0, cnt, t, ex, &q);
    if (f == IVP_DENSE_NONE) return f;
    const double *seg = cont + q * (size_t)(NCoef<M>::v * n);
    for (int c = 0; c < n; ++c) y[c] = dense_component<M>(dense_comp_view<M>(seg, n, c), t, xold[q], h[q]);
    return f;
}
extern "C" int dense_eval_host(int method, int n, unsigned long long cnt, const double *cont, const double *xold, const double *h,
                               double t, int ex, double *y)
{
    switch (method) {
    case M_RK23: return eval_one<M_RK23>(n, cnt, cont, xold, h, t, ex, y);
    case M_DOPRI5: return eval_one<M_DOPRI5>(n, cnt, cont, xold, h, t, ex, y);
    case M_DOP853: return eval_one<M_DOP853>(n, cnt, cont, xold, h, t, ex, y);
    case M_RK4: return eval_one<M_RK4>(n, cnt, cont, xold, h, t, ex, y);
    case M_BDF: return eval_one<M_BDF>(n, cnt, cont, xold, h, t, ex, y);
    }
    return -1;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "libshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                           "-DIVP_FAST=0", "-I", CSRC, str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.dense_eval_host.restype = C.c_int
    dp = C.POINTER(C.c_double)
    lib.dense_eval_host.argtypes = [C.c_int, C.c_int, C.c_ulonglong, dp, dp, dp, C.c_double, C.c_int, dp]
    return lib


def _run(method, n, k, rng, backward=False):
    """k contiguous segments of random coefficients (BDF: every state block carries the segment's order, 1..5, as the
    solver writes it)."""
    nc = method.coeffs_per_state() * n
    cont = rng.standard_normal((k, nc))
    if method == Method.BDF:
        cont.reshape(k, n, 7)[:, :, 6] = rng.integers(1, 6, size=(k, 1))
    h = rng.uniform(0.05, 0.4, size=k) * (-1.0 if backward else 1.0)
    xold = np.empty(k)
    x = 0.3
    for i in range(k):
        xold[i] = x
        x = x + h[i]
    return cont, xold, h


def _queries(xold, h):
    ends = np.concatenate([xold, xold + h])
    q = [ends + d for d in (0.0, 0.5e-12, -0.5e-12, 2e-12, -2e-12)]
    lo, hi = float(np.min(ends)), float(np.max(ends))
    q.append(np.array([lo - 1.0, lo - 1e-9, hi + 1e-9, hi + 1.0]))
    q.append(np.linspace(lo, hi, 37))
    return np.concatenate(q)


def _check(shim, method, n, cont, xold, h, ts):
    co = ContinuousOutput(method, n, cont, xold, h)
    flat = np.ascontiguousarray(cont.reshape(-1))
    xold, h = np.ascontiguousarray(xold, dtype=np.float64), np.ascontiguousarray(h, dtype=np.float64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    y = np.zeros(max(n, 1))
    for t in ts:
        for ex in (0, 1):
            want = co.evaluate_extrapolate(float(t)) if ex else co.evaluate(float(t))
            f = shim.dense_eval_host(int(method), n, len(h), dp(flat), dp(xold), dp(h), float(t), ex, dp(y))
            if want is None:
                assert f == 0, (method, n, t, ex)
                continue
            inside = co.evaluate(float(t)) is not None
            assert f == (1 if inside else 2), (method, n, t, ex, f)
            assert np.array_equal(y[:n].view(np.uint64), np.asarray(want, dtype=np.float64).view(np.uint64)), (method, n, t, ex)


METHODS = [Method.RK23, Method.DOPRI5, Method.DOP853, Method.RK4, Method.BDF]


@pytest.mark.parametrize("method", METHODS, ids=lambda m: m.name)
@pytest.mark.parametrize("n", [1, 2, 6, 8, 13, 100])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_device_search_and_interpolant_equal_the_host_continuous_output(shim, method, n, backward):
    rng = np.random.default_rng(1000 * n + int(method) * 10 + backward)
    cont, xold, h = _run(method, n, 9, rng, backward)
    _check(shim, method, n, cont, xold, h, _queries(xold, h))


@pytest.mark.parametrize("method", METHODS, ids=lambda m: m.name)
def test_empty_run_and_the_constant_segment(shim, method):
    n = 3
    nc = method.coeffs_per_state() * n
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    y = np.zeros(n)
    z = np.zeros(nc)
    for ex in (0, 1):
        assert shim.dense_eval_host(int(method), n, 0, dp(z), dp(np.zeros(1)), dp(np.zeros(1)), 0.5, ex, dp(y)) == 0
    co = ContinuousOutput.constant(method, 2.0, np.array([1.5, -2.0, 0.25]))
    _check(shim, method, n, co.cont, co.xold, co.h, np.array([2.0, 2.0 + 1e-15, 2.0 + 5e-13, 2.0 - 5e-13, 2.0 + 2e-12, 1.0, 3.0]))
