"""BdfBand::lu_decomp_band / lin_solve_band (ivp_amd/csrc/bdf_band.h) on the MI355X against a numpy restatement of the
DENSE lu_decomp / lin_solve (src/matrix/lu.rs:37-125, src/matrix/linear.rs:55-96; float64, one rounding per operation:
strict mode), in both residencies -- factors in LDS and factors in global memory.

Claim: pivots identical, every in-band factor entry and every solution component bit-identical, the
singular verdict identical; the slots of edge columns that correspond to no matrix entry keep their +0.0.

The matrices are random inside the band and NOT diagonally dominant, so partial pivoting really exchanges rows (asserted
from the numpy side: more than a quarter of all pivots); plus, per shape, a matrix with a zero column (singular at that
pivot) and one whose first column is zero below the diagonal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
SHAPES = [(12, 1, 1), (24, 2, 1), (40, 1, 3), (65, 1, 1), (100, 8, 8), (130, 4, 4), (512, 1, 1)]
NRAND = 5   # random matrices per shape: more than one workgroup at every group width (4 matrices per wave at n <= 16)


# ---- the dense reference ------------------------------------------------------------------------------------------------
def dense_lu(a):
    """lu_decomp in place on a dense (n, n) float64 array; returns (ok, piv, failed_at).  Row operations are numpy vector
    operations over the rows of ONE column: one multiply and one add per entry, each rounded once, as in the scalar loop."""
    n = a.shape[0]
    piv = np.zeros(n, dtype=np.int64)
    for k in range(n - 1):
        col = np.abs(a[k:, k])
        m = k
        if not np.isnan(col[0]):
            best = col[0]
            for i in range(1, n - k):          # first row attaining the maximum; NaNs never win
                if col[i] > best:
                    best, m = col[i], k + i
        piv[k] = m
        if a[m, k] == 0.0:
            return False, piv, k
        if m != k:
            a[[k, m], k:] = a[[m, k], k:]
        t = 1.0 / a[k, k]
        a[k + 1:, k] = -a[k + 1:, k] * t
        mult = a[k + 1:, k].copy()
        for j in range(k + 1, n):
            tj = a[k, j]
            if tj != 0.0:
                a[k + 1:, j] = a[k + 1:, j] + mult * tj
    return bool(a[n - 1, n - 1] != 0.0), piv, (None if a[n - 1, n - 1] != 0.0 else n - 1)


def dense_solve(a, piv, b):
    n = a.shape[0]
    b = b.copy()
    for k in range(n - 1):
        m = int(piv[k])
        t = b[m]
        b[m] = b[k]
        b[k] = t
        b[k + 1:] = b[k + 1:] + a[k + 1:, k] * t
    for k in range(n - 1, 0, -1):
        b[k] = b[k] / a[k, k]
        b[:k] = b[:k] + a[:k, k] * (-b[k])
    b[0] = b[0] / a[0, 0]
    return b


# ---- band packing (bdf_band.h): factor entry (i, j) at j * W + (ml + mu + i - j), W = 2 ml + mu + 1 -----------------------
def band_slots(n, ml, mu):
    """(rows, cols, flat slots) of every factor-band entry that is a matrix entry"""
    kd, w = ml + mu, 2 * ml + mu + 1
    j, off = np.meshgrid(np.arange(n), np.arange(w), indexing="ij")
    i = j + off - kd
    ok = (i >= 0) & (i < n)
    return i[ok], j[ok], (j * w + off)[ok]


def pack(a, ml, mu):
    n = a.shape[0]
    i, j, s = band_slots(n, ml, mu)
    out = np.zeros(n * (2 * ml + mu + 1))
    out[s] = a[i, j]
    return out


def make_set(n, ml, mu, rng):
    i, j = np.indices((n, n))
    band = (i - j <= ml) & (j - i <= mu)
    mats = []
    for _ in range(NRAND):
        a = np.where(band, rng.uniform(-1.0, 1.0, (n, n)), 0.0)
        mats.append(a)
    sing = np.where(band, rng.uniform(-1.0, 1.0, (n, n)), 0.0)
    sing[:, n // 2] = 0.0                                  # a zero pivot column
    mats.append(sing)
    first = np.where(band, rng.uniform(-1.0, 1.0, (n, n)), 0.0)
    first[1:, 0] = 0.0                                     # nothing to eliminate in the first column
    mats.append(first)
    return mats


_REF = {}


def reference(shape):
    """per shape, once: [(matrix, factors, ok, piv, failed_at, b, x)]"""
    if shape not in _REF:
        n, ml, mu = shape
        rng = np.random.default_rng(1000 * n + 10 * ml + mu)
        out = []
        for a in make_set(n, ml, mu, rng):
            f = a.copy()
            ok, piv, failed = dense_lu(f)
            b = rng.uniform(-1.0, 1.0, n)
            x = dense_solve(f, piv, b) if ok else None
            out.append((a, f, ok, piv, failed, b, x))
        _REF[shape] = out
    return _REF[shape]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import torch
    so = str(tmp_path_factory.mktemp("bandlu") / "libband_lu_probe.so")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-Wno-unused-function", os.path.join(HERE, "helpers", "band_lu_probe.hip"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.band_lu_probe.restype = ctypes.c_int
    lib.band_lu_probe.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 4 + [ctypes.c_int]

    def run(n, ml, mu, lds, blocks, rhs):
        dev = torch.device("cuda:0")
        lu = torch.as_tensor(np.ascontiguousarray(blocks), device=dev)
        b = torch.as_tensor(np.ascontiguousarray(rhs), device=dev)
        piv = torch.zeros((len(blocks), n), dtype=torch.int32, device=dev)
        ok = torch.full((len(blocks),), -1, dtype=torch.int32, device=dev)
        assert lib.band_lu_probe(n, ml, mu, int(lds), lu.data_ptr(), piv.data_ptr(), b.data_ptr(), ok.data_ptr(), len(blocks)) == 0
        return lu.cpu().numpy(), piv.cpu().numpy(), b.cpu().numpy(), ok.cpu().numpy()
    return run


def test_the_reference_set_really_pivots_and_stays_in_band():
    """From the numpy side alone: more than a quarter of all pivots are row exchanges, and what the dense elimination
    leaves outside the band (rows below j + ml, rows above j - ml - mu) is +-0 -- the premise of the band storage."""
    swaps = total = 0
    for shape in SHAPES:
        n, ml, mu = shape
        i, j = np.indices((n, n))
        outside = (i - j > ml) | (j - i > ml + mu)
        for a, f, ok, piv, failed, b, x in reference(shape):
            upto = n - 1 if failed is None or failed == n - 1 else failed + 1
            swaps += int((piv[:upto] != np.arange(upto)).sum())
            total += upto
            if ok:
                assert (f[outside] == 0.0).all(), shape
                assert np.isfinite(x).all()
    print(f"row exchanges: {swaps} of {total} pivots")
    assert swaps * 4 > total, (swaps, total)


@pytest.mark.parametrize("lds", [True, False], ids=["lds", "global"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"n{n}_ml{ml}_mu{mu}" for n, ml, mu in SHAPES])
def test_band_lu_and_solve_equal_the_dense_restatement(probe, shape, lds):
    n, ml, mu = shape
    ref = reference(shape)
    blocks = np.stack([pack(a, ml, mu) for a, *_ in ref])
    rhs = np.stack([b for *_, b, _ in ref])
    lu, piv, sol, ok = probe(n, ml, mu, lds, blocks, rhs)
    i, j, s = band_slots(n, ml, mu)
    unused = np.ones(blocks.shape[1], dtype=bool)
    unused[s] = False
    n_sing = 0
    for q, (a, f, want_ok, want_piv, failed, b, x) in enumerate(ref):
        tag = f"{shape} {'lds' if lds else 'global'} matrix {q}"
        assert int(ok[q]) == int(want_ok), tag
        assert (lu[q][unused].view(np.uint64) == 0).all(), tag + ": a slot outside the matrix was written"
        if not want_ok:
            n_sing += 1
            assert np.array_equal(piv[q][:failed + 1], want_piv[:failed + 1]), tag
            assert sol[q].tobytes() == b.tobytes(), tag + ": right-hand side of a singular matrix touched"
            continue
        assert np.array_equal(piv[q][:n - 1], want_piv[:n - 1]), tag
        got, want = lu[q][s], f[i, j]
        bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        assert bad.size == 0, (tag, [(int(i[e]), int(j[e]), got[e], want[e]) for e in bad[:5]])
        assert sol[q].tobytes() == x.tobytes(), (tag, float(np.abs(sol[q] - x).max()))
    assert n_sing >= 1
