"""RadauBand::lu_decomp_band_complex / lin_solve_band_complex (ivp_amd/csrc/radau_band.h) alone on the MI355X: one group of
G lanes per matrix, 64 / G matrices per one-wavefront workgroup, the band blocks in global memory, against the band model
(tests/radau_band_model.py, held to the dense restatements bit for bit by tests/test_radau_band_model_cpu.py).

Shapes (n, ml, mu) = (12,1,1), (24,2,1), (40,1,3), (65,1,1), (100,8,8), (130,4,4), (512,1,1): G = 16, 32, 64 and C = 1, 2, 3, 8
rows per lane, a window of 289 entries (five per lane) at ml = mu = 8.  Eight matrices per shape (band_families: two random
ones that are not diagonally dominant, each multiplier case, a tie, a zero column, a zero last diagonal entry), so more than
one wavefront runs at every group width.

Claim: verdicts equal; the pivot rows equal (through the failing column of a singular matrix); every in-band factor entry and
every solution component bit-equal; the right-hand sides of a singular matrix untouched; +0.0 in the slots of edge columns
that correspond to no matrix entry."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import radau_band_model as BM
from tests import radau_wide_model as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
SHAPES = [(12, 1, 1), (24, 2, 1), (40, 1, 3), (65, 1, 1), (100, 8, 8), (130, 4, 4), (512, 1, 1)]
_REF = {}


def reference(shape):
    if shape not in _REF:
        n, ml, mu = shape
        fams = BM.band_families(n, ml, mu)
        _REF[shape] = (fams, [BM.factorise_and_solve_band(f, ml, mu) for f in fams])
    return _REF[shape]


def families_take_their_branches(shape):
    """from the model alone: the set of a shape takes every branch the claim names; returns (row exchanges, pivots) of its
    two random matrices"""
    n, ml, mu = shape
    fams, ref = reference(shape)
    by = {r["tag"]: r for r in ref}
    assert len(fams) >= 5 and len(fams) > 64 // 16
    rnd = [by["random0"], by["random1"]]
    assert all(r["okc"] and len(r["swapsc"]) > 0 for r in rnd)
    assert by["real"]["cases"] == {"real"} and "imag" in by["imag"]["cases"] and "general" in by["general"]["cases"]
    assert by["tie"]["okc"] and by["tie"]["ipc"][0] == 0
    assert not by["zero_column"]["okc"] and not by["zero_last"]["okc"] and by["zero_last"]["ipc"][n - 2] == n - 2
    return sum(len(r["swapsc"]) for r in rnd), 2 * (n - 1)


def test_the_random_matrices_really_exchange_rows():
    """more than a quarter of all pivots of the matrices that are not diagonally dominant"""
    counts = [families_take_their_branches(shape) for shape in SHAPES]
    swaps, total = sum(c[0] for c in counts), sum(c[1] for c in counts)
    assert swaps * 4 > total, (swaps, total)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import torch
    so = str(tmp_path_factory.mktemp("radaubandlu") / "libradau_band_lu_probe.so")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-Wno-unused-function", os.path.join(HERE, "helpers", "radau_band_lu_probe.hip"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.radau_band_lu_probe.restype = ctypes.c_int
    lib.radau_band_lu_probe.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6 + [ctypes.c_int]

    def run(n, ml, mu, blocks_r, blocks_i, rhs_r, rhs_i):
        dev = torch.device("cuda:0")
        up = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
        ar, ai, br, bi = up(blocks_r), up(blocks_i), up(rhs_r), up(rhs_i)
        nm = len(blocks_r)
        piv = torch.zeros((nm, n), dtype=torch.int32, device=dev)
        ok = torch.full((nm,), -1, dtype=torch.int32, device=dev)
        rc = lib.radau_band_lu_probe(n, ml, mu, ar.data_ptr(), ai.data_ptr(), piv.data_ptr(), br.data_ptr(), bi.data_ptr(), ok.data_ptr(), nm)
        assert rc == 0, rc
        return tuple(t.cpu().numpy() for t in (ar, ai, piv, br, bi, ok))
    return run


@pytest.mark.parametrize("shape", SHAPES, ids=[f"n{n}_ml{ml}_mu{mu}" for n, ml, mu in SHAPES])
def test_band_complex_lu_and_solve_equal_the_model(probe, shape):
    n, ml, mu = shape
    fams, ref = reference(shape)
    families_take_their_branches(shape)

    fr, fi, piv, xr, xi, ok = probe(n, ml, mu, np.stack([BM.pack(f[3], ml, mu) for f in fams]), np.stack([BM.pack(f[4], ml, mu) for f in fams]),
                                    np.stack([f[5] for f in fams]), np.stack([f[6] for f in fams]))
    i, j, s = BM.band_slots(n, ml, mu)
    unused = np.ones(n * BM.width(ml, mu), dtype=bool)
    unused[s] = False
    for q, (fam, r) in enumerate(zip(fams, ref)):
        tag = f"{shape} matrix {q} ({r['tag']})"
        assert int(ok[q]) == int(r["okc"]), tag
        assert (fr[q][unused].view(np.uint64) == 0).all() and (fi[q][unused].view(np.uint64) == 0).all(), tag + ": a slot outside the matrix was written"
        upto = n - 1 if r["okc"] or r["tag"] != "zero_column" else n // 2 + 1
        assert [int(v) for v in piv[q][:upto]] == [int(v) for v in r["ipc"][:upto]], (tag, "pivots")
        bad = np.flatnonzero((fr[q][s].view(np.uint64) != r["fr"][s].view(np.uint64)) | (fi[q][s].view(np.uint64) != r["fi"][s].view(np.uint64)))
        assert bad.size == 0, (tag, [(int(i[e]), int(j[e]), fr[q][s][e], r["fr"][s][e], fi[q][s][e], r["fi"][s][e]) for e in bad[:5]])
        if r["okc"]:
            assert W.same_bits(xr[q], r["xr"]) and W.same_bits(xi[q], r["xi"]), (tag, "solution")
        else:
            assert xr[q].tobytes() == fam[5].tobytes() and xi[q].tobytes() == fam[6].tobytes(), tag + ": right-hand side of a singular matrix touched"
