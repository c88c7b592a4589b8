"""tests/radau_band_model.py -- the real and complex LU and both solves restated ON THE BAND LAYOUT of bdf_band.h /
radau_band.h -- held to the dense restatements radau_wide_model.NUMPY_FNS (themselves held to tests/radau_model.py by
tests/test_radau_wide_model_cpu.py) bit for bit: every in-band factor entry, the pivot rows, the verdicts, the solutions.

Shapes (n, ml, mu) = (12,1,1), (24,2,1), (40,1,3), (65,1,1), (130,4,4).  The families of radau_band_model.band_families cover:
matrices that are not diagonally dominant (more than a quarter of all pivots exchange rows), each of the three multiplier
cases of the complex elimination, a tie between two rows, a zero column and a zero last diagonal entry -- each asserted from
the model's pivots, cases and verdicts."""
import numpy as np
import pytest

from tests import radau_band_model as BM
from tests import radau_wide_model as W

_REF = {}


def reference(shape):
    """per shape, once: (families, dense results, band results)"""
    if shape not in _REF:
        n, ml, mu = shape
        fams = BM.band_families(n, ml, mu)
        _REF[shape] = (fams, [W.factorise_and_solve(f, W.NUMPY_FNS) for f in fams], [BM.factorise_and_solve_band(f, ml, mu) for f in fams])
    return _REF[shape]


def defined_pivots(ok, diag_zero_at, n):
    """how many pivot rows a factorisation defines: all n - 1 if it ran through, else through the column where it stopped"""
    return n - 1 if ok or diag_zero_at is None or diag_zero_at == n - 1 else diag_zero_at + 1


@pytest.mark.parametrize("shape", BM.SHAPES_CPU, ids=[f"n{n}_ml{ml}_mu{mu}" for n, ml, mu in BM.SHAPES_CPU])
def test_band_functions_equal_the_dense_restatements_bit_for_bit(shape):
    n, ml, mu = shape
    fams, dense, band = reference(shape)
    i, j, s = BM.band_slots(n, ml, mu)
    unused = np.ones(n * BM.width(ml, mu), dtype=bool)
    unused[s] = False
    outside = np.ones((n, n), dtype=bool)
    outside[i, j] = False
    for fam, d, b in zip(fams, dense, band):
        tag = f"{shape} {d['tag']}"
        assert b["ok"] == d["ok"] and b["okc"] == d["okc"], tag
        # in-band factor entries; what the dense elimination leaves outside the band is +-0 (the premise of the storage)
        assert W.same_bits(b["f"][s], d["f"][i, j]), (tag, "real factors")
        assert W.same_bits(b["fr"][s], d["fr"][i, j]) and W.same_bits(b["fi"][s], d["fi"][i, j]), (tag, "complex factors")
        assert (d["f"][outside] == 0.0).all() and (d["fr"][outside] == 0.0).all() and (d["fi"][outside] == 0.0).all(), tag
        for blk in (b["f"], b["fr"], b["fi"]):
            assert (blk[unused].view(np.uint64) == 0).all(), (tag, "a slot outside the matrix was written")
        stop = n // 2 if d["tag"] == "zero_column" else None
        upto = defined_pivots(d["ok"], stop, n)
        assert list(b["ip"][:upto]) == list(d["ip"][:upto]), (tag, "real pivots")
        upto = defined_pivots(d["okc"], stop, n)
        assert list(b["ipc"][:upto]) == list(d["ipc"][:upto]), (tag, "complex pivots")
        # solutions where the verdict is ok; the right-hand side of a singular matrix is untouched
        assert W.same_bits(b["x"], d["x"]) and W.same_bits(b["x"], d["x"] if d["ok"] else fam[2]), (tag, "real solution")
        assert W.same_bits(b["xr"], d["xr"]) and W.same_bits(b["xi"], d["xi"]), (tag, "complex solution")
        if not d["okc"]:
            assert W.same_bits(b["xr"], fam[5]) and W.same_bits(b["xi"], fam[6]), tag
        if d["ok"]:
            assert np.isfinite(d["x"]).all() and np.isfinite(d["xr"]).all() and np.isfinite(d["xi"]).all(), tag


def test_the_families_take_the_branches_they_name():
    swaps = swapsc = total = totalc = 0
    for shape in BM.SHAPES_CPU:
        n, ml, mu = shape
        fams, dense, band = reference(shape)
        by = {d["tag"]: d for d in dense}
        bb = {b["tag"]: b for b in band}
        for tag in ("random0", "random1"):
            assert by[tag]["ok"] and by[tag]["okc"], (shape, tag)
            swaps += len(by[tag]["swaps"]); total += n - 1
            swapsc += len(by[tag]["swapsc"]); totalc += n - 1
            assert by[tag]["swaps"] == bb[tag]["swaps"] and by[tag]["swapsc"] == bb[tag]["swapsc"]
        # each multiplier case, from the dense model's and the band model's own record
        assert by["real"]["cases"] - {"skipped"} == {"real"} == bb["real"]["cases"], shape
        assert "imag" in by["imag"]["cases"] and "imag" in bb["imag"]["cases"], shape
        assert "general" in by["general"]["cases"] and "general" in bb["general"]["cases"], shape
        # the tie: rows 0 and 1 of column 0 attain the same maximum, the first wins
        fam = fams[[f[0] for f in fams].index("tie")]
        assert abs(fam[1][0, 0]) == abs(fam[1][1, 0]) and abs(fam[3][0, 0]) + abs(fam[4][0, 0]) == abs(fam[3][1, 0]) + abs(fam[4][1, 0])
        assert by["tie"]["ip"][0] == 0 == by["tie"]["ipc"][0] and by["tie"]["ok"] and by["tie"]["okc"]
        # a zero column stops both factorisations at that pivot; a zero last diagonal entry after the last one
        z = by["zero_column"]
        assert not z["ok"] and not z["okc"] and z["f"][z["ip"][n // 2], n // 2] == 0.0
        zl = by["zero_last"]
        assert not zl["ok"] and not zl["okc"] and zl["ip"][n - 2] == n - 2 == zl["ipc"][n - 2]
    assert swaps * 4 > total and swapsc * 4 > totalc, (swaps, total, swapsc, totalc)
