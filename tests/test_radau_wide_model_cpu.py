"""tests/radau_wide_model.py -- the numpy restatements of radau_model's linear algebra, finite differences and dense linear
right-hand side that the wide Radau tests (64 < n <= 512) use as their yardstick -- held to tests/radau_model.py bit for bit.
No device.

Each of the five functions at n = 9, 33, 64 and 65 on the matrix families of radau_wide_model.lu_families: a row exchange at
every second pivot, each multiplier case of the complex elimination, a tie between two rows, a NaN at [k][k] and a NaN
elsewhere in column k, a zero pivot in the middle, a zero last diagonal entry (and, at n = 65, pivot rows beyond row 63).
The branch every family names is asserted on the MODEL's own record.  Whole solves at n = 17 and n = 65 (lin_matrix of
tests/test_gpu_radau_group.py, with and without `jac`) equal radau_model.solve in every member and every recorded output."""
import numpy as np
import pytest

from tests import radau_model as M
from tests import radau_wide_model as W

WIDTHS = (9, 33, 64, 65)
_REF = {}


def both(n):
    if n not in _REF:
        fams = W.lu_families(n)
        _REF[n] = ([W.factorise_and_solve(f, W.MODEL_FNS) for f in fams], [W.factorise_and_solve(f, W.NUMPY_FNS) for f in fams])
    return _REF[n]


@pytest.mark.parametrize("n", WIDTHS)
def test_the_families_take_the_branches_they_name(n):
    ref = {r["tag"]: r for r in both(n)[0]}
    ex = ref["exchange"]
    assert ex["ok"] and ex["okc"]
    assert [k for _, k, _ in ex["swaps"]] == list(range(0, n - 1, 2)) == [k for _, k, _ in ex["swapsc"]]
    assert ref["real"]["okc"] and ref["real"]["cases"] == {"real"}
    assert ref["imag"]["okc"] and "imag" in ref["imag"]["cases"]
    assert ref["general"]["okc"] and "general" in ref["general"]["cases"]
    t = ref["tie"]
    assert t["ok"] and t["okc"] and t["ip"][0] == 2 == t["ipc"][0]   # rows 2 and n - 1 tie: the first wins
    d = ref["nan_diagonal"]
    assert d["ip"][1] == 1 == d["ipc"][1] and np.isnan(d["f"]).any() and np.isnan(d["fr"]).any()
    b = ref["nan_below"]
    assert b["ip"][1] != n - 2 and b["ipc"][1] != n - 2 and np.isnan(b["f"][n - 2]).any() and np.isnan(b["fi"][n - 2]).any()
    z = ref["zero_middle"]
    assert not z["ok"] and not z["okc"] and z["f"][n // 2, n // 2] == 0.0 and z["ip"][n // 2 + 1:] == [0] * (n - n // 2 - 1)
    zl = ref["zero_last"]
    assert not zl["ok"] and not zl["okc"] and zl["f"][n - 1, n - 1] == 0.0 and zl["f"][n - 2, n - 2] != 0.0
    if n > 64:
        h = ref["higher_slot"]
        assert h["ok"] and h["okc"] and all(h["ip"][k] == k + 64 == h["ipc"][k] for k in range(n - 64))


@pytest.mark.parametrize("n", WIDTHS)
def test_lu_decomp_and_lin_solve_equal_the_models(n):
    for m, w in zip(*both(n)):
        tag = (n, m["tag"])
        assert m["ok"] == w["ok"] and m["ip"] == w["ip"] and m["swaps"] == w["swaps"], tag
        assert W.same_bits(w["f"], m["f"]), tag
        assert W.same_bits(w["x"], m["x"]), tag


@pytest.mark.parametrize("n", WIDTHS)
def test_lu_decomp_complex_and_lin_solve_complex_equal_the_models(n):
    for m, w in zip(*both(n)):
        tag = (n, m["tag"])
        assert m["okc"] == w["okc"] and m["ipc"] == w["ipc"] and m["swapsc"] == w["swapsc"], tag
        assert w["cases"] - {"skipped"} == m["cases"], tag
        assert W.same_bits(w["fr"], m["fr"]) and W.same_bits(w["fi"], m["fi"]), tag
        assert W.same_bits(w["xr"], m["xr"]) and W.same_bits(w["xi"], m["xi"]), tag
    by = {w["tag"]: w for w in both(n)[1]}
    assert "skipped" in by["zero_last"]["cases"] and "skipped" not in by["general"]["cases"]


def _nonlinear(n):
    """a right-hand side with a state-dependent Jacobian, and one whose component 3 is a NaN"""
    f = lambda x, y: [-(1.0 + 0.01 * i) * y[i] + 0.1 * y[(i + 1) % n] * y[(i + 2) % n] for i in range(n)]
    g = lambda x, y: [M.NAN if i == 3 else -y[i] + y[(i + 3) % n] for i in range(n)]
    return f, g


@pytest.mark.parametrize("n", WIDTHS)
def test_fd_jac_equals_the_models(n):
    f, g = _nonlinear(n)
    y = [0.5 + 0.01 * i * (-1) ** i for i in range(n)]
    y[4] = 0.0        # the perturbation's max(|y|, 1) takes both branches
    y[5] = -3.0
    for fn in (f, g):
        J0 = [[0.0] * n for _ in range(n)]
        J1 = [[0.0] * n for _ in range(n)]
        M.fd_jac(fn, 0.25, y, J0)
        W.fd_jac(fn, 0.25, y, J1)
        assert W.same_bits(np.array(J1), np.array(J0)), n


@pytest.mark.parametrize("n", WIDTHS)
def test_dense_linear_right_hand_side_equals_the_models(n):
    rng = np.random.default_rng(n)
    a = rng.uniform(-1.0, 1.0, (n, n)).tolist()
    a[1][2] = float("inf")
    y = rng.uniform(-1.0, 1.0, n).tolist()
    y[0] = -0.0
    assert W.same_bits(np.array(W.rhs_dense_linear(a)(0.0, y)), np.array(M.rhs_dense_linear(a)(0.0, y)))
    J0 = [[0.0] * n for _ in range(n)]
    J1 = [[0.0] * n for _ in range(n)]
    M.jac_dense_linear(a)(0.0, y, J0)
    W.jac_dense_linear(a)(0.0, y, J1)
    assert J0 == J1


def _lin_matrix(n):
    from tests.test_gpu_radau_group import lin_matrix   # the matrix of the device tests (no device is touched)
    return lin_matrix(n)


@pytest.mark.parametrize("with_jac", [False, True])
@pytest.mark.parametrize("n, t1", [(17, 0.5), (65, 0.02)])
def test_whole_solves_equal_the_models_in_every_member_and_every_recorded_output(n, t1, with_jac):
    a = _lin_matrix(n)
    y0 = [1.0 + 0.01 * i * (-1) ** i for i in range(n)]
    kw = dict(dense_output=True)
    m = M.solve(M.rhs_dense_linear(a), 0.0, t1, y0, 1e-6, 1e-8, jac=M.jac_dense_linear(a) if with_jac else None, **kw)
    w = W.solve(W.rhs_dense_linear(a), 0.0, t1, y0, 1e-6, 1e-8, jac=W.jac_dense_linear(a) if with_jac else None, **kw)
    assert m.status == M.SUCCESS and m.naccpt > 2 and m.pivots
    for k in ("status", "nfev", "njev", "nlu", "nstep", "naccpt", "nrejct", "n_reuse", "n_restart", "pivots", "newton_counts", "eval_idx"):
        assert getattr(m, k) == getattr(w, k), k
    assert w.cases - {"skipped"} == m.cases
    for k in ("t_end", "h_next", "y_end", "t", "h_tried"):
        assert W.same_bits(np.array(getattr(w, k)), np.array(getattr(m, k))), k
    assert len(m.y) == len(w.y) and all(W.same_bits(np.array(p), np.array(q)) for p, q in zip(w.y, m.y))
    assert len(m.segs) == len(w.segs) > 0
    for (c0, x0, h0), (c1, x1, h1) in zip(m.segs, w.segs):
        assert W.same_bits(np.array(c1), np.array(c0)) and x0 == x1 and h0 == h1
    assert M.lu_decomp is W.M_LU_DECOMP and M.fd_jac is W.M_FD_JAC   # the swap is undone
