"""Radau IIA(5) for M y' = f(t, y) and index-1/2/3 DAEs at 8 < n <= 64 on the device -- ``DeviceIVP(..., mass_col=True)``
(IVP_RHS_HAS_MASS_COL) through ``ivp_amd.Radau`` / ivp_radau_solve_dae* -> radau_group.h with the mass sites compiled in: one
group of G lanes per trajectory, one row per lane, M in a fifth n^2 block and in LDS -- against the CPU model
tests/radau_dae_model.py, BIT FOR BIT: status, t_end, y_end, h_next and the six counters of every trajectory, and every
recorded output.  No tolerance anywhere.

The problems (device snippet and model right-hand side, the same operations in the same order) are in
tests/radau_group_dae_problems.py; the linear systems are lin_matrix(n) of tests/test_gpu_radau_group.py.  Every test that
names a branch asserts on the MODEL's counters or `cases` that the input takes it.  Model runs are cached per input."""
import ctypes as C

import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import ConfigError, Options, Radau
from tests import radau_dae_model as D
from tests import radau_group_dae_problems as P
from tests import radau_model as M
from tests import test_gpu_radau_dae as DAE
from tests import test_gpu_radau_group as G
from tests import test_gpu_radau_unbounded as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RT, AT = G.RT, G.AT
END = U.END
_np, same, same_vec, dev, cols = U._np, U.same, U.same_vec, U.dev, U.cols
assert_rows = G.assert_rows

_CACHE = {}
_PROBLEMS = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def problem(key, make):
    if key not in _PROBLEMS:
        _PROBLEMS[key] = make()
    return _PROBLEMS[key]


def dae_models(tag, fs, masses, y0s, t0, t1, rtol=RT, atol=AT, nind=(None, None, None), jac=None, **kw):
    """one model run per trajectory, cached on everything that defines it"""
    key = (tag, t0, t1, repr(rtol), repr(atol), nind, tuple(sorted((k, repr(v)) for k, v in kw.items())))
    return [cached(key + (b, tuple(y0)), lambda f=f, ms=ms, y0=y0: D.solve(f, t0, t1, list(y0), rtol, atol, jac=jac, mass=ms, nind1=nind[0], nind2=nind[1],
                                                                              nind3=nind[2], **kw))
            for b, (f, ms, y0) in enumerate(zip(fs, masses, y0s))]


def same_bytes(a, b, names, what):
    for k in names:
        assert _np(getattr(a, k)).tobytes() == _np(getattr(b, k)).tobytes(), (what, k)


# ---- the linear problems ------------------------------------------------------------------------------------------------

def ident_problem(n, with_jac):
    return problem(("ident", n, with_jac), lambda: ivp_amd.DeviceIVP(G.lin_source(G.lin_matrix(n), with_jac) + P.identity_mass_source(), n, jac=with_jac, mass_col=True))


def dense_problem(n):
    a = G.lin_matrix(n)
    return problem(("dense", n), lambda: ivp_amd.DeviceIVP(P.lin_ode_source(a) + P.lin_jac_source(n) + P.dense_mass_source(n), n, params=(1.0,), jac=True, mass_col=True))


def dense_p0(B):
    return [1.0 + 0.5 * b for b in range(B)]


def dense_models(n, y0s, t0=0.0, t1=None, **kw):
    a = G.lin_matrix(n)
    t1 = G.t1_of(n) if t1 is None else t1
    p0 = dense_p0(len(y0s))
    return dae_models(("dense", n), [M.rhs_dense_linear(a)] * len(y0s), [P.dense_mass(n, v) for v in p0], y0s, t0, t1, jac=M.jac_dense_linear(a), **kw)


def dense_args(n, y0s, t0=0.0, t1=None):
    return (dense_problem(n), t0, G.t1_of(n) if t1 is None else t1, dev(G.col(y0s)), dev([dense_p0(len(y0s))]))


# ---- 1. the identity through mass_col: every group width, forward differences and jac_col -------------------------------------

@pytest.mark.parametrize("with_jac", [False, True])
@pytest.mark.parametrize("n", G.WIDTHS)
def test_identity_mass_equals_the_model_and_the_plain_call(n, with_jac):
    """B = 5 at n = 9: four groups in one wavefront, plus a wavefront with three absent groups"""
    B = 5 if n == 9 else (3 if n <= 17 else 2)
    y0s = G.lin_y0s(n, B)
    models = G.lin_models(n, y0s, with_jac)   # radau_model: tests/test_radau_group_dae_cpu.py holds the DAE model to it with M = I
    assert all(m.status == 0 and m.njev > 1 and m.n_reuse > 0 for m in models)
    r = Radau().solve_batch(ident_problem(n, with_jac), 0.0, G.t1_of(n), G.col(y0s), None, G.OPT)
    assert_rows(r, models, f"identity through mass_col, n = {n}, jac_col = {with_jac}")
    plain = Radau().solve_batch(G.lin_problem(n, with_jac), 0.0, G.t1_of(n), G.col(y0s), None, G.OPT)
    same_bytes(r, plain, END, f"mass_col identity against the plain call, n = {n}")


# ---- 2. a dense non-singular M, one per trajectory ------------------------------------------------------------------------------

@pytest.mark.parametrize("n, chunk", [(9, 0), (9, 1), (9, 7), (17, 0), (64, 0)])
def test_dense_mass_matrix_with_a_parameter_per_trajectory(n, chunk):
    """chunk_attempts = 1 / 7: M is brought into LDS by every launch, the factors only when call_decomp is clear"""
    B = 3 if n <= 17 else 2
    y0s = G.lin_y0s(n, B)
    models = dense_models(n, y0s)
    assert all(m.status == 0 and m.njev > 1 for m in models) and (n == 64 or any(m.n_reuse > 0 for m in models))
    assert len({(m.nstep, m.nfev) for m in models}) > 1                      # M differs per trajectory, and so do the runs
    ident = G.lin_models(n, [y0s[0]], True)[0]
    assert (ident.nstep, ident.nfev, ident.y_end) != (models[0].nstep, models[0].nfev, models[0].y_end)   # and M matters
    r = Radau().solve_batch(*dense_args(n, y0s), Options(rtol=RT, atol=AT, chunk_attempts=chunk))
    assert_rows(r, models, f"dense M, n = {n}, chunk_attempts = {chunk}")


# ---- 3. singular M, index 1 -----------------------------------------------------------------------------------------------------

def test_semi_explicit_index_1_system_at_n_10():
    """M = diag(1, .., 1, 0, 0): the last two rows of y' = A y are algebraic; the initial state satisfies them"""
    n = 10
    a = G.lin_matrix(n)
    y0s = []
    for y0 in G.lin_y0s(n, 2):
        r8 = -sum(a[8][j] * y0[j] for j in range(8))
        r9 = -sum(a[9][j] * y0[j] for j in range(8))
        det = a[8][8] * a[9][9] - a[8][9] * a[9][8]
        y0s.append(list(y0[:8]) + [(r8 * a[9][9] - a[8][9] * r9) / det, (a[8][8] * r9 - a[9][8] * r8) / det])
    models = dae_models(("semi", n), [M.rhs_dense_linear(a)] * 2, [P.diag_mass(n, 2)] * 2, y0s, 0.0, 0.5, jac=M.jac_dense_linear(a))
    assert all(m.status == M.SUCCESS and m.naccpt > 5 for m in models)
    prob = problem(("semi", n), lambda: ivp_amd.DeviceIVP(P.lin_ode_source(a) + P.lin_jac_source(n) + P.diag_mass_source(n, 2), n, jac=True, mass_col=True))
    r = Radau().solve_batch(prob, 0.0, 0.5, G.col(y0s), None, G.OPT)
    assert_rows(r, models, "M = diag(1, .., 1, 0, 0)")


def test_zero_mass_and_zero_jacobian_is_singular_matrix_after_five_restarts():
    """M = 0 (the hook writes nothing) and f = 1: E1 = 0 fac1 - 0 is exactly zero, every factorisation fails"""
    n = 9
    y0s = [[1.0 + 0.1 * i for i in range(n)], [0.5] * n]
    models = dae_models(("zero", n), [lambda x, y: [1.0] * n] * 2, [P.diag_mass(n, n)] * 2, y0s, 0.0, 1.0)
    assert all(m.status == M.SINGULAR_MATRIX and m.n_restart == 5 and m.n_restart_real == 6 and m.naccpt == 0 for m in models)
    prob = problem(("zero", n), lambda: ivp_amd.DeviceIVP(f"{P.ODE} {{ return 1.0; }}\n" + P.diag_mass_source(n, n), n, mass_col=True))
    for chunk in (0, 1):
        r = Radau().solve_batch(prob, 0.0, 1.0, G.col(y0s), None, Options(rtol=RT, atol=AT, chunk_attempts=chunk))
        assert_rows(r, models, f"M = 0, chunk_attempts = {chunk}")
        assert all(int(v) == ivp_amd.Status.SingularMatrix for v in _np(r.status))


# ---- 4. stacked pendulums: the index sets ---------------------------------------------------------------------------------------

def pend_states(taus, B, form):
    """trajectory b: every pendulum 0.05 b further along the reference orbit"""
    stack = P.pend2_state if form == 2 else P.pend3_state
    return [stack([P.orbit(tau + 0.05 * b) for tau in taus]) for b in range(B)]


def pend2_problem(k):
    return problem(("pend2", k), lambda: ivp_amd.DeviceIVP(P.pend2_source(k), 5 * k, mass_col=True))


@pytest.mark.parametrize("chunk", [1, 7, 0])
def test_index_2_at_n_10_with_scal_and_hhfac_across_launch_boundaries(chunk):
    """tolerance 1e-4: rejections and Newton dyth exits, whose hhfac and accumulated scal divisions cross launch boundaries"""
    k, B = 2, 3
    y0s = pend_states(P.TAUS_INDEX2_K2, B, 2)
    models = dae_models(("pend2", k), [P.pend2_rhs(k)] * B, [P.pend_mass(k)] * B, y0s, 0.0, 2.0, rtol=1e-4, atol=1e-4, nind=(4 * k, k, 0))
    assert all(m.status == M.SUCCESS for m in models) and models[0].n_dyth >= 1 and models[0].nrejct - models[0].n_dyth >= 1
    assert len({(m.nstep, m.nfev) for m in models}) > 1
    r = Radau(nind1=4 * k, nind2=k, nind3=0).solve_batch(pend2_problem(k), 0.0, 2.0, dev(cols(y0s)), None, Options(rtol=1e-4, atol=1e-4, chunk_attempts=chunk))
    assert_rows(r, models, f"two pendulums, index 2, chunk_attempts = {chunk}")


def test_index_2_at_n_20():
    """G = 32: two groups per wavefront"""
    k, B = 4, 2
    y0s = pend_states(P.TAUS_INDEX2_K4, B, 2)
    models = dae_models(("pend2", k), [P.pend2_rhs(k)] * B, [P.pend_mass(k)] * B, y0s, 0.0, 2.0, rtol=1e-6, atol=1e-6, nind=(None, k, None))
    assert all(m.status == M.SUCCESS and m.naccpt > 10 for m in models)
    r = Radau(nind2=k).solve_batch(pend2_problem(k), 0.0, 2.0, cols(y0s), None, Options(rtol=1e-6, atol=1e-6))   # nind1 inferred
    assert_rows(r, models, "four pendulums, index 2")


@pytest.mark.parametrize("tol", [1e-6, 1e-4])
def test_index_3_at_n_10(tol):
    """1e-6, from the phases tests/test_radau_group_dae_cpu.py holds to the reference orbit: no restart.  1e-4, released at
    rest at the angles 0.1 and 0.2: the model takes an `h *= 0.5` restart -- hhfac = 0.5 is squared into the scales of both lam"""
    k, B = 2, 2
    if tol == 1e-6:
        y0s = pend_states(P.TAUS_INDEX3_K2, B, 3)
    else:
        y0s = [P.pend3_state([P.pend_at_rest(0.1 + 0.05 * b), P.pend_at_rest(0.2 + 0.05 * b)]) for b in range(B)]
    models = dae_models(("pend3", k), [P.pend3_rhs(k)] * B, [P.pend_mass(k)] * B, y0s, 0.0, 2.0, rtol=tol, atol=tol, nind=(2 * k, 2 * k, k), first_step=1e-3)
    assert all(m.status == M.SUCCESS for m in models)
    assert models[0].n_restart == (1 if tol == 1e-4 else 0)
    prob = problem(("pend3", k), lambda: ivp_amd.DeviceIVP(P.pend3_source(k), 5 * k, mass_col=True))
    r = Radau(nind1=2 * k, nind2=2 * k, nind3=k).solve_batch(prob, 0.0, 2.0, cols(y0s), None, Options(rtol=tol, atol=tol, first_step=1e-3))
    assert_rows(r, models, f"two pendulums, index 3, tolerance {tol}")


def test_half_a_wavefront_has_the_wrong_partition_and_its_neighbours_are_untouched():
    """One call with nind2 given as 0, four groups in one wavefront: p[0] selects the constraints per trajectory -- the index-1
    form, for which the partition is right, or the index-2 form, which ends in StepSizeTooSmall"""
    k = 2
    sel = [0.0, 1.0, 1.0, 0.0]
    y0s = [P.pend2_state([P.pend_at_rest(0.1 * b), P.pend_at_rest(0.1 * b + 0.3)]) for b in range(4)]
    models = [cached(("pendsel", b), lambda b=b: D.solve(P.pend2_rhs(k, select=sel[b]), 0.0, 2.0, list(y0s[b]), 1e-6, 1e-6, mass=P.pend_mass(k),
                                                           nind1=5 * k, nind2=0, nind3=0)) for b in range(4)]
    assert [m.status for m in models] == [M.STEP_TOO_SMALL if s else M.SUCCESS for s in sel]
    prob = problem("pendsel", lambda: ivp_amd.DeviceIVP(P.pend2_source(k, selectable=True), 5 * k, params=(0.0,), mass_col=True))
    rad = Radau(nind1=5 * k, nind2=0, nind3=0)
    r = rad.solve_batch(prob, 0.0, 2.0, cols(y0s), cols([[s] for s in sel]), Options(rtol=1e-6, atol=1e-6))
    assert_rows(r, models, "mixed index-1 / index-2 in one wavefront")
    keep = [b for b in range(4) if not sel[b]]
    solo = rad.solve_batch(prob, 0.0, 2.0, np.ascontiguousarray(cols(y0s)[:, keep]), cols([[sel[b]] for b in keep]), Options(rtol=1e-6, atol=1e-6))
    for key in END:
        assert _np(getattr(r, key))[..., keep].tobytes() == _np(getattr(solo, key)).tobytes(), key


def test_index_sets_past_fifteen_variables_at_n_33():
    """nind2 = 17, nind3 = 16: both counts need the high halves of their fields in the kernel arguments.  The system is the
    linear one with M = I -- the sets only divide the error scales, which the model does in the same places"""
    n = 33
    y0s = G.lin_y0s(n, 2)
    a = G.lin_matrix(n)
    models = dae_models(("sets33",), [M.rhs_dense_linear(a)] * 2, [P.identity(n)] * 2, y0s, 0.0, 0.5, nind=(None, 17, 16), jac=M.jac_dense_linear(a))
    plain = G.lin_models(n, y0s, True)
    assert all((m.nstep, m.nfev, m.y_end) != (q.nstep, q.nfev, q.y_end) for m, q in zip(models, plain))   # the sets change the run
    low = dae_models(("sets33",), [M.rhs_dense_linear(a)] * 2, [P.identity(n)] * 2, y0s, 0.0, 0.5, nind=(None, 1, 0), jac=M.jac_dense_linear(a))
    assert all((m.nstep, m.nfev, m.y_end) != (q.nstep, q.nfev, q.y_end) for m, q in zip(models, low))     # ... and not as (17 & 15, 16 & 15) would
    r = Radau(nind2=17, nind3=16).solve_batch(ident_problem(n, True), 0.0, 0.5, G.col(y0s), None, G.OPT)
    assert_rows(r, models, "nind2 = 17, nind3 = 16 at n = 33")


# ---- 5. a NaN neighbour ---------------------------------------------------------------------------------------------------------

def test_nan_initial_state_in_one_group_leaves_the_other_three_of_the_wavefront_untouched():
    n, bad = 9, 2
    y0s = G.lin_y0s(n, 4)
    y0s[bad][3] = float("nan")
    models = dense_models(n, y0s)
    assert models[bad].status != M.SUCCESS or any(v != v for v in models[bad].y_end)
    assert all(models[b].status == M.SUCCESS for b in range(4) if b != bad)
    prob, t0, t1, y0, par = dense_args(n, y0s)
    r = Radau().solve_batch(prob, t0, t1, y0, par, G.OPT)
    assert_rows(r, models, "NaN initial state in group 2 of 4")
    keep = [b for b in range(4) if b != bad]
    solo = Radau().solve_batch(prob, t0, t1, y0[:, keep].contiguous(), par[:, keep].contiguous(), G.OPT)
    for key in END:
        assert _np(getattr(r, key))[..., keep].tobytes() == _np(getattr(solo, key)).tobytes(), key


# ---- 6. every output at n = 17 with a dense M -----------------------------------------------------------------------------------

@pytest.mark.parametrize("t0, t1", [(0.0, 0.5), (0.25, 0.0)])
def test_shared_t_eval_grid_forward_and_backward(t0, t1):
    n = 17
    y0s = G.lin_y0s(n, 2)
    grid = [t0 + f * (t1 - t0) for f in (0.0, 0.2, 0.6, 0.9, 1.0)] + [t1 + 2.0 * (t1 - t0)]   # the ends, inside, a point outside
    models = dense_models(n, y0s, t0, t1, t_eval=grid)
    r = Radau().solve_batch(*dense_args(n, y0s, t0, t1), Options(rtol=RT, atol=AT, t_eval=grid))
    assert_rows(r, models, f"t_eval from {t0} to {t1}")
    for b, m in enumerate(models):
        k = int(r.n_filled[b])
        assert k == len(m.t) == 5 and list(_np(r.eval_idx)[:k, b]) == m.eval_idx
        for q in range(k):
            assert same_vec(_np(r.y_eval)[q, :, b], m.y[q]), (b, q)


@pytest.mark.parametrize("t0, t1", [(0.0, 0.5), (0.25, 0.0)])
def test_per_trajectory_t_eval_grids_forward_and_backward(t0, t1):
    n, B = 17, 3
    y0s = G.lin_y0s(n, B)
    grids = [np.linspace(t0, t1, 3 + 2 * b) if b != 1 else np.zeros(0) for b in range(B)]
    models = [dense_models(n, y0s, t0, t1, t_eval=[float(v) for v in grids[b]])[b] for b in range(B)]
    r = Radau().solve_batch(*dense_args(n, y0s, t0, t1), Options(rtol=RT, atol=AT, t_eval_per_trajectory=grids))
    assert_rows(r, models, f"ragged t_eval from {t0} to {t1}")
    for b, m in enumerate(models):
        idx, y = r.eval_of(b)
        assert list(idx) == m.eval_idx and len(y) == len(m.y)
        for q in range(len(y)):
            assert same_vec(y[q], m.y[q]), (b, q)


def test_bounded_step_log_with_one_trajectory_that_overflows():
    n = 17
    y0s = G.lin_y0s(n, 2)
    t1s = [0.5, 0.025]
    models = [dense_models(n, y0s, 0.0, t1s[b])[b] for b in range(2)]
    ml = len(models[1].t) + 2
    assert len(models[0].t) > ml >= len(models[1].t)
    r = Radau().solve_batch(*dense_args(n, y0s, 0.0, dev(t1s)), Options(rtol=RT, atol=AT, max_log=ml))
    assert_rows(r, models, "bounded step log")
    for b, m in enumerate(models):
        assert int(r.n_log[b]) == len(m.t)
        for q in range(min(ml, len(m.t))):
            assert same(_np(r.t_log)[q, b], m.t[q]) and same_vec(_np(r.y_log)[q, :, b], m.y[q]), (b, q)


def test_dense_segments_and_their_evaluation_on_the_device():
    n, B = 17, 2
    y0s = G.lin_y0s(n, B)
    models = dense_models(n, y0s, dense_output=True)
    ml = max(len(m.segs) for m in models) + 1
    r = Radau().solve_batch(*dense_args(n, y0s), Options(rtol=RT, atol=AT, dense_output=True, max_log=ml))
    assert_rows(r, models, "dense output")
    seg_cont, seg_xold, seg_h = _np(r.seg_cont), _np(r.seg_xold), _np(r.seg_h)
    for b, m in enumerate(models):
        assert int(r.n_seg[b]) == len(m.segs) == m.naccpt
        for q, (cont, xold, h) in enumerate(m.segs):
            assert same(seg_xold[q, b], xold) and same(seg_h[q, b], h) and same_vec(seg_cont[q, :, b], cont), (b, q)
    counts = np.array([int(v) for v in _np(r.n_seg)])
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    cont = np.concatenate([seg_cont[:counts[b], :, b] for b in range(B)])
    xold = np.concatenate([seg_xold[:counts[b], b] for b in range(B)])
    hh = np.concatenate([seg_h[:counts[b], b] for b in range(B)])
    dense = ivp_amd.BatchContinuousOutput(ivp_amd.Method.RADAU, n, torch.as_tensor(off, device=DEV), dev(cont), dev(xold), dev(hh),
                                          ivp_amd.FpMode.STRICT, ivp_amd.default_context(0))   # ivp_dense_eval_device(IVP_RADAU)
    grid = np.array([-0.25, 0.0, 1e-7, 0.16665, 0.25, 0.5, 0.625])
    for extrapolate in (False, True):
        y, found = dense(grid, extrapolate=extrapolate)
        y, found = _np(y), _np(found)
        for b, m in enumerate(models):
            for q, t in enumerate(grid):
                seg, kind = G._find_segment(m.segs, float(t), extrapolate)
                assert int(found[q, b]) == kind, (b, q, extrapolate)
                if kind == 0:
                    assert np.isnan(y[q, :, b]).all()
                else:
                    assert same_vec(y[q, :, b], M.interpolate(float(t), *seg)), (b, q, extrapolate)


def test_logged_and_dense_csr_through_the_dae_call():
    """solve_batch_logged and solve_batch_dense with a `dae`; max_log = 0 is a pool so small that the second pass runs"""
    n, B = 17, 3
    y0s = G.lin_y0s(n, B)
    models = dense_models(n, y0s, dense_output=True)
    assert all(m.status == 0 and len(m.segs) == m.naccpt > 8 for m in models)
    r = Radau().solve_batch_logged(*dense_args(n, y0s), Options(rtol=RT, atol=AT))
    assert r.log_info["passes"] == 1
    U.hold_log(r, models, "dense M, logged")
    for ml in (0, 1 << 12):
        d = Radau().solve_batch_dense(*dense_args(n, y0s), Options(rtol=RT, atol=AT, max_log=ml))
        assert d.dense_info["passes"] == (2 if ml == 0 else 1), d.dense_info
        U.hold_dense(d, models, f"dense M, dense CSR, max_log = {ml}")
        U.hold_sol(d, models, f"dense M, sol, max_log = {ml}")


def test_wait_false_equals_the_model():
    n, B = 17, 3
    y0s = G.lin_y0s(n, B)
    models = dense_models(n, y0s)
    pend = Radau().solve_batch(*dense_args(n, y0s), Options(rtol=RT, atol=AT, chunk_attempts=7), ctx=ivp_amd.Context(0), wait=False)
    assert isinstance(pend, ivp_amd.api.PendingBatch)
    U.hold_end(pend.result(), models, "dense M, wait=False, chunk_attempts = 7")


# ---- 7. per-component tolerances with an index-2 set ----------------------------------------------------------------------------

def test_vector_tolerances_and_the_same_vectors_reversed_at_n_10_with_an_index_2_set():
    k, n = 2, 10
    rt = [10.0 ** -(4 + (i % 3)) for i in range(n)]
    at = [10.0 ** -(5 + (i % 4)) for i in range(n)]
    y0s = pend_states(P.TAUS_INDEX2_K2, 2, 2)
    run = lambda r_, a_: dae_models(("pend2", k), [P.pend2_rhs(k)] * 2, [P.pend_mass(k)] * 2, y0s, 0.0, 2.0, rtol=r_, atol=a_, nind=(4 * k, k, 0))
    fwd, rev = run(rt, at), run(rt[::-1], at[::-1])
    assert all(a.status == b.status == M.SUCCESS and (a.nstep, a.nfev, a.y_end) != (b.nstep, b.nfev, b.y_end) for a, b in zip(fwd, rev))
    rad = Radau(nind1=4 * k, nind2=k, nind3=0)
    assert_rows(rad.solve_batch(pend2_problem(k), 0.0, 2.0, cols(y0s), None, Options(rtol=rt, atol=at)), fwd, "vector tolerances")
    assert_rows(rad.solve_batch(pend2_problem(k), 0.0, 2.0, cols(y0s), None, Options(rtol=rt[::-1], atol=at[::-1])), rev, "vector tolerances reversed")


# ---- 8. sequences on one context ------------------------------------------------------------------------------------------------

def test_mass_col_n17_plain_n17_thread_dae_n5_mass_col_n17_on_one_context_equal_fresh_contexts():
    """the matrix block is 5 n^2 doubles per trajectory, then 4 n^2 in the same buffer, then the thread form's SoA arrays"""
    y17 = G.lin_y0s(17, 3)
    p17 = G.lin_problem(17, True)
    pend = ivp_amd.DeviceIVP(DAE.PEND2_SRC, 5, mass=True)
    y5 = cols([DAE.pend_y0(0.0), DAE.pend_y0(0.6435011087932844)])
    o_end, o_dense = G.OPT, Options(rtol=RT, atol=AT, dense_output=True, max_log=200)
    calls = (lambda c: Radau().solve_batch(*dense_args(17, y17), o_end, ctx=c),
             lambda c: Radau().solve_batch(p17, 0.0, 0.5, dev(G.col(y17)), None, o_end, ctx=c),
             lambda c: Radau(nind1=4, nind2=1, nind3=0).solve_batch(pend, 0.0, 2.0, dev(y5), None, Options(rtol=1e-4, atol=1e-4), ctx=c),
             lambda c: Radau().solve_batch(*dense_args(17, y17), o_dense, ctx=c))
    fresh = [call(ivp_amd.Context(0)) for call in calls]
    one = ivp_amd.Context(0)
    seq = [call(one) for call in calls]
    for a, b in zip(seq, fresh):
        for k in END + ("n_seg", "seg_cont", "seg_xold", "seg_h"):
            va, vb = getattr(a, k, None), getattr(b, k, None)
            assert (va is None) == (vb is None), k
            if va is None:
                continue
            va, vb = _np(va), _np(vb)
            if k.startswith("seg_"):   # slots past a trajectory's count are never written
                ns = _np(a.n_seg)
                for t in range(va.shape[-1]):
                    assert va[:ns[t], ..., t].tobytes() == vb[:ns[t], ..., t].tobytes(), (k, t)
            else:
                assert va.tobytes() == vb.tobytes(), k
    assert_rows(seq[0], dense_models(17, y17), "first solve of the sequence")
    assert_rows(seq[3], dense_models(17, y17), "fourth solve of the sequence")
    assert_rows(seq[1], G.lin_models(17, y17, True), "second solve of the sequence")


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------

def test_compile_time_refusals():
    from ivp_amd import _lib
    lib, ctx = _lib.load(), ivp_amd.default_context(0)
    h = C.c_void_p()
    src = (f"{P.ODE} {{ return -y[i]; }}\n" + P.identity_mass_source()).encode()
    small = ("__device__ void ode(double x, const double* y, double* d, const double* p) { for (int i = 0; i < 8; ++i) d[i] = -y[i]; }\n"
             + P.identity_mass_source()).encode()
    assert lib.ivp_rhs_compile_ex(ctx.handle, small, 8, 0, 0, 16, C.byref(h)) == -100
    assert "IVP_RHS_HAS_MASS_COL" in ctx.last_error() and "8 < n <= 64" in ctx.last_error() and "use IVP_RHS_HAS_MASS" in ctx.last_error()
    assert lib.ivp_rhs_compile_ex(ctx.handle, src, 65, 0, 0, 16, C.byref(h)) == -100
    assert "IVP_RHS_HAS_MASS_COL" in ctx.last_error() and "8 < n <= 64" in ctx.last_error()
    ev = src + b"__device__ void events(double x, const double* y, double* g, const double* p) { g[0] = y[0]; }\n"
    assert lib.ivp_rhs_compile_ex(ctx.handle, ev, 10, 0, 1, 16, C.byref(h)) == -100
    assert "IVP_RHS_HAS_MASS_COL" in ctx.last_error() and "n_events == 0" in ctx.last_error()
    assert lib.ivp_rhs_compile_ex(ctx.handle, src, 10, 0, 0, 16 | 4, C.byref(h)) == -100 and "IVP_RHS_HAS_MASS_COL" in ctx.last_error()
    col_ptr = (C.c_int32 * 11)(*range(11))
    row_idx = (C.c_int32 * 10)(*range(10))
    assert lib.ivp_rhs_compile_sparse(ctx.handle, src, 10, 0, 0, 16, col_ptr, row_idx, C.byref(h)) == -100 and "unknown flags" in ctx.last_error()
    # a mass_col of the wrong signature surfaces when the problem is compiled: the group Radau module is the one built eagerly
    bad = f"{P.ODE} {{ return -y[i]; }}\n__device__ void mass_col(int col, double* column) {{ column[col] = 1.0; }}\n"
    assert lib.ivp_rhs_compile_ex(ctx.handle, bad.encode(), 10, 0, 0, 16, C.byref(h)) == -104
    with pytest.raises(ConfigError) as e:
        ivp_amd.DeviceIVP(bad, 10, mass_col=True)
    assert e.value.code == -104


def test_a_mass_col_problem_is_refused_by_everything_but_the_dae_call():
    from ivp_amd import _lib
    n = 9
    prob = ident_problem(n, True)
    y0 = G.col(G.lin_y0s(n, 1))
    for method in ("DOPRI5", "BDF"):
        with pytest.raises(ConfigError) as e:
            ivp_amd.solve_ivp_batch(prob, 0.0, 0.5, y0, None, Options(method=method))
        assert e.value.code == -100 and "mass matrix" in str(e.value) and "Radau DAE call only" in str(e.value)
    lib, ctx = _lib.load(), ivp_amd.default_context(0)
    p = _lib.ProblemT()
    p.rhs_id, p.n, p.n_params, p.jit = 1000, n, 0, prob.handle
    o = _lib.OptionsT()
    lib.ivp_options_default(C.byref(o))
    r = _lib.BatchResultT()
    t = np.zeros(1)
    rc = lib.ivp_radau_solve(ctx.handle, C.byref(p), 1, y0.ctypes.data, None, t.ctypes.data, 1, t.ctypes.data, 1, C.byref(o), None, C.byref(r))
    assert rc == -100 and "Radau DAE call only" in ctx.last_error()
    msg = C.create_string_buffer(512)
    assert lib.ivp_radau_check(C.byref(p), 1, C.byref(o), None, msg, 512) == -100 and b"Radau DAE call only" in msg.value
    assert lib.ivp_radau_dae_check(C.byref(p), 1, C.byref(o), None, None, msg, 512) == 0


def test_partitions_with_and_without_the_hook():
    from ivp_amd import _lib
    lib = _lib.load()
    # nind2 = 1 on a hook-less n = 9 problem: still "not yet"
    with pytest.raises(ConfigError) as e:
        Radau(nind2=1).solve_batch(G.lin_problem(9, True), 0.0, 0.5, G.col(G.lin_y0s(9, 1)), None, G.OPT)
    assert e.value.code == -100 and "not yet" in str(e.value)
    # a bad partition at n = 10: code -7
    with pytest.raises(ConfigError) as e:
        Radau(nind1=4, nind2=4, nind3=1).solve_batch(pend2_problem(2), 0.0, 2.0, cols(pend_states(P.TAUS_INDEX2_K2, 1, 2)), None, G.OPT)
    assert e.value.code == -7
    # nind2 = 40 at n = 64 with the hook: counts past 15 are accepted
    p = _lib.ProblemT()
    p.rhs_id, p.n, p.n_params, p.jit = 1000, 64, 0, ident_problem(64, True).handle
    o = _lib.OptionsT()
    lib.ivp_options_default(C.byref(o))
    d = _lib.RadauDaeT()
    d.has_nind2, d.nind2 = 1, 40
    msg = C.create_string_buffer(512)
    assert lib.ivp_radau_dae_check(C.byref(p), 2, C.byref(o), None, C.byref(d), msg, 512) == 0, msg.value
    d.has_nind3, d.nind3 = 1, 25
    assert lib.ivp_radau_dae_check(C.byref(p), 2, C.byref(o), None, C.byref(d), msg, 512) == -7
