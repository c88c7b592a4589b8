"""Radau IIA(5) for 64 < n <= 512 on the device (ivp_amd.Radau -> ivp_radau_solve*() -> the wide form of radau_group.h: one
wavefront per trajectory, lane l owns rows l, l + 64, ..., J and the three factors in global memory) against the CPU model,
BIT FOR BIT: status, t_end, y_end, h_next and the six counters of every trajectory, and every recorded output.  No tolerance
anywhere.

The yardstick is tests/radau_model.py run through tests/radau_wide_model.py (its linear algebra and finite differences
restated in numpy, held to it bit for bit by tests/test_radau_wide_model_cpu.py).  The systems are lin_matrix(n) of
tests/test_gpu_radau_group.py -- y' = A y, a negative diagonal, 2000 below the diagonal in every odd row so that both
factorisations exchange rows -- with the entries computed in the device code (the same IEEE operations as the table's, so
the module text stays small at n = 512), the heat equation, and one problem whose Jacobian is a 2 x 2 block in rows 63 and
64 beside a diagonal.  Every test that names a branch asserts on the MODEL's counters or `cases` that its input takes it.
Model runs are cached per input.  Before the wide form existed every solve here was refused: ConfigError -100, "not yet on
the accelerated path (n <= 64)"."""
import ctypes as C

import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import Options, Radau
from ivp_amd.pipeline import BatchPipeline
from tests import radau_model as M
from tests import radau_wide_model as W
from tests import test_gpu_radau_group as G
from tests import test_gpu_radau_unbounded as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RT, AT = 1e-6, 1e-8
OPT = Options(rtol=RT, atol=AT)
WIDTHS = (65, 100, 128, 129, 257, 512)   # C = 2, 2, 2, 3, 5, 8 rows per lane
_CACHE = {}


def model(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


# ---- inputs -----------------------------------------------------------------------------------------------------------

def wide_source(n, with_jac):
    """lin_matrix(n), n > 33, entry by entry in the device code: 1e-3 * (1 + (3 i + 5 j) % 7), -1 - 0.25 i on the diagonal, 2000
    at [i][i - 1] in odd rows; every row summed left to right (M.rhs_dense_linear)"""
    src = ("__device__ double lin_a(int i, int j) {\n"
           "  if (i == j) return -1.0 - 0.25 * (double)i;\n"
           "  if ((i & 1) && j == i - 1) return 2000.0;\n"
           "  return 1e-3 * (double)(1 + ((3 * i + 5 * j) % 7));\n}\n"
           "__device__ double ode_comp(int i, double x, const double* y, const double* p) {\n"
           "  double s = lin_a(i, 0) * y[0];\n"
           f"  for (int j = 1; j < {n}; ++j) s = s + lin_a(i, j) * y[j];\n"
           "  return s;\n}\n")
    if with_jac:
        src += ("__device__ void jac_col(int col, double x, const double* y, double* column, const double* p) {\n"
                f"  for (int r = 0; r < {n}; ++r) column[r] = lin_a(r, col);\n}}\n")
    return src


def wide_problem(n, with_jac):
    return ivp_amd.DeviceIVP(wide_source(n, with_jac), n, jac=with_jac)


def setup_of(n):
    """(rtol, atol, first_step, t1 of the two trajectories).  At n >= 257 the model must stay quick: a first step of 4e-3
    that these tolerances accept (U1 / h and |ALPH + i BETA| / h are then below the coupling of 2000: both factorisations
    exchange rows) and an interval of three such steps."""
    if n >= 257:
        return 1e-2, 1e-4, 4e-3, [0.012, 0.006]
    return RT, AT, None, [0.02, 0.017 if n == 100 else 0.013]   # (second ends chosen so that the two step counts differ)


def wide_models(n, y0s, with_jac, t0=0.0, t1s=None, rtol=None, atol=None, **kw):
    a = G.lin_matrix(n)
    rt, at, fs, t1d = setup_of(n)
    rtol, atol = rt if rtol is None else rtol, at if atol is None else atol
    t1s = t1d if t1s is None else t1s
    if fs is not None:
        kw.setdefault("first_step", fs)
    key = ("lin", n, with_jac, t0, repr(rtol), repr(atol), tuple(sorted((k, repr(v)) for k, v in kw.items())))
    settings = kw.pop("settings_kw", None)
    if settings:
        kw["settings"] = M.Settings(**settings)
    return [model(key + (tuple(y0), t1), lambda y0=y0, t1=t1: W.solve(W.rhs_dense_linear(a), t0, t1, list(y0), rtol, atol,
                                                                          jac=W.jac_dense_linear(a) if with_jac else None, **kw))
            for y0, t1 in zip(y0s, t1s)]


def wide_options(n, **kw):
    rt, at, fs, _ = setup_of(n)
    if fs is not None:
        kw.setdefault("first_step", fs)
    return Options(rtol=rt, atol=at, **kw)


# a 2 x 2 block in rows 63 and 64 -- the last row of slot 0 and the only row of slot 1 -- beside a diagonal, n = 65
BLOCK_SRC = ("__device__ double ode_comp(int i, double x, const double* y, const double* p) {\n"
             "  if (i == 63) return p[0] * y[63] + p[1] * y[64];\n"
             "  if (i == 64) return p[2] * y[63] + p[3] * y[64];\n"
             "  return p[4] * y[i];\n}\n"
             "__device__ void jac_col(int col, double x, const double* y, double* column, const double* p) {\n"
             "  if (col == 63) { column[63] = p[0]; column[64] = p[2]; }\n"
             "  else if (col == 64) { column[63] = p[1]; column[64] = p[3]; }\n"
             "  else column[col] = p[4];\n}\n")


def block_rhs(p):
    return lambda x, y: [p[4] * y[i] for i in range(63)] + [p[0] * y[63] + p[1] * y[64], p[2] * y[63] + p[3] * y[64]]


def block_jac(p):
    def jac(x, y, J):
        J[63][63], J[63][64], J[64][63], J[64][64] = p[0], p[1], p[2], p[3]
        for i in range(63):
            J[i][i] = p[4]
    return jac


def block_run(ps, y0s, t1, h=None, **okw):
    kw = {} if h is None else dict(first_step=h)
    models = [W.solve(block_rhs(p), 0.0, t1, list(y0), RT, AT, jac=block_jac(p), **kw) for p, y0 in zip(ps, y0s)]
    prob = ivp_amd.DeviceIVP(BLOCK_SRC, 65, params=ps[0], jac=True)
    r = Radau().solve_batch(prob, 0.0, t1, G.col(y0s), np.array(ps).T.copy(), Options(rtol=RT, atol=AT, **kw, **okw))
    return models, r


def block_y0s():
    return [[1.0] * 65, [0.5 + 0.01 * i for i in range(63)] + [0.3, -0.7]]


# ---- 1. every width, forward differences and jac_col --------------------------------------------------------------------

def test_the_device_codes_matrix_is_lin_matrix():
    for n in (65, 512):
        a = G.lin_matrix(n)
        f = lambda i, j: -1.0 - 0.25 * float(i) if i == j else (2000.0 if (i & 1) and j == i - 1 else 1e-3 * float(1 + ((3 * i + 5 * j) % 7)))
        assert all(a[i][j] == f(i, j) for i in range(n) for j in range(0, n, 7)) and all(a[i][i - 1] == f(i, i - 1) for i in range(1, n))


@pytest.mark.parametrize("with_jac", [False, True])
@pytest.mark.parametrize("n", WIDTHS)
def test_every_width_with_forward_differences_and_with_jac_col(n, with_jac):
    y0s = G.lin_y0s(n, 2)
    models = wide_models(n, y0s, with_jac)
    # every trajectory factorises at least twice (nlu counts two factorisations per round and one solve per error estimate)
    assert all(m.status == 0 and m.nlu >= 6 and m.nstep >= 2 for m in models) and models[0].njev > 1
    assert all(any(p[0] == "real" for p in m.pivots) and any(p[0] == "complex" for p in m.pivots) for m in models)
    assert models[0].nstep != models[1].nstep   # the two workgroups take different step counts
    if n >= 257:
        assert all(m.nstep <= 4 for m in models)
    r = Radau().solve_batch(wide_problem(n, with_jac), 0.0, np.array(setup_of(n)[3]), G.col(y0s), None, wide_options(n))
    G.assert_rows(r, models, f"n = {n}, jac_col = {with_jac}")


# ---- 2. a tridiagonal system: the skipped-columns path ------------------------------------------------------------------

HEAT_N = 129
HEAT_SRC = ("__device__ double ode_comp(int i, double x, const double* y, const double* p) {\n"
            "  const double left = i > 0 ? y[i - 1] : 0.0;\n"
            f"  const double right = i < {HEAT_N - 1} ? y[i + 1] : 0.0;\n"
            "  return p[0] * ((left - 2.0 * y[i]) + right);\n}\n"
            "__device__ void jac_col(int col, double x, const double* y, double* column, const double* p) {\n"
            "  if (col > 0) column[col - 1] = p[0];\n"
            "  column[col] = -2.0 * p[0];\n"
            f"  if (col < {HEAT_N - 1}) column[col + 1] = p[0];\n}}\n")


def heat_rhs(k, n=HEAT_N):
    return lambda x, y: [k * (((y[i - 1] if i > 0 else 0.0) - 2.0 * y[i]) + (y[i + 1] if i < n - 1 else 0.0)) for i in range(n)]


def heat_jac(k, n=HEAT_N):
    def jac(x, y, J):
        for c in range(n):
            if c > 0:
                J[c - 1][c] = k
            J[c][c] = -2.0 * k
            if c < n - 1:
                J[c + 1][c] = k
    return jac


def test_heat_equation_with_jac_col_skips_the_columns_outside_the_band():
    n = HEAT_N
    ks = [float((n + 1) ** 2) * 0.1, float((n + 1) ** 2) * 0.25]
    y0s = [[np.sin(np.pi * (i + 1) / (n + 1)) + 0.1 * b * np.sin(3.0 * np.pi * (i + 1) / (n + 1)) for i in range(n)] for b in range(2)]
    y0s = [[float(v) for v in y0] for y0 in y0s]
    models = [model(("heat", b), lambda b=b: W.solve(heat_rhs(ks[b]), 0.0, 0.05, y0s[b], RT, AT, jac=heat_jac(ks[b]))) for b in range(2)]
    assert all(m.status == 0 and m.naccpt > 3 and "skipped" in m.cases for m in models)
    prob = ivp_amd.DeviceIVP(HEAT_SRC, n, params=[ks[0]], jac=True)
    r = Radau().solve_batch(prob, 0.0, 0.05, G.col(y0s), np.array([ks]), OPT)
    G.assert_rows(r, models, "heat equation, n = 129")


# ---- 3. n = 65: launch boundaries, every output path, backward, restarts ---------------------------------------------------

def models65(**kw):
    return wide_models(65, G.lin_y0s(65, 2), True, **kw)


def y65():
    return G.col(G.lin_y0s(65, 2))


T65 = np.array(setup_of(65)[3])


@pytest.mark.parametrize("chunk", [1, 7, 0])
def test_chunk_length_does_not_change_a_bit_or_nlu(chunk):
    y0s = G.lin_y0s(65, 2)
    models = wide_models(65, y0s, False, t1s=[0.02, 0.02])
    assert all(m.n_reuse > 0 for m in models)   # accepted steps that keep the factors: with chunk = 1 another launch uses them
    r = Radau().solve_batch(wide_problem(65, False), 0.0, 0.02, dev(G.col(y0s)), None, Options(rtol=RT, atol=AT, chunk_attempts=chunk))
    G.assert_rows(r, models, f"chunk_attempts = {chunk}")


def test_shared_t_eval_grid():
    t1 = float(T65[0])
    grid = [0.0, 0.2 * t1, 0.2 * t1 + 1e-13, 0.6 * t1, 0.9 * t1, t1, t1 + 0.5]
    models = models65(t1s=[t1, t1], t_eval=grid)
    r = Radau().solve_batch(wide_problem(65, True), 0.0, t1, y65(), None, Options(rtol=RT, atol=AT, t_eval=grid))
    G.assert_rows(r, models, "t_eval")
    for b, m in enumerate(models):
        k = int(r.n_filled[b])
        assert k == len(m.t) == 6 and list(r.eval_idx[:k, b]) == m.eval_idx
        assert all(G.same_vec(r.y_eval[q, :, b], m.y[q]) for q in range(k)), b


def test_bounded_step_log_with_one_trajectory_that_overflows():
    models = models65()
    ml = len(models[1].t)
    assert len(models[0].t) > ml >= len(models[1].t)
    r = Radau().solve_batch(wide_problem(65, True), 0.0, T65, y65(), None, Options(rtol=RT, atol=AT, max_log=ml))
    G.assert_rows(r, models, "step log")
    for b, m in enumerate(models):
        assert int(r.n_log[b]) == len(m.t)
        for q in range(min(ml, len(m.t))):
            assert G.same(r.t_log[q, b], m.t[q]) and G.same_vec(r.y_log[q, :, b], m.y[q]), (b, q)


def test_bounded_dense_segments():
    models = models65(dense_output=True)
    ml = max(len(m.segs) for m in models) + 1
    r = Radau().solve_batch(wide_problem(65, True), 0.0, T65, y65(), None, Options(rtol=RT, atol=AT, dense_output=True, max_log=ml))
    G.assert_rows(r, models, "dense output")
    for b, m in enumerate(models):
        assert int(r.n_seg[b]) == len(m.segs) == m.naccpt
        for q, (cont, xold, h) in enumerate(m.segs):
            assert G.same(r.seg_xold[q, b], xold) and G.same(r.seg_h[q, b], h) and G.same_vec(r.seg_cont[q, :, b], cont), (b, q)


def test_wait_false_logged_and_dense_csr():
    models = models65(dense_output=True)
    prob, args = wide_problem(65, True), (0.0, dev(T65), dev(y65()), None)
    pend = Radau().solve_batch(prob, *args, Options(rtol=RT, atol=AT, chunk_attempts=3), ctx=ivp_amd.Context(0), wait=False)
    assert isinstance(pend, ivp_amd.api.PendingBatch)
    U.hold_end(pend.result(), models, "wait=False")
    r = Radau().solve_batch_logged(prob, *args, Options(rtol=RT, atol=AT, chunk_attempts=3))
    assert r.log_info["passes"] == 1
    U.hold_log(r, models, "logged")
    for ml in (1 << 10, 1):
        d = Radau().solve_batch_dense(prob, *args, Options(rtol=RT, atol=AT, max_log=ml))
        assert d.dense_info["passes"] == (1 if ml > 1 else 2), d.dense_info
        U.hold_dense(d, models, f"dense CSR, max_log = {ml}")
        U.hold_sol(d, models, f"BatchContinuousOutput, max_log = {ml}")


def test_pipeline_map_and_the_scipy_front_end():
    models = models65()
    prob, o = wide_problem(65, True), OPT
    batches = [dict(t0=0.0, t1=float(T65[k]), y0=dev(y65()[:, k:k + 1]), params=None) for k in range(2)]
    got = BatchPipeline(streams=2).map(prob, batches, o, radau=Radau())
    for k in range(2):
        U.hold_end(got[k], models[k:k + 1], f"pipeline batch {k}")
    y0 = G.lin_y0s(65, 1)[0]
    grid = np.linspace(0.0, float(T65[0]), 5)
    src = wide_source(65, True)
    cut = src.index("__device__ void jac_col")
    res = ivp_amd.pyfront.solve_ivp(src[:cut], (0.0, float(T65[0])), y0, method="Radau", rtol=RT, atol=AT, t_eval=grid, jac=src[cut:])
    m = wide_models(65, [y0], True, t1s=[float(T65[0])], t_eval=[float(v) for v in grid])[0]
    assert res.success and res.status == 0 and (res.nfev, res.njev, res.nlu) == (m.nfev, m.njev, m.nlu)
    assert len(res.t) == len(m.t) == 5 and all(G.same_vec(np.asarray(res.y)[:, q], m.y[q]) for q in range(5))


def test_backward_integration():
    y0s = G.lin_y0s(65, 2)
    models = wide_models(65, y0s, True, t0=0.01, t1s=[0.0, 0.003])
    assert all(m.status == 0 and m.h_next < 0.0 for m in models) and models[0].t_end == 0.0
    r = Radau().solve_batch(wide_problem(65, True), 0.01, np.array([0.0, 0.003]), G.col(y0s), None, OPT)
    G.assert_rows(r, models, "backwards")


def test_step_rejections():
    y0s = G.lin_y0s(65, 2)
    models = wide_models(65, y0s, True, first_step=5e-3)
    assert all(m.status == 0 and (m.nrejct > 0 or m.n_first_reject > 0) for m in models)
    r = Radau().solve_batch(wide_problem(65, True), 0.0, T65, G.col(y0s), None, Options(rtol=RT, atol=AT, first_step=5e-3))
    G.assert_rows(r, models, "a rejected first step")


def test_newton_maxiter_1_is_status_singular_matrix_after_five_restarts():
    models = models65(settings_kw=dict(newton_maxiter=1))
    assert all(m.status == M.SINGULAR_MATRIX and m.n_restart == 5 and m.n_restart_newton == 6 and m.naccpt == 0 for m in models)
    for chunk in (0, 1):
        r = Radau(newton_maxiter=1).solve_batch(wide_problem(65, True), 0.0, T65, y65(), None, Options(rtol=RT, atol=AT, chunk_attempts=chunk))
        G.assert_rows(r, models, f"newton_maxiter = 1, chunk_attempts = {chunk}")


def test_real_zero_pivot_at_row_64():
    """J = diag(-1, ..., -1, k) with k = U1 / h: E1[64][64] = U1 / h - k is exactly zero, the only row of slot 1"""
    h = 0.01
    k = M.U1 / h
    ps = [[-1.0, 0.0, 0.0, k, -1.0]] * 2
    models, r = block_run(ps, block_y0s(), 0.03, h)
    assert all(m.n_restart_real == 1 and m.n_restart == 1 and m.n_restart_complex == 0 and m.h_tried[0] == 0.5 * h for m in models)
    G.assert_rows(r, models, "real zero pivot at row 64")


def test_complex_zero_pivot_at_row_64():
    """The rotation block [[a, -b], [b, a]], a = ALPH / h, b = BETA / h, in rows 63 and 64: E2 = [[i b, b], [-b, i b]] there,
    the pivot of row 64 exactly zero."""
    h = 2.0 ** -6
    a, b = M.ALPH / h, M.BETA / h
    ps = [[a, -b, b, a, -1.0]] * 2
    models, r = block_run(ps, block_y0s(), 4.0 * h, h)
    assert all(m.n_restart_complex == 1 and m.n_restart == 1 and m.n_restart_real == 0 and m.h_tried[0] == 0.5 * h for m in models)
    G.assert_rows(r, models, "complex zero pivot at row 64")


def test_purely_imaginary_multiplier_with_the_pivot_row_in_slot_1():
    h = 2.0 ** -10
    ps = [[0.0, 1.0, -1e5, M.ALPH / h, -1.0]] * 2
    models, r = block_run(ps, block_y0s(), 8.0 * h, h)
    assert all("imag" in m.cases and ("complex", 63, 64) in m.pivots for m in models)
    G.assert_rows(r, models, "imaginary multiplier")


def test_nan_right_hand_side_beside_a_healthy_trajectory():
    ps = [[-2.0, 1.0, -1.0, -3.0, -1.5], [-2.0, 1.0, -1.0, -3.0, float("nan")]]
    y0s = block_y0s()
    models, r = block_run(ps, y0s, 0.25)
    assert models[0].status == M.SUCCESS and (models[1].status != M.SUCCESS or any(v != v for v in models[1].y_end))
    G.assert_rows(r, models, "NaN right-hand side in workgroup 1 of 2")


# ---- 4. sequences on one context -------------------------------------------------------------------------------------------

def test_n65_n64_n65_and_bdf_between_two_radau_solves_on_one_context_equal_fresh_contexts():
    p65, p64 = wide_problem(65, True), G.lin_problem(64, True)
    y64 = G.col(G.lin_y0s(64, 2))
    o_dense = Options(rtol=RT, atol=AT, dense_output=True, max_log=64)
    calls = (lambda c: Radau().solve_batch(p65, 0.0, dev(T65), dev(y65()), None, OPT, ctx=c),
             lambda c: Radau().solve_batch(p64, 0.0, 0.02, dev(y64), None, OPT, ctx=c),
             lambda c: Radau().solve_batch(p65, 0.0, dev(T65), dev(y65()), None, o_dense, ctx=c),
             lambda c: ivp_amd.solve_ivp_batch(p65, 0.0, dev(T65), dev(y65()), None, Options(method="BDF", rtol=RT, atol=AT), ctx=c),
             lambda c: Radau().solve_batch(p65, 0.0, dev(T65), dev(y65()), None, OPT, ctx=c))
    fresh = [call(ivp_amd.Context(0)) for call in calls]
    one = ivp_amd.Context(0)
    seq = [call(one) for call in calls]
    for q, (a, b) in enumerate(zip(seq, fresh)):
        for k in G.MEMBERS + ("y_end", "n_seg"):
            va, vb = getattr(a, k, None), getattr(b, k, None)
            assert (va is None) == (vb is None), (q, k)
            if va is not None:
                assert G._np(va).tobytes() == G._np(vb).tobytes(), (q, k)
    G.assert_rows(seq[0], models65(), "first solve of the sequence")
    G.assert_rows(seq[4], models65(), "last solve of the sequence")
    for b, m in enumerate(models65(dense_output=True)):
        assert int(seq[2].n_seg[b]) == len(m.segs)
        assert all(G.same_vec(seq[2].seg_cont[q, :, b], s[0]) for q, s in enumerate(m.segs)), b


# ---- 5. what stays refused ---------------------------------------------------------------------------------------------------

def _refused(prob, n, word, rad=None, **okw):
    with pytest.raises(ivp_amd.ConfigError) as e:
        (rad or Radau()).solve_batch(prob, 0.0, 1.0, np.ones((n, 1)), None, Options(rtol=RT, atol=AT, **okw))
    assert e.value.code == -100 and "not yet" in str(e.value) and word in str(e.value), str(e.value)


def test_the_built_ins_beyond_n_64_stay_refused():
    _refused(ivp_amd.LinearDecay100(), 100, "n = 100")
    with pytest.raises(ivp_amd.ConfigError) as e:
        Radau().solve_batch(ivp_amd.Heat1D256(), 0.0, 1.0, np.ones((256, 1)), np.ones((1, 1)), OPT)
    assert e.value.code == -100 and "not yet" in str(e.value) and "n = 256" in str(e.value) and "n <= 64" in str(e.value)


def test_patterns_banded_storage_fma_and_variant_3_stay_refused_at_n_65():
    n = 65
    src = ("__device__ double ode_comp(int i, double x, const double* y, const double* p) "
           "{ return (i > 0 ? y[i - 1] : 0.0) - 2.0 * y[i] + (i < 64 ? y[i + 1] : 0.0); }\n")
    pattern = np.array([[1 if abs(i - j) <= 1 else 0 for j in range(n)] for i in range(n)])
    _refused(ivp_amd.DeviceIVP(src, n, jac_sparsity=pattern), n, "jac_sparsity")
    _refused(ivp_amd.DeviceIVP(src, n, jac_sparsity=pattern, jac_storage="banded"), n, "IVP_RHS_BANDED")
    plain = ivp_amd.DeviceIVP(src, n)
    _refused(plain, n, "FMA", fp_mode=ivp_amd.FpMode.FMA)
    _refused(plain, n, "variant = 3", variant=3)


def test_event_functions_stay_refused_at_n_65():
    n = 65
    src = ("__device__ double ode_comp(int i, double x, const double* y, const double* p) { return -y[i]; }\n"
           "__device__ void events(double x, const double* y, double* g, const double* p) { g[0] = y[0] - 0.5; }\n")
    _refused(ivp_amd.DeviceIVP(src, n, events=[ivp_amd.EventConfig()]), n, "event functions")


def test_a_mass_hook_at_n_65_and_n_513_are_refused_when_the_problem_is_compiled():
    src = "__device__ double ode_comp(int i, double x, const double* y, const double* p) { return -y[i]; }\n"
    with pytest.raises(ValueError) as e:
        ivp_amd.DeviceIVP(src + "__device__ void mass_col(int col, double* column, const double* p) { column[col] = 1.0; }\n", 65, mass_col=True)
    assert "8 < n <= 64" in str(e.value)
    ctx = ivp_amd.default_context(0)
    h = C.c_void_p()
    rc = ctx.lib.ivp_rhs_compile_ex(ctx.handle, src.encode(), 65, 0, 0, ivp_amd.api.RHS_HAS_MASS_COL, C.byref(h))
    assert rc == -100 and "IVP_RHS_HAS_MASS_COL" in ctx.last_error() and "8 < n <= 64" in ctx.last_error()
    with pytest.raises(ivp_amd.ConfigError) as e:
        ivp_amd.DeviceIVP(src, 513)
    assert e.value.code == -100
