"""Radau IIA(5) for 8 < n <= 64 on the device (ivp_amd.Radau -> ivp_radau_solve*() -> radau_group.h: one group of G lanes per
trajectory, one row per lane, the three factors in LDS) against the CPU model tests/radau_model.py, BIT FOR BIT: status,
t_end, y_end, h_next and the six counters of every trajectory, and every recorded output.  No tolerance anywhere.

Widths: n = 9 (G = 16: seven idle lanes per group; B = 5 is four groups in one wavefront plus a wavefront with three absent
groups), n = 16 (a full group), n = 17 (G = 32), n = 33 and n = 64 (G = 64, partial and full).  The systems are
lin_matrix(n) of tests/test_gpu_radau.py at these widths -- y' = A y, a negative diagonal, 200 (2000 at n = 64, whose
diagonal reaches -16.75 and whose steps stay shorter) below the diagonal in every odd row, so that both factorisations
exchange rows -- in component form through hiprtc, with forward differences and with
jac_col.  Every test that names a branch asserts on the MODEL's counters or `cases` that the input takes it.  Model runs are
cached per input and shared between tests."""
import math

import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import Options, Radau
from tests import radau_model as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MEMBERS = ("status", "t_end", "h_next", "nfev", "njev", "nlu", "nstep", "naccpt", "nrejct")
RT, AT = 1e-6, 1e-8
OPT = Options(rtol=RT, atol=AT)
WIDTHS = (9, 16, 17, 33, 64)
T1 = 0.5


def t1_of(n):
    """end of the interval: the model takes about 1 s per n = 64 trajectory to t = 0.1"""
    return T1 if n <= 33 else 0.1

_CACHE = {}


def model(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def same(a, b):
    """bit equality of two floats, NaN equal to NaN"""
    a, b = float(a), float(b)
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def same_vec(a, b):
    return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))


def gpu_row(r, b):
    d = {k: (float(_np(getattr(r, k))[b]) if k in ("t_end", "h_next") else int(_np(getattr(r, k))[b])) for k in MEMBERS}
    d["y_end"] = [float(v) for v in _np(r.y_end)[:, b]]
    return d


def model_row(m):
    d = {k: getattr(m, k) for k in MEMBERS}
    d["y_end"] = list(m.y_end)
    return d


def assert_rows(r, models, what=""):
    bad = []
    for b, m in enumerate(models):
        g, w = gpu_row(r, b), model_row(m)
        ok = all(g[k] == w[k] for k in MEMBERS if k not in ("t_end", "h_next")) and same(g["t_end"], w["t_end"]) and \
            same(g["h_next"], w["h_next"]) and same_vec(g["y_end"], w["y_end"])
        if not ok:
            bad.append((b, g, w))
    assert not bad, f"{what}: {len(bad)} of {len(models)} trajectories differ from the model; first: {bad[0]}"


# ---- inputs -----------------------------------------------------------------------------------------------------------

def lin_matrix(n):
    """tests/test_gpu_radau.py's lin_matrix at width n (the coupling is 2000 at n = 64: see the module docstring)."""
    a = [[1e-3 * (1 + ((3 * i + 5 * j) % 7)) for j in range(n)] for i in range(n)]
    for i in range(n):
        a[i][i] = -1.0 - 0.25 * i
        if i % 2:
            a[i][i - 1] = 200.0 if n <= 33 else 2000.0
    return a


def lin_jac_source(n):
    return ("__device__ void jac_col(int col, double x, const double* y, double* column, const double* p) {\n"
            f"  for (int r = 0; r < {n}; ++r) column[r] = lin_a[r * {n} + col];\n}}\n")


def lin_source(a, with_jac):
    """y' = A y in component form, A fixed in the module, every row summed left to right (M.rhs_dense_linear)."""
    n = len(a)
    src = f"__device__ const double lin_a[{n * n}] = {{" + ", ".join(float(a[i][j]).hex() for i in range(n) for j in range(n)) + "};\n"
    src += ("__device__ double ode_comp(int i, double x, const double* y, const double* p) {\n"
            f"  double s = lin_a[i * {n}] * y[0];\n"
            f"  for (int j = 1; j < {n}; ++j) s = s + lin_a[i * {n} + j] * y[j];\n"
            "  return s;\n}\n")
    return src + (lin_jac_source(n) if with_jac else "")


def lin_problem(n, with_jac):
    return ivp_amd.DeviceIVP(lin_source(lin_matrix(n), with_jac), n, jac=with_jac)


def lin_y0s(n, B):
    """distinct initial states: the groups of one wavefront take different step counts"""
    base = [1.0, 0.5, -0.5, 0.25, 0.0, 1e-3, -1.0, 2.0]
    return [[base[i % 8] * (1.0 + 0.5 * b) + 1e-3 * (b + 1) * (i + 1) + (3.0 * b if i == 1 else 0.0) for i in range(n)] for b in range(B)]


def lin_models(n, y0s, with_jac, t0=0.0, t1=None, rtol=RT, atol=AT, **kw):
    a = lin_matrix(n)
    t1 = t1_of(n) if t1 is None else t1
    key = ("lin", n, with_jac, t0, t1, repr(rtol), repr(atol), tuple(sorted((k, repr(v)) for k, v in kw.items())))
    settings = kw.pop("settings_kw", None)
    if settings:
        kw["settings"] = M.Settings(**settings)
    return [model(key + (tuple(y0),), lambda y0=y0: M.solve(M.rhs_dense_linear(a), t0, t1, list(y0), rtol, atol,
                                                                jac=M.jac_dense_linear(a) if with_jac else None, **kw))
            for b, y0 in enumerate(y0s)]


def col(y0s):
    return np.array(y0s).T.copy()


# one problem, n = 9, whose Jacobian is a 2 x 2 block in the parameters beside a diagonal: the zero pivots, the imaginary
# multiplier and the NaN right-hand side below
BLOCK_SRC = ("__device__ double ode_comp(int i, double x, const double* y, const double* p) {\n"
             "  if (i == 0) return p[0] * y[0] + p[1] * y[1];\n"
             "  if (i == 1) return p[2] * y[0] + p[3] * y[1];\n"
             "  return p[4] * y[i];\n}\n"
             "__device__ void jac_col(int col, double x, const double* y, double* column, const double* p) {\n"
             "  if (col == 0) { column[0] = p[0]; column[1] = p[2]; }\n"
             "  else if (col == 1) { column[0] = p[1]; column[1] = p[3]; }\n"
             "  else column[col] = p[4];\n}\n")


def block_rhs(p):
    return lambda x, y: [p[0] * y[0] + p[1] * y[1], p[2] * y[0] + p[3] * y[1]] + [p[4] * y[i] for i in range(2, 9)]


def block_jac(p):
    def jac(x, y, J):
        J[0][0], J[0][1], J[1][0], J[1][1] = p[0], p[1], p[2], p[3]
        for i in range(2, 9):
            J[i][i] = p[4]
    return jac


# stiff Van der Pol in the first two components beside seven decays, n = 9, forward differences: the one NONLINEAR system
# here (the Newton iteration of a linear system converges in its first pass)
VDP9_SRC = ("__device__ double ode_comp(int i, double x, const double* y, const double* p) {\n"
            "  if (i == 0) return y[1];\n"
            "  if (i == 1) return ((1.0 - y[0] * y[0]) * y[1] - y[0]) / p[0];\n"
            "  return -y[i];\n}\n")


def vdp9_rhs(eps):
    return lambda x, y: [y[1], M.fdiv((1.0 - y[0] * y[0]) * y[1] - y[0], eps)] + [-y[i] for i in range(2, 9)]


def vdp9_inputs(B):
    eps = [1e-3 * (1.0 + 0.25 * b) for b in range(B)]
    y0s = [[2.0 + 0.01 * b, 0.0] + [1.0 + 0.1 * i for i in range(7)] for b in range(B)]
    return eps, y0s


def block_run(ps, y0s, t1, h, **okw):
    models = [M.solve(block_rhs(p), 0.0, t1, list(y0), RT, AT, jac=block_jac(p), first_step=h) for p, y0 in zip(ps, y0s)]
    prob = ivp_amd.DeviceIVP(BLOCK_SRC, 9, params=ps[0], jac=True)
    r = Radau().solve_batch(prob, 0.0, t1, col(y0s), np.array(ps).T.copy(), Options(rtol=RT, atol=AT, first_step=h, **okw))
    return models, r


# ---- 1. every width, forward differences and jac_col --------------------------------------------------------------------

@pytest.mark.parametrize("with_jac", [False, True])
@pytest.mark.parametrize("n", WIDTHS)
def test_every_group_width_with_forward_differences_and_with_jac_col(n, with_jac):
    B = 5 if n == 9 else (3 if n <= 17 else 2)
    y0s = lin_y0s(n, B)
    models = lin_models(n, y0s, with_jac)
    assert all(m.status == 0 and m.njev > 1 and m.n_reuse > 0 for m in models) and any(m.nrejct > 0 for m in models)
    assert all(any(p[0] == "real" for p in m.pivots) and any(p[0] == "complex" for p in m.pivots) for m in models)
    assert len({m.nstep for m in models}) > 1 or len({m.nfev for m in models}) > 1   # the groups of a wavefront diverge
    r = Radau().solve_batch(lin_problem(n, with_jac), 0.0, t1_of(n), col(y0s), None, OPT)
    assert_rows(r, models, f"n = {n}, jac_col = {with_jac}")


# ---- 2. chunk lengths: the LDS factors reloaded at launch boundaries ---------------------------------------------------

@pytest.mark.parametrize("chunk", [1, 7, 0])
def test_chunk_length_does_not_change_a_bit_at_n17(chunk):
    y0s = lin_y0s(17, 3)
    models = lin_models(17, y0s, False)
    assert all(m.n_reuse > 0 for m in models)   # accepted steps that keep the factors: with chunk = 1 they come from global memory
    r = Radau().solve_batch(lin_problem(17, False), 0.0, T1, torch.as_tensor(col(y0s), device=DEV), None,
                            Options(rtol=RT, atol=AT, chunk_attempts=chunk))
    assert_rows(r, models, f"chunk_attempts = {chunk}")


# ---- 3. backward integration -------------------------------------------------------------------------------------------

def test_backward_integration():
    y0s = lin_y0s(9, 2)
    models = lin_models(9, y0s, True, t0=0.25, t1=0.0)
    assert all(m.status == 0 and m.t_end == 0.0 and m.h_next < 0.0 for m in models)
    r = Radau().solve_batch(lin_problem(9, True), 0.25, 0.0, col(y0s), None, OPT)
    assert_rows(r, models, "backwards")


# ---- 4. outputs at n = 17 and n = 64 -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [17, 64])
def test_shared_t_eval_grid(n):
    y0s = lin_y0s(n, 2)
    t1 = t1_of(n)
    grid = [0.0, 0.2 * t1, 0.2 * t1 + 1e-13, 0.6 * t1, 0.9 * t1, t1, t1 + 0.5]   # t0, a pair closer than the tolerance, t1, a point outside
    models = lin_models(n, y0s, True, t_eval=grid)
    r = Radau().solve_batch(lin_problem(n, True), 0.0, t1, col(y0s), None, Options(rtol=RT, atol=AT, t_eval=grid))
    assert_rows(r, models, f"n = {n}, t_eval")
    for b, m in enumerate(models):
        k = int(r.n_filled[b])
        assert k == len(m.t) == 6 and list(r.eval_idx[:k, b]) == m.eval_idx
        for q in range(k):
            assert same_vec(r.y_eval[q, :, b], m.y[q]), (b, q)


@pytest.mark.parametrize("n", [17, 64])
def test_per_trajectory_ragged_t_eval_grids(n):
    B = 3 if n == 17 else 2
    y0s, t1 = lin_y0s(n, B), t1_of(n)
    grids = [np.linspace(0.0, t1, 3 + 2 * b) if b != 1 else np.zeros(0) for b in range(B)]
    models = [lin_models(n, [y0s[b]], True, t_eval=[float(v) for v in grids[b]])[0] for b in range(B)]
    r = Radau().solve_batch(lin_problem(n, True), 0.0, t1, col(y0s), None, Options(rtol=RT, atol=AT, t_eval_per_trajectory=grids))
    assert_rows(r, models, f"n = {n}, ragged t_eval")
    for b, m in enumerate(models):
        idx, y = r.eval_of(b)
        assert list(idx) == m.eval_idx and len(y) == len(m.y)
        for q in range(len(y)):
            assert same_vec(y[q], m.y[q]), (b, q)


@pytest.mark.parametrize("n", [17, 64])
def test_bounded_step_log_with_one_trajectory_that_overflows(n):
    y0s = lin_y0s(n, 2)
    t1s = np.array([t1_of(n), 0.05 * t1_of(n)])
    models = [lin_models(n, [y0s[b]], True, t1=float(t1s[b]))[0] for b in range(2)]
    ml = len(models[1].t) + 2
    assert len(models[0].t) > ml >= len(models[1].t)
    r = Radau().solve_batch(lin_problem(n, True), 0.0, t1s, col(y0s), None, Options(rtol=RT, atol=AT, max_log=ml))
    assert_rows(r, models, f"n = {n}, step log")
    for b, m in enumerate(models):
        assert int(r.n_log[b]) == len(m.t)                       # the count runs on past the capacity
        for q in range(min(ml, len(m.t))):
            assert same(r.t_log[q, b], m.t[q]) and same_vec(r.y_log[q, :, b], m.y[q]), (b, q)


def _find_segment(segs, t, extrapolate):
    """ContinuousOutput::find_segment / find_segment_extrapolate (cont.rs:104-153) on the model's segments"""
    tol = 1e-12
    for cont, xold, h in segs:
        lo, hi = min(xold, xold + h), max(xold, xold + h)
        if lo - tol <= t <= hi + tol:
            return (cont, xold, h), 1
    if extrapolate and segs:
        first, last = segs[0], segs[-1]
        if t < min(first[1], first[1] + first[2]):
            return first, 2
        if t > max(last[1], last[1] + last[2]):
            return last, 2
    return None, 0


@pytest.mark.parametrize("n", [17, 64])
def test_dense_output_segments_and_their_evaluation_on_the_device(n):
    B = 2
    y0s = lin_y0s(n, B)
    models = lin_models(n, y0s, True, dense_output=True)
    ml = max(len(m.segs) for m in models) + 1
    t1 = t1_of(n)
    r = Radau().solve_batch(lin_problem(n, True), 0.0, t1, col(y0s), None, Options(rtol=RT, atol=AT, dense_output=True, max_log=ml))
    assert_rows(r, models, f"n = {n}, dense output")
    for b, m in enumerate(models):
        assert int(r.n_seg[b]) == len(m.segs) == m.naccpt
        for q, (cont, xold, h) in enumerate(m.segs):
            assert same(r.seg_xold[q, b], xold) and same(r.seg_h[q, b], h) and same_vec(r.seg_cont[q, :, b], cont), (b, q)
    counts = np.array([int(v) for v in r.n_seg])
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    cont = np.concatenate([r.seg_cont[:counts[b], :, b] for b in range(B)])
    xold = np.concatenate([r.seg_xold[:counts[b], b] for b in range(B)])
    hh = np.concatenate([r.seg_h[:counts[b], b] for b in range(B)])
    ctx = ivp_amd.default_context(0)
    dense = ivp_amd.BatchContinuousOutput(ivp_amd.Method.RADAU, n, torch.as_tensor(off, device=DEV), torch.as_tensor(np.ascontiguousarray(cont), device=DEV),
                                          torch.as_tensor(xold, device=DEV), torch.as_tensor(hh, device=DEV), ivp_amd.FpMode.STRICT, ctx)
    grid = np.array([-0.25, 0.0, 1e-7, 0.3333 * t1, 0.5 * t1, t1, t1 + 0.125])   # before the span, inside, the ends, past the span
    for extrapolate in (False, True):
        y, found = dense(grid, extrapolate=extrapolate)
        y, found = _np(y), _np(found)
        for b, m in enumerate(models):
            for q, t in enumerate(grid):
                seg, kind = _find_segment(m.segs, float(t), extrapolate)
                assert int(found[q, b]) == kind, (b, q, extrapolate)
                if kind == 0:
                    assert np.isnan(y[q, :, b]).all()
                else:
                    assert same_vec(y[q, :, b], M.interpolate(float(t), *seg)), (b, q, extrapolate)


# ---- 5. the built-in 64-state problem ----------------------------------------------------------------------------------

def rhs_dense64(k):
    """RhsDense64 (rk_group.h) in the kernel's summation order: the diagonal term first, then j = 0 .. 63 without j == i"""
    a = [[float(((i * 5 + j * 3) & 15) - 8) * 0.00390625 for j in range(64)] for i in range(64)]   # in [-8, 7] / 256, exact
    d = [-k * (4.0 + float(i % 5)) for i in range(64)]

    def f(x, y):
        out = []
        for i in range(64):
            s = d[i] * y[i]
            ai = a[i]
            for j in range(64):
                if j != i:
                    s = s + ai[j] * y[j]
            out.append(s)
        return out
    return f


def test_built_in_dense64():
    ks = [1.0, 2.0]
    y0s = [[1.0 + 0.01 * i for i in range(64)], [math.cos(0.3 * i) for i in range(64)]]
    models = [model(("dense64", b), lambda b=b: M.solve(rhs_dense64(ks[b]), 0.0, 0.25, y0s[b], RT, AT)) for b in range(2)]
    assert all(m.status == 0 and m.naccpt > 5 for m in models) and models[0].nstep != models[1].nstep
    r = Radau().solve_batch(ivp_amd.Dense64(), 0.0, 0.25, col(y0s), np.array([ks]), OPT)
    assert_rows(r, models, "Dense64")
    s = Radau().solve(ivp_amd.Dense64(k=2.0), 0.0, 0.25, y0s[1], OPT)   # and one trajectory with its step log
    assert same_vec(s.t, models[1].t) and all(same_vec(a, b) for a, b in zip(s.y, models[1].y)) and len(s.y) == len(models[1].y)


# ---- 6. restarts -------------------------------------------------------------------------------------------------------

def test_newton_maxiter_1_is_status_singular_matrix_after_five_restarts():
    y0s = lin_y0s(17, 2)
    models = lin_models(17, y0s, True, settings_kw=dict(newton_maxiter=1))
    assert all(m.status == M.SINGULAR_MATRIX and m.n_restart == 5 and m.n_restart_newton == 6 and m.naccpt == 0 for m in models)
    for chunk in (0, 1):
        r = Radau(newton_maxiter=1).solve_batch(lin_problem(17, True), 0.0, T1, col(y0s), None, Options(rtol=RT, atol=AT, chunk_attempts=chunk))
        assert_rows(r, models, f"newton_maxiter = 1, chunk_attempts = {chunk}")
        assert all(int(v) == ivp_amd.Status.SingularMatrix == 5 for v in _np(r.status))


def test_newton_maxiter_2_restarts_across_launch_boundaries():
    """chunk_attempts = 1: h, reject, call_decomp and singular_count cross a launch boundary after every restart"""
    eps, y0s = vdp9_inputs(5)
    models = [model(("vdp9", 2, b), lambda b=b: M.solve(vdp9_rhs(eps[b]), 0.0, 0.5, y0s[b], RT, AT, settings=M.Settings(newton_maxiter=2))) for b in range(5)]
    assert all(m.n_restart_newton > 20 and m.naccpt > 0 and m.status == M.SUCCESS for m in models)
    prob = ivp_amd.DeviceIVP(VDP9_SRC, 9, params=[eps[0]])
    r = Radau(newton_maxiter=2).solve_batch(prob, 0.0, 0.5, col(y0s), np.array([eps]), Options(rtol=RT, atol=AT, chunk_attempts=1))
    assert_rows(r, models, "newton_maxiter = 2, chunk_attempts = 1")


def test_nonlinear_system_with_iteration_counts_that_differ_between_the_groups_of_a_wavefront():
    """Five stiff Van der Pol trajectories in the groups of two wavefronts: Newton iteration counts differ between the groups
    of a wavefront, steps are rejected, factors are reused."""
    eps, y0s = vdp9_inputs(5)
    models = [model(("vdp9", 7, b), lambda b=b: M.solve(vdp9_rhs(eps[b]), 0.0, 2.0, y0s[b], RT, AT)) for b in range(5)]
    assert all(m.status == M.SUCCESS and m.nrejct > 0 and m.n_reuse > 0 for m in models)
    assert len({tuple(m.newton_counts) for m in models[:4]}) > 1 and max(max(m.newton_counts) for m in models) > 1
    prob = ivp_amd.DeviceIVP(VDP9_SRC, 9, params=[eps[0]])
    r = Radau().solve_batch(prob, 0.0, 2.0, col(y0s), np.array([eps]), OPT)
    assert_rows(r, models, "stiff VdP at n = 9")


def test_real_zero_pivot_on_the_first_factorisation():
    """J = k I with k = U1 / h: E1 = (U1 / h) I - J is exactly zero, its first pivot fails; the restart halves h."""
    h = 0.01
    k = M.U1 / h
    ps = [[k, 0.0, 0.0, k, k]] * 2
    y0s = [[1.0] * 9, [0.5 + 0.1 * i for i in range(9)]]
    models, r = block_run(ps, y0s, 0.03, h)
    assert all(m.n_restart_real == 1 and m.n_restart == 1 and m.n_restart_complex == 0 and m.h_tried[0] == 0.5 * h for m in models)
    assert_rows(r, models, "real zero pivot")


def test_complex_zero_pivot_on_the_first_factorisation():
    """The rotation block [[a, -b], [b, a]], a = ALPH / h, b = BETA / h: E2 = [[i b, b], [-b, i b]] in the leading block,
    second pivot exactly zero."""
    h = 2.0 ** -6
    a, b = M.ALPH / h, M.BETA / h
    ps = [[a, -b, b, a, -1.0]] * 2
    y0s = [[1.0, 0.0] + [1.0] * 7, [0.3, -0.7] + [0.1 * i for i in range(7)]]
    models, r = block_run(ps, y0s, 4.0 * h, h)
    assert all(m.n_restart_complex == 1 and m.n_restart == 1 and m.n_restart_real == 0 and m.h_tried[0] == 0.5 * h for m in models)
    assert_rows(r, models, "complex zero pivot")


def test_purely_imaginary_multiplier_in_the_complex_elimination():
    h = 2.0 ** -10
    ps = [[0.0, 1.0, -1e5, M.ALPH / h, -1.0]] * 2
    y0s = [[1.0, 0.0] + [1.0] * 7, [0.5, 0.25] + [0.1 * i for i in range(7)]]
    models, r = block_run(ps, y0s, 8.0 * h, h)
    assert all("imag" in m.cases and ("complex", 0, 1) in m.pivots for m in models)
    assert_rows(r, models, "imaginary multiplier")


# ---- 7. failing and non-finite trajectories ----------------------------------------------------------------------------

def test_nan_right_hand_side_in_one_group_leaves_the_other_three_of_the_wavefront_untouched():
    ps = [[-2.0, 1.0, -1.0, -3.0, -1.0 - 0.5 * b] for b in range(4)]
    bad = 2
    ps[bad][4] = float("nan")   # rows 2..8 of that trajectory are NaN from the first call
    y0s = [[1.0 + 0.1 * b, 0.5] + [0.1 * (i + 1) for i in range(7)] for b in range(4)]
    models = [M.solve(block_rhs(p), 0.0, 0.5, list(y0), RT, AT, jac=block_jac(p)) for p, y0 in zip(ps, y0s)]
    assert models[bad].status != M.SUCCESS or any(v != v for v in models[bad].y_end)
    assert all(models[b].status == M.SUCCESS for b in range(4) if b != bad)
    prob = ivp_amd.DeviceIVP(BLOCK_SRC, 9, params=ps[0], jac=True)
    r = Radau().solve_batch(prob, 0.0, 0.5, col(y0s), np.array(ps).T.copy(), OPT)
    assert_rows(r, models, "NaN right-hand side in group 2 of 4")
    keep = [b for b in range(4) if b != bad]
    solo = Radau().solve_batch(prob, 0.0, 0.5, np.ascontiguousarray(col(y0s)[:, keep]), np.ascontiguousarray(np.array(ps).T[:, keep]), OPT)
    for k in MEMBERS + ("y_end",):
        assert _np(getattr(r, k))[..., keep].tobytes() == _np(getattr(solo, k)).tobytes(), k


def test_max_steps_gives_need_larger_nmax_with_the_models_step_count():
    y0s = lin_y0s(9, 5)
    models = lin_models(9, y0s, True, max_steps=10)
    assert all(m.status == M.NEED_LARGER_NMAX and m.nstep == 11 for m in models)
    r = Radau().solve_batch(lin_problem(9, True), 0.0, T1, col(y0s), None, Options(rtol=RT, atol=AT, max_steps=10))
    assert_rows(r, models, "max_steps = 10")


def test_vector_tolerances_and_the_same_vectors_reversed():
    n = 9
    rt = [10.0 ** -(4 + (i % 3)) for i in range(n)]
    at = [10.0 ** -(6 + (i % 4)) for i in range(n)]
    y0s = lin_y0s(n, 2)
    fwd = lin_models(n, y0s, True, rtol=rt, atol=at)
    rev = lin_models(n, y0s, True, rtol=rt[::-1], atol=at[::-1])
    assert all(a.status == b.status == M.SUCCESS and (a.nstep, a.nfev, a.y_end) != (b.nstep, b.nfev, b.y_end) for a, b in zip(fwd, rev))
    prob = lin_problem(n, True)
    assert_rows(Radau().solve_batch(prob, 0.0, T1, col(y0s), None, Options(rtol=rt, atol=at)), fwd, "vector tolerances")
    assert_rows(Radau().solve_batch(prob, 0.0, T1, col(y0s), None, Options(rtol=rt[::-1], atol=at[::-1])), rev, "vector tolerances reversed")


# ---- 8. what is still refused -------------------------------------------------------------------------------------------

def test_banded_storage_and_sparsity_patterns_are_refused_beyond_n_8():
    n = 9
    src = ("__device__ double ode_comp(int i, double x, const double* y, const double* p) "
           "{ return (i > 0 ? y[i - 1] : 0.0) - 2.0 * y[i] + (i < 8 ? y[i + 1] : 0.0); }\n")
    pattern = np.array([[1 if abs(i - j) <= 1 else 0 for j in range(n)] for i in range(n)])
    for kw, word in ((dict(jac_sparsity=pattern), "jac_sparsity"), (dict(jac_sparsity=pattern, jac_storage="banded"), "IVP_RHS_BANDED")):
        with pytest.raises(ivp_amd.ConfigError) as e:
            Radau().solve_batch(ivp_amd.DeviceIVP(src, n, **kw), 0.0, 1.0, np.ones((n, 1)), None, OPT)
        assert e.value.code == -100 and "not yet" in str(e.value) and word in str(e.value)
    with pytest.raises(ivp_amd.ConfigError) as e:
        Radau().solve_batch(ivp_amd.LinearDecay100(), 0.0, 1.0, np.ones((100, 1)), None, OPT)
    assert e.value.code == -100 and "not yet" in str(e.value) and "n = 100" in str(e.value)


# ---- 9. sequences on one context, and the front end ----------------------------------------------------------------------

def test_radau_n17_bdf_n17_radau_n3_radau_n17_on_one_context_equal_fresh_contexts():
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    y17 = col(lin_y0s(17, 3))
    p17 = lin_problem(17, True)
    y3 = np.array([[1.0], [0.0], [0.0]])
    o_end, o_dense = OPT, Options(rtol=RT, atol=AT, dense_output=True, max_log=200)
    calls = (lambda c: Radau().solve_batch(p17, 0.0, T1, dev(y17), None, o_end, ctx=c),
             lambda c: ivp_amd.solve_ivp_batch(p17, 0.0, T1, dev(y17[:, :2]), None, Options(method="BDF", rtol=RT, atol=AT), ctx=c),
             lambda c: Radau().solve_batch(ivp_amd.Robertson(), 0.0, 10.0, dev(y3), None, o_end, ctx=c),
             lambda c: Radau().solve_batch(p17, 0.0, T1, dev(y17), None, o_dense, ctx=c))
    fresh = [call(ivp_amd.Context(0)) for call in calls]
    one = ivp_amd.Context(0)
    seq = [call(one) for call in calls]
    for a, b in zip(seq, fresh):
        for k in MEMBERS + ("y_end", "n_seg", "seg_cont", "seg_xold", "seg_h"):
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
    assert_rows(seq[3], lin_models(17, lin_y0s(17, 3), True), "fourth solve of the sequence")


def test_scipy_front_end_solves_a_component_form_system_with_radau():
    n = 17
    y0 = lin_y0s(n, 1)[0]
    grid = np.linspace(0.0, T1, 5)
    res = ivp_amd.pyfront.solve_ivp(lin_source(lin_matrix(n), False), (0.0, T1), y0, method="Radau", rtol=RT, atol=AT, t_eval=grid, jac=lin_jac_source(n))
    m = lin_models(n, [y0], True, t_eval=[float(v) for v in grid])[0]
    assert res.success and res.status == 0 and (res.nfev, res.njev, res.nlu) == (m.nfev, m.njev, m.nlu)
    assert len(res.t) == len(m.t) == 5 and all(same_vec(np.asarray(res.y)[:, q], m.y[q]) for q in range(5))
