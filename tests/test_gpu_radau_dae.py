"""Radau IIA(5) for M y' = f(t, y) on the device -- ``DeviceIVP(..., mass=True)`` through ``ivp_amd.Radau`` /
ivp_radau_solve_dae* -- against the CPU model tests/radau_dae_model.py, BIT FOR BIT: y, t_end, h_next, status and all six
counters of every trajectory, and the samples / log records / dense segments where requested.  No tolerance anywhere.

The forcing terms are rational (t / (1 + t^2)), not sin / cos: the device's and the host's libm do not agree to the bit.
Every hiprtc module costs a second or two, so the file keeps to a handful of snippets."""
import math

import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import ConfigError, Options, Radau
from tests import radau_dae_model as D
from tests import radau_model as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MEMBERS = ("status", "t_end", "h_next", "nfev", "njev", "nlu", "nstep", "naccpt", "nrejct")
RT, AT = 1e-6, 1e-8
ODE = "__device__ void ode(double x, const double* y, double* d, const double* p)"
MASS = "__device__ void mass(double* m, const double* p)"


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def same(a, b):
    a, b = float(a), float(b)
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def same_vec(a, b):
    return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))


def assert_rows(r, models, what=""):
    bad = []
    for b, m in enumerate(models):
        g = {k: (float(_np(getattr(r, k))[b]) if k in ("t_end", "h_next") else int(_np(getattr(r, k))[b])) for k in MEMBERS}
        w = {k: getattr(m, k) for k in MEMBERS}
        ok = all(g[k] == w[k] for k in MEMBERS if k not in ("t_end", "h_next")) and same(g["t_end"], w["t_end"]) and \
            same(g["h_next"], w["h_next"]) and same_vec([float(v) for v in _np(r.y_end)[:, b]], m.y_end)
        if not ok:
            bad.append((b, g, [float(v) for v in _np(r.y_end)[:, b]], w, m.y_end))
    assert not bad, f"{what}: {len(bad)} of {len(models)} trajectories differ from the model; first: {bad[0]}"


def lit(v):
    return float(v).hex()


def flat(m):
    return [v for row in m for v in row]


# ---- the problems: device snippet and the model's right-hand side, the same operations in the same order --------------------
SCALAR_SRC = f"{ODE} {{ d[0] = p[1] / (1.0 + x * x) - y[0]; }}\n{MASS} {{ m[0] = p[0]; }}\n"


def f_scalar(p1):
    return lambda x, y: [M.fdiv(p1, 1.0 + x * x) - y[0]]


SEMI_SRC = (f"{ODE} {{ d[0] = -y[0] + y[1]; d[1] = y[1] - x / (1.0 + x * x); }}\n"
            f"{MASS} {{ m[0] = p[0]; m[1] = p[1]; m[2] = p[2]; m[3] = p[3]; }}\n")


def f_semi(x, y):
    return [-y[0] + y[1], y[1] - M.fdiv(x, 1.0 + x * x)]


SEMI = [[1.0, 0.0], [0.0, 0.0]]
DENSE2 = [[2.0, 1.0], [1.0, 2.0]]

ROB_SRC = (f"{ODE} {{ const double xx = y[0], yy = y[1], zz = y[2];\n"
           "  d[0] = -0.04 * xx + 1e4 * yy * zz; d[1] = 0.04 * xx - 1e4 * yy * zz - 3e7 * yy * yy; d[2] = xx + yy + zz - 1.0; }\n"
           f"{MASS} {{ m[0] = 1.0; m[4] = 1.0; }}\n")   # the zeros are the storage's


def pend_src(constraint):
    return (f"{ODE} {{ const double p1 = y[0], p2 = y[1], v1 = y[2], v2 = y[3], lam = y[4];\n"
            f"  d[0] = v1; d[1] = v2; d[2] = -lam * p1; d[3] = -lam * p2 - 1.0; d[4] = {constraint}; }}\n"
            f"{MASS} {{ m[0] = 1.0; m[6] = 1.0; m[12] = 1.0; m[18] = 1.0; }}\n")


PEND2_SRC = pend_src("p1 * v1 + p2 * v2")
PEND3_SRC = pend_src("p1 * p1 + p2 * p2 - 1.0")
# p[0] selects the last equation per trajectory: the index-2 constraint p.v = 0, or lam = |v|^2 - p2 (the constraint
# differentiated once more and solved for lam: index 1)
PENDSEL_SRC = pend_src("p[0] != 0.0 ? p1 * v1 + p2 * v2 : lam - (v1 * v1 + v2 * v2 - p2)")


def f_pend_index1(x, s):
    p1, p2, v1, v2, lam = s
    return [v1, v2, -lam * p1, -lam * p2 - 1.0, lam - (v1 * v1 + v2 * v2 - p2)]


def pend_y0(phi):
    """at rest at angle phi: lam = -sin phi balances gravity along the rod"""
    return [math.cos(phi), math.sin(phi), 0.0, 0.0, 0.0 - math.sin(phi)]


def lin_matrix(n):
    """tests/test_gpu_radau.py's dense test matrix"""
    a = [[1e-3 * (1 + ((3 * i + 5 * j) % 7)) for j in range(n)] for i in range(n)]
    for i in range(n):
        a[i][i] = -1.0 - 0.25 * i
        if i % 2:
            a[i][i - 1] = 200.0
    return a


def full_mass(n):
    return [[(1.0 + 0.125 * r) if r == c else (0.01 * (1 + (r + 2 * c) % 5)) * (-1.0 if (r + c) % 3 == 0 else 1.0) for c in range(n)]
            for r in range(n)]


def lin_mass_source(a, ms):
    n = len(a)
    src = ODE + " {\n"
    for i in range(n):
        src += f"  d[{i}] = " + " + ".join(f"{lit(a[i][j])} * y[{j}]" for j in range(n)) + ";\n"
    src += "}\n" + MASS + " {\n" + "".join(f"  m[{r * n + c}] = {lit(ms[r][c])};\n" for r in range(n) for c in range(n)) + "}\n"
    return src


VDP_SRC = f"{ODE} {{ d[0] = y[1]; d[1] = ((1.0 - y[0] * y[0]) * y[1] - y[0]) / p[0]; }}\n"
VDP_IDENT_SRC = VDP_SRC + f"{MASS} {{ m[0] = 1.0; m[3] = 1.0; }}\n"


def models_of(fs, masses, y0s, t0, t1, rtol=RT, atol=AT, nind=(None, None, None), **kw):
    return [D.solve(f, t0, t1, list(y0), rtol, atol, mass=ms, nind1=nind[0], nind2=nind[1], nind3=nind[2], **kw) for f, ms, y0 in zip(fs, masses, y0s)]


def cols(rows):
    return np.array(rows, dtype=np.float64).T.copy()


# ---- n = 1 --------------------------------------------------------------------------------------------------------------------
def test_n1_algebraic_equation_batch_of_1():
    prob = ivp_amd.DeviceIVP(SCALAR_SRC, 1, params=(0.0, 1.0), mass=True)
    ms = models_of([f_scalar(1.0)], [[[0.0]]], [[1.0]], 0.0, 2.0)
    r = Radau().solve_batch(prob, 0.0, 2.0, cols([[1.0]]), cols([[0.0, 1.0]]), Options(rtol=RT, atol=AT))
    assert ms[0].status == M.SUCCESS
    assert_rows(r, ms, "M = [0]")


@pytest.mark.parametrize("chunk", [0, 1])
def test_n1_a_mass_per_trajectory_65_trajectories(chunk):
    """65 trajectories: the batch is one trajectory longer than a wavefront is wide, but at this size the device runs one
    trajectory per wavefront (lpw = ceil(65 / cus) = 1); tests/test_gpu_wave_density.py (dae_n1_mass_per_trajectory) runs it
    with full wavefronts.  chunk_attempts = 1 puts a launch boundary after every attempt"""
    p0 = [0.0 if b % 13 == 0 else 0.25 + 0.125 * b for b in range(65)]
    p1 = [1.0 + 0.01 * b for b in range(65)]
    ms = models_of([f_scalar(v) for v in p1], [[[v]] for v in p0], [[1.0]] * 65, 0.0, 2.0)
    prob = ivp_amd.DeviceIVP(SCALAR_SRC, 1, params=(0.0, 1.0), mass=True)
    y0 = torch.ones((1, 65), dtype=torch.float64, device=DEV)
    par = torch.as_tensor(cols([[a, b] for a, b in zip(p0, p1)]), device=DEV)
    r = Radau().solve_batch(prob, 0.0, 2.0, y0, par, Options(rtol=RT, atol=AT, chunk_attempts=chunk))
    assert all(m.status == M.SUCCESS for m in ms)
    assert_rows(r, ms, f"M = [p0], chunk_attempts = {chunk}")


# ---- n = 2 --------------------------------------------------------------------------------------------------------------------
def test_n2_semi_explicit_and_dense_mass_with_dense_segments_evaluated_on_the_device():
    y0s = [[0.0, 0.0], [1.0, -0.5]]
    ms = models_of([f_semi, f_semi], [SEMI, DENSE2], y0s, 0.0, 2.0, dense_output=True)
    prob = ivp_amd.DeviceIVP(SEMI_SRC, 2, params=flat(SEMI), mass=True)
    ml = max(len(m.segs) for m in ms) + 1
    r = Radau().solve_batch(prob, 0.0, 2.0, cols(y0s), cols([flat(SEMI), flat(DENSE2)]), Options(rtol=RT, atol=AT, dense_output=True, max_log=ml))
    assert_rows(r, ms, "semi-explicit / dense M")
    for b, m in enumerate(ms):
        assert int(r.n_seg[b]) == len(m.segs) == m.naccpt
        for q, (cont, xold, h) in enumerate(m.segs):
            assert same(r.seg_xold[q, b], xold) and same(r.seg_h[q, b], h) and same_vec(r.seg_cont[q, :, b], cont), (b, q)
    counts = np.array([int(v) for v in r.n_seg])
    off = np.zeros(3, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    cont = np.concatenate([r.seg_cont[:counts[b], :, b] for b in range(2)])
    xold = np.concatenate([r.seg_xold[:counts[b], b] for b in range(2)])
    hh = np.concatenate([r.seg_h[:counts[b], b] for b in range(2)])
    dense = ivp_amd.BatchContinuousOutput(ivp_amd.Method.RADAU, 2, torch.as_tensor(off, device=DEV), torch.as_tensor(np.ascontiguousarray(cont), device=DEV),
                                          torch.as_tensor(xold, device=DEV), torch.as_tensor(hh, device=DEV), ivp_amd.FpMode.STRICT, ivp_amd.default_context(0))
    grid = np.array([0.0, 1e-7, 0.3333, 1.0, 2.0])
    y, found = dense(grid, extrapolate=False)
    y, found = _np(y), _np(found)
    for b, m in enumerate(ms):
        for q, t in enumerate(grid):
            seg = next(s for s in m.segs if min(s[1], s[1] + s[2]) - 1e-12 <= t <= max(s[1], s[1] + s[2]) + 1e-12)
            assert int(found[q, b]) == 1 and same_vec(y[q, :, b], M.interpolate(float(t), *seg)), (b, q)


def test_n2_backward_with_a_shared_t_eval_grid():
    y0s = [[0.3, 0.4], [1.0, -0.5]]
    grid = [2.0, 1.5, 1.0, 0.25, 0.0]
    ms = models_of([f_semi, f_semi], [SEMI, DENSE2], y0s, 2.0, 0.0, t_eval=grid)
    prob = ivp_amd.DeviceIVP(SEMI_SRC, 2, params=flat(SEMI), mass=True)
    r = Radau().solve_batch(prob, 2.0, 0.0, cols(y0s), cols([flat(SEMI), flat(DENSE2)]), Options(rtol=RT, atol=AT, t_eval=grid))
    assert_rows(r, ms, "backward")
    for b, m in enumerate(ms):
        k = int(r.n_filled[b])
        assert k == len(m.t) == len(grid) and list(r.eval_idx[:k, b]) == m.eval_idx
        for q in range(k):
            assert same_vec(r.y_eval[q, :, b], m.y[q]), (b, q)


# ---- n = 3 --------------------------------------------------------------------------------------------------------------------
def test_n3_robertson_as_an_index_1_dae_with_per_component_tolerances():
    rt, at = [1e-6, 1e-5, 1e-6], [1e-10, 1e-12, 1e-9]
    ms = models_of([D.rhs_robertson_dae], [D.MASS_ROBERTSON], [[1.0, 0.0, 0.0]], 0.0, 40.0, rtol=rt, atol=at)
    prob = ivp_amd.DeviceIVP(ROB_SRC, 3, mass=True)
    r = Radau().solve_batch(prob, 0.0, 40.0, cols([[1.0, 0.0, 0.0]]), None, Options(rtol=rt, atol=at))
    assert ms[0].status == M.SUCCESS and ms[0].nrejct > 0
    assert_rows(r, ms, "Robertson DAE")
    s = Radau().solve(prob, 0.0, 40.0, [1.0, 0.0, 0.0], Options(rtol=rt, atol=at))   # the single-trajectory front end
    assert same_vec(s.y[-1], ms[0].y_end) and len(s.t) == len(ms[0].t)


# ---- n = 5: the index sets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 1])
def test_n5_pendulum_index_2_with_a_bounded_log(chunk):
    """tolerance 1e-4: rejections and Newton dyth exits, whose hhfac and accumulated scal divisions cross launch boundaries"""
    y0s = [pend_y0(0.0), pend_y0(0.6435011087932844)]
    ms = models_of([D.rhs_pendulum_index2] * 2, [D.MASS_PENDULUM] * 2, y0s, 0.0, 2.0, rtol=1e-4, atol=1e-4, nind=(4, 1, 0))
    assert ms[0].n_dyth >= 5 and ms[0].nrejct - ms[0].n_dyth >= 5 and all(m.status == M.SUCCESS for m in ms)
    prob = ivp_amd.DeviceIVP(PEND2_SRC, 5, mass=True)
    r = Radau(nind1=4, nind2=1, nind3=0).solve_batch(prob, 0.0, 2.0, cols(y0s), None, Options(rtol=1e-4, atol=1e-4, max_log=16, chunk_attempts=chunk))
    assert_rows(r, ms, "pendulum, index 2")
    for b, m in enumerate(ms):
        assert int(r.n_log[b]) == len(m.t)
        for q in range(min(16, len(m.t))):
            assert same(r.t_log[q, b], m.t[q]) and same_vec(r.y_log[q, :, b], m.y[q]), (b, q)


@pytest.mark.parametrize("tol", [1e-4, 1e-6])
def test_n5_pendulum_index_3(tol):
    """tolerance 1e-4 takes an `h *= 0.5` restart: hhfac = 0.5 is squared into the scale of lam"""
    ms = models_of([D.rhs_pendulum_index3], [D.MASS_PENDULUM], [pend_y0(0.0)], 0.0, 2.0, rtol=tol, atol=tol, nind=(2, 2, 1), first_step=1e-3)
    assert ms[0].status == M.SUCCESS and (ms[0].n_restart == 1 if tol == 1e-4 else ms[0].naccpt == 34)
    prob = ivp_amd.DeviceIVP(PEND3_SRC, 5, mass=True)
    r = Radau(nind2=2, nind3=1).solve_batch(prob, 0.0, 2.0, cols([pend_y0(0.0)]), None, Options(rtol=tol, atol=tol, first_step=1e-3))
    assert_rows(r, ms, f"pendulum, index 3, tolerance {tol}")


def test_half_the_batch_has_the_wrong_partition_and_its_neighbours_are_untouched():
    """One call, the pure-ODE partition (5, 0, 0): right for the trajectories whose last equation is the index-1 form, wrong for
    those with the index-2 constraint, which end in StepSizeTooSmall.  The six are neighbours in the batch; on the device each
    has a wavefront to itself (lpw = 1 at this batch size).  tests/test_gpu_wave_density.py (dae_n5_wrong_partition)
    alternates the two kinds inside one wavefront."""
    sel = [0.0, 1.0, 0.0, 1.0, 1.0, 0.0]
    y0s = [pend_y0(0.1 * b) for b in range(6)]
    fs = [D.rhs_pendulum_index2 if s else f_pend_index1 for s in sel]
    ms = models_of(fs, [D.MASS_PENDULUM] * 6, y0s, 0.0, 2.0, rtol=1e-6, atol=1e-6, nind=(5, 0, 0))
    assert [m.status for m in ms] == [M.STEP_TOO_SMALL if s else M.SUCCESS for s in sel]
    prob = ivp_amd.DeviceIVP(PENDSEL_SRC, 5, params=(0.0,), mass=True)
    r = Radau(nind1=5, nind2=0, nind3=0).solve_batch(prob, 0.0, 2.0, cols(y0s), cols([[s] for s in sel]), Options(rtol=1e-6, atol=1e-6))
    assert_rows(r, ms, "mixed index-1 / index-2")


# ---- n = 8 --------------------------------------------------------------------------------------------------------------------
def test_n8_dense_linear_system_with_a_full_mass_matrix():
    a, mm = lin_matrix(8), full_mass(8)
    y0s = [[1.0 + 0.25 * i for i in range(8)], [(-1.0) ** i * (0.5 + 0.125 * i) for i in range(8)]]
    ms = models_of([M.rhs_dense_linear(a)] * 2, [mm] * 2, y0s, 0.0, 1.5)
    assert all(m.status == M.SUCCESS for m in ms) and ms[0].pivots
    prob = ivp_amd.DeviceIVP(lin_mass_source(a, mm), 8, mass=True)
    r = Radau().solve_batch(prob, 0.0, 1.5, cols(y0s), None, Options(rtol=RT, atol=AT))
    assert_rows(r, ms, "M y' = A y, n = 8")


# ---- the identity, and one context serving both kinds of problem ------------------------------------------------------------------
def test_identity_mass_equals_the_plain_radau_call_and_one_context_alternates():
    eps = [1e-3, 7e-4, 1.5e-3]
    y0 = cols([[2.0, 0.0], [1.9, 0.1], [2.1, -0.1]])
    par = cols([[e] for e in eps])
    plain = ivp_amd.DeviceIVP(VDP_SRC, 2, params=(1e-3,))
    ident = ivp_amd.DeviceIVP(VDP_IDENT_SRC, 2, params=(1e-3,), mass=True)
    opt = Options(rtol=RT, atol=AT)
    runs = [Radau().solve_batch(f, 0.0, 2.0, y0, par, opt) for f in (ident, plain, ident, plain)]   # buffer sizes 5 n n, 4 n n, 5 n n, ...
    ms = [M.solve(M.rhs_vdp_eps(e), 0.0, 2.0, [float(v) for v in y0[:, b]], RT, AT) for b, e in enumerate(eps)]
    for r in runs:
        assert_rows(r, ms, "identity mass / no mass")


# ---- refusals that need a context ---------------------------------------------------------------------------------------------------
def test_a_problem_with_a_mass_matrix_is_refused_everywhere_else():
    prob = ivp_amd.DeviceIVP(SCALAR_SRC, 1, params=(2.0, 1.0), mass=True)
    y0, par = cols([[1.0]]), cols([[2.0, 1.0]])
    for method in ("DOPRI5", "BDF", "RK4"):
        with pytest.raises(ConfigError) as e:
            ivp_amd.solve_ivp_batch(prob, 0.0, 1.0, y0, par, Options(method=method, first_step=0.1))
        assert e.value.code == -100 and "mass matrix" in str(e.value) and "Radau DAE call only" in str(e.value)
    with pytest.raises(ConfigError) as e:
        ivp_amd.solve_ivp_batch_logged(prob, 0.0, 1.0, y0, par, Options())
    assert e.value.code == -100 and "mass matrix" in str(e.value)
    with pytest.raises(ConfigError) as e:
        ivp_amd.solve_ivp_batch_dense(prob, 0.0, 1.0, y0, par, Options())
    assert e.value.code == -100 and "mass matrix" in str(e.value)
    # ivp_radau_solve* without the DAE argument, and the two checks
    import ctypes as C
    from ivp_amd import _lib
    lib, ctx = _lib.load(), ivp_amd.default_context(0)
    p = _lib.ProblemT()
    p.rhs_id, p.n, p.n_params, p.jit = 1000, 1, 2, prob.handle
    o = _lib.OptionsT()
    lib.ivp_options_default(C.byref(o))
    msg = C.create_string_buffer(256)
    assert lib.ivp_options_check(C.byref(p), 1, C.byref(o), msg, 256) == -100 and b"mass matrix" in msg.value
    assert lib.ivp_radau_check(C.byref(p), 1, C.byref(o), None, msg, 256) == -100 and b"mass matrix" in msg.value
    assert lib.ivp_radau_dae_check(C.byref(p), 1, C.byref(o), None, None, msg, 256) == 0
    d = _lib.RadauDaeT()
    d.has_nind2, d.nind2 = 1, 1
    assert lib.ivp_radau_dae_check(C.byref(p), 1, C.byref(o), None, C.byref(d), msg, 256) == 0   # with the hook, index sets pass
    d.nind2 = 2
    assert lib.ivp_radau_dae_check(C.byref(p), 1, C.byref(o), None, C.byref(d), msg, 256) == -7
    r = _lib.BatchResultT()
    rc = lib.ivp_radau_solve(ctx.handle, C.byref(p), 1, y0.ctypes.data, par.ctypes.data, y0.ctypes.data, 1, y0.ctypes.data, 1, C.byref(o), None, C.byref(r))
    assert rc == -100 and "Radau DAE call only" in ctx.last_error()
    # the remaining entry points, one call each: all of them validate before they read a data pointer
    yd, pd = torch.as_tensor(y0, device=DEV), torch.as_tensor(par, device=DEV)
    td = torch.zeros(1, dtype=torch.float64, device=DEV)
    args = (ctx.handle, C.byref(p), 1, yd.data_ptr(), pd.data_ptr(), td.data_ptr(), 1, td.data_ptr(), 1, C.byref(o))
    for call in (lambda: lib.ivp_batch_submit_device(*args, C.byref(r), None),
                 lambda: lib.ivp_batch_solve_device(*args, C.byref(r), None),
                 lambda: lib.ivp_radau_solve_device(*args, None, C.byref(r), None)):
        assert call() == -100 and "Radau DAE call only" in ctx.last_error()
    off = torch.zeros(2, dtype=torch.int64, device=DEV)
    ev = _lib.EventLogT()
    ev.offsets = off.data_ptr()
    assert lib.ivp_batch_solve_events_device(*args, C.byref(r), C.byref(ev), None) == -100 and "Radau DAE call only" in ctx.last_error()
    sh = _lib.ShardT()
    sh.ctx, sh.first, sh.count = ctx.handle, 0, 1
    sh.y0, sh.params, sh.t0, sh.t0_len, sh.t1, sh.t1_len = yd.data_ptr(), pd.data_ptr(), td.data_ptr(), 1, td.data_ptr(), 1
    assert lib.ivp_batch_solve_multi(C.byref(sh), 1, C.byref(p), 1, C.byref(o), 0, None) == -100 and "Radau DAE call only" in ctx.last_error()
    ctxs = (C.c_void_p * 1)(ctx.handle)
    rc = lib.ivp_batch_solve_multi_host(ctxs, 1, C.byref(p), 1, y0.ctypes.data, par.ctypes.data, y0.ctypes.data, 1, y0.ctypes.data, 1, C.byref(o), C.byref(r))
    assert rc == -100 and "Radau DAE call only" in ctx.last_error()


def test_compile_time_refusals():
    from ivp_amd import _lib
    import ctypes as C
    lib, ctx = _lib.load(), ivp_amd.default_context(0)
    h = C.c_void_p()
    big = "__device__ double ode_comp(int i, double x, const double* y, const double* p) { return -y[i]; }\n" + MASS + " { }\n"
    assert lib.ivp_rhs_compile_ex(ctx.handle, big.encode(), 9, 0, 0, 4, C.byref(h)) == -100 and "n <= 8" in ctx.last_error()
    assert lib.ivp_rhs_compile_ex(ctx.handle, SCALAR_SRC.encode(), 1, 2, 0, 4 | 2, C.byref(h)) == -100   # IVP_RHS_BANDED is ivp_rhs_compile_sparse's
    assert lib.ivp_rhs_compile_ex(ctx.handle, SCALAR_SRC.encode(), 1, 2, 0, 8, C.byref(h)) == -100 and "unknown flags" in ctx.last_error()
    col_ptr = (C.c_int32 * 11)(*range(11))
    row_idx = (C.c_int32 * 10)(*range(10))
    assert lib.ivp_rhs_compile_sparse(ctx.handle, big.encode(), 10, 0, 0, 4 | 2, col_ptr, row_idx, C.byref(h)) == -100
    assert lib.ivp_rhs_compile_sparse(ctx.handle, big.encode(), 10, 0, 0, 4, col_ptr, row_idx, C.byref(h)) == -100 and "unknown flags" in ctx.last_error()
    # a mass() of the wrong shape surfaces when the problem is compiled: the Radau module is the one built eagerly
    bad = ODE + " { d[0] = -y[0]; }\n__device__ void mass(double* m) { m[0] = 1.0; }\n"
    assert lib.ivp_rhs_compile_ex(ctx.handle, bad.encode(), 1, 0, 0, 4, C.byref(h)) == -104
    with pytest.raises(ValueError):
        ivp_amd.DeviceIVP(SCALAR_SRC, 1, params=(0.0, 1.0), jac_sparsity=([0, 1], [0]), mass=True)
    with pytest.raises(ValueError):
        ivp_amd.DeviceIVP(big, 9, mass=True)
    with pytest.raises(ValueError):
        ivp_amd.DeviceIVP(big, 10, jac_sparsity=(np.arange(11, dtype=np.int32), np.arange(10, dtype=np.int32)), jac_storage="banded", mass=True)
    # index-2 variables for a problem without the hook: "not yet"; a bad partition: code -7
    plain = ivp_amd.DeviceIVP(VDP_SRC, 2, params=(1e-3,))
    y0, par = cols([[2.0, 0.0]]), cols([[1e-3]])
    with pytest.raises(ConfigError) as e:
        Radau(nind2=1).solve_batch(plain, 0.0, 1.0, y0, par, Options())
    assert e.value.code == -100 and "not yet" in str(e.value)
    with pytest.raises(ConfigError) as e:
        Radau(nind1=1).solve_batch(plain, 0.0, 1.0, y0, par, Options())
    assert e.value.code == -7
