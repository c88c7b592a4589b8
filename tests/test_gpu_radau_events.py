"""Radau IIA(5) with event functions on the device (ivp_amd.Radau.solve_batch_events -> ivp_radau_solve_events_device)
against the CPU model tests/radau_events_model.py, BIT FOR BIT: the CSR offsets, every event time and state, n_event_hits,
the end state, status and every counter of every trajectory, and the outputs delivered alongside.  No tolerance anywhere.

Thread form (n <= 8): the built-in SHO with a zero-crossing event and the bouncing ball (terminal) at B = 70 -- one full
wavefront plus six lanes -- and hiprtc problems at n = 3 (Robertson, analytic jac, a threshold on y[1]), n = 8 (a dense
linear system, two events on different components) and n = 5 with a mass matrix (the index-2 pendulum, an event on the
angle), each at chunk lengths 1, 7 and unbounded.  Group form (8 < n <= 64): n = 9 (G = 16, B = 5: a wavefront of four
groups plus one of one), n = 17 (G = 32, B = 3), n = 64 (G = 64, B = 2), forward differences and jac_col, one event on
component 0 and one on the component the last active lane owns; and a wavefront in which one group retires on a terminal
event while its wave-mates integrate on (every trajectory is compared with the model, which integrates it alone).
Model runs are cached per input and shared between tests."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import Direction, EventConfig, Options, Radau, _lib, api
from tests import radau_dae_model as DM, radau_events_model as EM, radau_model as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MEMBERS = ("status", "t_end", "h_next", "nfev", "njev", "nlu", "nstep", "naccpt", "nrejct")
RT, AT = 1e-6, 1e-8
CHUNKS = [1, 7, 1 << 30]   # attempts per launch: every boundary between two attempts, some, none
_CACHE = {}


def model(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def cfg_of(c):
    return EM.EventConfig(int(c.direction), c.terminal_count)


def assert_batch(r, models, what=""):
    """end state, status, counters, hit counts and the whole CSR event log of every trajectory against its model"""
    B, nev = len(models), len(models[0].t_events)
    off = _np(r.event_offsets)
    assert off.shape == (nev * B + 1,) and off[0] == 0 and int(off[-1]) == int(r.t_events_csr.shape[0]) == r.event_info["total"]
    hits = _np(r.n_event_hits)
    tcsr, ycsr = _np(r.t_events_csr), _np(r.y_events_csr)
    for b, m in enumerate(models):
        for k in MEMBERS:
            g, w = _np(getattr(r, k))[b], getattr(m, k)
            assert (bits(g) == bits(w)).all() if k in ("t_end", "h_next") else int(g) == w, (what, b, k, g, w)
        assert (bits(_np(r.y_end)[:, b]) == bits(m.y_end)).all(), (what, b, "y_end")
        for i in range(nev):
            lo, hi = int(off[i * B + b]), int(off[i * B + b + 1])
            assert hi - lo == len(m.t_events[i]) == int(hits[i, b]), (what, b, i, hi - lo, len(m.t_events[i]), int(hits[i, b]))
            assert (bits(tcsr[lo:hi]) == bits(m.t_events[i])).all(), (what, b, i, "t_events")
            if hi > lo:
                assert (bits(ycsr[lo:hi]) == bits(m.y_events[i])).all(), (what, b, i, "y_events")


def solve(f, t0, t1, y0s, params=None, opt=None, rad=None, ctx=None):
    y0 = torch.as_tensor(np.array(y0s, dtype=np.float64).T.copy(), device=DEV)
    p = None if params is None else torch.as_tensor(np.array(params, dtype=np.float64).T.copy(), device=DEV)
    return (rad or Radau()).solve_batch_events(f, t0, t1, y0, p, opt or Options(rtol=RT, atol=AT), ctx)


# ---- thread form: the built-ins ----------------------------------------------------------------------------------------

def sho_y0s(B):
    return [[math.cos(0.09 * b) * (1.0 + 0.01 * b), -math.sin(0.09 * b)] for b in range(B)]


def sho_models(y0s, t1, cfg, **kw):
    return [model(("sho", tuple(y0), t1, cfg.direction, cfg.terminal_count, tuple(sorted((k, repr(v)) for k, v in kw.items()))),
                  lambda y0=y0: EM.solve(M.rhs_sho, lambda x, y: [y[0]], [cfg], 0.0, t1, y0, RT, AT, **kw)) for y0 in y0s]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_builtin_sho_zero_crossings_b70(chunk):
    y0s = sho_y0s(70)
    r = solve(ivp_amd.SHOZeroEvent(), 0.0, 10.0, y0s, opt=Options(rtol=RT, atol=AT, chunk_attempts=chunk, max_events=8))
    ms = sho_models(y0s, 10.0, EM.EventConfig())
    assert min(sum(m.n_event_hits) for m in ms) >= 3 and r.event_info["passes"] == 1
    assert_batch(r, ms, "sho")


def ball_rhs(g, drag):
    return lambda x, s: [s[1], -g - (drag * s[1]) * abs(s[1])]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_builtin_bouncing_ball_terminal_b70(chunk):
    B = 70
    y0s = [[0.2 + 0.05 * b, 1.0 if b % 3 == 0 else 0.0] for b in range(B)]
    par = [[9.81, 0.02 + 0.001 * (b % 5)] for b in range(B)]
    f = ivp_amd.BouncingBall()
    r = solve(f, 0.0, 0.6, y0s, par, Options(rtol=RT, atol=AT, chunk_attempts=chunk, max_log=200))
    cfg = cfg_of(f.event_config(0))
    ms = [model(("ball", b), lambda b=b: EM.solve(ball_rhs(*par[b]), lambda x, y: [y[0]], [cfg], 0.0, 0.6, y0s[b], RT, AT)) for b in range(B)]
    landed = [m.status == M.INTERRUPT for m in ms]
    assert any(landed) and not all(landed)   # the low ones land before t1 (terminal), the high ones are still falling
    assert_batch(r, ms, "ball")
    nlog, tl, yl = _np(r.n_log), _np(r.t_log), _np(r.y_log)
    for b, m in enumerate(ms):   # the bounded step log, with the terminal point appended
        assert int(nlog[b]) == len(m.t) and (bits(tl[:len(m.t), b]) == bits(m.t)).all() and (bits(yl[:len(m.t), :, b]) == bits(m.y)).all()


# ---- thread form: hiprtc -----------------------------------------------------------------------------------------------

ROB_SRC = """
__device__ void ode(double t, const double* s, double* d, const double* p) {
  const double xx = s[0], y = s[1], z = s[2];
  d[0] = -0.04 * xx + 1e4 * y * z;
  d[1] = 0.04 * xx - 1e4 * y * z - 3e7 * y * y;
  d[2] = 3e7 * y * y;
}
__device__ void jac(double t, const double* s, double* j, const double* p) {
  const double y = s[1], z = s[2];
  j[0] = -0.04; j[1] = 1e4 * z; j[2] = 1e4 * y;
  j[3] = 0.04; j[4] = -1e4 * z - 6e7 * y; j[5] = -1e4 * y;
  j[6] = 0.0; j[7] = 6e7 * y; j[8] = 0.0;
}
__device__ void events(double t, const double* y, double* g, const double* p) { g[0] = y[1] - p[0]; }
"""


@pytest.mark.parametrize("chunk", CHUNKS)
def test_hiprtc_n3_robertson_threshold_with_jac(chunk):
    levels = [3e-5, 2e-5, 3.5e-5]
    f = ivp_amd.DeviceIVP(ROB_SRC, 3, params=(3e-5,), events=[EventConfig()], jac=True)
    r = solve(f, 0.0, 40.0, [[1.0, 0.0, 0.0]] * 3, [[v] for v in levels], Options(rtol=RT, atol=AT, chunk_attempts=chunk))
    ms = [model(("rob", lv), lambda lv=lv: EM.solve(M.rhs_robertson, lambda x, y: [y[1] - lv], [EM.EventConfig()], 0.0, 40.0, [1.0, 0.0, 0.0],
                                                    RT, AT, jac=M.jac_robertson)) for lv in levels]
    assert [m.n_event_hits for m in ms] == [[2], [2], [2]]
    assert_batch(r, ms, "robertson")


def a8(i, j):
    return -1.0 - 0.25 * i if i == j else (200.0 if (i % 2 and j == i - 1) else 1e-3 * (1 + ((3 * i + 5 * j) % 7)))


A8 = [[a8(i, j) for j in range(8)] for i in range(8)]
LIN8_SRC = ("__device__ const double lin_a[64] = {" + ", ".join(float(A8[i][j]).hex() for i in range(8) for j in range(8)) + "};\n"
            "__device__ void ode(double t, const double* y, double* d, const double* p) {\n"
            "  for (int i = 0; i < 8; ++i) { double s = lin_a[i * 8] * y[0]; for (int j = 1; j < 8; ++j) s = s + lin_a[i * 8 + j] * y[j]; d[i] = s; }\n}\n"
            "__device__ void events(double t, const double* y, double* g, const double* p) { g[0] = y[0] - p[0]; g[1] = y[7] - p[1]; }\n")


@pytest.mark.parametrize("chunk", CHUNKS)
def test_hiprtc_n8_two_events_on_different_components_b5(chunk):
    B = 5
    par = [[0.9 + 0.01 * b, 10.0 + b] for b in range(B)]
    y0s = [[1.0 + 0.02 * b * (i % 3) for i in range(8)] for b in range(B)]
    f = ivp_amd.DeviceIVP(LIN8_SRC, 8, params=(0.9, 10.0), events=[EventConfig().negative(), EventConfig()])
    r = solve(f, 0.0, 2.0, y0s, par, Options(rtol=RT, atol=AT, chunk_attempts=chunk))
    cfg = [EM.EventConfig(EM.NEGATIVE), EM.EventConfig()]
    ms = [model(("lin8", b), lambda b=b: EM.solve(M.rhs_dense_linear(A8), lambda x, y: [y[0] - par[b][0], y[7] - par[b][1]], cfg, 0.0, 2.0,
                                                  y0s[b], RT, AT)) for b in range(B)]
    assert all(m.n_event_hits[0] == 1 and m.n_event_hits[1] >= 1 for m in ms)
    assert_batch(r, ms, "lin8")


PEND_SRC = """
__device__ void ode(double t, const double* s, double* d, const double* p) {
  const double p1 = s[0], p2 = s[1], v1 = s[2], v2 = s[3], lam = s[4];
  d[0] = v1; d[1] = v2; d[2] = -lam * p1; d[3] = -lam * p2 - 1.0; d[4] = p1 * v1 + p2 * v2;
}
__device__ void mass(double* m, const double* p) { for (int i = 0; i < 4; ++i) m[i * 5 + i] = 1.0; }
__device__ void events(double t, const double* y, double* g, const double* p) { g[0] = y[0]; }
"""


def pend_y0s():
    out = []
    for deg in (90.0, 60.0, 45.0):   # released at rest: p = (sin, -cos), lam = -p2
        a = math.radians(deg)
        out.append([math.sin(a), -math.cos(a), 0.0, 0.0, math.cos(a)])
    return out


@pytest.mark.parametrize("chunk", CHUNKS)
def test_hiprtc_n5_index2_pendulum_mass_b3(chunk):
    y0s = pend_y0s()
    f = ivp_amd.DeviceIVP(PEND_SRC, 5, events=[EventConfig()], mass=True)
    r = solve(f, 0.0, 6.0, y0s, None, Options(rtol=RT, atol=AT, chunk_attempts=chunk), rad=Radau(nind2=1))
    ms = [model(("pend", tuple(y0)), lambda y0=y0: EM.solve_dae(DM.rhs_pendulum_index2, lambda x, y: [y[0]], [EM.EventConfig()], 0.0, 6.0, y0,
                                                                RT, AT, mass=DM.MASS_PENDULUM, nind2=1)) for y0 in y0s]
    assert all(m.n_event_hits[0] >= 2 for m in ms)
    assert_batch(r, ms, "pendulum")


# ---- group form --------------------------------------------------------------------------------------------------------

def lin_matrix(n):
    """the systems of tests/test_gpu_radau_group.py: a negative diagonal, 200 (2000 at n = 64) below it in every odd row"""
    a = [[1e-3 * (1 + ((3 * i + 5 * j) % 7)) for j in range(n)] for i in range(n)]
    for i in range(n):
        a[i][i] = -1.0 - 0.25 * i
        if i % 2:
            a[i][i - 1] = 200.0 if n <= 33 else 2000.0
    return a


def group_source(a, with_jac):
    n = len(a)
    src = f"__device__ const double lin_a[{n * n}] = {{" + ", ".join(float(a[i][j]).hex() for i in range(n) for j in range(n)) + "};\n"
    src += ("__device__ double ode_comp(int i, double x, const double* y, const double* p) {\n"
            f"  double s = lin_a[i * {n}] * y[0];\n  for (int j = 1; j < {n}; ++j) s = s + lin_a[i * {n} + j] * y[j];\n  return s;\n}}\n")
    src += f"__device__ void events(double x, const double* y, double* g, const double* p) {{ g[0] = y[0] - p[0]; g[1] = y[{n - 1}] - p[1]; }}\n"
    if with_jac:
        src += ("__device__ void jac_col(int col, double x, const double* y, double* column, const double* p) {\n"
                f"  for (int r = 0; r < {n}; ++r) column[r] = lin_a[r * {n} + col];\n}}\n")
    return src


def group_y0s(n, B):
    base = [1.0, 0.5, -0.5, 0.25, 0.0, 1e-3, -1.0, 2.0]
    return [[base[i % 8] * (1.0 + 0.5 * b) + 1e-3 * (b + 1) * (i + 1) + (3.0 * b if i == 1 else 0.0) for i in range(n)] for b in range(B)]


# n -> (B, t1, level on y[0] as a fraction of y0[0], level on y[n-1]): y[0] decays through its level; y[n-1] decays through
# its own (n = 9, 17: an even row) or is driven through zero by its neighbour (n = 64: an odd row, 2000 y[62])
GROUP = {9: (5, 0.5, 0.97, 0.9), 17: (3, 0.5, 0.97, 0.8), 64: (2, 0.1, 0.97, 0.0)}


def group_case(n, with_jac, terminal0=None, only=None):
    B, t1, f0, l1 = GROUP[n]
    a = lin_matrix(n)
    y0s = group_y0s(n, B)
    # `only`: the one trajectory whose y[0] level can be reached; the others' lies below anything y[0] visits
    par = [[f0 * y0s[b][0] if only in (None, b) else -1e3, l1 * (1.0 if n == 64 else y0s[b][n - 1])] for b in range(B)]
    cfg = [EM.EventConfig(EM.ALL, terminal0), EM.EventConfig()]
    ms = [model(("group", n, with_jac, terminal0, only, b),
                lambda b=b: EM.solve(M.rhs_dense_linear(a), lambda x, y: [y[0] - par[b][0], y[n - 1] - par[b][1]], cfg, 0.0, t1, y0s[b], RT, AT,
                                     jac=M.jac_dense_linear(a) if with_jac else None)) for b in range(B)]
    f = ivp_amd.DeviceIVP(group_source(a, with_jac), n, params=(0.0, 0.0), jac=with_jac,
                          events=[EventConfig(Direction.All, terminal0), EventConfig()])
    return f, t1, y0s, par, ms


@pytest.mark.parametrize("with_jac", [False, True])
@pytest.mark.parametrize("n", [9, 17, 64])
def test_group_events_on_first_and_last_component(n, with_jac):
    f, t1, y0s, par, ms = group_case(n, with_jac)
    r = solve(f, 0.0, t1, y0s, par)
    assert all(m.n_event_hits[0] >= 1 and m.n_event_hits[1] >= 1 for m in ms), [m.n_event_hits for m in ms]
    assert_batch(r, ms, f"group n={n}")


def test_group_one_retires_on_a_terminal_event_its_wave_mates_go_on():
    """n = 9, B = 5: trajectories 0..3 are the four groups of one wavefront.  Only trajectory 1 can reach its (terminal) level
    on y[0]; the others end at t1 with the results of their solo solves (the model integrates each alone)."""
    f, t1, y0s, par, ms = group_case(9, False, terminal0=1, only=1)
    r = solve(f, 0.0, t1, y0s, par)
    assert [m.status for m in ms] == [M.SUCCESS, M.INTERRUPT, M.SUCCESS, M.SUCCESS, M.SUCCESS]
    assert ms[1].nstep < min(m.nstep for i, m in enumerate(ms) if i != 1)   # it retires while the others still step
    assert_batch(r, ms, "group terminal")
    solo = solve(f, 0.0, t1, [y0s[2]], [par[2]])
    assert_batch(solo, [ms[2]], "group solo")


# ---- staging -----------------------------------------------------------------------------------------------------------

def test_staging_count_only_filling_and_one_pass_agree(monkeypatch):
    y0s = sho_y0s(5)
    ms = sho_models(y0s, 20.0, EM.EventConfig())
    assert min(m.n_event_hits[0] for m in ms) > 1
    f = ivp_amd.SHOZeroEvent()
    for mev, passes in ((0, 2), (1, 2), (64, 1)):
        r = solve(f, 0.0, 20.0, y0s, opt=Options(rtol=RT, atol=AT, max_events=mev))
        assert r.event_info["passes"] == passes, (mev, r.event_info)
        assert_batch(r, ms, f"max_events={mev}")
    most = max(m.n_event_hits[0] for m in ms)
    monkeypatch.setenv("IVP_EVENT_STAGING_BYTES", str(3 * most * 3 * 8))   # three trajectories' blocks of (n + 1) doubles: two ranges
    r = solve(f, 0.0, 20.0, y0s, opt=Options(rtol=RT, atol=AT, max_events=0))
    assert r.event_info["passes"] == 2 and 0 < r.event_info["staging_bytes"] <= 3 * most * 3 * 8
    assert_batch(r, ms, "staging cap")


# ---- outputs alongside -------------------------------------------------------------------------------------------------

def test_t_eval_with_a_terminal_event_sample_and_t_term():
    te = [0.05 * k for k in range(13)]
    f = ivp_amd.BouncingBall()
    y0s, par = [[0.5, 0.0], [5.0, 0.0]], [[9.81, 0.02]] * 2
    r = solve(f, 0.0, 0.6, y0s, par, Options(rtol=RT, atol=AT, t_eval=te))
    cfg = cfg_of(f.event_config(0))
    ms = [EM.solve(ball_rhs(9.81, 0.02), lambda x, y: [y[0]], [cfg], 0.0, 0.6, y0, RT, AT, t_eval=te) for y0 in y0s]
    assert ms[0].status == M.INTERRUPT and ms[0].eval_idx[-1] == -1 and ms[1].status == M.SUCCESS
    assert_batch(r, ms, "t_eval")
    nf, idx, ye = _np(r.n_filled), _np(r.eval_idx), _np(r.y_eval)
    for b, m in enumerate(ms):
        k = len(m.t)
        assert int(nf[b]) == k and list(idx[:k, b]) == m.eval_idx and (bits(ye[:k, :, b]) == bits(m.y)).all()
    assert (bits(_np(r.t_term)[0]) == bits(ms[0].t_term)).all()


def test_dense_output_segments_and_backward_integration():
    y0s = sho_y0s(3)
    r = solve(ivp_amd.SHOZeroEvent(), 0.0, -10.0, y0s, opt=Options(rtol=RT, atol=AT, dense_output=True, max_log=400))
    ms = [EM.solve(M.rhs_sho, lambda x, y: [y[0]], [EM.EventConfig()], 0.0, -10.0, y0, RT, AT, dense_output=True) for y0 in y0s]
    assert all(m.n_event_hits[0] >= 3 and m.t_events[0][0] < 0.0 for m in ms)
    assert_batch(r, ms, "backward")
    ns, sc, sx, sh = _np(r.n_seg), _np(r.seg_cont), _np(r.seg_xold), _np(r.seg_h)
    for b, m in enumerate(ms):
        assert int(ns[b]) == len(m.segs)
        for q, (cont, xold, h) in enumerate(m.segs):
            assert (bits(sc[q, :, b]) == bits(cont)).all() and sx[q, b] == xold and sh[q, b] == h


SHO6_SRC = ("__device__ void ode(double t, const double* y, double* d, const double* p) { d[0] = y[1]; d[1] = -y[0]; }\n"
            "__device__ void events(double t, const double* y, double* g, const double* p) {\n"
            "  for (int i = 0; i < 6; ++i) g[i] = y[i & 1] - (-0.5 + 0.2 * i);\n}\n")


def test_more_than_four_event_functions_through_the_vec_arrays():
    evs = [EventConfig(), EventConfig().positive(), EventConfig().negative(), EventConfig(), EventConfig(Direction.All, 2), EventConfig()]
    f = ivp_amd.DeviceIVP(SHO6_SRC, 2, events=evs)
    y0s = [[1.0, 0.0], [0.8, 0.1]]
    r = solve(f, 0.0, 10.0, y0s)
    ev = lambda x, y: [y[i & 1] - (-0.5 + 0.2 * i) for i in range(6)]
    ms = [EM.solve(M.rhs_sho, ev, [cfg_of(c) for c in evs], 0.0, 10.0, y0, RT, AT) for y0 in y0s]
    assert all(m.status == M.INTERRUPT and m.n_event_hits[4] == 2 for m in ms)
    assert_batch(r, ms, "six events")


def test_host_pointer_form():
    """ivp_radau_solve_events on numpy arrays: the library allocates the log with malloc and the caller frees it."""
    y0s = sho_y0s(4)
    ms = sho_models(y0s, 10.0, EM.EventConfig())
    f, ctx = ivp_amd.SHOZeroEvent(), ivp_amd.Context(0)
    B = len(y0s)
    y0 = np.array(y0s).T.copy()
    t0, t1 = np.array([0.0]), np.array([10.0])
    keep = []
    opt = Options(rtol=RT, atol=AT, max_events=1)._c(2, keep)
    out = _lib.BatchResultT()
    arrs = dict(y_end=np.zeros((2, B)), t_end=np.zeros(B), status=np.zeros(B, np.int32), n_event_hits=np.zeros((1, B), np.uint32))
    for k, v in arrs.items():
        setattr(out, k, C.c_void_p(v.ctypes.data))
    off = np.zeros(B + 1, np.uint64)
    el = _lib.EventLogT()
    el.offsets = off.ctypes.data
    prob, rs = api._problem_c(f), Radau()._c()
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = ctx.lib.ivp_radau_solve_events(ctx.handle, C.byref(prob), B, p(y0), None, p(t0), 1, p(t1), 1, C.byref(opt), C.byref(rs), None,
                                        C.byref(out), C.byref(el))
    try:
        assert rc == 0, ctx.last_error()
        assert el.owned == 1 and el.device == -1 and el.passes == 2 and int(el.total) == int(off[-1]) == sum(m.n_event_hits[0] for m in ms)
        t = np.ctypeslib.as_array(C.cast(el.t, C.POINTER(C.c_double)), shape=(int(el.total),)).copy()
        y = np.ctypeslib.as_array(C.cast(el.y, C.POINTER(C.c_double)), shape=(int(el.total), 2)).copy()
    finally:
        ctx.lib.ivp_event_log_free(C.byref(el))
    for b, m in enumerate(ms):
        lo, hi = int(off[b]), int(off[b + 1])
        assert (bits(t[lo:hi]) == bits(m.t_events[0])).all() and (bits(y[lo:hi]) == bits(m.y_events[0])).all()
        assert (bits(arrs["y_end"][:, b]) == bits(m.y_end)).all() and int(arrs["status"][b]) == m.status


# ---- refusals and neighbours -------------------------------------------------------------------------------------------

def test_refusals():
    y0 = torch.as_tensor(np.array([[1.0], [0.0]]), device=DEV)
    with pytest.raises(ivp_amd.ConfigError, match="defines no event functions") as e:
        Radau().solve_batch_events(ivp_amd.SHO(), 0.0, 1.0, y0)
    assert e.value.code == -100
    with pytest.raises(ivp_amd.ConfigError, match="fp_mode = FMA") as e:
        Radau().solve_batch_events(ivp_amd.SHOZeroEvent(), 0.0, 1.0, y0, options=Options(fp_mode=ivp_amd.FpMode.FMA))
    assert e.value.code == -100
    src65 = ("__device__ double ode_comp(int i, double x, const double* y, const double* p) { return -y[i]; }\n"
             "__device__ void events(double x, const double* y, double* g, const double* p) { g[0] = y[0] - 0.5; }\n")
    f65 = ivp_amd.DeviceIVP(src65, 65, events=[EventConfig()])
    with pytest.raises(ivp_amd.ConfigError, match=r"Radau with event functions for n = 65: not yet \(n <= 64\)") as e:
        Radau().solve_batch_events(f65, 0.0, 1.0, torch.ones((65, 1), dtype=torch.float64, device=DEV))
    assert e.value.code == -100
    fm = ivp_amd.DeviceIVP(PEND_SRC, 5, events=[EventConfig()], mass=True)
    with pytest.raises(ivp_amd.ConfigError, match="mass matrix") as e:   # dae == NULL: the ODE rules
        api.solve_ivp_batch_events(fm, 0.0, 1.0, torch.as_tensor(np.array(pend_y0s()[:1]).T.copy(), device=DEV), _radau=Radau()._c(), _radau_dae=None)
    assert e.value.code == -100
    # the other Radau calls keep refusing a problem with event functions
    with pytest.raises(ivp_amd.ConfigError, match="event functions: not yet on the accelerated path"):
        Radau().solve_batch(ivp_amd.SHOZeroEvent(), 0.0, 1.0, y0)


def test_sequence_on_one_context_leaves_no_stale_event_state():
    """DOPRI5 events, Radau events, a plain Radau solve, BDF events on ONE context: prev_event / n_ev / the event block are
    context scratch that every solve must set up afresh."""
    y0s = sho_y0s(6)
    y0 = torch.as_tensor(np.array(y0s).T.copy(), device=DEV)
    fe, fp = ivp_amd.SHOZeroEvent(), ivp_amd.SHO()
    o5, ob = Options(method="DOPRI5", rtol=RT, atol=AT), Options(method="BDF", rtol=RT, atol=AT)
    fresh = ivp_amd.Context(0)
    want5 = ivp_amd.solve_ivp_batch_events(fe, 0.0, 10.0, y0, None, o5, fresh)
    wantb = ivp_amd.solve_ivp_batch_events(fe, 0.0, 7.0, y0, None, ob, ivp_amd.Context(0))
    ctx = ivp_amd.Context(0)
    got5 = ivp_amd.solve_ivp_batch_events(fe, 0.0, 10.0, y0, None, o5, ctx)
    rr = Radau().solve_batch_events(fe, 0.0, 8.0, y0, None, Options(rtol=RT, atol=AT), ctx)
    plain = Radau().solve_batch(fp, 0.0, 8.0, y0, None, Options(rtol=RT, atol=AT), ctx)
    gotb = ivp_amd.solve_ivp_batch_events(fe, 0.0, 7.0, y0, None, ob, ctx)
    assert_batch(rr, sho_models(y0s, 8.0, EM.EventConfig()), "radau in sequence")
    pm = [model(("sho plain", tuple(v)), lambda v=v: M.solve(M.rhs_sho, 0.0, 8.0, v, RT, AT)) for v in y0s]
    for b, m in enumerate(pm):
        assert (bits(_np(plain.y_end)[:, b]) == bits(m.y_end)).all() and int(_np(plain.nstep)[b]) == m.nstep
    for got, want in ((got5, want5), (gotb, wantb)):
        for k in ("event_offsets", "t_events_csr", "y_events_csr", "y_end", "n_event_hits", "nstep"):
            assert torch.equal(getattr(got, k), getattr(want, k)), k
