"""Unbounded batch event output in CSR form on the MI355X (solve_ivp_batch_events / ivp_batch_solve_events_device).
Everything bit for bit, with one stated exception: the two rational events whose event functions call pow() are compared
bit for bit with solve_ivp_batch's bounded layout and only to rtol 1e-9 with the oracle (device pow against libm; their
placement is compared with the oracle exactly):

  * every run (event i, trajectory b) -- record event_offsets[i * B + b] + k -- equals the oracle's t_events[i] /
    y_events[i] of that solve_ivp() call: ragged end times (zero-length intervals, no hit, 120 hits) at a block that is too
    small (filling solve), large enough (one integration) and absent (max_events = 0), backward integration, three
    events with mixed directions, a terminal event, every kernel variant and method, both arithmetic modes;
  * hiprtc problems (no oracle): equal to solve_ivp_batch at a max_events above the largest count -- CR3BP with g = y,
    a 9-state system on the wavefront-per-trajectory kernels, a 100-state system through the wide-record fallback;
  * a staging cap that splits the filling solve into trajectory ranges, caller-owned buffers through the C ABI, argument
    errors, and a context that goes on to other solves.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import _lib
from ivp_amd import api as A
from ivp_amd import workloads as W
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U64 = np.uint64


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(U64)


def _solve(f, t0, t1, y0, p=None, ctx=None, **kw):
    """solve_ivp_batch_events; no overflow warning may ever come out of it"""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = ivp_amd.solve_ivp_batch_events(f, t0, t1, torch.as_tensor(np.ascontiguousarray(y0), device=DEV),
                                           None if p is None else torch.as_tensor(np.ascontiguousarray(p), device=DEV), ivp_amd.Options(**kw), ctx)
    assert r.t_events is None and r.y_events is None and not r.event_overflow
    off = r.event_offsets.cpu().numpy()
    hits = r.n_event_hits.cpu().numpy().astype(np.int64)
    assert off[0] == 0 and np.array_equal(np.diff(off), hits.reshape(-1))
    assert int(off[-1]) == r.event_info["total"] == r.t_events_csr.shape[0] == r.y_events_csr.shape[0]
    return r, off, r.t_events_csr.cpu().numpy(), r.y_events_csr.cpu().numpy(), hits


def _same_log(a, b):
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(_bits(x) if x.dtype == np.float64 else x, _bits(y) if y.dtype == np.float64 else y)


def _equals_oracle(res, runs):
    """runs[i][b] = (t_events, y_events) of the oracle for event i on trajectory b"""
    _, off, t, y, hits = res
    nev, B = hits.shape
    for i in range(nev):
        for b in range(B):
            lo, hi = int(off[i * B + b]), int(off[i * B + b + 1])
            ot, oy = runs[i][b]
            assert hi - lo == len(ot), (i, b, hi - lo, len(ot))
            assert np.array_equal(_bits(t[lo:hi]), _bits(ot)), (i, b)
            assert np.array_equal(_bits(y[lo:hi]), _bits(oy).reshape(len(ot), y.shape[1])), (i, b)


def _oracle_runs(rhs, t0, t1, y0, nev, params=None, **kw):
    B = y0.shape[1]
    t0, t1 = np.broadcast_to(t0, B), np.broadcast_to(t1, B)
    runs = [[None] * B for _ in range(nev)]
    status = np.zeros(B, np.int64)
    for b in range(B):
        extra = {} if params is None else {"params": list(params[:, b])}
        o = O.solve_ivp(rhs, float(t0[b]), float(t1[b]), list(y0[:, b]), **extra, **kw)
        status[b] = o.status
        for i in range(nev):   # a zero-length interval returns before the events are set up: no event lists at all
            runs[i][b] = (o.t_events[i], o.y_events[i]) if i < len(o.t_events) else (np.zeros(0), np.zeros((0, y0.shape[0])))
    return runs, status


# ---- 1. ragged end times: a wave of 64, a wave of 64, a partial wave of 2 ----
SHO_OPTS = dict(method="DOPRI5", rtol=1e-8, atol=1e-10)
SHO_EV = dict(event_direction=[0], event_terminal=[0])


def _ragged(B=130):
    rng = np.random.default_rng(17)
    y0 = np.stack([1.0 + 0.1 * rng.standard_normal(B), 0.1 * rng.standard_normal(B)])
    t1 = rng.uniform(0.0, 60.0, B) * 2 * np.pi
    t1[[0, 64, 129]] = 60 * 2 * np.pi            # 120 hits in every wave
    t1[[1, 65, 128]] = 0.0                         # zero-length intervals
    t1[[2, 66]] = 0.05                             # a fraction of a period: no hit
    return y0, t1


@pytest.fixture(scope="module")
def ragged_oracle():
    y0, t1 = _ragged()
    runs, _ = _oracle_runs("sho_ev", 0.0, t1, y0, 1, detpow=True, **SHO_EV, **SHO_OPTS)
    return y0, t1, runs


def test_ragged_end_times_every_block_size_equals_the_oracle(ragged_oracle):
    y0, t1, runs = ragged_oracle
    f = ivp_amd.SHOZeroEvent(ivp_amd.EventConfig())
    t1d = torch.as_tensor(t1, device=DEV)
    small = _solve(f, 0.0, t1d, y0, max_events=16, **SHO_OPTS)
    hits = small[4]
    assert small[0].event_info["passes"] == 2
    assert hits.max() == 120 and hits[0, 1] == 0 and hits[0, 2] == 0 and hits[0, 129] == 120
    _equals_oracle(small, runs)
    large = _solve(f, 0.0, t1d, y0, max_events=128, **SHO_OPTS)
    assert large[0].event_info["passes"] == 1
    _same_log(large, small)
    none = _solve(f, 0.0, t1d, y0, max_events=0, **SHO_OPTS)
    assert none[0].event_info["passes"] == 2
    _same_log(none, small)
    # the accessors: one run, and all roots of the event with their trajectories
    t, y = small[0].events_of(129, 0)
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(runs[0][129][0])) and tuple(y.shape) == (120, 2)
    ta, ya, traj = small[0].events_all(0)
    assert np.array_equal(traj.cpu().numpy(), np.repeat(np.arange(130), hits[0]))
    assert np.array_equal(_bits(ta.cpu().numpy()), _bits(small[2])) and tuple(ya.shape) == (int(hits.sum()), 2)


def test_backward_integration_equals_the_oracle():
    B = 67
    rng = np.random.default_rng(23)
    y0 = np.stack([1.0 + 0.1 * rng.standard_normal(B), 0.1 * rng.standard_normal(B)])
    t0 = rng.uniform(0.0, 12.0, B) * 2 * np.pi
    runs, _ = _oracle_runs("sho_ev", t0, 0.0, y0, 1, detpow=True, **SHO_EV, **SHO_OPTS)
    res = _solve(ivp_amd.SHOZeroEvent(ivp_amd.EventConfig()), torch.as_tensor(t0, device=DEV), 0.0, y0, max_events=4, **SHO_OPTS)
    assert res[0].event_info["passes"] == 2 and res[4].max() > 4
    _equals_oracle(res, runs)


# ---- 2. three events, event-major run placement ----
def test_three_events_with_mixed_directions_are_placed_event_major():
    """The placement -- which run holds how many records -- against the oracle for all three events.  The values of event 2
    (g = t - 7.4) against the oracle bit for bit.  Events 0 and 1 evaluate pow() inside the event function, where the
    device's pow and the oracle's libm differ in the last bits (tests/test_gpu_parity.py, test_event_detection_matches_oracle:
    the one problem that suite does not compare exactly): their values are compared bit for bit with the bounded layout
    of solve_ivp_batch on the same batch, and with the oracle at that suite's rtol 1e-9 / atol 1e-11."""
    B = 65
    rng = np.random.default_rng(29)
    y0 = np.stack([np.full(B, 1 / 3), np.full(B, 2 / 9)]) * (1.0 + 1e-3 * rng.standard_normal((1, B)))
    t1 = np.linspace(5.2, 8.0, B)                  # from before the first root to past the last
    f = ivp_amd.RationalEvents(ivp_amd.EventConfig().positive(), ivp_amd.EventConfig().negative(), ivp_amd.EventConfig())
    opts = dict(method="DOPRI5", rtol=1e-8, atol=1e-10)
    runs, _ = _oracle_runs("rational_ev", 5.0, t1, y0, 3, detpow=True, event_direction=[1, -1, 0], event_terminal=[0, 0, 0], **opts)
    t1d = torch.as_tensor(t1, device=DEV)
    bnd = ivp_amd.solve_ivp_batch(f, 5.0, t1d, torch.as_tensor(y0, device=DEV), None, ivp_amd.Options(max_events=2, **opts))
    bt, by = bnd.t_events.cpu().numpy(), bnd.y_events.cpu().numpy()
    for me in (0, 1):
        res = _solve(f, 5.0, t1d, y0, max_events=me, **opts)
        assert res[0].event_info["passes"] == (2 if me == 0 else 1)
        _, off, t, y, hits = res
        assert hits.shape == (3, B) and all(0 < hits[i].sum() < B for i in range(3))     # every event: some with, some without
        assert np.array_equal(hits, bnd.n_event_hits.cpu().numpy().astype(np.int64)) and hits.max() == 1
        for i in range(3):
            for b in range(B):
                lo, hi = int(off[i * B + b]), int(off[i * B + b + 1])
                ot, oy = runs[i][b]
                assert hi - lo == len(ot), (i, b)                                        # the placement
                assert np.array_equal(_bits(t[lo:hi]), _bits(bt[i, :hi - lo, b])) and np.array_equal(_bits(y[lo:hi]), _bits(by[i, :hi - lo, :, b])), (i, b)
                if i == 2:
                    assert np.array_equal(_bits(t[lo:hi]), _bits(ot)) and np.array_equal(_bits(y[lo:hi]), _bits(oy).reshape(hi - lo, 2)), b
                else:
                    assert np.allclose(t[lo:hi], ot, rtol=1e-9, atol=1e-11) and np.allclose(y[lo:hi], oy.reshape(hi - lo, 2), rtol=1e-9, atol=1e-11), (i, b)
        for i in range(3):                          # all roots of event i over the batch: one contiguous slice
            ti, _, traj = res[0].events_all(i)
            assert np.array_equal(traj.cpu().numpy(), np.repeat(np.arange(B), hits[i]))
            assert np.array_equal(_bits(ti.cpu().numpy()), _bits(t[int(off[i * B]):int(off[(i + 1) * B])]))


# ---- 3. a terminal event ----
def test_terminal_event_one_record_per_run_and_the_end_state_of_the_bounded_solve():
    B = 70
    rng = np.random.default_rng(31)
    y0 = np.stack([rng.uniform(1.0, 30.0, B), rng.uniform(-3.0, 8.0, B)])
    f = ivp_amd.BouncingBall(9.81, 0.02)           # ground event: terminal, negative direction
    p = np.repeat(np.array([[9.81], [0.02]]), B, axis=1)
    opts = dict(method="DOPRI5", rtol=1e-8, atol=1e-10)
    res = _solve(f, 0.0, 100.0, y0, p, max_events=1, **opts)
    r = res[0]
    assert res[0].event_info["passes"] == 1 and np.array_equal(res[4], np.ones((1, B), np.int64))
    assert (r.status.cpu().numpy() == int(ivp_amd.Status.UserInterrupt)).all()
    bnd = ivp_amd.solve_ivp_batch(f, 0.0, 100.0, torch.as_tensor(y0, device=DEV), torch.as_tensor(p, device=DEV), ivp_amd.Options(max_events=1, **opts))
    for k in ("t_end", "y_end", "status", "naccpt", "nfev", "t_term"):
        assert np.array_equal(getattr(r, k).cpu().numpy(), getattr(bnd, k).cpu().numpy()), k
    assert np.array_equal(_bits(res[2]), _bits(bnd.t_events.cpu().numpy()[0, 0]))
    assert np.array_equal(_bits(res[3]), _bits(bnd.y_events.cpu().numpy()[0, 0].T))
    runs, status = _oracle_runs("ball", 0.0, 100.0, y0, 1, params=p, detpow=True, event_direction=[-1], event_terminal=[1], **opts)
    assert (status == int(ivp_amd.Status.UserInterrupt)).all()
    _equals_oracle(res, runs)
    zero = _solve(f, 0.0, 100.0, y0, p, max_events=0, **opts)      # count, then fill: the same records
    assert zero[0].event_info["passes"] == 2
    _same_log(zero, res)


# ---- 4. kernel shapes and arithmetic ----
def _shapes_case(B=80):
    rng = np.random.default_rng(37)
    y0 = np.stack([1.0 + 0.1 * rng.standard_normal(B), 0.1 * rng.standard_normal(B)])
    return y0, rng.uniform(0.0, 8.0, B) * 2 * np.pi


@pytest.mark.parametrize("method,variants,tol", [("DOPRI5", (0, 1, 3), (1e-8, 1e-10)), ("DOP853", (0, 1, 3), (1e-9, 1e-11)), ("RK23", (0,), (1e-5, 1e-8)),
                                                 ("BDF", (0,), (1e-5, 1e-8))], ids=["dopri5", "dop853", "rk23", "bdf"])
def test_every_kernel_variant_and_method_equals_the_oracle(method, variants, tol):
    y0, t1 = _shapes_case()
    opts = dict(method=method, rtol=tol[0], atol=tol[1])
    runs, _ = _oracle_runs("sho_ev", 0.0, t1, y0, 1, detpow=True, **SHO_EV, **opts)
    first = None
    for v in variants:
        res = _solve(ivp_amd.SHOZeroEvent(ivp_amd.EventConfig()), 0.0, torch.as_tensor(t1, device=DEV), y0, max_events=3, variant=v, **opts)
        assert res[0].event_info["passes"] == 2
        if first is None:
            first = res
            _equals_oracle(res, runs)
        else:
            _same_log(res, first)


def test_fma_mode_equals_the_fma_oracle():
    y0, t1 = _shapes_case()
    runs, _ = _oracle_runs("sho_ev", 0.0, t1, y0, 1, fma=True, **SHO_EV, **SHO_OPTS)
    for me in (3, 64):
        res = _solve(ivp_amd.SHOZeroEvent(ivp_amd.EventConfig()), 0.0, torch.as_tensor(t1, device=DEV), y0, max_events=me, fp_mode=ivp_amd.FpMode.FMA, **SHO_OPTS)
        assert res[0].event_info["passes"] == (2 if me == 3 else 1)
        _equals_oracle(res, runs)


# ---- 5. hiprtc problems: against solve_ivp_batch with room for every occurrence ----
CR3BP_EVENT_SRC = r"""
__device__ void ode(double t, const double* s, double* d, const double* p)
{
    const double mu = p[0];
    const double x = s[0], y = s[1], z = s[2], vx = s[3], vy = s[4], vz = s[5];
    const double a = x + mu, b = x - 1.0 + mu;
    const double r1 = sqrt(a * a + y * y + z * z), r2 = sqrt(b * b + y * y + z * z);
    const double r13 = r1 * r1 * r1, r23 = r2 * r2 * r2;
    d[0] = vx; d[1] = vy; d[2] = vz;
    d[3] = x + 2.0 * vy - (1.0 - mu) * (x + mu) / r13 - mu * (x - 1.0 + mu) / r23;
    d[4] = y - 2.0 * vx - (1.0 - mu) * y / r13 - mu * y / r23;
    d[5] = -(1.0 - mu) * z / r13 - mu * z / r23;
}
__device__ void events(double t, const double* s, double* g, const double* p) { g[0] = s[1]; }   // crossings of the x axis
"""


def _ring_src(masses, extra):
    """`masses` masses on a ring (positions, then velocities) and `extra` decaying states behind them"""
    m = masses
    return f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{{
    if (i < {m}) return y[{m} + i];
    if (i >= {2 * m}) return -0.5 * y[i];
    const int k = i - {m}, l = (k + {m - 1}) % {m}, r = (k + 1) % {m};
    return p[0] * (y[l] - 2.0 * y[k] + y[r]);
}}
__device__ void events(double t, const double* y, double* g, const double* p)
{{
    g[0] = y[0];                      // mass 0 passes the origin
    g[1] = y[1] - y[{m - 1}];         // two masses at the same displacement
}}"""


def _against_bounded(f, t0, t1, y0, p, max_events, **opts):
    """the CSR log (max_events below the largest count: a filling solve) against solve_ivp_batch with room for everything"""
    res = _solve(f, t0, t1, y0, p, max_events=max_events, **opts)
    _, off, t, y, hits = res
    nev, B = hits.shape
    most = int(hits.max())
    assert most > max_events and res[0].event_info["passes"] == 2
    bnd = ivp_amd.solve_ivp_batch(f, t0, t1, torch.as_tensor(y0, device=DEV), None if p is None else torch.as_tensor(p, device=DEV),
                                  ivp_amd.Options(max_events=most + 1, **opts))
    assert np.array_equal(bnd.n_event_hits.cpu().numpy().astype(np.int64), hits)
    bt, by = bnd.t_events.cpu().numpy(), bnd.y_events.cpu().numpy()
    ii, bb = np.repeat(np.repeat(np.arange(nev), B), hits.reshape(-1)), np.repeat(np.tile(np.arange(B), nev), hits.reshape(-1))
    kk = np.concatenate([np.arange(c) for c in hits.reshape(-1)])
    assert np.array_equal(_bits(t), _bits(bt[ii, kk, bb]))
    assert np.array_equal(_bits(y), _bits(by[ii, kk, :, bb]))
    for k in ("t_end", "y_end", "status", "naccpt", "nfev"):
        assert np.array_equal(getattr(res[0], k).cpu().numpy(), getattr(bnd, k).cpu().numpy()), k
    return res


def test_hiprtc_cr3bp_x_axis_crossings():
    B = 200
    y0, p, t0, t1 = W.cr3bp_batch(B)
    f = ivp_amd.DeviceIVP(CR3BP_EVENT_SRC, n=6, params=(W.ARENSTORF_MU,), events=[ivp_amd.EventConfig()])
    res = _against_bounded(f, t0, t1, y0, p, 2, method="DOPRI5", rtol=1e-6, atol=1e-9)
    one = _solve(f, t0, t1, y0, p, max_events=int(res[4].max()), method="DOPRI5", rtol=1e-6, atol=1e-9)
    assert one[0].event_info["passes"] == 1
    _same_log(one, res)


@pytest.mark.parametrize("masses,extra,B", [(4, 1, 70), (48, 4, 5)], ids=["n9-tiled", "n100-wide-record-fallback"])
def test_hiprtc_wavefront_per_trajectory_systems(masses, extra, B):
    n = 2 * masses + extra
    f = ivp_amd.DeviceIVP(_ring_src(masses, extra), n=n, params=(3.0,), events=[ivp_amd.EventConfig(), ivp_amd.EventConfig().positive()])
    y0 = np.random.default_rng(41).standard_normal((n, B))
    t1 = np.linspace(1.0, 9.0, B)
    _against_bounded(f, 0.0, torch.as_tensor(t1, device=DEV), y0, np.full((1, B), 3.0), 1, method="DOPRI5", rtol=1e-7, atol=1e-9)


# ---- 6. a small staging cap ----
def test_staging_cap_splits_the_filling_solve_into_trajectory_ranges(monkeypatch):
    B = 200
    y0, p, t0, t1 = W.cr3bp_batch(B)
    f = ivp_amd.DeviceIVP(CR3BP_EVENT_SRC, n=6, params=(W.ARENSTORF_MU,), events=[ivp_amd.EventConfig()])
    opts = dict(method="DOPRI5", rtol=1e-6, atol=1e-9, max_events=0)
    whole = _solve(f, t0, t1, y0, p, **opts)
    most = int(whole[4].max())
    one = most * 7 * 8                              # one trajectory's block: [1 event][most][n + 1] doubles
    assert whole[0].event_info["staging_bytes"] == one * B
    cap = one * B // 3 - 8                          # fewer than B / 3 trajectories fit: at least 4 ranges
    monkeypatch.setenv("IVP_EVENT_STAGING_BYTES", str(cap))
    split = _solve(f, t0, t1, y0, p, **opts)
    assert split[0].event_info["passes"] == 2
    sb = split[0].event_info["staging_bytes"]
    assert 0 < sb <= cap or sb == one
    assert sb < one * B // 3 + 1
    _same_log(split, whole)
    monkeypatch.setenv("IVP_EVENT_STAGING_BYTES", "8")   # below any block: one trajectory per range
    tiny = _solve(f, t0, t1, y0[:, :5], p[:, :5], **opts)
    assert tiny[0].event_info["staging_bytes"] == int(tiny[4].max()) * 7 * 8
    monkeypatch.delenv("IVP_EVENT_STAGING_BYTES")
    _same_log(tiny, _solve(f, t0, t1, y0[:, :5], p[:, :5], **opts))


# ---- 7. the caller's buffers through the C ABI ----
def _c_call(f, y0, t1, opts, cap=None, r=None):
    L, ctx = _lib.load(), ivp_amd.default_context(0)
    keep = []
    copt = opts._c(f.n, keep)
    for i in range(f.n_events()):
        copt.ev_direction[i], copt.ev_terminal[i] = int(f.event_config(i).direction), int(f.event_config(i).terminal_count or 0)
    B = y0.shape[1]
    y0d = torch.as_tensor(np.ascontiguousarray(y0), device=DEV)
    t0d, t1d = torch.zeros(1, dtype=torch.float64, device=DEV), torch.as_tensor(np.asarray(t1, np.float64), device=DEV)
    off = torch.zeros(max(f.n_events(), 1) * B + 1, dtype=torch.int64, device=DEV)
    el = _lib.EventLogT()
    el.offsets = off.data_ptr()
    bufs = None
    if cap is not None:
        bufs = torch.zeros(max(cap, 1), dtype=torch.float64, device=DEV), torch.zeros((max(cap, 1), f.n), dtype=torch.float64, device=DEV)
        el.t, el.y, el.capacity = bufs[0].data_ptr(), bufs[1].data_ptr(), cap
    r = r or _lib.BatchResultT()
    prob = A._problem_c(f)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rc = L.ivp_batch_solve_events_device(ctx.handle, C.byref(prob), B, y0d.data_ptr(), None, t0d.data_ptr(), 1, t1d.data_ptr(), B,
                                         C.byref(copt), C.byref(r), C.byref(el), stream)
    return rc, el, off, bufs, ctx, stream


def test_callers_buffers_owned_log_and_argument_errors():
    y0, t1 = _shapes_case(40)
    f = ivp_amd.SHOZeroEvent(ivp_amd.EventConfig())
    opts = ivp_amd.Options(max_events=2, **SHO_OPTS)
    ref = _solve(f, 0.0, torch.as_tensor(t1, device=DEV), y0, max_events=2, **SHO_OPTS)
    total = ref[0].event_info["total"]
    L = _lib.load()
    for cap in (total - 1, total):
        rc, el, off, bufs, ctx, _ = _c_call(f, y0, t1, opts, cap)
        assert int(el.total) == total and el.owned == 0 and el.n_events == 1
        assert np.array_equal(off.cpu().numpy(), ref[1])
        if cap < total:
            assert rc == -105 and "hold" in ctx.last_error()
            assert not bufs[0].any() and not bufs[1].any()           # nothing was written: never a truncated log
        else:
            assert rc == 0, ctx.last_error()
            assert el.passes == 2
            assert np.array_equal(_bits(bufs[0].cpu().numpy()), _bits(ref[2])) and np.array_equal(_bits(bufs[1].cpu().numpy()), _bits(ref[3]))
    # an owned log, fetched into exact-size buffers
    rc, el, off, _, ctx, stream = _c_call(f, y0, t1, opts)
    assert rc == 0 and el.owned == 1 and el.device == 0 and int(el.total) == total and int(el.capacity) == total
    t, y = torch.zeros(total, dtype=torch.float64, device=DEV), torch.zeros((total, 2), dtype=torch.float64, device=DEV)
    assert L.ivp_event_log_fetch_device(C.byref(el), t.data_ptr(), y.data_ptr(), stream) == 0
    assert el.owned == 0 and el.t == t.data_ptr() and el.y == y.data_ptr()
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(ref[2])) and np.array_equal(_bits(y.cpu().numpy()), _bits(ref[3]))
    L.ivp_event_log_free(C.byref(el))                                # not owned any more: a no-op
    assert el.t == t.data_ptr()
    # the bounded members are not accepted beside the CSR log
    dummy = torch.zeros(2 * 2 * 40, dtype=torch.float64, device=DEV)
    for member in ("t_events", "y_events"):
        r = _lib.BatchResultT()
        setattr(r, member, dummy.data_ptr())
        rc, el, _, _, ctx, _ = _c_call(f, y0, t1, opts, r=r)
        assert rc == -100 and "bounded layout" in ctx.last_error() and el.owned == 0
    # a problem without event functions has no event log
    rc, el, _, _, ctx, _ = _c_call(ivp_amd.SHO(), y0, t1, opts)
    assert rc == -100 and "no event functions" in ctx.last_error()
    with pytest.raises(ValueError):
        ivp_amd.solve_ivp_batch_events(ivp_amd.SHO(), 0.0, 1.0, torch.as_tensor(y0, device=DEV))


# ---- 8. the context goes on to other solves ----
def test_context_reuse_after_an_events_solve_gives_the_bits_of_a_fresh_context():
    y0, t1 = _shapes_case(96)
    f = ivp_amd.SHOZeroEvent(ivp_amd.EventConfig())
    y0d, t1d = torch.as_tensor(y0, device=DEV), torch.as_tensor(t1, device=DEV)
    plain_o = ivp_amd.Options(max_events=8, max_log=16, **SHO_OPTS)
    logged_o = ivp_amd.Options(**SHO_OPTS)

    def follow_ups(ctx):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # solve_ivp_batch's own overflow report: unchanged
            a = ivp_amd.solve_ivp_batch(f, 0.0, t1d, y0d, None, plain_o, ctx)
        b = ivp_amd.solve_ivp_batch_logged(f, 0.0, t1d, y0d, None, logged_o, ctx)
        return a, b

    used = ivp_amd.Context(0)
    ev = _solve(f, 0.0, t1d, y0, ctx=used, max_events=2, **SHO_OPTS)
    assert ev[0].event_info["passes"] == 2
    got = follow_ups(used)
    again = _solve(f, 0.0, t1d, y0, ctx=used, max_events=2, **SHO_OPTS)
    _same_log(again, ev)
    want = follow_ups(ivp_amd.Context(0))
    for k in ("y_end", "t_end", "status", "nfev", "naccpt", "t_events", "y_events", "n_event_hits", "t_log", "y_log", "n_log"):
        assert np.array_equal(getattr(got[0], k).cpu().numpy(), getattr(want[0], k).cpu().numpy()), k
    for k in ("y_end", "t_end", "log_offsets", "t_log", "y_log", "n_event_hits", "t_events"):
        assert np.array_equal(getattr(got[1], k).cpu().numpy(), getattr(want[1], k).cpu().numpy()), k
    assert got[0].event_overflow and want[0].event_overflow


# ---- 9. a block deeper than one sweep of the grid: cap > 64 record blocks x 8 records ----
def test_one_pass_from_a_block_of_more_than_512_slots(ragged_oracle):
    """grid.y is clamped to 64 record blocks of 8 records: with max_events = 520 the blocks stride on to a second sweep
    (nothing to move there: 120 hits at most), and the records are those of the small blocks"""
    y0, t1, runs = ragged_oracle
    res = _solve(ivp_amd.SHOZeroEvent(ivp_amd.EventConfig()), 0.0, torch.as_tensor(t1, device=DEV), y0, max_events=520, **SHO_OPTS)
    assert res[0].event_info["passes"] == 1
    _equals_oracle(res, runs)


def test_one_pass_second_sweep_moves_records():
    """more than 512 occurrences per run in a one-pass solve: the second sweep of the record blocks carries records"""
    B = 66
    rng = np.random.default_rng(43)
    y0 = np.stack([1.0 + 0.1 * rng.standard_normal(B), 0.1 * rng.standard_normal(B)])
    t1 = rng.uniform(250.0, 300.0, B) * 2 * np.pi
    t1[5] = 1.0
    f = ivp_amd.SHOZeroEvent(ivp_amd.EventConfig())
    opts = dict(method="DOPRI5", rtol=1e-6, atol=1e-9)
    one = _solve(f, 0.0, torch.as_tensor(t1, device=DEV), y0, max_events=640, **opts)
    assert one[0].event_info["passes"] == 1 and 512 < one[4].max() <= 640
    two = _solve(f, 0.0, torch.as_tensor(t1, device=DEV), y0, max_events=0, **opts)
    assert two[0].event_info["passes"] == 2
    _same_log(one, two)
    for b in (0, 5, 65):
        o = O.solve_ivp("sho_ev", 0.0, float(t1[b]), list(y0[:, b]), detpow=True, **SHO_EV, **opts)
        t, y = one[0].events_of(b, 0)
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(o.t_events[0])) and np.array_equal(_bits(y.cpu().numpy()), _bits(o.y_events[0]))


# ---- 10. the host-pointer entry point ----
def _host_form(f, y0, t1, opts, cap=None, alias=False):
    """ivp_batch_solve_events: host pointers throughout; cap = None: a library-owned host log"""
    L, ctx = _lib.load(), ivp_amd.default_context(0)
    keep = []
    copt = opts._c(f.n, keep)
    for i in range(f.n_events()):
        copt.ev_direction[i], copt.ev_terminal[i] = int(f.event_config(i).direction), int(f.event_config(i).terminal_count or 0)
    B, nev = y0.shape[1], f.n_events()
    y0 = np.ascontiguousarray(y0, dtype=np.float64).copy()
    t0a, t1a = np.zeros(1), np.ascontiguousarray(t1, dtype=np.float64)
    y_end = y0 if alias else np.zeros((f.n, B))
    hits, t_end = np.zeros((nev, B), np.uint32), np.zeros(B)
    r = _lib.BatchResultT()
    r.y_end, r.t_end, r.n_event_hits = y_end.ctypes.data, t_end.ctypes.data, hits.ctypes.data
    off = np.zeros(nev * B + 1, np.uint64)
    el = _lib.EventLogT()
    el.offsets = off.ctypes.data
    bufs = None
    if cap is not None:
        bufs = np.zeros(max(cap, 1)), np.zeros((max(cap, 1), f.n))
        el.t, el.y, el.capacity = bufs[0].ctypes.data, bufs[1].ctypes.data, cap
    prob = A._problem_c(f)
    rc = L.ivp_batch_solve_events(ctx.handle, C.byref(prob), B, y0.ctypes.data, None, t0a.ctypes.data, 1, t1a.ctypes.data, B,
                                  C.byref(copt), C.byref(r), C.byref(el))
    total = int(el.total)
    if rc == 0 and cap is None:
        assert el.owned == 1 and el.device == -1 and int(el.capacity) == total
        get = lambda ptr, k: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(k,)).copy()
        t, y = get(el.t, total), get(el.y, total * f.n).reshape(total, f.n)
        L.ivp_event_log_free(C.byref(el))
        assert el.owned == 0 and not el.t
    elif rc == 0:
        assert el.owned == 0
        t, y = bufs[0][:total], bufs[1][:total]
    else:
        t = y = None
    return rc, ctx.last_error(), off, t, y, hits, y_end, int(el.passes), total, bufs, int(el.staging_bytes)


@pytest.mark.parametrize("max_events,passes", [(64, 1), (2, 2), (0, 2)], ids=["one-pass-host-pack", "filling-solve", "count-only-then-fill"])
def test_host_entry_point_equals_the_device_form(max_events, passes):
    y0, t1 = _shapes_case(70)
    f = ivp_amd.SHOZeroEvent(ivp_amd.EventConfig())
    opts = ivp_amd.Options(max_events=max_events, **SHO_OPTS)
    dev = _solve(f, 0.0, torch.as_tensor(t1, device=DEV), y0, max_events=max_events, **SHO_OPTS)
    total = dev[0].event_info["total"]
    y_end_dev = dev[0].y_end.cpu().numpy()

    def same(h):
        rc, err, off, t, y, hits, y_end, p, tot, _, _ = h
        assert rc == 0, err
        assert p == passes == dev[0].event_info["passes"] and tot == total
        assert np.array_equal(off.astype(np.int64), dev[1]) and np.array_equal(hits.astype(np.int64), dev[4])
        assert np.array_equal(_bits(t), _bits(dev[2])) and np.array_equal(_bits(y), _bits(dev[3]))
        assert np.array_equal(_bits(y_end), _bits(y_end_dev))

    same(_host_form(f, y0, t1, opts))                         # an owned host log
    same(_host_form(f, y0, t1, opts, cap=total))              # the caller's buffers, exactly large enough
    same(_host_form(f, y0, t1, opts, alias=True))             # y_end written over y0: the filling solve still starts from y0
    rc, err, off, _, _, hits, _, _, tot, bufs, _ = _host_form(f, y0, t1, opts, cap=total - 1)
    assert rc == -105 and "hold" in err and tot == total
    assert np.array_equal(off.astype(np.int64), dev[1]) and np.array_equal(hits.astype(np.int64), dev[4])
    assert not bufs[0].any() and not bufs[1].any()            # never a truncated log


def test_host_entry_point_under_a_staging_cap_runs_trajectory_ranges(monkeypatch):
    """IVP_EVENT_STAGING_BYTES below one whole-batch block: the host-pointer form's filling solve runs over more than one
    range, same log"""
    B = 70
    y0, t1 = _shapes_case(B)
    f = ivp_amd.SHOZeroEvent(ivp_amd.EventConfig())
    opts = ivp_amd.Options(max_events=0, **SHO_OPTS)
    whole = _host_form(f, y0, t1, opts)
    assert whole[0] == 0 and whole[7] == 2, whole[1]
    one = int(whole[5].max()) * 3 * 8                         # one trajectory's block: [1 event][most hits][n + 1] doubles
    assert whole[10] == one * B                               # one range
    cap = one * B // 3                                        # 23 trajectories' worth of the deepest block: at least 4 ranges
    monkeypatch.setenv("IVP_EVENT_STAGING_BYTES", str(cap))
    split = _host_form(f, y0, t1, opts)
    assert split[0] == 0 and split[7] == 2, split[1]
    assert 0 < split[10] <= cap
    assert split[8] == whole[8]
    for i in (2, 5):                                          # offsets, hits
        assert np.array_equal(split[i], whole[i])
    for i in (3, 4, 6):                                       # t, y, y_end
        assert np.array_equal(_bits(split[i]), _bits(whole[i]))
