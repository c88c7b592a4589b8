"""Batch dense output in CSR form on the MI355X (solve_ivp_batch_dense / ivp_batch_solve_dense_device and the device
evaluation ivp_dense_eval_device).  Everything bit-exact:

  * the CSR segments equal the bounded [max_log] layout of the same solve (max_log >= every count): cont, xold, h, n_seg,
    for every method on CR3BP (n = 6) and Van der Pol (n = 2), kernel variants, chunk sizes, both arithmetic modes, events
    and t_eval in the same solve, wave-per-trajectory systems (LinearDecay100, Heat1D256);
  * no cap: a 60-period SHO at rtol 1e-10 beside short trajectories delivers all of its segments, equal to the single
    solve_ivp(.., dense_output=True); a zero-length interval gives the constant segment; backward integration works;
  * the device evaluation equals the host ContinuousOutput (found and extrapolation included) in strict mode, and the
    solve's own t_eval samples away from step boundaries in both modes.
"""
import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import workloads as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U64 = np.uint64


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(U64)


def _problem(name, B):
    if name == "cr3bp":
        y0, p, t0, t1 = W.cr3bp_batch(B)
        return ivp_amd.CR3BP(), y0, p, t0, t1
    y0, p, t0, t1 = W.vdp_batch(B)
    return ivp_amd.VanDerPol(), y0, p, t0, np.minimum(t1, 60.0)


def _dense_vs_bounded(f, y0, p, t0, t1, **kw):
    """solve_ivp_batch_dense against solve_ivp_batch(dense_output, max_log >= every count) of the same batch"""
    y0d = torch.as_tensor(y0, device=DEV)
    pd = None if p is None else torch.as_tensor(p, device=DEV)
    d = ivp_amd.solve_ivp_batch_dense(f, t0, t1, y0d, pd, ivp_amd.Options(**kw))
    ns = d.n_seg.cpu().numpy().astype(np.int64)
    off = d.seg_offsets.cpu().numpy()
    assert off[0] == 0 and np.array_equal(np.diff(off), ns) and int(off[-1]) == d.dense_info["segments"] == d.seg_cont.shape[0]
    ml = max(int(ns.max()), 1)
    b = ivp_amd.solve_ivp_batch(f, t0, t1, y0d, pd, ivp_amd.Options(**{**kw, "dense_output": True, "max_log": max(ml, kw.get("max_log", 0))}))
    assert np.array_equal(b.n_seg.cpu().numpy().astype(np.int64), ns)
    B = len(ns)
    kk = np.concatenate([np.arange(c) for c in ns]) if B else np.zeros(0, np.int64)
    bb = np.repeat(np.arange(B), ns)
    bc, bx, bh = b.seg_cont.cpu().numpy(), b.seg_xold.cpu().numpy(), b.seg_h.cpu().numpy()
    assert np.array_equal(_bits(d.seg_xold.cpu().numpy()), _bits(bx[kk, bb]))
    assert np.array_equal(_bits(d.seg_h.cpu().numpy()), _bits(bh[kk, bb]))
    assert np.array_equal(_bits(d.seg_cont.cpu().numpy()), _bits(bc[kk, :, bb]))
    for name in ("y_end", "t_end", "status", "naccpt", "nfev", "y_eval", "n_filled", "t_events", "n_event_hits"):
        x, y = getattr(d, name), getattr(b, name)
        if x is not None:
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy()), name
    return d, b


CFG = {"DOPRI5": {}, "DOP853": {}, "RK23": {}, "RK4": {"first_step": 0.01}, "BDF": {}}


@pytest.mark.parametrize("method", list(CFG))
@pytest.mark.parametrize("prob", ["cr3bp", "vdp"])
def test_csr_segments_equal_the_bounded_layout(method, prob):
    f, y0, p, t0, t1 = _problem(prob, 96)
    d, _ = _dense_vs_bounded(f, y0, p, t0, t1, method=method, rtol=1e-6, atol=1e-9, **CFG[method])
    assert d.dense_info["passes"] == 2 and d.dense_info["segments"] > 96


@pytest.mark.parametrize("variant,chunk,fp", [(0, 0, "strict"), (1, 7, "strict"), (2, 1, "fma"), (3, 0, "fma"), (3, 7, "strict"), (0, 7, "fma")])
def test_csr_segments_every_kernel_shape_and_mode(variant, chunk, fp):
    f, y0, p, t0, t1 = _problem("cr3bp", 200)
    fpm = ivp_amd.FpMode.FMA if fp == "fma" else ivp_amd.FpMode.STRICT
    _dense_vs_bounded(f, y0, p, t0, t1, method="DOP853" if variant == 3 else "DOPRI5", rtol=1e-7, atol=1e-10, variant=variant,
                      chunk_attempts=chunk, fp_mode=fpm)


def test_csr_segments_beside_events_t_eval_and_a_bounded_step_log():
    B = 64
    f = ivp_amd.SHOZeroEvent(ivp_amd.EventConfig())
    rng = np.random.default_rng(7)
    y0 = np.stack([1.0 + 0.1 * rng.standard_normal(B), 0.1 * rng.standard_normal(B)])
    _dense_vs_bounded(f, y0, None, 0.0, 20.0, method="DOPRI5", rtol=1e-8, atol=1e-10, t_eval=list(np.linspace(0.0, 20.0, 41)))
    d, b = _dense_vs_bounded(f, y0, None, 0.0, 20.0, method="DOPRI5", rtol=1e-8, atol=1e-10, max_log=4096)
    assert d.dense_info["passes"] == 1     # every run fitted the counting solve's own block
    assert np.array_equal(d.t_log.cpu().numpy(), b.t_log.cpu().numpy()) and np.array_equal(d.n_log.cpu().numpy(), b.n_log.cpu().numpy())


@pytest.mark.parametrize("f,method,B,t1", [(ivp_amd.LinearDecay100(), "DOPRI5", 16, 2.0), (ivp_amd.LinearDecay100(), "BDF", 8, 2.0),
                                           (ivp_amd.Heat1D256(), "BDF", 4, 0.05)], ids=["decay100-dopri5", "decay100-bdf", "heat256-bdf"])
def test_csr_segments_wave_per_trajectory_systems(f, method, B, t1):
    rng = np.random.default_rng(11)
    y0 = 1.0 + 0.1 * rng.standard_normal((f.n, B))
    p = np.repeat(np.asarray(f.params(), dtype=np.float64).reshape(-1, 1), B, axis=1) if f.n_params else None
    _dense_vs_bounded(f, y0, p, 0.0, t1, method=method, rtol=1e-6, atol=1e-9)


def test_no_cap_long_trajectory_zero_interval_and_backward():
    B = 6
    opts = dict(method="DOPRI5", rtol=1e-10, atol=1e-12)
    y0 = np.array([[1.0, 0.5, 1.0, 0.2, 1.0, 0.3], [0.0, 0.0, 0.0, 0.1, 0.0, 0.0]])
    t0 = np.array([0.0, 0.0, 1.5, 0.0, 3.0, 0.0])
    t1 = np.array([60 * 2 * np.pi, 0.5, 1.5, 1.0, 1.0, -2.0])          # long, short, zero-length, short, backward, backward
    d = ivp_amd.solve_ivp_batch_dense(ivp_amd.SHO(), torch.as_tensor(t0, device=DEV), torch.as_tensor(t1, device=DEV),
                                      torch.as_tensor(y0, device=DEV), None, ivp_amd.Options(**opts))
    ns = d.n_seg.cpu().numpy()
    assert np.array_equal(np.diff(d.seg_offsets.cpu().numpy()), ns) and ns[0] > 20 * ns[1]
    for b in range(B):
        s = ivp_amd.solve_ivp(ivp_amd.SHO(), float(t0[b]), float(t1[b]), y0[:, b], ivp_amd.Options(dense_output=True, **opts))
        cs, co = s.continuous_sol, d.dense.of(b)
        assert len(co.h) == len(cs.h) == ns[b], b
        assert np.array_equal(_bits(co.cont), _bits(cs.cont)) and np.array_equal(_bits(co.xold), _bits(cs.xold)) and np.array_equal(_bits(co.h), _bits(cs.h)), b
    assert ns[2] == 1 and float(d.seg_h[int(d.seg_offsets[2])]) == 1e-15     # ContinuousOutput::constant
    assert float(d.seg_h[int(d.seg_offsets[4])]) < 0.0
    start, end = d.dense.t_span()
    assert float(start[4]) == 3.0 and abs(float(end[4]) - 1.0) < 1e-12


def _queries(co, rng):
    """every step boundary of up to 24 segments (exactly, +0.5e-12 inside the tolerance, -2e-12 outside it), random
    interior points, before the start and past the end"""
    ends = np.concatenate([co.xold, co.xold + co.h])
    lo, hi = float(np.min(ends)), float(np.max(ends))
    pick = rng.choice(len(co.h), size=min(24, len(co.h)), replace=False)
    e = np.concatenate([co.xold[pick], co.xold[pick] + co.h[pick], [co.xold[0], co.xold[-1] + co.h[-1]]])
    return np.concatenate([e, e + 0.5e-12, e - 2e-12, rng.uniform(lo, hi, 48), [lo - 1.0, hi + 1.0]])


@pytest.mark.parametrize("method", list(CFG))
def test_device_eval_equals_the_host_continuous_output(method):
    B = 6
    f, y0, p, t0, t1 = _problem("vdp", B)
    t1 = np.minimum(t1, 20.0)
    d = ivp_amd.solve_ivp_batch_dense(f, t0, t1, torch.as_tensor(y0, device=DEV), torch.as_tensor(p, device=DEV),
                                      ivp_amd.Options(method=method, rtol=1e-6, atol=1e-9, **CFG[method]))
    _eval_equals_host(d, B, 25.0)


def _eval_equals_host(d, B, t_hi):
    n = d.dense.n_states
    rng = np.random.default_rng(3)
    cos = [d.dense.of(b) for b in range(B)]
    grids = [_queries(co, rng) for co in cos]
    for ex in (False, True):
        y, found = d.dense(grids, extrapolate=ex)
        y, found = y.cpu().numpy(), found.cpu().numpy()
        q = 0
        for b in range(B):
            co = cos[b]
            for t in grids[b]:
                want = co.evaluate_extrapolate(float(t)) if ex else co.evaluate(float(t))
                if want is None:
                    assert found[q] == 0 and np.isnan(y[q]).all()
                else:
                    assert found[q] == (1 if co.evaluate(float(t)) is not None else 2)
                    assert np.array_equal(_bits(y[q]), _bits(want)), (b, t)
                q += 1
    # the shared-grid form: the same values in the SoA layout [m][n][B]
    g = np.linspace(-1.0, t_hi, 97)
    ys, fs = d.dense(g)
    yc, fc = d.dense([g] * B)
    assert np.array_equal(_bits(ys.cpu().numpy().transpose(2, 0, 1).reshape(-1, n)), _bits(yc.cpu().numpy()))
    assert np.array_equal(fs.cpu().numpy().T.reshape(-1), fc.cpu().numpy())


@pytest.mark.parametrize("fp", ["strict", "fma"])
def test_device_eval_equals_the_solves_t_eval_samples_off_the_boundaries(fp):
    f, y0, p, t0, t1 = _problem("cr3bp", 256)
    grid = np.linspace(0.0, float(t1), 257)
    fpm = ivp_amd.FpMode.FMA if fp == "fma" else ivp_amd.FpMode.STRICT
    d = ivp_amd.solve_ivp_batch_dense(f, t0, t1, torch.as_tensor(y0, device=DEV), torch.as_tensor(p, device=DEV),
                                      ivp_amd.Options(method="DOPRI5", rtol=1e-7, atol=1e-10, fp_mode=fpm, t_eval=list(grid)))
    assert np.array_equal(d.n_filled.cpu().numpy(), np.full(256, 257))
    y, found = d.dense(grid)
    y, found = y.cpu().numpy(), found.cpu().numpy()
    assert (found == 1).all()
    ye = d.y_eval.cpu().numpy()[:257]
    off = d.seg_offsets.cpu().numpy()
    xo, hh = d.seg_xold.cpu().numpy(), d.seg_h.cpu().numpy()
    checked = 0
    for b in range(256):
        ends = np.concatenate([xo[off[b]:off[b + 1]], xo[off[b]:off[b + 1]] + hh[off[b]:off[b + 1]]])
        near = np.min(np.abs(grid[:, None] - ends[None, :]), axis=1) <= 1e-12
        k = ~near
        assert np.array_equal(_bits(y[k, :, b]), _bits(ye[k, :, b])), b
        checked += int(k.sum())
    assert checked > 0.9 * 256 * 257


# ---- the oracle, a hiprtc system, wide and odd-width evaluation, the host entry point, caller buffers, trajectory ranges ----
import ctypes as C  # noqa: E402

from ivp_amd import _lib  # noqa: E402
from ivp_amd import api as A  # noqa: E402
from oracle import oracle as O  # noqa: E402


def test_c2_segments_equal_the_oracle():
    """200 sampled BASELINE C2 trajectories: the CSR runs equal the reference restatement's (detpow) segments"""
    y0, p, t0, t1 = W.cr3bp_batch(100_000)
    d = ivp_amd.solve_ivp_batch_dense(ivp_amd.CR3BP(), t0, t1, torch.as_tensor(y0, device=DEV), torch.as_tensor(p, device=DEV),
                                      ivp_amd.Options(method="DOPRI5", rtol=1e-6, atol=1e-9))
    off = d.seg_offsets.cpu().numpy()
    for b in np.random.default_rng(5).choice(100_000, 200, replace=False):
        o = O.solve_ivp("cr3bp", t0, t1, y0[:, b], params=list(p[:, b]), method="DOPRI5", rtol=1e-6, atol=1e-9, detpow=True,
                        dense_output=True)
        lo, hi = int(off[b]), int(off[b + 1])
        assert hi - lo == len(o.seg_h), b
        assert np.array_equal(_bits(d.seg_cont[lo:hi].cpu().numpy()), _bits(o.seg_cont)), b
        assert np.array_equal(_bits(d.seg_xold[lo:hi].cpu().numpy()), _bits(o.seg_xold)), b
        assert np.array_equal(_bits(d.seg_h[lo:hi].cpu().numpy()), _bits(o.seg_h)), b


def test_csr_segments_hiprtc_system():
    src = "__device__ void ode(double x, const double* y, double* dydx, const double* p) { dydx[0] = y[1]; dydx[1] = -p[0] * y[0] - 0.1 * y[1]; }"
    f = ivp_amd.DeviceIVP(src, 2, params=(1.7,))
    y0 = np.random.default_rng(9).standard_normal((2, 64))
    _dense_vs_bounded(f, y0, None, 0.0, 10.0, method="DOPRI5", rtol=1e-7, atol=1e-10)
    _dense_vs_bounded(f, y0, None, 0.0, 10.0, method="DOP853", rtol=1e-7, atol=1e-10, variant=3)


@pytest.mark.parametrize("f,method,B,t1", [(ivp_amd.LinearDecay100(), "DOPRI5", 3, 1.0), (ivp_amd.LinearDecay100(), "BDF", 2, 1.0),
                                           (ivp_amd.Lorenz(), "DOPRI5", 4, 2.0), (ivp_amd.ExponentialDecay(), "DOPRI5", 4, 3.0)],
                         ids=["n100-dopri5", "n100-bdf", "lorenz-n3-odd", "decay-n1-odd"])
def test_device_eval_equals_the_host_wide_and_odd_systems(f, method, B, t1):
    """n > 8: one wavefront per query (lane-0 search, broadcast); ncoef n odd: the scalar-load path"""
    y0 = 1.0 + 0.1 * np.random.default_rng(21).standard_normal((f.n, B))
    d = ivp_amd.solve_ivp_batch_dense(f, 0.0, t1, torch.as_tensor(y0, device=DEV), None, ivp_amd.Options(method=method, rtol=1e-6, atol=1e-9))
    _eval_equals_host(d, B, t1 + 1.0)


def _host_form(f, y0, p, t0, t1, opts, alias=False):
    """ivp_batch_solve_dense (host pointers throughout, library-owned host log); alias: y_end is written over (a private
    copy of) y0"""
    L, ctx = _lib.load(), ivp_amd.default_context(0)
    keep = []
    copt = opts._c(f.n, keep)
    B = y0.shape[1]
    y0 = np.array(y0, dtype=np.float64, order="C") if alias else np.ascontiguousarray(y0, dtype=np.float64)
    p = None if p is None else np.ascontiguousarray(p, dtype=np.float64)
    y_end, n_seg = y0 if alias else np.zeros((f.n, B)), np.zeros(B, np.uint32)
    r = _lib.BatchResultT()
    r.y_end, r.n_seg = y_end.ctypes.data, n_seg.ctypes.data
    off = np.zeros(B + 1, np.uint64)
    dl = _lib.DenseLogT()
    dl.offsets = off.ctypes.data
    t0a, t1a = np.atleast_1d(np.asarray(t0, np.float64)), np.atleast_1d(np.asarray(t1, np.float64))
    prob = A._problem_c(f)
    rc = L.ivp_batch_solve_dense(ctx.handle, C.byref(prob), B, y0.ctypes.data, None if p is None else p.ctypes.data, t0a.ctypes.data, len(t0a),
                                 t1a.ctypes.data, len(t1a), C.byref(copt), C.byref(r), C.byref(dl))
    assert rc == 0, ctx.last_error()
    total, nc = int(dl.total), int(dl.ncoef_n)
    assert dl.owned == 1 and dl.device == -1 and int(off[-1]) == total
    get = lambda ptr, k: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(k,)).copy()
    out = off, get(dl.cont, total * nc).reshape(total, nc), get(dl.xold, total), get(dl.h, total), n_seg, y_end, int(dl.passes), int(dl.staging_bytes)
    L.ivp_dense_log_free(C.byref(dl))
    return out


def _equals_the_device_form(got, d):
    """offsets, cont, xold, h, n_seg and y_end of a C ABI call against solve_ivp_batch_dense's, bit for bit"""
    off, cont, xold, h, ns, y_end = got
    assert np.array_equal(off.astype(np.int64), d.seg_offsets.cpu().numpy()) and np.array_equal(ns, d.n_seg.cpu().numpy().astype(np.uint32))
    assert np.array_equal(_bits(cont), _bits(d.seg_cont.cpu().numpy())) and np.array_equal(_bits(xold), _bits(d.seg_xold.cpu().numpy()))
    assert np.array_equal(_bits(h), _bits(d.seg_h.cpu().numpy())) and np.array_equal(_bits(y_end), _bits(d.y_end.cpu().numpy()))


@pytest.mark.parametrize("max_log", [0, 4096], ids=["filling-solve-on-the-device", "from-the-counting-block"])
def test_host_entry_point_equals_the_device_form(max_log):
    f, y0, p, t0, t1 = _problem("cr3bp", 48)
    opts = ivp_amd.Options(method="DOPRI5", rtol=1e-6, atol=1e-9, max_log=max_log)
    *got, passes, _ = _host_form(f, y0, p, t0, t1, opts)
    assert passes == (2 if max_log == 0 else 1)
    d = ivp_amd.solve_ivp_batch_dense(f, t0, t1, torch.as_tensor(y0, device=DEV), torch.as_tensor(p, device=DEV), opts)
    _equals_the_device_form(got, d)


def test_y_end_aliased_onto_y0_the_filling_solve_still_starts_from_y0():
    """out.y_end == y0 with max_log = 0 (the counting solve writes the end state over y0, then a filling solve has to
    run): host form and device form against the device form that does not alias"""
    f, y0, p, t0, t1 = _problem("cr3bp", 48)
    B = 48
    opts = ivp_amd.Options(method="DOPRI5", rtol=1e-6, atol=1e-9, max_log=0)
    d = ivp_amd.solve_ivp_batch_dense(f, t0, t1, torch.as_tensor(y0, device=DEV), torch.as_tensor(p, device=DEV), opts)
    assert d.dense_info["passes"] == 2
    *got, passes, _ = _host_form(f, y0, p, t0, t1, opts, alias=True)
    assert passes == 2
    _equals_the_device_form(got, d)
    # the device entry point, out.y_end pointing at the y0 tensor; the log goes to buffers of exactly `total` records
    total, nc = d.dense_info["segments"], int(d.seg_cont.shape[1])
    L, ctx = _lib.load(), ivp_amd.default_context(0)
    keep = []
    copt = opts._c(f.n, keep)
    prob = A._problem_c(f)
    y0d, pd = torch.as_tensor(y0, device=DEV).clone(), torch.as_tensor(p, device=DEV)
    t0d = torch.as_tensor(np.atleast_1d(np.asarray(t0, np.float64)), device=DEV)
    t1d = torch.as_tensor(np.atleast_1d(np.asarray(t1, np.float64)), device=DEV)
    off = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    cont = torch.zeros((total, nc), dtype=torch.float64, device=DEV)
    xold, h = torch.zeros(total, dtype=torch.float64, device=DEV), torch.zeros(total, dtype=torch.float64, device=DEV)
    n_seg = torch.zeros(B, dtype=torch.int32, device=DEV)
    dl = _lib.DenseLogT()
    dl.offsets, dl.cont, dl.xold, dl.h, dl.capacity = off.data_ptr(), cont.data_ptr(), xold.data_ptr(), h.data_ptr(), total
    r = _lib.BatchResultT()
    r.y_end, r.n_seg = y0d.data_ptr(), n_seg.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rc = L.ivp_batch_solve_dense_device(ctx.handle, C.byref(prob), B, y0d.data_ptr(), pd.data_ptr(), t0d.data_ptr(), len(t0d), t1d.data_ptr(), len(t1d),
                                        C.byref(copt), C.byref(r), C.byref(dl), stream)
    assert rc == 0, ctx.last_error()
    assert dl.passes == 2 and dl.owned == 0 and int(dl.total) == total
    _equals_the_device_form((off.cpu().numpy(), cont.cpu().numpy(), xold.cpu().numpy(), h.cpu().numpy(), n_seg.cpu().numpy().astype(np.uint32),
                             y0d.cpu().numpy()), d)


def test_host_entry_point_under_a_staging_cap_runs_trajectory_ranges(monkeypatch):
    """IVP_DENSE_STAGING_BYTES below one whole-batch block: the host-pointer form's filling solve runs over more than one
    range, same log"""
    f, y0, p, t0, t1 = _problem("cr3bp", 48)
    opts = ivp_amd.Options(method="DOPRI5", rtol=1e-6, atol=1e-9, max_log=0)
    *whole, passes, staging = _host_form(f, y0, p, t0, t1, opts)
    nc = whole[1].shape[1]
    assert passes == 2 and staging == int(whole[4].max()) * (nc + 2) * 8 * 48    # one range: [max n_seg][ncoef n + 2] doubles x 48
    cap = staging // 3                                                           # 16 trajectories' worth of the deepest block
    monkeypatch.setenv("IVP_DENSE_STAGING_BYTES", str(cap))
    *split, passes, sb = _host_form(f, y0, p, t0, t1, opts)
    assert passes == 2 and 0 < sb <= cap
    for a, b in zip(split, whole):
        assert np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)


def test_caller_buffers_too_small_report_the_total_then_fill():
    f, y0, p, t0, t1 = _problem("vdp", 32)
    ref = ivp_amd.solve_ivp_batch_dense(f, t0, t1, torch.as_tensor(y0, device=DEV), torch.as_tensor(p, device=DEV),
                                        ivp_amd.Options(method="DOPRI5", rtol=1e-6, atol=1e-9))
    total, nc = ref.dense_info["segments"], int(ref.seg_cont.shape[1])
    L, ctx = _lib.load(), ivp_amd.default_context(0)
    keep = []
    copt = ivp_amd.Options(method="DOPRI5", rtol=1e-6, atol=1e-9)._c(2, keep)
    prob = A._problem_c(f)
    y0d, pd = torch.as_tensor(y0, device=DEV), torch.as_tensor(p, device=DEV)
    t0d, t1d = torch.as_tensor(np.atleast_1d(np.float64(t0)), device=DEV), torch.as_tensor(np.asarray(t1, np.float64), device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for cap in (total - 1, total):
        off = torch.zeros(33, dtype=torch.int64, device=DEV)
        cont = torch.zeros((cap, nc), dtype=torch.float64, device=DEV)
        xold, h = torch.zeros(cap, dtype=torch.float64, device=DEV), torch.zeros(cap, dtype=torch.float64, device=DEV)
        dl = _lib.DenseLogT()
        dl.offsets, dl.cont, dl.xold, dl.h, dl.capacity = off.data_ptr(), cont.data_ptr(), xold.data_ptr(), h.data_ptr(), cap
        r = _lib.BatchResultT()
        rc = L.ivp_batch_solve_dense_device(ctx.handle, C.byref(prob), 32, y0d.data_ptr(), pd.data_ptr(), t0d.data_ptr(), 1, t1d.data_ptr(), 32,
                                            C.byref(copt), C.byref(r), C.byref(dl), stream)
        assert int(dl.total) == total and dl.owned == 0
        assert np.array_equal(off.cpu().numpy(), ref.seg_offsets.cpu().numpy())
        if cap < total:
            assert rc == -105 and "hold" in ctx.last_error()
        else:
            assert rc == 0, ctx.last_error()
            assert np.array_equal(_bits(cont.cpu().numpy()), _bits(ref.seg_cont.cpu().numpy()))
            assert np.array_equal(_bits(xold.cpu().numpy()), _bits(ref.seg_xold.cpu().numpy()))
            assert np.array_equal(_bits(h.cpu().numpy()), _bits(ref.seg_h.cpu().numpy()))


def test_filling_solve_split_into_trajectory_ranges(monkeypatch):
    """a staging cap (IVP_DENSE_STAGING_BYTES) below one block: the filling solve runs over trajectory ranges (sliced
    y0 / params / per-trajectory t1), same segments"""
    f, y0, p, t0, t1 = _problem("vdp", 300)
    whole, _ = _dense_vs_bounded(f, y0, p, t0, t1, method="DOPRI5", rtol=1e-6, atol=1e-9)
    cap = whole.dense_info["staging_bytes"] // 5
    monkeypatch.setenv("IVP_DENSE_STAGING_BYTES", str(cap))
    d, _ = _dense_vs_bounded(f, y0, p, t0, t1, method="DOPRI5", rtol=1e-6, atol=1e-9)
    assert d.dense_info["passes"] == 2 and 0 < d.dense_info["staging_bytes"] <= cap
    for k in ("seg_cont", "seg_xold", "seg_h", "seg_offsets"):
        assert np.array_equal(getattr(d, k).cpu().numpy(), getattr(whole, k).cpu().numpy()), k
