"""The wave-per-trajectory RK kernels (rk_group.h) at every lane slice C = ceil(n / G) and every group width G, in both
arithmetic modes, bit for bit against the oracle.

The group kernels are templates over G (16, 32 or 64 lanes per trajectory) and C (1..8 components per lane).  A wrong
`i < n` guard, a wrong `lane + G c` index or state of slot c that does not survive a launch boundary is invisible at C = 1
and wherever no slot is ragged; a butterfly that leaves its group is invisible at G = 64.  The system of tests/group_cases.py
(a ring with per-component decay rates) runs here at

    WIDE   65 128 129 192 257 320 383 385 449 511 512   C = 2, 2, 3, 3, 5, 5, 6, 7, 8, 8, 8: one lane in the top slot (65, 129,
                                                        257, 385, 449), one lane short (383, 511), full (128, 192, 320, 512)
    SMALL  9 16 17 32 33                                G = 16 | 32 | 64 on both sides of each switch, 11 trajectories per batch

STRICT is compared with the oracle's portable-pow build, FMA with its FMA build (fused multiply-add sites and the
lane-partial + butterfly norm of the kernels restated, oracle/ivp_oracle.c orc_sum), per trajectory through the numpy twin
of the device snippet.  One test runs both modes of one (n, method), so a failure names the width.  What the references have
to be for this to mean something (rejected steps, several launches per trajectory, FMA bits that differ from the strict
ones, events that occur) is asserted by tests/test_group_cases_cpu.py."""
import warnings

import numpy as np
import pytest
import torch

import ivp_amd
from tests import group_cases as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = (("strict", ivp_amd.FpMode.STRICT, False), ("fma", ivp_amd.FpMode.FMA, True))


def _same(a, b):
    """bit equality of two float64 arrays (NaN equals NaN: the payload is the hardware's)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _problem(n, events=()):
    src, _, ev_src, _ = G.ring(n)
    return ivp_amd.DeviceIVP(src + (ev_src if events else ""), n=n, params=(40.0,), events=list(events))


def _end_state_equals(r, refs, what):
    """y_end, t_end, h_next, status and the counters of every trajectory against its oracle run.  A trajectory that a
    terminal event ended is the exception: y_end / t_end are the integrator's state after its last step, which a Solution
    does not carry (its last record is the event); its event records, status, counters and h_next are compared."""
    y_end, t_end, h_next = _np(r.y_end), _np(r.t_end), _np(r.h_next)
    for b, o in enumerate(refs):
        assert int(_np(r.status)[b]) == int(o.status), (what, b, "status")
        got = tuple(int(_np(getattr(r, k))[b]) for k in ("naccpt", "nrejct", "nfev", "nstep"))
        assert got == (o.naccpt, o.nrejct, o.nfev, o.nstep), (what, b, got, (o.naccpt, o.nrejct, o.nfev, o.nstep))
        assert _same(h_next[b], o.h_next), (what, b, h_next[b], o.h_next)
        if int(o.status) == 1:
            continue
        assert _same(y_end[:, b], o.y[-1]), (what, b, "y_end", int(np.count_nonzero(y_end[:, b] != o.y[-1])))
        assert _same(t_end[b], o.t[-1]), (what, b, t_end[b], o.t[-1])


# ---- a. end state and counters ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,method", G.end_state_pairs())
def test_end_state_and_counters_equal_the_oracle_in_both_modes(n, method):
    """chunk_attempts = 7: every slot of every per-lane array crosses at least two launch boundaries through the SoA state
    (test_group_cases_cpu: more than 14 attempts per trajectory); the two widest one-lane and full top slots also in one
    launch.  The batch holds a backward run, a zero-length interval and couplings that make the trajectories of one
    wavefront (n <= 32) take different numbers of steps."""
    f = _problem(n)
    y0, p, t0, t1 = G.method_batch(n, method)
    for name, fp, fma in MODES:
        refs = G.references(n, method, fma)
        for chunk in (G.CHUNK, 0) if n in (449, 512) else (G.CHUNK,):
            r = ivp_amd.solve_ivp_batch(f, t0, t1, y0, p, ivp_amd.Options(fp_mode=fp, chunk_attempts=chunk, **G.method_options(method)))
            _end_state_equals(r, refs, f"n = {n} {method} {name} chunk {chunk}")


# ---- b. the full device DefaultSolOut -------------------------------------------------------------------------------------
T_EVAL = tuple(np.concatenate([[-0.25, -0.04, -0.02], np.linspace(0.0, 2.0, 21), [2.5]]))     # both ends lie outside every span
OUTPUT_METHODS = ["RK23", "DOPRI5", "DOP853"]


@pytest.mark.parametrize("method", OUTPUT_METHODS)
@pytest.mark.parametrize("n", G.OUTPUT_WIDTHS)
def test_t_eval_samples_equal_the_oracle_in_both_modes(n, method):
    """t_eval samples (the interpolant evaluated inside the stepping kernel, per lane slice) of a shared grid that starts
    before t0 and ends past every t1; the backward run and the zero-length interval take what the reference gives them."""
    f = _problem(n)
    y0, p, t0, t1 = G.method_batch(n, method)
    te = np.array(T_EVAL)
    for name, fp, fma in MODES:
        refs = G.references(n, method, fma, t_eval=T_EVAL)
        r = ivp_amd.solve_ivp_batch(f, t0, t1, y0, p, ivp_amd.Options(fp_mode=fp, chunk_attempts=G.CHUNK, t_eval=list(T_EVAL), **G.method_options(method)))
        _end_state_equals(r, G.references(n, method, fma, dense=True), f"t_eval n = {n} {method} {name}")    # sampling changes no step
        assert max(len(o.t) for o in refs) >= 10
        for b, o in enumerate(refs):
            m = int(r.n_filled[b])
            assert m == len(o.t), (name, b, m, len(o.t))
            assert _same(te[r.eval_idx[:m, b]], o.t) and _same(r.y_eval[:m, :, b], o.y), (name, b)


@pytest.mark.parametrize("method", OUTPUT_METHODS)
@pytest.mark.parametrize("n", G.OUTPUT_WIDTHS)
def test_step_log_and_dense_segments_equal_the_oracle_in_both_modes(n, method):
    """Solution.t / Solution.y and the ContinuousOutput of every trajectory through four mechanisms: the bounded step log
    and dense segments of solve_ivp_batch (max_log above the reference's largest count), the one-pass CSR step log
    (the log-only kernel flavour, the wide-record path of the gather), the CSR dense log, and its evaluation on the device
    (n > 64 * 7: eight trips of the wave's `c += 64` loop) at both ends of every span and inside it -- strict against the
    strict oracle's interpolant, FMA against the FMA oracle's fused one."""
    f = _problem(n)
    y0, p, t0, t1 = G.method_batch(n, method)
    B = y0.shape[1]
    y0d, pd, t1d = (torch.as_tensor(np.ascontiguousarray(a), device=DEV) for a in (y0, p, t1))
    opts = G.method_options(method)
    for name, fp, fma in MODES:
        refs = G.references(n, method, fma, dense=True)
        ml = max(len(o.t) for o in refs) + 3
        what = f"n = {n} {method} {name}"
        # bounded layout [max_log][.][B]
        r = ivp_amd.solve_ivp_batch(f, t0, t1, y0, p, ivp_amd.Options(fp_mode=fp, chunk_attempts=G.CHUNK, dense_output=True, max_log=ml, **opts))
        _end_state_equals(r, refs, what + " bounded")
        for b, o in enumerate(refs):
            k, s = int(r.n_log[b]), int(r.n_seg[b])
            assert (k, s) == (len(o.t), len(o.seg_h)), (what, b, k, s, len(o.t), len(o.seg_h))
            assert _same(r.t_log[:k, b], o.t) and _same(r.y_log[:k, :, b], o.y), (what, b, "step log")
            assert _same(r.seg_xold[:s, b], o.seg_xold) and _same(r.seg_h[:s, b], o.seg_h), (what, b, "segment spans")
            assert _same(r.seg_cont[:s, :, b], o.seg_cont), (what, b, "segment coefficients")
        # one-pass CSR step log
        lg = ivp_amd.solve_ivp_batch_logged(f, t0, t1d, y0d, pd, ivp_amd.Options(fp_mode=fp, chunk_attempts=G.CHUNK, **opts))
        assert lg.log_info["passes"] == 1, lg.log_info
        _end_state_equals(lg, refs, what + " logged")
        off, tl, yl = _np(lg.log_offsets), _np(lg.t_log), _np(lg.y_log)
        assert off[0] == 0 and int(off[-1]) == tl.shape[0]
        for b, o in enumerate(refs):
            lo, hi = int(off[b]), int(off[b + 1])
            assert hi - lo == len(o.t), (what, b, hi - lo, len(o.t))
            assert _same(tl[lo:hi], o.t) and _same(yl[lo:hi], o.y), (what, b, "CSR step log")
        # CSR dense log and its evaluation on the device
        d = ivp_amd.solve_ivp_batch_dense(f, t0, t1d, y0d, pd, ivp_amd.Options(fp_mode=fp, chunk_attempts=G.CHUNK, **opts))
        _end_state_equals(d, refs, what + " dense")
        off, sc, sx, sh = _np(d.seg_offsets), _np(d.seg_cont), _np(d.seg_xold), _np(d.seg_h)
        grids = []
        for b, o in enumerate(refs):
            lo, hi = int(off[b]), int(off[b + 1])
            assert hi - lo == len(o.seg_h), (what, b, hi - lo, len(o.seg_h))
            assert _same(sx[lo:hi], o.seg_xold) and _same(sh[lo:hi], o.seg_h) and _same(sc[lo:hi], o.seg_cont), (what, b, "CSR segments")
            start, end = o.sol_span()
            grids.append(np.array([start] + [start + w * (end - start) for w in (0.013, 0.37, 0.5, 0.77, 0.9991)] + [end]))
        y, found = d.dense(grids)
        y, found = _np(y), _np(found)
        assert y.shape == (7 * B, n) and (found == 1).all(), (what, found)
        for b, o in enumerate(refs):
            for q, tq in enumerate(grids[b]):
                assert _same(y[7 * b + q], o.sol(float(tq))), (what, b, q, float(tq))


# ---- c. events ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["DOPRI5", "DOP853"])
@pytest.mark.parametrize("n", G.EVENT_WIDTHS)
def test_events_equal_the_oracle_in_both_modes(n, method):
    """Two event functions that see the whole state (the LDS copy; g[0] reads across the ragged top slot): the first ends a
    trajectory at its 2nd occurrence, the second counts in the negative direction only.  t_events, y_events, status and
    counters of the bounded form against the oracle; the CSR form (solve_ivp_batch_events) against the same runs.  With
    DOP853's eight dense coefficients per component at n = 512 this is the largest LDS footprint a group kernel has."""
    cfgs = [ivp_amd.EventConfig(ivp_amd.Direction(d), t or None) for d, t in zip(G.EVENT_DIRECTION, G.EVENT_TERMINAL)]
    f = _problem(n, cfgs)
    y0, p, t0, t1 = G.event_batch(n)
    B = y0.shape[1]
    y0d, pd, t1d = (torch.as_tensor(np.ascontiguousarray(a), device=DEV) for a in (y0, p, t1))
    for name, fp, fma in MODES:
        refs = G.event_references(n, method, fma)
        what = f"n = {n} {method} {name}"
        opt = ivp_amd.Options(fp_mode=fp, chunk_attempts=G.CHUNK, max_events=8, **G.method_options(method))
        with warnings.catch_warnings():
            warnings.simplefilter("error")                 # no event buffer may overflow
            r = ivp_amd.solve_ivp_batch(f, t0, t1, y0, p, opt)
            e = ivp_amd.solve_ivp_batch_events(f, t0, t1d, y0d, pd, opt)
        _end_state_equals(r, refs, what + " bounded")
        _end_state_equals(e, refs, what + " CSR")
        assert _same(_np(e.y_end), r.y_end) and _same(_np(e.t_end), r.t_end)          # the terminated trajectories included
        # a terminated trajectory's last step reaches past its event, by less than the step the controller proposes next
        for b, o in enumerate(refs):
            if int(o.status) == 1:
                assert o.t_events[0][-1] <= r.t_end[b] < G.EVENT_T1, (what, b, r.t_end[b])
        off, te, ye, hits = _np(e.event_offsets), _np(e.t_events_csr), _np(e.y_events_csr), _np(e.n_event_hits)
        assert off[0] == 0 and int(off[-1]) == te.shape[0] == e.event_info["total"]
        for b, o in enumerate(refs):
            for i in range(2):
                k = int(r.n_event_hits[i, b])
                assert k == len(o.t_events[i]) == int(hits[i, b]), (what, b, i, k, len(o.t_events[i]))
                assert _same(r.t_events[i, :k, b], o.t_events[i]) and _same(r.y_events[i, :k, :, b], o.y_events[i]), (what, b, i)
                lo, hi = int(off[i * B + b]), int(off[i * B + b + 1])
                assert hi - lo == k and _same(te[lo:hi], o.t_events[i]) and _same(ye[lo:hi], o.y_events[i]), (what, b, i, "CSR")


# ---- d. limits ------------------------------------------------------------------------------------------------------------
def test_a_system_wider_than_the_group_kernels_is_refused():
    """n = 513 would need a ninth component per lane: IVP_ERR_BAD_ARGUMENT when the problem is compiled, no kernel built"""
    src, _, _, _ = G.ring(513)
    with pytest.raises(ivp_amd.ConfigError) as e:
        ivp_amd.DeviceIVP(src, n=513, params=(40.0,))
    assert e.value.code == -100
