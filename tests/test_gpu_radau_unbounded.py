"""The direct Radau call without a bound to guess and without blocking: Radau.solve_batch_logged (ivp_radau_solve_logged_device:
the page sink of radau_core.h / radau_group.h and the gather), Radau.solve_batch_dense (ivp_radau_solve_dense_device: counting
solve, scan, packing or filling solves) and Radau.solve_batch(wait=False) (ivp_radau_submit_device), against
tests/radau_model.py and tests/radau_dae_model.py BIT FOR BIT: offsets, every record, every segment, the end state and the
counters.  No tolerance anywhere.

What the models do not have is the early return of solve_ivp for a zero-length interval (solve_ivp.rs:110-145: one record
[t0, y0], one constant segment [y0, 0, 0, 0] with h = 1e-15, status 0 and zero counters): `zero_length()` writes that result
down.  Model runs are cached per input and shared between the tests.
"""
import ctypes as C
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import ConfigError, Options, Radau
from ivp_amd.pipeline import BatchPipeline
from tests import radau_dae_model as D
from tests import radau_model as M
from tests import test_gpu_radau_dae as DAE
from tests import test_gpu_radau_group as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tests", "helpers", "radau_logged_dump.py")
MEMBERS = ("status", "t_end", "h_next", "nfev", "njev", "nlu", "nstep", "naccpt", "nrejct")
END = MEMBERS + ("y_end",)

_CACHE = {}


def model(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64)), device=DEV)


def cols(rows):
    return np.array(rows, dtype=np.float64).T.copy()


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def same(a, b):
    a, b = float(a), float(b)
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def same_vec(a, b):
    return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))


_byref = C.byref


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _result(B, n):
    """a BatchResultT with the end-state members, and the tensors that own them"""
    t = dict(y_end=torch.zeros((n, B), dtype=torch.float64, device=DEV), t_end=torch.zeros(B, dtype=torch.float64, device=DEV),
             status=torch.zeros(B, dtype=torch.int32, device=DEV), h_next=torch.zeros(B, dtype=torch.float64, device=DEV))
    for k in ("nfev", "nstep", "naccpt", "nrejct", "njev", "nlu"):
        t[k] = torch.zeros(B, dtype=torch.int64, device=DEV)
    r = ivp_amd._lib.BatchResultT()
    for k, v in t.items():
        setattr(r, k, _ptr(v))
    return r, t


def zero_length(t0, y0):
    """what solve_ivp returns for t1 == t0 (module docstring)"""
    m = M.Result()
    m.status, m.t_end, m.h_next = 0, float(t0), 0.0
    m.nfev = m.njev = m.nlu = m.nstep = m.naccpt = m.nrejct = 0
    m.y_end = [float(v) for v in y0]
    m.t, m.y = [float(t0)], [list(m.y_end)]
    m.segs = [(list(m.y_end) + [0.0] * (3 * len(y0)), float(t0), 1e-15)]
    return m


def hold_end(r, models, what):
    bad = []
    for b, m in enumerate(models):
        g = {k: (float(_np(getattr(r, k))[b]) if k in ("t_end", "h_next") else int(_np(getattr(r, k))[b])) for k in MEMBERS}
        w = {k: getattr(m, k) for k in MEMBERS}
        y = [float(v) for v in _np(r.y_end)[:, b]]
        ok = all(g[k] == w[k] for k in MEMBERS if k not in ("t_end", "h_next")) and same(g["t_end"], w["t_end"]) and \
            same(g["h_next"], w["h_next"]) and same_vec(y, m.y_end)
        if not ok:
            bad.append((b, g, y, w, list(m.y_end)))
    assert not bad, f"{what}: {len(bad)} of {len(models)} trajectories differ from the model; first: {bad[0]}"


def hold_log(r, models, what):
    """offsets, n_log, t_log, y_log, the end state and the counters"""
    hold_end(r, models, what)
    off, t, y, cnt = _np(r.log_offsets), _np(r.t_log), _np(r.y_log), _np(r.n_log)
    want = np.concatenate([[0], np.cumsum([len(m.t) for m in models])])
    assert [int(v) for v in off] == [int(v) for v in want], (what, off, want)
    assert [int(v) for v in cnt] == [len(m.t) for m in models], what
    assert t.shape[0] == int(want[-1]) == y.shape[0] == r.log_info.get("records", t.shape[0]), what
    for b, m in enumerate(models):
        lo = int(off[b])
        assert same_vec(t[lo:lo + len(m.t)], m.t), (what, b, "t_log")
        for q in range(len(m.t)):
            assert same_vec(y[lo + q], m.y[q]), (what, b, q, "y_log")


def hold_dense(r, models, what):
    """offsets, n_seg, xold, h, cont against Result.segs, the end state and the counters"""
    hold_end(r, models, what)
    off, c, x, h, cnt = _np(r.seg_offsets), _np(r.seg_cont), _np(r.seg_xold), _np(r.seg_h), _np(r.n_seg)
    want = np.concatenate([[0], np.cumsum([len(m.segs) for m in models])])
    assert [int(v) for v in off] == [int(v) for v in want], (what, off, want)
    assert [int(v) for v in cnt] == [len(m.segs) for m in models], what
    assert c.shape[0] == int(want[-1]) == r.dense_info["segments"], what
    for b, m in enumerate(models):
        lo = int(off[b])
        for q, (cont, xold, hh) in enumerate(m.segs):
            assert same(x[lo + q], xold) and same(h[lo + q], hh) and same_vec(c[lo + q], cont), (what, b, q)


def hold_sol(r, models, what):
    """`sol` at 16 times per trajectory -- both ends, every kind of segment boundary, interior points -- against
    radau_model.interpolate on the segment ContinuousOutput::find_segment picks (the first that holds t within 1e-12)"""
    assert r.dense.method == ivp_amd.Method.RADAU
    grids = []
    for m in models:
        ends = [s[1] for s in m.segs] + [m.segs[-1][1] + m.segs[-1][2]]
        if len(ends) < 16:   # few segments (the zero-length trajectory has one): its ends and points between them
            lo, hi = ends[0], ends[-1]
            ends = sorted(set(ends + [lo + (hi - lo) * k / 15.0 for k in range(16)]))
        pick = sorted({int(round(k * (len(ends) - 1) / 7.0)) for k in range(8)})
        bounds = [ends[i] for i in pick]
        mids = [0.5 * (ends[i] + ends[min(i + 1, len(ends) - 1)]) for i in pick]
        g = (bounds + mids + [ends[0]] * 16)[:16]
        g[0], g[15] = ends[0], ends[-1]
        grids.append(np.array(g))
    y, found = r.dense(grids)
    y, found = _np(y), _np(found)
    assert y.shape[0] == 16 * len(models)
    for b, m in enumerate(models):
        for q, t in enumerate(grids[b]):
            seg = next(s for s in m.segs if min(s[1], s[1] + s[2]) - 1e-12 <= t <= max(s[1], s[1] + s[2]) + 1e-12)
            assert int(found[16 * b + q]) == 1 and same_vec(y[16 * b + q], M.interpolate(float(t), *seg)), (what, b, q, float(t))


# ---- inputs -----------------------------------------------------------------------------------------------------------
# Stiff Van der Pol at 1e-8 takes ~690 attempts per trajectory and Robertson at 1e-11 to t = 1e8 ~2000: with one trajectory
# per wavefront (what the launch policy gives a batch this small) a launch of 64 attempts draws an arena of four pages of
# 784 (n = 2) / 1040 (n = 3) doubles per wavefront, 170 K / 260 K doubles in all -- a pool of reserve = 1, 2^16 doubles, runs dry.
VDP_T1, VDP_RT, VDP_AT = 2.0, 1e-8, 1e-10
VDP_EPS = [1e-3 * (1.0 + 0.25 * b) for b in range(5)]
VDP_Y0 = [[2.0 + 0.01 * b, 0.05 * b] for b in range(5)]
ROB_T1, ROB_RT, ROB_AT = 1e8, 1e-11, 1e-15
ROB_Y0 = [[1.0, 0.0, 0.0], [0.9, 0.0, 0.1]]


def vdp_models(**kw):
    key = tuple(sorted((k, repr(v)) for k, v in kw.items()))
    return [model(("vdp", b, key), lambda b=b: M.solve(M.rhs_vdp_eps(VDP_EPS[b]), 0.0, VDP_T1, VDP_Y0[b], VDP_RT, VDP_AT, **kw)) for b in range(5)]


def rob_models(**kw):
    key = tuple(sorted((k, repr(v)) for k, v in kw.items()))
    return [model(("rob", b, key), lambda b=b: M.solve(M.rhs_robertson, 0.0, ROB_T1, ROB_Y0[b], ROB_RT, ROB_AT, **kw)) for b in range(2)]


def vdp_logged(ctx=None, **kw):
    return Radau().solve_batch_logged(ivp_amd.StiffVanDerPol(), 0.0, VDP_T1, dev(cols(VDP_Y0)), dev([VDP_EPS]), Options(rtol=VDP_RT, atol=VDP_AT), ctx, **kw)


def rob_logged(ctx=None, **kw):
    return Radau().solve_batch_logged(ivp_amd.Robertson(), 0.0, ROB_T1, dev(cols(ROB_Y0)), None, Options(rtol=ROB_RT, atol=ROB_AT), ctx, **kw)


# ---- 1. logged, thread form -------------------------------------------------------------------------------------------

def test_logged_thread_form_stiff_van_der_pol_and_robertson():
    for name, run, models in (("stiff VdP", vdp_logged, vdp_models()), ("Robertson", rob_logged, rob_models())):
        assert all(m.status == 0 and len(m.t) == m.naccpt + 1 > 64 for m in models)
        r = run()
        assert r.log_info["passes"] == 1 and 0 < r.log_info["pool_used_bytes"] <= r.log_info["pool_bytes"], r.log_info
        hold_log(r, models, name)
    assert len({len(m.t) for m in vdp_models()}) > 1   # the step counts differ: the offsets are not a multiple of one length


# ---- 2. the pool runs dry ---------------------------------------------------------------------------------------------

def test_a_pool_that_runs_dry_costs_a_second_integration_and_no_record():
    for name, run, models in (("stiff VdP", vdp_logged, vdp_models()), ("Robertson", rob_logged, rob_models())):
        ctx = ivp_amd.Context(0)   # its own pool: a context that has logged before keeps the larger one
        r = run(ctx, reserve=1)
        assert r.log_info["passes"] == 2, (name, r.log_info)
        hold_log(r, models, name + ", reserve = 1")
        nxt = run(ctx)             # the context has learnt the total
        assert nxt.log_info["passes"] == 1, (name, nxt.log_info)
        hold_log(nxt, models, name + ", after the dry pool")
        ctx.close()


def test_the_counted_two_pass_form_gives_the_same_log():
    hold_log(vdp_logged(two_pass=True), vdp_models(), "two_pass")


# ---- 3. the awkward records -------------------------------------------------------------------------------------------
AWK_EPS = 1e-3
AWK_Y0 = [[1.5, 0.25], [2.0, 0.0], [2.0, 0.0]]
AWK_T1 = [0.0, 2.0, 0.5]        # zero-length; stopped by max_steps; finishes, with first_step
AWK_KW = dict(max_steps=60, first_step=0.125)


def awkward_models(**kw):
    run = lambda b: M.solve(M.rhs_vdp_eps(AWK_EPS), 0.0, AWK_T1[b], AWK_Y0[b], 1e-6, 1e-8, **AWK_KW, **kw)
    key = tuple(sorted(kw))
    return [zero_length(0.0, AWK_Y0[0]), model(("awk", 1, key), lambda: run(1)), model(("awk", 2, key), lambda: run(2))]


def awkward_args():
    return (ivp_amd.StiffVanDerPol(), 0.0, dev(AWK_T1), dev(cols(AWK_Y0)), dev([[AWK_EPS] * 3]))


def records_twice(m, target):
    """the model's own evidence that one callback recorded twice: t[1] is the target x0 + first_step, and no accepted step ends
    there (within SolOut's 1e-12): it was interpolated in the callback that also recorded that step's end, t[2]"""
    return len(m.t) > 2 and m.t[1] == target and m.t[2] > target and all(abs((xo + hh) - target) > 1e-12 for _, xo, hh in m.segs)


def test_zero_length_interval_max_steps_exit_and_first_step_in_one_batch():
    models = awkward_models(dense_output=True)
    assert models[1].status == M.NEED_LARGER_NMAX and models[1].nstep == 61 and models[2].status == 0
    assert records_twice(models[2], 0.125) and records_twice(models[1], 0.125)
    assert len(models[2].t) < models[2].naccpt + 1   # the accepted steps before the target are not recorded
    for chunk in (0, 1, 7):
        r = Radau().solve_batch_logged(*awkward_args(), Options(rtol=1e-6, atol=1e-8, chunk_attempts=chunk, **AWK_KW))
        assert r.log_info["passes"] == 1
        hold_log(r, models, f"awkward records, chunk_attempts = {chunk}")


# ---- 4. page columns --------------------------------------------------------------------------------------------------

def decay_models(B):
    return [model(("decay", b), lambda b=b: M.solve(M.rhs_decay(0.5 + 0.75 * b), 0.0, 2.0, [1.0], 1e-6, 1e-8)) for b in range(B)]


@pytest.mark.parametrize("lpw,B", [(64, 70), (2, 5)])
def test_pages_with_many_columns_in_a_process_of_their_own(lpw, B, tmp_path):
    """IVP_TUNE_BDF_LPW is read once per process.  64 with B = 70: a full wavefront -- a page of 8 column groups -- and a page
    of 6 columns, trajectories longer than one page (16 attempts).  2 with B = 5: two full pages of two columns and one of one."""
    models = decay_models(B)
    attempts = [m.nstep + m.n_restart_real + m.n_restart_complex for m in models]
    assert max(attempts) > 16 and len(set(attempts)) > 4
    env = {k: v for k, v in os.environ.items() if not k.startswith("IVP_TUNE_")}
    env["IVP_TUNE_BDF_LPW"] = str(lpw)
    out = str(tmp_path / "log.npz")
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, HELPER, out, str(B)], env=env, capture_output=True, text=True)
    assert p.returncode == 0, f"child ended with status {p.returncode}\n{p.stdout[-1000:]}\n{p.stderr[-4000:]}"
    got = dict(np.load(out))
    assert int(got["passes"]) == 1
    hold_log(types.SimpleNamespace(log_info={"records": int(got["log_offsets"][-1])}, **got), models, f"IVP_TUNE_BDF_LPW = {lpw}, B = {B}")
    # the density took effect: one trajectory per wavefront counts exactly 64 sum(attempts) (tests/test_gpu_wave_density.py);
    # `lpw` per wavefront at most 64 max(attempts) per wavefront of the first launch
    slots, waves = int(got["slots"]), (B + lpw - 1) // lpw
    print(f"[radau unbounded] lpw {lpw} B {B}: lane_attempt_slots {slots}, 64 sum {64 * sum(attempts)}, 64 waves max {64 * waves * max(attempts)}")
    assert 64 * max(attempts) <= slots <= 64 * waves * max(attempts) and slots < 64 * sum(attempts)


# ---- 5. logged, group form --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,B,chunk", [(9, 5, 0), (17, 3, 0), (17, 3, 1), (17, 3, 7), (64, 2, 0)])
def test_logged_group_form(n, B, chunk):
    """n = 9: G = 16, four groups per wavefront and a wavefront with three absent groups; n = 17: G = 32; n = 64: G = 64"""
    y0s = G.lin_y0s(n, B)
    models = G.lin_models(n, y0s, True)
    assert all(m.status == 0 and len(m.t) > 16 for m in models)
    r = Radau().solve_batch_logged(G.lin_problem(n, True), 0.0, G.t1_of(n), dev(G.col(y0s)), None, Options(rtol=G.RT, atol=G.AT, chunk_attempts=chunk))
    assert r.log_info["passes"] == 1
    hold_log(r, models, f"n = {n}, chunk_attempts = {chunk}")


# ---- 6. logged and dense, DAE call ------------------------------------------------------------------------------------

def dae_cases():
    rt, at = [1e-6, 1e-5, 1e-6], [1e-10, 1e-12, 1e-9]
    y0p = [DAE.pend_y0(0.0), DAE.pend_y0(0.6435011087932844)]
    return [("Robertson, index 1", DAE.ROB_SRC, 3, Radau(), [[1.0, 0.0, 0.0]], 40.0, Options(rtol=rt, atol=at),
             lambda: DAE.models_of([D.rhs_robertson_dae], [D.MASS_ROBERTSON], [[1.0, 0.0, 0.0]], 0.0, 40.0, rtol=rt, atol=at, dense_output=True)),
            ("pendulum, index 2", DAE.PEND2_SRC, 5, Radau(nind1=4, nind2=1, nind3=0), y0p, 2.0, Options(rtol=1e-4, atol=1e-4),
             lambda: DAE.models_of([D.rhs_pendulum_index2] * 2, [D.MASS_PENDULUM] * 2, y0p, 0.0, 2.0, rtol=1e-4, atol=1e-4, nind=(4, 1, 0), dense_output=True))]


@pytest.mark.parametrize("which", [0, 1])
def test_logged_and_dense_through_the_dae_call(which):
    name, src, n, rad, y0s, t1, opt, run = dae_cases()[which]
    models = model(("dae", which), run)
    assert all(m.status == 0 and len(m.segs) == m.naccpt > 8 for m in models)
    prob = ivp_amd.DeviceIVP(src, n, mass=True)
    r = rad.solve_batch_logged(prob, 0.0, t1, dev(cols(y0s)), None, opt)
    assert r.log_info["passes"] == 1
    hold_log(r, models, name + ", logged")
    for ml in (0, 1 << 12):
        d = rad.solve_batch_dense(prob, 0.0, t1, dev(cols(y0s)), None, Options(**{**opt.__dict__, "max_log": ml}))
        assert d.dense_info["passes"] == (2 if ml == 0 else 1), d.dense_info
        hold_dense(d, models, f"{name}, dense, max_log = {ml}")
        hold_sol(d, models, f"{name}, sol, max_log = {ml}")


# ---- 7. dense CSR -----------------------------------------------------------------------------------------------------

def _dense_batches():
    """(name, problem, Radau, t0, t1, y0 columns, params, Options fields, models with segments)"""
    vdp = vdp_models(dense_output=True)
    awk = awkward_models(dense_output=True)
    y17 = G.lin_y0s(17, 3)
    return [("stiff VdP", ivp_amd.StiffVanDerPol(), 0.0, VDP_T1, cols(VDP_Y0), [VDP_EPS], dict(rtol=VDP_RT, atol=VDP_AT), vdp),
            ("Robertson", ivp_amd.Robertson(), 0.0, ROB_T1, cols(ROB_Y0), None, dict(rtol=ROB_RT, atol=ROB_AT), rob_models(dense_output=True)),
            ("awkward", ivp_amd.StiffVanDerPol(), 0.0, AWK_T1, cols(AWK_Y0), [[AWK_EPS] * 3], dict(rtol=1e-6, atol=1e-8, **AWK_KW), awk),
            ("n = 17", G.lin_problem(17, True), 0.0, G.t1_of(17), G.col(y17), None, dict(rtol=G.RT, atol=G.AT), G.lin_models(17, y17, True, dense_output=True))]


def _dense(case, max_log):
    name, prob, t0, t1, y0, par, okw, models = case
    t1d = dev(t1) if isinstance(t1, list) else t1
    return Radau().solve_batch_dense(prob, t0, t1d, dev(y0), dev(par), Options(max_log=max_log, **okw))


@pytest.mark.parametrize("which", [0, 1, 2, 3])
@pytest.mark.parametrize("max_log", [1 << 12, 1])
def test_dense_csr_segments_and_sol(which, max_log):
    case = _dense_batches()[which]
    models = case[-1]
    assert max(len(m.segs) for m in models) < (1 << 12) and max(len(m.segs) for m in models) > 1
    r = _dense(case, max_log)
    assert r.dense_info["passes"] == (1 if max_log > 1 else 2), r.dense_info
    hold_dense(r, models, f"{case[0]}, max_log = {max_log}")
    hold_sol(r, models, f"{case[0]}, max_log = {max_log}")
    if which == 2:   # the zero-length trajectory: the one constant segment [y, 0, 0, 0]
        lo, hi = int(r.seg_offsets[0]), int(r.seg_offsets[1])
        assert hi - lo == 1 and same_vec(_np(r.seg_cont)[lo], AWK_Y0[0] + [0.0] * 6) and same(_np(r.seg_h)[lo], 1e-15)


def test_dense_csr_fill_over_at_least_two_trajectory_ranges(monkeypatch):
    """IVP_DENSE_STAGING_BYTES (read per call) below the block of the whole batch: the fill takes one filling solve per range"""
    case = _dense_batches()[0]
    models = case[-1]
    rec = (4 * 2 + 2) * 8
    most = max(len(m.segs) for m in models)
    monkeypatch.setenv("IVP_DENSE_STAGING_BYTES", str(2 * most * rec))   # two trajectories' blocks: ranges of 2, 2, 1
    r = _dense(case, 1)
    assert r.dense_info["passes"] == 2 and r.dense_info["staging_bytes"] <= 2 * most * rec, r.dense_info
    hold_dense(r, models, "two ranges")
    hold_sol(r, models, "two ranges")


# ---- 8. resumable -----------------------------------------------------------------------------------------------------

def _same_members(a, b, names, what):
    for k in names:
        va, vb = getattr(a, k, None), getattr(b, k, None)
        assert (va is None) == (vb is None), (what, k)
        if va is not None:
            assert _np(va).tobytes() == _np(vb).tobytes(), (what, k)


def test_wait_false_polled_to_completion_equals_the_blocking_solve():
    args = (ivp_amd.StiffVanDerPol(), 0.0, VDP_T1, dev(cols(VDP_Y0)), dev([VDP_EPS]), Options(rtol=VDP_RT, atol=VDP_AT, max_log=8))
    blocking = Radau().solve_batch(*args, ctx=ivp_amd.Context(0))
    ctx = ivp_amd.Context(0)
    pend = Radau().solve_batch(*args, ctx=ctx, wait=False)
    assert isinstance(pend, ivp_amd.api.PendingBatch)
    with pytest.raises(ConfigError) as e:   # a second submit on the busy context
        Radau().solve_batch(*args, ctx=ctx, wait=False)
    assert e.value.code == -100 and "already in flight" in str(e.value)
    polls = 0
    while not pend.done():
        polls += 1
        assert polls < 10_000_000
    r = pend.result()
    _same_members(r, blocking, END + ("n_log", "t_log", "y_log"), "wait=False")
    hold_end(r, vdp_models(), "wait=False")


def test_a_dae_submit_keeps_nothing_of_the_callers_structs():
    """Radau._c() / _dae() are temporaries of the call: the rounds after the first run with the partition the context kept"""
    name, src, n, rad, y0s, t1, opt, run = dae_cases()[1]
    models = model(("dae", 1), run)
    pend = rad.solve_batch(ivp_amd.DeviceIVP(src, n, mass=True), 0.0, t1, dev(cols(y0s)), None, Options(rtol=1e-4, atol=1e-4, chunk_attempts=1), wait=False)
    hold_end(pend.result(), models, "index-2 pendulum, wait=False, chunk_attempts = 1")


def test_pipeline_map_over_three_radau_batches_equals_three_solves():
    f, o = ivp_amd.StiffVanDerPol(), Options(rtol=VDP_RT, atol=VDP_AT)
    batches = [dict(t0=0.0, t1=VDP_T1, y0=dev(cols(VDP_Y0)[:, k:k + 3]), params=dev([VDP_EPS[k:k + 3]])) for k in range(3)]
    single = [Radau().solve_batch(f, b["t0"], b["t1"], b["y0"], b["params"], o) for b in batches]
    pipe = BatchPipeline(streams=2)
    for got in (pipe.map(f, batches, o, radau=Radau()), pipe.map_threads(f, batches, o, radau=Radau())):
        assert len(got) == 3
        for k in range(3):
            _same_members(got[k], single[k], END, f"pipeline batch {k}")
            hold_end(got[k], vdp_models()[k:k + 3], f"pipeline batch {k}")


# ---- 9. sequences on one context ----------------------------------------------------------------------------------------

def test_a_sequence_on_one_context_equals_fresh_contexts():
    vdp = (ivp_amd.StiffVanDerPol(), 0.0, VDP_T1, dev(cols(VDP_Y0)), dev([VDP_EPS]))
    o = Options(rtol=VDP_RT, atol=VDP_AT)
    calls = [("Radau logged", lambda c: Radau().solve_batch_logged(*vdp, o, c), END + ("log_offsets", "t_log", "y_log", "n_log")),
             ("DOPRI5 logged", lambda c: ivp_amd.solve_ivp_batch_logged(ivp_amd.SHO(), 0.0, 3.0, dev(cols([[1.0, 0.0], [0.3, -0.7]])), None,
                                                                       Options(method="DOPRI5", rtol=1e-6, atol=1e-9), c), END[:1] + ("y_end", "log_offsets", "t_log", "y_log", "n_log")),
             ("Radau dense", lambda c: Radau().solve_batch_dense(*vdp[:3], dev(cols(VDP_Y0)[:, :3]), dev([VDP_EPS[:3]]), Options(rtol=VDP_RT, atol=VDP_AT, max_log=1), c),
              END + ("seg_offsets", "seg_cont", "seg_xold", "seg_h", "n_seg")),
             ("BDF bounded", lambda c: ivp_amd.solve_ivp_batch(*vdp, Options(method="BDF", rtol=1e-6, atol=1e-8, max_log=16), c), END + ("n_log", "t_log", "y_log")),
             ("Radau logged again", lambda c: rob_logged(c), END + ("log_offsets", "t_log", "y_log", "n_log"))]
    fresh = []
    for _, call, _ in calls:
        c = ivp_amd.Context(0)
        fresh.append(call(c))
    one = ivp_amd.Context(0)
    for (name, call, names), want in zip(calls, fresh):
        _same_members(call(one), want, names, name)
    hold_log(fresh[0], vdp_models(), "first of the sequence")
    hold_log(fresh[4], rob_models(), "last of the sequence")
    # a plain Radau solve ends the life of the log in the pool
    Radau().solve_batch(*vdp, o, ctx=one)
    log = ivp_amd._lib.StepLogT()
    rc = one.lib.ivp_step_log_fetch_device(one.handle, _byref(log), None)
    assert rc == -100 and "no complete step log" in one.last_error()


# ---- 10. refusals carry over --------------------------------------------------------------------------------------------
MASS_2 = ("__device__ void ode(double x, const double* y, double* d, const double* p) { d[0] = -y[0]; d[1] = y[0] - y[1]; }\n"
          "__device__ void mass(double* m, const double* p) { m[0] = 1.0; m[3] = 1.0; }\n")


@pytest.mark.parametrize("what", ["events", "n = 100", "FMA", "mass with dae = NULL"])
def test_refusals_answer_through_every_new_entry_point_as_through_the_blocking_one(what):
    f, okw = {"events": (ivp_amd.SHOZeroEvent(), {}), "n = 100": (ivp_amd.LinearDecay100(), {}),
              "FMA": (ivp_amd.SHO(), dict(fp_mode=ivp_amd.FpMode.FMA)), "mass with dae = NULL": (ivp_amd.DeviceIVP(MASS_2, 2, mass=True), {})}[what]
    n, B = f.n, 2
    ctx = ivp_amd.Context(0)
    prob, copt, rad = ivp_amd.api._problem_c(f), Options(**okw)._c(n, []), Radau()._c()
    y0, t0, t1 = torch.ones((n, B), dtype=torch.float64, device=DEV), dev([0.0]), dev([1.0])
    par = torch.ones((max(f.n_params, 1), B), dtype=torch.float64, device=DEV) if f.n_params else None
    out, keep = _result(B, n)
    common = (ctx.handle, _byref(prob), B, _ptr(y0), _ptr(par), _ptr(t0), 1, _ptr(t1), 1, _byref(copt), _byref(rad))
    want = (ctx.lib.ivp_radau_solve_device(*common, _byref(out), None), ctx.last_error())
    assert want[0] != 0 and want[1]
    off = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    log, dense = ivp_amd._lib.StepLogT(), ivp_amd._lib.DenseLogT()
    log.offsets, dense.offsets = off.data_ptr(), off.data_ptr()
    got = {"submit": (ctx.lib.ivp_radau_submit_device(*common, None, _byref(out), None), ctx.last_error()),
           "logged": (ctx.lib.ivp_radau_solve_logged_device(*common, None, _byref(out), _byref(log), None), ctx.last_error()),
           "dense": (ctx.lib.ivp_radau_solve_dense_device(*common, None, _byref(out), _byref(dense), None), ctx.last_error())}
    assert all(v == want for v in got.values()), (want, got)
    done = C.c_int(0)
    assert ctx.lib.ivp_batch_poll(ctx.handle, _byref(done)) == 0 and done.value == 1   # nothing was left in flight
    word = {"events": "event functions", "n = 100": "n = 100", "FMA": "FMA", "mass with dae = NULL": "mass matrix"}[what]
    assert word in want[1] and want[0] == -100
    ctx.close()
