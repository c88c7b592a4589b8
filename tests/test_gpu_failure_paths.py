"""Failing and non-finite trajectories on every kernel shape of libivp_hip.so (run with -m gpu).

The batches and reference helpers are those of tests/test_failure_paths_cpu.py, where every input is first shown, on the
oracle, to take the branch it is named after.  The bar is DESIGN section 5's and nothing else: strict GPU == liboracle_detpow
and FMA GPU == liboracle_fma bit for bit (NaN equal to NaN, as assert_bitexact has it) for y_end, t_end, h_next, status and
every counter of every trajectory -- the failing ones and their neighbours in the same wavefront.  No tolerance anywhere.
(For the thread-per-trajectory BDF kernel the neighbours share a batch, not a wavefront: below cus + 1 trajectories the
launch loop gives every trajectory a wavefront of its own.  tests/test_gpu_wave_density.py runs BDF with 2 .. 64 per wave.)

  1. one mixed batch per kernel shape: thread-per-trajectory (rk_core.h / bdf_core.h), lane-cooperative (rk_coop.h),
     wave-per-trajectory explicit (rk_group.h) and wave-per-trajectory BDF (bdf_group.h), each at chunk 0 and an odd chunk;
  2. the exactly singular I - cJ of BDF (LU failure on the first attempt) and a NaN Jacobian entry;
  3. bounded and CSR outputs of trajectories that fail part-way.

RK23 follows the existing parity test (the reference never returns from RK23 with a NaN error estimate): bad lanes end with
status 3, healthy lanes equal an oracle run of the healthy lanes alone.
"""
import warnings

import numpy as np
import pytest

import ivp_amd
from oracle import oracle as O
from tests.common import assert_bitexact, gpu_batch, oracle_batch
from tests import test_failure_paths_cpu as F
from tests.test_failure_paths_cpu import MAXSTEPS, OK, STIFF, TOOSMALL, per_trajectory

pytestmark = pytest.mark.gpu
END = ("y_end", "t_end", "h_next", "status", "nfev", "nstep", "naccpt", "nrejct", "njev", "nlu")
OUT = END + ("y_eval", "eval_idx", "n_filled", "t_log", "y_log", "n_log", "seg_cont", "seg_xold", "seg_h", "n_seg",
             "t_events", "y_events", "n_event_hits")


def device_batch(f, y0, params, t0, t1, *, fast=False, chunk=0, **opts):
    """solve_ivp_batch of any IVP (hiprtc systems included) with host arrays, in the result shape of gpu_batch"""
    o = ivp_amd.Options(fp_mode=ivp_amd.FpMode.FAST if fast else ivp_amd.FpMode.STRICT, chunk_attempts=chunk, **opts)
    r = ivp_amd.solve_ivp_batch(f, t0, t1, np.ascontiguousarray(y0), params if f.n_params else None, o)
    out = {k: np.asarray(getattr(r, k)) for k in OUT if getattr(r, k, None) is not None}
    if "n_event_hits" in out:
        out["n_ev"] = out["n_event_hits"]
    out["stats"] = r.stats
    return out


_refs = {}


def cached(key, make):
    """a reference is computed once, shared by the cases that need it and never modified"""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


# ---- 1a. thread-per-trajectory, n <= 8 (BDF included) ----------------------------------------------------------------------

@pytest.mark.parametrize("fp", ["strict", "fma"])
@pytest.mark.parametrize("rhs,method", F.THREAD_SHAPES)
def test_thread_per_trajectory_mixed_status_batch(rhs, method, fp):
    y0, p, t0, t1, o, want = F.thread_batch(rhs, method)
    if fp == "strict":
        ref = F.thread_reference(rhs, method)
    else:
        ref = oracle_batch(rhs, y0, p, t0, t1, fma=True, **o)
        bad = [b for b, _, _ in F.BAD70]
        assert (ref["status"][bad] == (OK if method == "RK4" else TOOSMALL)).all() and set(int(v) for v in ref["status"]) == want
    for chunk in (0, 7):
        got = gpu_batch(rhs, y0, p, t0, t1, chunk=chunk, fast=fp == "fma", **o)
        assert_bitexact(got, ref, f"{rhs} {method} {fp} chunk={chunk}: ")


@pytest.mark.parametrize("rhs", ["sho", "robertson"])
def test_thread_per_trajectory_rk23_mixed_status_batch(rhs):
    y0, p, t0, t1, o, _ = F.thread_batch(rhs, "DOPRI5")
    o = dict(o, method="RK23", rtol=1e-4, atol=1e-7)
    bad = [b for b, _, _ in F.BAD70]
    good = np.ones(70, bool)
    good[bad] = False
    ref = oracle_batch(rhs, y0[:, good], p, t0, t1[good], **o)
    assert MAXSTEPS in ref["status"] and OK in ref["status"]
    for chunk in (0, 7):
        F.assert_rk23_rule(gpu_batch(rhs, y0, p, t0, t1, chunk=chunk, **o), y0, ref, bad)


# ---- 1b. lane-cooperative kernels: eight lanes per trajectory, DPP norms and row broadcasts -------------------------------

@pytest.mark.parametrize("where", [0, -1], ids=["nan-first-comp", "nan-last-comp"])
@pytest.mark.parametrize("B", [1, 9, 65])
@pytest.mark.parametrize("method", ["DOPRI5", "DOP853"])
@pytest.mark.parametrize("rhs", ["sho", "lorenz", "cr3bp"])
def test_cooperative_kernels_with_failing_groups_beside_healthy_ones(rhs, method, B, where):
    y0, p, t0, t1, o, bad, long = F.coop_batch(rhs, method, B, where)
    ref = oracle_batch(rhs, y0, p, t0, t1, **o)
    F.check_group_reference(ref, bad, long)
    for chunk in (0, 5):
        got = gpu_batch(rhs, y0, p, t0, t1, variant=3, chunk=chunk, profile=1, **o)
        assert_bitexact(got, ref, f"{rhs} {method} B={B} coop chunk={chunk}: ")
        assert got["stats"]["coop_launches"] == got["stats"]["launches"] > 0
    assert_bitexact(gpu_batch(rhs, y0, p, t0, t1, **o), ref, f"{rhs} {method} B={B} default policy: ")


# ---- 1c. wave-per-trajectory kernels, explicit methods ----------------------------------------------------------------------

RING_POS = [(6, 0), (6, 1), (6, 2), (6, 3), (12, 0), (12, 1), (20, 0)]      # n = 12: four groups per wavefront, 24: two, 40: one


def ring_ivp(K, **kw):
    return ivp_amd.DeviceIVP(F.ring_source(K, events=bool(kw.get("events"))), n=2 * K, params=(3.0,), **kw)


def ring_reference(K, method, pos):
    def make():
        y0, par, t0, t1, o, bad, long = F.ring_batch(K, method, pos)
        r = per_trajectory(F.ring_fun(K), y0, par, t0, t1, **o)
        F.check_group_reference(r, bad, long)
        return r
    return cached(("ring", K, method, pos), make)


@pytest.mark.parametrize("K,pos", RING_POS)
@pytest.mark.parametrize("method", ["DOPRI5", "DOP853"])
def test_wave_per_trajectory_ring_with_a_failing_group_at_every_position(K, pos, method):
    y0, par, t0, t1, o, bad, long = F.ring_batch(K, method, pos)
    ref = ring_reference(K, method, pos)
    f = ring_ivp(K)
    for chunk in (0, 7):
        assert_bitexact(device_batch(f, y0, par, t0, t1, chunk=chunk, **o), ref, f"ring n={2 * K} {method} pos={pos} chunk={chunk}: ")


@pytest.mark.parametrize("K,pos", RING_POS)
def test_wave_per_trajectory_ring_rk23_with_a_failing_group_at_every_position(K, pos):
    y0, par, t0, t1, o, bad, long = F.ring_batch(K, "RK23", pos)
    good = np.ones(11, bool)
    good[bad] = False
    ref = per_trajectory(F.ring_fun(K), y0[:, good], par[:, good], t0, t1[good], **o)
    assert MAXSTEPS in ref["status"] and OK in ref["status"]
    f = ring_ivp(K)
    for chunk in (0, 7):
        F.assert_rk23_rule(device_batch(f, y0, par, t0, t1, chunk=chunk, **o), y0, ref, bad)


@pytest.mark.parametrize("method", ["DOPRI5", "DOP853", "RK23"])
@pytest.mark.parametrize("rhs", ["linear_decay100", "heat1d256"])
def test_wave_per_trajectory_builtin_systems_mixed_status_batch(rhs, method):
    """linear_decay100: NaN in component 0 and in component 99 (the second lane slice); heat1d256: a NaN trajectory, an inf
    trajectory and kappa = 4000 members that end ProbablyStiff"""
    y0, p, t0, t1, o, bad, long = F.decay100_batch(method) if rhs == "linear_decay100" else F.heat256_batch(method)
    long_status = MAXSTEPS if rhs == "linear_decay100" else STIFF
    if method == "RK23":
        good = np.ones(y0.shape[1], bool)
        good[bad] = False
        ref = oracle_batch(rhs, y0[:, good], None if p is None else p[:, good], t0, t1[good], **o)
        assert MAXSTEPS in ref["status"] and OK in ref["status"]     # RK23 has no stiffness detector: max_steps ends the stiff members
        for chunk in (0, 7):
            F.assert_rk23_rule(gpu_batch(rhs, y0, p, t0, t1, chunk=chunk, **o), y0, ref, bad)
        return
    ref = oracle_batch(rhs, y0, p, t0, t1, **o)
    F.check_group_reference(ref, bad, long, long_status)
    for chunk in (0, 7):
        assert_bitexact(gpu_batch(rhs, y0, p, t0, t1, chunk=chunk, **o), ref, f"{rhs} {method} chunk={chunk}: ")


# ---- 1d. wave-per-trajectory BDF: LDS-resident and global-memory factors ---------------------------------------------------

@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("K,pos", RING_POS[:6])
def test_wave_per_trajectory_bdf_ring_with_a_failing_group_at_every_position(K, pos, variant):
    y0, par, t0, t1, o, bad, long = F.ring_batch(K, "BDF", pos)
    ref = ring_reference(K, "BDF", pos)
    assert (ref["nlu"][bad[0]] > 1000) and ref["nlu"][bad[1]] == 0
    f = ring_ivp(K)
    for chunk in (0, 5):
        got = device_batch(f, y0, par, t0, t1, chunk=chunk, variant=variant, **o)
        assert_bitexact(got, ref, f"ring n={2 * K} BDF pos={pos} variant={variant} chunk={chunk}: ")


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("rhs", ["linear_decay100", "dense64"])
def test_wave_per_trajectory_bdf_builtin_systems_with_nan_and_inf_trajectories(rhs, variant):
    y0, p, t0, t1, o, bad, long = F.decay100_batch("BDF") if rhs == "linear_decay100" else F.dense64_batch()

    def make():
        r = oracle_batch(rhs, y0, p, t0, t1, **o)
        F.check_group_reference(r, bad, long)
        return r
    ref = cached(("bdf", rhs), make)
    for chunk in (0, 5):
        got = gpu_batch(rhs, y0, p, t0, t1, chunk=chunk, variant=variant, **o)
        assert_bitexact(got, ref, f"{rhs} BDF variant={variant} chunk={chunk}: ")


# ---- 2. the singular-matrix branch of BDF -----------------------------------------------------------------------------------

def singular_reference(n, fma):
    def make():
        fun, jac = F.sing_fun(n)
        y0, par, t0, t1 = F.sing_batch(n)
        first = per_trajectory(fun, y0, par, t0, t1, jac=jac, fma=fma, max_steps=1, **F.SING_OPTS)
        full = per_trajectory(fun, y0, par, t0, t1, jac=jac, fma=fma, **F.SING_OPTS)
        F.check_singular_reference(first, full, par)
        return first, full
    return cached(("singular", n, fma), make)


@pytest.mark.parametrize("fp", ["strict", "fma"])
@pytest.mark.parametrize("n", [3, 12, 24, 40])
def test_bdf_singular_iteration_matrix_beside_regular_ones(n, fp):
    """lambda = 16 makes 1 - c lambda exactly zero on the first attempt: that trajectory leaves the LU early (no Newton
    evaluation: nfev stays 1) while its neighbours in the wavefront (lambda = 15, nextafter(16)) factorise and iterate."""
    fma = fp == "fma"
    first, full = singular_reference(n, fma)
    y0, par, t0, t1 = F.sing_batch(n)
    f = ivp_amd.DeviceIVP(F.sing_source(n), n=n, params=(16.0, -1.0), jac=True)
    for variant in ((0,) if n <= 8 else (0, 1)):
        got = device_batch(f, y0, par, t0, t1, fast=fma, variant=variant, max_steps=1, **F.SING_OPTS)
        assert_bitexact(got, first, f"singular n={n} {fp} variant={variant} first attempt: ")
        for chunk in (0, 5):
            got = device_batch(f, y0, par, t0, t1, fast=fma, variant=variant, chunk=chunk, **F.SING_OPTS)
            assert_bitexact(got, full, f"singular n={n} {fp} variant={variant} chunk={chunk}: ")


@pytest.mark.parametrize("n", [3, 12, 24])
def test_bdf_nan_jacobian_entry_beside_regular_trajectories(n):
    """the Jacobian override writes NaN into J[0][0] of one trajectory: the pivot search meets a NaN diagonal ("NaNs never
    win", then the akk == akk fallback); the trajectory halves its step down to StepSizeTooSmall, the others finish"""
    fun, jac = F.sing_fun(n)
    y0, par, t0, t1 = F.nan_jac_batch(n)

    def make():
        r = per_trajectory(fun, y0, par, t0, t1, jac=jac, **F.SING_OPTS)
        F.check_nan_jac_reference(r)
        return r
    ref = cached(("nanjac", n), make)
    f = ivp_amd.DeviceIVP(F.sing_source(n), n=n, params=(16.0, -1.0), jac=True)
    for variant in ((0,) if n <= 8 else (0, 1)):
        for chunk in (0, 5):
            got = device_batch(f, y0, par, t0, t1, variant=variant, chunk=chunk, **F.SING_OPTS)
            assert_bitexact(got, ref, f"NaN Jacobian n={n} variant={variant} chunk={chunk}: ")


# ---- 3. output paths of a trajectory that fails part-way ------------------------------------------------------------------------

RING_EV = dict(events=lambda t, y, p: [y[0] - y[3]], n_events=1, event_direction=[0], event_terminal=[0])


def out_problem(system, method):
    """-> (IVP without events, IVP with one non-terminal event or None, y0, params, t1, options, solve(b, **kw) -> oracle Solution)"""
    if system == "sho":
        y0, p, t0, t1, o, _ = F.thread_batch("sho", method)
        idx = F.OUT_IDX

        def sol(b, events=False, **kw):
            ev = dict(event_direction=[0], event_terminal=[0]) if events else {}
            return O.solve_ivp("sho_ev" if events else "sho", 0.0, float(t1[b]), y0[:, b], detpow=True, **o, **ev, **kw)
        return ivp_amd.SHO(), ivp_amd.SHOZeroEvent(ivp_amd.EventConfig()), y0, None, t1, o, idx, sol
    if system == "ring12":
        y0, p, t0, t1, o, bad, long = F.ring_batch(6, method, 1)
        idx = (0, 1, 5, 9, 10)

        def sol(b, events=False, **kw):
            ev = RING_EV if events else {}
            return O.solve_ivp(F.ring_fun(6), 0.0, float(t1[b]), list(y0[:, b]), params=[float(p[0, b])], detpow=True, **o, **ev, **kw)
        return ring_ivp(6), ring_ivp(6, events=[ivp_amd.EventConfig()]), y0, p, t1, o, idx, sol
    y0, p, t0, t1, o, bad, long = F.decay100_batch(method)
    idx = tuple(range(y0.shape[1]))

    def sol(b, events=False, **kw):
        return O.solve_ivp("linear_decay100", 0.0, float(t1[b]), y0[:, b], detpow=True, **o, **kw)
    return ivp_amd.LinearDecay100(), None, y0, None, t1, o, idx, sol


def out_solutions(system, method, idx, sol, **kw):
    return cached(("out", system, method, tuple(sorted(kw))), lambda: [sol(b, **kw) for b in idx])


T_EVAL = {"sho": F.T_EVAL, "ring12": np.concatenate([[-0.5], np.linspace(0.0, 60.0, 61)]),
          "decay100": np.concatenate([[-0.5], np.linspace(0.0, 120.0, 61)])}
SYSTEM_METHODS = [(s, m) for s in ("sho", "ring12", "decay100") for m in ("DOPRI5", "DOP853", "BDF")]


@pytest.mark.parametrize("system,method", SYSTEM_METHODS)
def test_bounded_outputs_of_trajectories_that_fail_part_way(system, method):
    f, fe, y0, p, t1, o, idx, sol = out_problem(system, method)
    te = T_EVAL[system]
    variants = (0, 3) if (system == "sho" and method != "BDF") else (0,)
    ml = 1300
    for variant in variants:
        kw = dict(variant=variant, chunk=7)
        g = device_batch(f, y0, p, 0.0, t1, t_eval=list(te), **kw, **o)
        F.check_bounded_outputs(g, out_solutions(system, method, idx, sol, t_eval=te), idx, t_eval=te)
        g = device_batch(f, y0, p, 0.0, t1, max_log=ml, dense_output=True, **kw, **o)
        F.check_bounded_outputs(g, out_solutions(system, method, idx, sol, dense_output=True), idx, dense=True)
        if fe is not None:
            g = device_batch(fe, y0, p, 0.0, t1, max_log=ml, max_events=64, **kw, **o)
            sols = out_solutions(system, method, idx, sol, events=True)
            F.check_bounded_outputs(g, sols, idx, events=True)
            assert max(len(s.t_events[0]) for s in sols) >= 3


_TRACE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from tests import test_failure_paths_cpu as F
from tests.common import gpu_batch
y0, p, t0, t1, o, _ = F.thread_batch("sho", "DOP853")
g = gpu_batch("sho", y0, None, t0, t1, chunk=7, profile=1, t_eval=list(F.T_EVAL), **o)
np.savez(sys.argv[2], **{k: g[k] for k in ("status", "nfev", "naccpt", "n_filled", "eval_idx", "y_eval")})
"""


def test_deferred_sampling_kernel_is_reached_by_the_failing_batch(tmp_path):
    """n = 2, DOP853, t_eval and no events: the library hands the samples to the deferred sampling kernel (flavour 3).  That it
    did is visible only in the launch trace, which is switched on per process: one child process.  (The deferred EVENT kernel
    has no trace line or counter; that the n = 2 batches without a terminal event reach it rests on the library's rule --
    explicit method, no terminal event, thread-per-trajectory -- and on the host emulation, which reports its record block.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script, out = tmp_path / "trace_child.py", tmp_path / "out.npz"
    script.write_text(_TRACE_CHILD)
    env = dict(os.environ, IVP_TRACE_LAUNCHES="1")
    for k in ("IVP_TUNE_DEFER_EVAL", "IVP_DEFER_EVAL_BYTES"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script), root, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "deferred t_eval sampling, 70 trajectories" in r.stderr
    f, fe, y0, p, t1, o, idx, sol = out_problem("sho", "DOP853")
    F.check_bounded_outputs(dict(np.load(out)), out_solutions("sho", "DOP853", idx, sol, t_eval=F.T_EVAL), idx, t_eval=F.T_EVAL)


def _dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=torch.device("cuda:0"))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("system,method", SYSTEM_METHODS)
def test_csr_step_log_of_trajectories_that_fail_part_way(system, method):
    f, fe, y0, p, t1, o, idx, sol = out_problem(system, method)
    sols = out_solutions(system, method, idx, sol, dense_output=True)
    seen = set()
    for two_pass in (False, True):
        r = ivp_amd.solve_ivp_batch_logged(f, 0.0, _dev(t1), _dev(y0), _dev(p), ivp_amd.Options(**o), two_pass=two_pass)
        off = r.log_offsets.cpu().numpy()
        assert off[0] == 0 and int(off[-1]) == r.t_log.shape[0]
        for b, s in zip(idx, sols):
            seen.add(s.status)
            assert off[b + 1] - off[b] == len(s.t), (b, off[b + 1] - off[b], len(s.t))
            t, y = r.log_of(b)
            assert _same(t.cpu().numpy(), s.t) and _same(y.cpu().numpy(), s.y), (b, two_pass)
            assert int(r.status[b]) == s.status
            if s.status == MAXSTEPS:
                assert len(s.t) == s.naccpt + 1        # exactly its accepted steps after the start record
            if s.status == TOOSMALL:
                assert len(s.t) == 1 and np.array_equal(s.t, [0.0])      # failed before its first accepted step: the start record
    assert {OK, MAXSTEPS, TOOSMALL} <= seen


@pytest.mark.parametrize("system,method", SYSTEM_METHODS)
def test_csr_dense_output_of_trajectories_that_fail_part_way(system, method):
    f, fe, y0, p, t1, o, idx, sol = out_problem(system, method)
    sols = out_solutions(system, method, idx, sol, dense_output=True)
    B = y0.shape[1]
    for max_log, passes in ((8, 2), (1300, 1)):
        d = ivp_amd.solve_ivp_batch_dense(f, 0.0, _dev(t1), _dev(y0), _dev(p), ivp_amd.Options(max_log=max_log, **o))
        assert d.dense_info["passes"] == passes
        off = d.seg_offsets.cpu().numpy()
        xo, hh, cc = d.seg_xold.cpu().numpy(), d.seg_h.cpu().numpy(), d.seg_cont.cpu().numpy()
        grids = [np.zeros(0)] * B
        for b, s in zip(idx, sols):
            ns = 0 if s.seg_h is None else len(s.seg_h)
            lo, hi = int(off[b]), int(off[b + 1])
            assert hi - lo == ns == int(d.n_seg[b]), (b, hi - lo, ns)
            if ns:
                assert _same(xo[lo:hi], s.seg_xold) and _same(hh[lo:hi], s.seg_h) and _same(cc[lo:hi], s.seg_cont), b
                end = float(s.seg_xold[-1] + s.seg_h[-1])
                grids[b] = np.array([0.0, 0.37 * end, end, end + 0.5, float(t1[b]) + 1.0])
            else:
                grids[b] = np.array([0.0, 0.1, float(t1[b])])
        y, found = d.dense(grids)
        y, found = y.cpu().numpy(), found.cpu().numpy()
        q = 0
        failed_beyond = 0
        for b in range(B):
            s = sols[idx.index(b)] if b in idx else None
            for tq in grids[b]:
                if s is not None:
                    span = s.sol_span()
                    inside = span is not None and min(span) - 1e-12 <= tq <= max(span) + 1e-12
                    if inside:
                        assert found[q] == 1 and _same(y[q], s.sol(float(tq))), (b, tq)
                    else:      # beyond what a failed trajectory covered (or a trajectory with no segment at all)
                        assert found[q] == 0 and np.isnan(y[q]).all(), (b, tq)
                        failed_beyond += s.status != OK and tq <= t1[b]
                q += 1
        assert failed_beyond >= 2


@pytest.mark.parametrize("system,method", [c for c in SYSTEM_METHODS if c[0] != "decay100"])
def test_csr_event_log_of_trajectories_that_fail_part_way(system, method):
    f, fe, y0, p, t1, o, idx, sol = out_problem(system, method)
    sols = out_solutions(system, method, idx, sol, events=True)
    assert max(len(s.t_events[0]) for s in sols) >= 3
    for max_events, passes in ((2, 2), (64, 1)):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            r = ivp_amd.solve_ivp_batch_events(fe, 0.0, _dev(t1), _dev(y0), _dev(p), ivp_amd.Options(max_events=max_events, **o))
        assert r.event_info["passes"] == passes
        off = r.event_offsets.cpu().numpy()
        t, y = r.t_events_csr.cpu().numpy(), r.y_events_csr.cpu().numpy()
        assert off[0] == 0 and np.array_equal(np.diff(off), r.n_event_hits.cpu().numpy().astype(np.int64).reshape(-1))
        for b, s in zip(idx, sols):
            lo, hi = int(off[b]), int(off[b + 1])
            assert hi - lo == len(s.t_events[0]), (b, hi - lo, len(s.t_events[0]))
            assert _same(t[lo:hi], s.t_events[0]) and _same(y[lo:hi], s.y_events[0].reshape(hi - lo, y.shape[1])), b
            assert int(r.status[b]) == s.status
