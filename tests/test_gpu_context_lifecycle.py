"""Contracts of the C ABI about what an ivp_ctx keeps from one call to the next (include/ivp_hip.h), through ctypes:

  * a deferred step log (ivp_step_log_t.defer = 1) lives until the context's next solve of ANY kind: a fetch after a
    non-paged solve fails with IVP_ERR_BAD_ARGUMENT and writes nothing -- whether or not that solve reallocated the buffer
    the counts lived in.  (Every ivp_batch_submit_device clears log_state.valid.  Before that fix the fetch scanned counts
    the second solve had rewritten or freed and gathered at offsets that had nothing to do with the destination; that
    state is not reproduced here, the fix is argued from the code.)
  * out.n_seg counts ContinuousOutput segments only: all zero after a DOP853 t_eval solve, although the deferred sampling
    kernels (flavour 3) count their noted steps in an array of that name;
  * solve_ivp_batch_logged integrates again only when the library says that the pool ran dry; any other failure of the
    fetch is raised;
  * with host pointers the slots of a capacity-bounded output past its count return as the caller gave them, not as the
    context's previous solve left them in the staging buffers;
  * the deferred t_eval sampling kernels (flavour 3) against sampling in the stepping kernels (flavour 1) on the real
    kernels, and the fall-back to flavour 1 when the block of noted steps does not fit (IVP_DEFER_EVAL_BYTES): the same
    bits in every output, and the launch trace shows which path ran.  The mode is read once per process: child processes.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import _lib
from ivp_amd import api as A
from ivp_amd import workloads as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT, ERR_HIP = -100, -103


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float64).view(np.uint64)


class DeviceCall:
    """the arguments of one ivp_batch_solve*_device call: device tensors, the options struct, an ivp_batch_result_t whose
    members are the tensors in `out`"""

    def __init__(self, f, y0, p, t0, t1, options, **out):
        self.keep = []
        self.f, self.B = f, int(y0.shape[1])
        self.prob = A._problem_c(f)
        self.copt = options._c(f.n, self.keep)
        dev = lambda a: torch.as_tensor(np.atleast_1d(np.asarray(a, dtype=np.float64)), device=DEV)
        self.y0, self.p, self.t0, self.t1 = dev(y0), (None if p is None else dev(p)), dev(t0), dev(t1)
        self.out = out
        self.r = _lib.BatchResultT()
        for k, v in out.items():
            setattr(self.r, k, v.data_ptr())
        self.stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def args(self):
        return (C.byref(self.prob), self.B, self.y0.data_ptr(), None if self.p is None else self.p.data_ptr(), self.t0.data_ptr(), int(self.t0.numel()),
                self.t1.data_ptr(), int(self.t1.numel()), C.byref(self.copt), C.byref(self.r))


def _cr3bp64():
    y0, p, t0, t1 = W.cr3bp_batch(64)
    return ivp_amd.CR3BP(), y0, p, t0, t1, ivp_amd.Options(method="DOPRI5", rtol=1e-6, atol=1e-9)


def _logged_deferred(ctx):
    """ivp_batch_solve_logged_device with defer = 1: CR3BP, B = 64.  Returns (call, offsets, total)."""
    L = ctx.lib
    f, y0, p, t0, t1, o = _cr3bp64()
    call = DeviceCall(f, y0, p, t0, t1, o, y_end=torch.zeros((6, 64), dtype=torch.float64, device=DEV))
    offsets = torch.zeros(65, dtype=torch.int64, device=DEV)
    sl = _lib.StepLogT()
    sl.offsets, sl.defer = offsets.data_ptr(), 1
    rc = L.ivp_batch_solve_logged_device(ctx.handle, *call.args(), C.byref(sl), call.stream)
    assert rc == 0, ctx.last_error()
    assert sl.passes == 1 and int(sl.total) == int(offsets[-1]) > 64
    return call, offsets, int(sl.total)


def _fetch(ctx, total):
    t = torch.full((total,), -1.0, dtype=torch.float64, device=DEV)
    y = torch.full((total, 6), -1.0, dtype=torch.float64, device=DEV)
    sl = _lib.StepLogT()
    sl.t, sl.y, sl.capacity = t.data_ptr(), y.data_ptr(), total
    rc = ctx.lib.ivp_step_log_fetch_device(ctx.handle, C.byref(sl), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc, t, y


@pytest.mark.parametrize("B2", [700, 64], ids=["second-solve-reallocates", "second-solve-same-size"])
def test_a_deferred_log_ends_with_the_next_solve_of_any_kind(B2):
    ctx = ivp_amd.Context(0)
    try:
        _, _, total = _logged_deferred(ctx)
        # a non-paged full solve: Van der Pol with t_eval (B2 = 700 grows every per-trajectory scratch buffer, n_log's included)
        y0, p, t0, t1 = W.vdp_batch(B2)
        grid = list(np.linspace(0.0, 20.0, 9))
        call = DeviceCall(ivp_amd.VanDerPol(), y0, p, t0, np.minimum(t1, 20.0), ivp_amd.Options(method="DOPRI5", rtol=1e-6, atol=1e-9, t_eval=grid),
                          y_eval=torch.zeros((9, 2, B2), dtype=torch.float64, device=DEV), n_filled=torch.zeros(B2, dtype=torch.int32, device=DEV))
        rc = ctx.lib.ivp_batch_solve_device(ctx.handle, *call.args(), call.stream)
        assert rc == 0, ctx.last_error()
        assert (call.out["n_filled"] >= 8).all().item()       # (the point at t1 itself may fall a rounding behind t_end)
        rc, t, y = _fetch(ctx, total)
        assert rc == BAD_ARGUMENT and "no complete step log" in ctx.last_error(), (rc, ctx.last_error())
        assert (t == -1.0).all().item() and (y == -1.0).all().item()
    finally:
        ctx.close()


def test_a_deferred_log_fetched_at_once_is_the_counted_two_pass_log():
    ctx = ivp_amd.Context(0)
    try:
        call, offsets, total = _logged_deferred(ctx)
        rc, t, y = _fetch(ctx, total)
        assert rc == 0, ctx.last_error()
        f, y0, p, t0, t1, o = _cr3bp64()
        two = ivp_amd.solve_ivp_batch_logged(f, t0, t1, call.y0, call.p, o, ctx, two_pass=True)
        assert torch.equal(offsets, two.log_offsets) and total == int(two.t_log.shape[0])
        assert np.array_equal(_bits(t), _bits(two.t_log)) and np.array_equal(_bits(y), _bits(two.y_log))
        assert np.array_equal(_bits(call.out["y_end"]), _bits(two.y_end))
        # ... and that two-pass solve was the context's next solve: the log is gone
        rc, t, y = _fetch(ctx, total)
        assert rc == BAD_ARGUMENT and (t == -1.0).all().item()
    finally:
        ctx.close()


def test_n_seg_is_zero_after_a_dop853_t_eval_solve():
    ctx = ivp_amd.Context(0)
    try:
        B = 67
        y0, p, t0, t1 = W.vdp_batch(B)
        o = ivp_amd.Options(method="DOP853", rtol=1e-8, atol=1e-10, t_eval=list(np.linspace(0.0, 60.0, 33)))
        outs = []
        for with_n_seg in (True, False):
            m = dict(y_eval=torch.zeros((33, 2, B), dtype=torch.float64, device=DEV), n_filled=torch.zeros(B, dtype=torch.int32, device=DEV),
                     y_end=torch.zeros((2, B), dtype=torch.float64, device=DEV))
            if with_n_seg:
                m["n_seg"] = torch.full((B,), -1, dtype=torch.int32, device=DEV)     # 0xFFFFFFFF
            call = DeviceCall(ivp_amd.VanDerPol(), y0, p, t0, np.minimum(t1, 60.0), o, **m)
            rc = ctx.lib.ivp_batch_solve_device(ctx.handle, *call.args(), call.stream)
            assert rc == 0, ctx.last_error()
            torch.cuda.synchronize()
            outs.append(m)
        a, b = outs
        assert not a["n_seg"].any().item(), a["n_seg"]
        assert int(a["n_filled"].min()) > 10
        assert torch.equal(a["n_filled"], b["n_filled"])
        assert np.array_equal(_bits(a["y_eval"]), _bits(b["y_eval"])) and np.array_equal(_bits(a["y_end"]), _bits(b["y_end"]))
    finally:
        ctx.close()


class _FetchFails:
    """ctx.lib with one difference: the next ivp_step_log_fetch_device returns IVP_ERR_HIP without reaching the library"""

    def __init__(self, lib):
        self._lib, self.fetches, self.logged_solves = lib, 0, 0

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def ivp_step_log_fetch_device(self, *args):
        self.fetches += 1
        return ERR_HIP if self.fetches == 1 else self._lib.ivp_step_log_fetch_device(*args)

    def ivp_batch_solve_logged_device(self, *args):
        self.logged_solves += 1
        return self._lib.ivp_batch_solve_logged_device(*args)


def test_a_failed_fetch_is_raised_not_answered_by_a_second_integration():
    ctx = ivp_amd.Context(0)
    try:
        f, y0, p, t0, t1, o = _cr3bp64()
        y0d, pd = torch.as_tensor(y0, device=DEV), torch.as_tensor(p, device=DEV)
        ctx.lib = stub = _FetchFails(ctx.lib)
        with pytest.raises(ivp_amd.ConfigError) as e:
            ivp_amd.solve_ivp_batch_logged(f, t0, t1, y0d, pd, o, ctx)
        assert e.value.code == ERR_HIP and stub.fetches == 1 and stub.logged_solves == 1
        # the context is none the worse: the same call again (the stub lets the second fetch through)
        r = ivp_amd.solve_ivp_batch_logged(f, t0, t1, y0d, pd, o, ctx)
        assert r.log_info["passes"] == 1 and stub.fetches == 2 and stub.logged_solves == 2
        ctx.lib = stub._lib
        # (a pool that really ran dry is still answered by a second integration:
        # tests/test_gpu_one_pass_log.py::test_a_pool_that_runs_dry_costs_an_integration_not_a_record)
    finally:
        ctx.close()


def test_host_arrays_keep_the_callers_content_past_the_counts():
    """The host-pointer entry point returns whole device mirrors of the outputs, and the mirrors are the context's grow-only
    staging buffers: the slots past n_event_hits must come back as the caller gave them (zeros from the Python API), not as
    the context's previous solve left them.  (Found by test_gpu_context_sequences: recipe 04 after recipe 03.)"""
    ctx = ivp_amd.Context(0)
    try:
        rng = np.random.default_rng(8)
        y0 = np.stack([1.0 + 0.1 * rng.standard_normal(9), 0.1 * rng.standard_normal(9)])
        o = ivp_amd.Options(method="DOP853", rtol=1e-9, atol=1e-12, max_events=8)
        with pytest.warns(RuntimeWarning, match="event buffers overflowed"):
            full = ivp_amd.solve_ivp_batch(ivp_amd.SHOZeroEvent(ivp_amd.EventConfig()), 0.0, 40.0, y0, None, o, ctx)
        assert (full.n_event_hits > 8).all() and (full.t_events > 0.0).all()          # every slot of the mirror is now non-zero
        r = ivp_amd.solve_ivp_batch(ivp_amd.SHOZeroEvent(ivp_amd.EventConfig(ivp_amd.Direction.All, 3)), 0.0, 40.0, y0, None, o, ctx)
        assert (r.n_event_hits == 3).all()
        assert (r.t_events[:, :3] > 0.0).all()
        assert not r.t_events[:, 3:].any() and not r.y_events[:, 3:].any()
    finally:
        ctx.close()


# ---- flavour 3 against flavour 1 on the real kernels, and the fall-back ----

_DUMPS = {}


def _dump(tmp_path_factory, mode):
    """tests/helpers/teval_dump.py in a child process, once per mode: (arrays, lines of the launch trace about the sample kernel)"""
    if mode not in _DUMPS:
        env = dict(os.environ, IVP_TRACE_LAUNCHES="1")
        env.pop("IVP_TUNE_DEFER_EVAL", None)
        env.pop("IVP_DEFER_EVAL_BYTES", None)
        env.update({"inline": {"IVP_TUNE_DEFER_EVAL": "0"}, "deferred": {"IVP_TUNE_DEFER_EVAL": "1"},
                    "capped": {"IVP_TUNE_DEFER_EVAL": "1", "IVP_DEFER_EVAL_BYTES": "1024"}}[mode])
        out = str(tmp_path_factory.mktemp("teval") / f"{mode}.npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "teval_dump.py"), out], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        z = np.load(out)
        _DUMPS[mode] = ({k: z[k] for k in z.files}, [ln for ln in r.stderr.splitlines() if ln.startswith("ivp launch sample")])
    return _DUMPS[mode]


def _same_arrays(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        if x.dtype == np.float64:
            x, y = np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)
        assert np.array_equal(x, y), f"{what}: {k}: {np.count_nonzero(x != y)} of {x.size} values differ"


def test_deferred_t_eval_sampling_equals_sampling_in_the_stepping_kernels(tmp_path_factory):
    inline, tr0 = _dump(tmp_path_factory, "inline")
    deferred, tr1 = _dump(tmp_path_factory, "deferred")
    assert len(tr1) == 3 and not tr0, (tr0, tr1)          # one sample kernel per solve of the helper; none with IVP_TUNE_DEFER_EVAL=0
    assert int(inline["vdp.n_filled"].min()) > 10 and int(inline["cr3bp.n_filled"].min()) > 10
    assert inline["vdp.y_eval"].shape == (65, 2, 3000) and inline["cr3bp.y_eval"].shape == (65, 6, 500)
    lengths = np.diff(inline["ragged.eval_offsets"])
    assert lengths.min() == 0 and lengths.max() == 40 and int(inline["ragged.n_filled"].sum()) > 500
    _same_arrays(deferred, inline, "flavour 3 against flavour 1")


def test_a_block_of_noted_steps_that_does_not_fit_falls_back_to_the_stepping_kernels(tmp_path_factory):
    inline, _ = _dump(tmp_path_factory, "inline")
    capped, tr = _dump(tmp_path_factory, "capped")
    assert not tr, tr                                      # IVP_DEFER_EVAL_BYTES=1024: no solve of the helper fits, none is deferred
    _same_arrays(capped, inline, "capped deferred sampling against flavour 1")
