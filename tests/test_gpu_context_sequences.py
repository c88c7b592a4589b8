"""Order independence on one context: what a solve returns must not depend on what its ivp_ctx solved before.

The kernels are pinned bit for bit elsewhere; this file pins the host library that decides what they are handed.  An ivp_ctx
keeps some forty grow-only device buffers (DevBuf::reserve frees and reallocates when a later solve is larger), a page pool, a
"learnt" log size, pinned error flags and a log_state from one solve to the next.  The recipes below are different KINDS of
solve whose shapes grow and shrink B, n and the output kinds from one to the next; each builds its inputs from fixed seeds,
solves on the context it is given and returns every output member the solve produced.

  * every recipe whose problem the CPU oracle has equals the oracle on a fresh context (the baseline is anchored to
    something that is not the code under test);
  * the whole list run on ONE context -- in table order, reversed, and in a fixed random order -- gives, recipe by recipe and
    member by member, the bits of the fresh-context run;
  * a solve that ends in an error (RK4's IVP_ERR_INVALID_STEP_SIZE travels through the sticky pinned flag word) leaves the
    context fit for the next solves.

log_info["passes"] is not compared: a pool sized from another problem's learnt total may legitimately run dry and cost a
second integration; the records may not differ.

Recipe 5 is the stiff Van der Pol workload as the library defines it (workloads.vdp_stiff_batch: the VanDerPol problem with
mu ~ 1000 to t = 3000, BASELINE C5)."""
import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import workloads as W
from tests.common import oracle_batch
from tests.test_gpu_log_gather_widths import RING_OPTIONS, linear_ring_source, ring_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

MEMBERS = ("y_end", "t_end", "h_next", "status", "nfev", "nstep", "naccpt", "nrejct", "njev", "nlu", "y_eval", "eval_idx", "n_filled",
           "t_log", "y_log", "n_log", "seg_cont", "seg_xold", "seg_h", "n_seg", "t_events", "y_events", "n_event_hits", "t_term",
           "log_offsets", "seg_offsets")


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _members(r):
    return {k: _np(getattr(r, k)).copy() for k in MEMBERS if getattr(r, k, None) is not None}


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def _sho_y0(B, seed):
    rng = np.random.default_rng(seed)
    return np.stack([1.0 + 0.1 * rng.standard_normal(B), 0.1 * rng.standard_normal(B)])


class Recipe:
    """name, problem (an IVP or a function ctx -> IVP), inputs, options, the call; `oracle` = (rhs name, extra oracle options)
    where the CPU oracle has the problem"""

    def __init__(self, name, problem, inputs, options, call="batch", oracle=None, device=True):
        self.name, self.problem, self.inputs, self.options, self.call, self.oracle, self.device = name, problem, inputs, options, call, oracle, device

    def args(self):
        y0, p, t0, t1 = self.inputs()
        return np.ascontiguousarray(y0, dtype=np.float64), p, t0, t1

    def run(self, ctx):
        y0, p, t0, t1 = self.args()
        f = self.problem(ctx) if callable(self.problem) else self.problem
        o = ivp_amd.Options(**self.options)
        if self.device or self.call != "batch":
            y0, p = _dev(y0), _dev(p)
            t1 = _dev(t1) if np.ndim(t1) else t1
        if self.call == "logged":
            r = ivp_amd.solve_ivp_batch_logged(f, t0, t1, y0, p, o, ctx)
            return _members(r)
        if self.call == "dense":
            d = ivp_amd.solve_ivp_batch_dense(f, t0, t1, y0, p, o, ctx)
            out = _members(d)
            y, found = d.dense(np.linspace(-1.0, 25.0, 97))
            out["dense_y"], out["dense_found"] = _np(y).copy(), _np(found).copy()
            return out
        return _members(ivp_amd.solve_ivp_batch(f, t0, t1, y0, p, o, ctx))


def _vdp(B, cap=None):
    y0, p, t0, t1 = W.vdp_batch(B)
    return y0, p, t0, (t1 if cap is None else np.minimum(t1, cap))


def _ring8(ctx):
    return ivp_amd.DeviceIVP(linear_ring_source(8), 8, ctx=ctx)


def _ring8_inputs():
    y0, t1 = ring_inputs(8)
    return y0, None, 0.0, t1


def _rk4_wrong_sign(ctx):
    """RK4 with a first_step against the direction of integration: Err(InvalidStepSize), reported by the kernels through the
    context's error flag word"""
    return ivp_amd.solve_ivp_batch(ivp_amd.SHO(), 0.0, 3.0, _dev(_sho_y0(16, 12)), None, ivp_amd.Options(method="RK4", first_step=-0.01), ctx)


class ErrorRecipe(Recipe):
    def __init__(self):
        super().__init__("12-sho16-rk4-wrong-sign-error", None, None, None)

    def run(self, ctx):
        try:
            _rk4_wrong_sign(ctx)
        except ivp_amd.ConfigError as e:
            return {"rc": np.array([e.code], dtype=np.int64)}
        raise AssertionError("RK4 with a first_step of the wrong sign must raise ConfigError")


TOL6 = dict(rtol=1e-6, atol=1e-9)
RECIPES = [
    Recipe("01-cr3bp300-dopri5-end", ivp_amd.CR3BP(), lambda: W.cr3bp_batch(300), dict(method="DOPRI5", **TOL6), oracle=("cr3bp", {})),
    Recipe("02-vdp67-dop853-teval33", ivp_amd.VanDerPol(), lambda: _vdp(67, 60.0),
           dict(method="DOP853", rtol=1e-8, atol=1e-10, t_eval=list(np.linspace(0.0, 60.0, 33))), oracle=("vdp", {})),
    Recipe("03-shoev64-dopri5-deferred-events", ivp_amd.SHOZeroEvent(ivp_amd.EventConfig()), lambda: (_sho_y0(64, 7), None, 0.0, 20.0),
           dict(method="DOPRI5", rtol=1e-8, atol=1e-10, max_events=4), oracle=("sho_ev", dict(event_direction=[0], event_terminal=[0]))),
    Recipe("04-shoev9-dop853-terminal", ivp_amd.SHOZeroEvent(ivp_amd.EventConfig(ivp_amd.Direction.All, 3)), lambda: (_sho_y0(9, 8), None, 0.0, 40.0),
           dict(method="DOP853", rtol=1e-9, atol=1e-12), oracle=("sho_ev", dict(event_direction=[0], event_terminal=[3])), device=False),
    Recipe("05-stiffvdp40-bdf", ivp_amd.VanDerPol(), lambda: W.vdp_stiff_batch(40), dict(method="BDF", rtol=1e-4, atol=1e-6), oracle=("vdp", {})),
    Recipe("06-decay100x5-dopri5-logged", ivp_amd.LinearDecay100(), lambda: (1.0 + 0.1 * np.random.default_rng(3).standard_normal((100, 5)), None, 0.0, 5.0),
           dict(method="DOPRI5", **TOL6), call="logged", oracle=("linear_decay100", {})),
    Recipe("07-cr3bp700-dopri5-logged", ivp_amd.CR3BP(), lambda: W.cr3bp_batch(700), dict(method="DOPRI5", **TOL6), call="logged", oracle=("cr3bp", {})),
    Recipe("08-cr3bp700-dopri5-bounded-dense", ivp_amd.CR3BP(), lambda: W.cr3bp_batch(700), dict(method="DOPRI5", dense_output=True, max_log=256, **TOL6),
           oracle=("cr3bp", {})),
    Recipe("09-vdp700-dop853-logged", ivp_amd.VanDerPol(), lambda: _vdp(700), dict(method="DOP853", rtol=1e-8, atol=1e-10), call="logged", oracle=("vdp", {})),
    Recipe("10-vdp96-csr-dense-and-eval", ivp_amd.VanDerPol(), lambda: _vdp(96, 20.0), dict(method="DOPRI5", **TOL6), call="dense", oracle=("vdp", {})),
    Recipe("11-decay1-rk23-teval7", ivp_amd.ExponentialDecay(), lambda: (np.array([[1.5]]), np.array([[0.5]]), 0.0, 4.0),
           dict(method="RK23", rtol=1e-5, atol=1e-8, t_eval=list(np.linspace(0.0, 4.0, 7))), oracle=("decay", {}), device=False),
    ErrorRecipe(),
    Recipe("13-cr3bp300-dopri5-fma-coop-teval23", ivp_amd.CR3BP(), lambda: W.cr3bp_batch(300),
           dict(method="DOPRI5", fp_mode=ivp_amd.FpMode.FMA, variant=3, t_eval=list(np.linspace(0.0, W.ARENSTORF_PERIOD, 23)), **TOL6),
           oracle=("cr3bp", dict(fma=True))),
    Recipe("14-ring8x130-dopri5-logged-hiprtc", _ring8, _ring8_inputs, dict(RING_OPTIONS), call="logged"),
]
assert len(RECIPES) == 14

_FRESH = {}


def fresh(i):
    """recipe i on a context of its own, once per session"""
    if i not in _FRESH:
        ctx = ivp_amd.Context(0)
        try:
            _FRESH[i] = RECIPES[i].run(ctx)
        finally:
            ctx.close()
    return _FRESH[i]


def _same(got, ref, where):
    assert sorted(got) == sorted(ref), f"{where}: members {sorted(got)} != {sorted(ref)}"
    for k in ref:
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{where}, {k}: {a.dtype}{a.shape} != {b.dtype}{b.shape}"
        if a.dtype == np.float64:
            a, b = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
        assert np.array_equal(a, b), f"{where}, {k}: {np.count_nonzero(a != b)} of {a.size} values differ from the fresh-context run"


WITH_ORACLE = [i for i, r in enumerate(RECIPES) if r.oracle is not None]


@pytest.mark.parametrize("i", WITH_ORACLE, ids=[RECIPES[i].name for i in WITH_ORACLE])
def test_fresh_context_matches_oracle(i):
    rc = RECIPES[i]
    got = fresh(i)
    y0, p, t0, t1 = rc.args()
    rhs, extra = rc.oracle
    opts = {k: v for k, v in rc.options.items() if k not in ("fp_mode", "dense_output")}
    ref = oracle_batch(rhs, y0, p, t0, t1, **{**opts, **extra})
    for k in ("y_end", "t_end"):
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint64), ref[k].view(np.uint64)), (rc.name, k)
    for k in ("status", "naccpt", "nrejct", "nfev"):
        assert np.array_equal(got[k].astype(np.int64), ref[k].astype(np.int64)), (rc.name, k)


ORDERS = {"table": list(range(14)), "reversed": list(range(13, -1, -1)), "rng1": [int(v) for v in np.random.default_rng(1).permutation(14)]}


@pytest.mark.parametrize("order", list(ORDERS))
def test_sequence_equals_fresh_contexts(order):
    refs = [fresh(i) for i in range(14)]          # every fresh context is closed again before the sequence starts
    ctx = ivp_amd.Context(0)
    try:
        for pos, i in enumerate(ORDERS[order]):
            got = RECIPES[i].run(ctx)
            _same(got, refs[i], f"order {order} {ORDERS[order]}, position {pos}, recipe {RECIPES[i].name}")
    finally:
        ctx.close()


def test_an_error_leaves_the_context_usable():
    ctx = ivp_amd.Context(0)
    try:
        with pytest.raises(ivp_amd.ConfigError) as e:
            _rk4_wrong_sign(ctx)
        assert e.value.code == -5 and "step size" in str(e.value)      # IVP_ERR_INVALID_STEP_SIZE
        _same(RECIPES[0].run(ctx), fresh(0), "after the RK4 error, recipe 01")
        _same(RECIPES[6].run(ctx), fresh(6), "after the RK4 error and recipe 01, recipe 07")
    finally:
        ctx.close()
