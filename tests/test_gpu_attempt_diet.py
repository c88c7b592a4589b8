"""The DOPRI5 attempt on the GPU after the rework of the lane-cooperative data movement (rk_coop.h: 64-bit group
broadcasts, hops that write a fresh register), and the step controller across chunk boundaries in every kernel variant.

Nothing may change by a bit: every kernel variant (0 = auto, 1 = lean, 2 = coefficients resident, 3 = lane-cooperative), in
both arithmetic modes and at chunk lengths that store and reload the controller memory around every attempt (1), often (7)
and rarely (64), against the oracle and against the lean variant."""
import numpy as np
import pytest

from oracle import oracle as O
from ivp_amd import workloads as W
from tests.common import assert_bitexact, gpu_batch, oracle_batch
from tests.test_controller_carry_cpu import CASES

pytestmark = pytest.mark.gpu

VARIANTS = (0, 1, 2, 3)
CHUNKS = (1, 7, 64)
_REF = {}


def reference(name, fast):
    if (name, fast) not in _REF:
        rhs, y0, p, t0, t1, o = CASES[name]()
        _REF[name, fast] = oracle_batch(rhs, y0, p, t0, t1, fma=True, **o) if fast else oracle_batch(rhs, y0, p, t0, t1, **o)
    return _REF[name, fast]


@pytest.mark.parametrize("fast", [False, True], ids=["strict", "fma"])
@pytest.mark.parametrize("name", list(CASES))
def test_every_variant_and_chunk_matches_oracle(name, fast):
    rhs, y0, p, t0, t1, o = CASES[name]()
    ref = reference(name, fast)
    for chunk in CHUNKS:
        lean = None
        for variant in (1, 0, 2, 3):
            got = gpu_batch(rhs, y0, p, t0, t1, fast=fast, chunk=chunk, variant=variant, **o)
            assert_bitexact(got, ref, f"{name} fast={fast} chunk={chunk} variant={variant} vs oracle: ")
            if lean is None:
                lean = got
            else:
                assert_bitexact(got, lean, f"{name} fast={fast} chunk={chunk} variant={variant} vs lean: ")


@pytest.mark.parametrize("beta", [0.0, 0.08])
def test_direct_method_settings(beta):
    """has_settings: beta and safety_factor are run-time values (beta == 0 must give facold^beta == 1 exactly) -- the CTL = true
    kernels, among them every cooperative kernel."""
    y0, p, t0, t1 = W.cr3bp_batch(16)
    o = dict(method="DOPRI5", rtol=1e-6, atol=1e-9, settings=dict(beta=beta, safety_factor=0.8))
    for fast in (False, True):
        ref = oracle_batch("cr3bp", y0, p, t0, t1, fma=True, **o) if fast else oracle_batch("cr3bp", y0, p, t0, t1, **o)
        for chunk in CHUNKS:
            for variant in VARIANTS:
                got = gpu_batch("cr3bp", y0, p, t0, t1, fast=fast, chunk=chunk, variant=variant, **o)
                assert_bitexact(got, ref, f"beta={beta} fast={fast} chunk={chunk} variant={variant}: ")


def _lorenz(B):
    rng = np.random.default_rng(11)
    y0 = 1.0 + 0.1 * rng.standard_normal((3, B))
    p = np.repeat(np.array([[10.0], [28.0], [8.0 / 3.0]]), B, axis=1) * (1.0 + 0.01 * rng.standard_normal((3, B)))
    return "lorenz", y0, p, 0.0, 1.5, dict(method="DOPRI5", rtol=1e-8, atol=1e-10)


def _cr3bp(B):
    y0, p, t0, t1 = W.cr3bp_batch(B)
    return "cr3bp", y0, p, t0, 6.0, dict(method="DOPRI5", rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("B", [1, 7, 9, 67])
@pytest.mark.parametrize("problem", [_cr3bp, _lorenz], ids=["cr3bp", "lorenz"])
def test_cooperative_ragged_groups(problem, B):
    """Partly filled 8-lane groups, rows (two groups) and waves through the cooperative kernels: CR3BP with its own
    cooperative right-hand side, Lorenz (n = 3) through the generic gather."""
    rhs, y0, p, t0, t1, o = problem(B)
    for fast in (False, True):
        ref = oracle_batch(rhs, y0, p, t0, t1, fma=True, **o) if fast else oracle_batch(rhs, y0, p, t0, t1, **o)
        lean = gpu_batch(rhs, y0, p, t0, t1, fast=fast, variant=1, **o)
        coop = gpu_batch(rhs, y0, p, t0, t1, fast=fast, variant=3, **o)
        assert_bitexact(lean, ref, f"{rhs} B={B} fast={fast} lean vs oracle: ")
        assert_bitexact(coop, ref, f"{rhs} B={B} fast={fast} coop vs oracle: ")
        assert_bitexact(coop, lean, f"{rhs} B={B} fast={fast} coop vs lean: ")


def test_cooperative_t_eval_run():
    """The FULL flavour of the cooperative kernels (device DefaultSolOut) uses the same primitives: t_eval samples of 9
    trajectories against the lean kernels and the oracle."""
    rhs, y0, p, t0, t1, o = _cr3bp(9)
    te = np.linspace(t0, t1, 23)
    ref = oracle_batch(rhs, y0, p, t0, t1, t_eval=te, **o)
    lean = gpu_batch(rhs, y0, p, t0, t1, t_eval=te, variant=1, **o)
    coop = gpu_batch(rhs, y0, p, t0, t1, t_eval=te, variant=3, **o)
    for got, what in ((lean, "lean"), (coop, "coop")):
        assert_bitexact(got, ref, f"t_eval {what}: ")
        assert np.array_equal(got["n_filled"], ref["n_filled"]), what
        for b in range(9):
            m = int(ref["n_filled"][b])
            assert m == te.size and np.array_equal(got["y_eval"][:m, :, b], ref["y_eval"][:m, :, b]), (what, b)


def test_cooperative_step_log_run():
    """Every accepted step of 9 trajectories recorded by the cooperative kernels: the lean kernels' records and the oracle's
    Solution.t / Solution.y, bit for bit."""
    rhs, y0, p, t0, t1, o = _cr3bp(9)
    lean = gpu_batch(rhs, y0, p, t0, t1, max_log=400, variant=1, **o)
    coop = gpu_batch(rhs, y0, p, t0, t1, max_log=400, variant=3, **o)
    assert_bitexact(coop, lean, "step log coop vs lean: ")
    for k in ("n_log", "t_log", "y_log"):
        assert np.array_equal(coop[k], lean[k], equal_nan=True), k
    for b in range(9):
        s = O.solve_ivp(rhs, t0, t1, y0[:, b], params=list(p[:, b]), detpow=True, **o)
        n = int(coop["n_log"][b])
        assert n == len(s.t) <= 400
        assert np.array_equal(coop["t_log"][:n, b], s.t) and np.array_equal(coop["y_log"][:n, :, b], s.y), b
