"""The DOPRI5 step controller across chunk boundaries: the kernel bodies of rk_core.h, run lane by lane on the CPU, against
the oracle, bit for bit.

The controller memory (facold, the reject flag, h) lives in the lane for one chunk of attempts and in the state arrays
between chunks, so the chunk length decides how often it takes either way: chunk = 1 stores and reloads it around every
attempt, chunk = 64 carries it.  The four cases cover the controller's branches: accepted and rejected steps (CR3BP, Van
der Pol), err below the 1e-4 clamp of facold on every step (SHO under a small max_step) and err == 0, where the power
err^expo1 leaves its common path (y' = 0).  Written for a carried log2(facold) in the lane (profiles/EXPERIMENTS.md 4f:
measured, no kernel time gained, dropped); the cases hold for any change to this part of dopri5_attempt."""
import numpy as np
import pytest

from ivp_amd import workloads as W
from tests.common import assert_bitexact, emul_batch, oracle_batch

CHUNKS = (1, 2, 7, 64)


def _cr3bp():
    y0, p, t0, t1 = W.cr3bp_batch(72)
    return "cr3bp", y0, p, t0, t1, dict(method="DOPRI5", rtol=1e-6, atol=1e-9)


def _vdp():
    # stiff-ish Van der Pol: the step size is limited by stability, so rejections are frequent
    B = 16
    y0 = np.repeat(np.array([[2.0], [0.0]]), B, axis=1) * (1.0 + 0.01 * np.arange(B) / B)
    p = np.linspace(5.0, 60.0, B).reshape(1, B)
    return "vdp", y0, p, 0.0, 12.0, dict(method="DOPRI5", rtol=1e-5, atol=1e-8)


def _sho_clamped():
    # max_step far below what rtol = 1e-3 allows: err < 1e-4 in every attempt, so facold is the clamp constant 1e-4
    rng = np.random.default_rng(5)
    B = 9
    y0 = np.stack([np.cos(rng.uniform(0, 1, B)), np.sin(rng.uniform(0, 1, B))])
    return "sho", y0, None, 0.0, 1.0, dict(method="DOPRI5", rtol=1e-3, atol=1e-6, max_step=1e-2)


def _zero():
    # y' = 0: err == 0 exactly, the first power leaves the common path
    return "zero", np.ones((3, 5)), None, 0.0, 10.0, dict(method="DOPRI5", rtol=1e-9, atol=1e-12)


CASES = {"cr3bp": _cr3bp, "vdp": _vdp, "sho-clamped": _sho_clamped, "zero": _zero}
_REF = {}


def reference(name):
    if name not in _REF:
        rhs, y0, p, t0, t1, o = CASES[name]()
        _REF[name] = oracle_batch(rhs, y0, p, t0, t1, **o)
    return _REF[name]


@pytest.mark.parametrize("fast", [False, True], ids=["strict", "fma"])
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", list(CASES))
def test_controller_matches_oracle_at_every_chunk_length(name, chunk, fast):
    rhs, y0, p, t0, t1, o = CASES[name]()
    ref = reference(name) if not fast else oracle_batch(rhs, y0, p, t0, t1, fma=True, **o)
    got = emul_batch(rhs, y0, p, t0, t1, chunk=chunk, fast=fast, **o)
    assert_bitexact(got, ref, f"{name} chunk={chunk} fast={fast}: ")


def test_vdp_case_rejects_and_recovers():
    """Not vacuous: the Van der Pol case rejects steps, and a rejection is directly followed by an accept -- a trajectory that
    ends with Success ends with an accepted attempt, so the last of its rejections has an accept right behind it."""
    ref = reference("vdp")
    assert ref["nrejct"].sum() > 0
    assert ((ref["nrejct"] > 0) & (ref["status"] == 0)).any()
    # a counted rejection comes after at least two accepted steps (dopri5.rs:455), so the facold it meets is one that an
    # accepted attempt left, not the initial constant
    assert (ref["naccpt"][ref["nrejct"] > 0] >= 2).all()


def test_sho_case_uses_the_clamp_constant_on_every_step():
    """Every step of the clamped case is max_step long (about (t1 - t0) / max_step accepted steps, none rejected).  At
    h = 1e-2 the local error of a fifth-order pair on y'' = -y is of the order h^6 = 1e-12, against a scale of
    atol + rtol |y| ~ 1e-3: err ~ 1e-9, four decades below the clamp at 1e-4, so facold is the constant throughout."""
    ref = reference("sho-clamped")
    assert ref["nrejct"].sum() == 0
    assert (ref["naccpt"] >= 100).all() and (ref["naccpt"] <= 102).all()


def test_zero_case_has_zero_error():
    ref = reference("zero")
    assert (ref["status"] == 0).all() and ref["nrejct"].sum() == 0
    assert np.array_equal(ref["y_end"], np.ones((3, 5)))
