"""Preconditions of tests/test_gpu_wave_density.py, checked on the references alone (no device).

A dense wavefront proves nothing if its lanes walk in step, so every base batch of tests/wave_density_cases.py must show,
among its first 64 entries (the lanes of its first full wavefront), what it claims: different Newton iteration count
sequences, different attempt counts, a rejected step, different pivot rows at the same factorisation index, and the
NaN / zero-length / max_steps trajectories of the mixed batch.  The cases whose lane_attempt_slots are compared across
wave densities must have max nstep <= 2 mean nstep (see the GPU module's docstring).  These are conditions on the inputs,
not measurements: an input that fails one is replaced.

Wall time: 16 s for the whole module on one CPU core (the Radau models of the 16 Radau batches take 11 s of it, the C
oracle's 11 BDF batches under 1 s).
"""
import numpy as np
import pytest

from tests import radau_model as M
from tests import wave_density_cases as C

CASES = C.all_cases()


def _first64(case):
    ref, models = C.reference(case)
    return {k: v[..., :64] for k, v in ref.items() if not k.startswith("csr_")}, models[:64]


def test_the_base_batches_have_the_sizes_the_wave_arithmetic_assumes():
    assert C.B0_RADAU == 67 and C.B0_BDF == 130
    for c in CASES:
        assert c.B0 == (C.B0_BDF if c.family == "bdf" else C.B0_RADAU), c.name
    assert len({c.name for c in CASES}) == len(CASES)
    # every family the launch policy treats alike is there, built-in and hiprtc
    assert {c.kernel_family for c in CASES} >= {"BDF strict", "BDF FMA", "BDF strict (hiprtc)", "Radau", "Radau (hiprtc)", "Radau DAE (hiprtc)"}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_first_wave_of_every_base_batch_diverges_where_the_case_claims_it(case):
    ref, models = _first64(case)
    claims = set(case.claims)
    assert claims, "a case that claims nothing tests nothing"
    if "newton" in claims:
        assert len({tuple(m.newton_counts) for m in models}) >= 2
    if "attempts" in claims:
        if case.family == "bdf":   # attempts = nstep or nstep + 1 (the GPU module's docstring): two apart is different for sure
            assert int(ref["nstep"].max()) - int(ref["nstep"].min()) >= 2
        else:
            assert len({C.attempts_of_model(m) for m in models}) >= 2
    if "reject" in claims:
        assert (ref["nrejct"] > 0).any()
    if "pivots" in claims:
        per = [C.pivots_by_factorisation(m) for m in models]
        assert any(len({p[k] for p in per if len(p) > k}) >= 2 for k in range(max(len(p) for p in per)))
        assert any(len(v) > 1 and v[0] == "real" for p in per for v in p) and any(len(v) > 1 and v[0] == "complex" for p in per for v in p)
    if "nan" in claims:
        assert ref["status"][17] != M.SUCCESS or np.isnan(ref["y_end"][:, 17]).any()
        assert np.isnan(case.params[0, 17])
    if "zero_length" in claims:
        assert case.t1[5] == case.t0 and ref["status"][5] == 0 and ref["nstep"][5] == 0 and ref["h_next"][5] == 0.0
    if "max_steps" in claims:
        out = ref["status"] == M.NEED_LARGER_NMAX
        assert out.any() and (ref["status"] == M.SUCCESS).sum() > 1 and (ref["nstep"][out] == case.opts["max_steps"] + 1).all()
    if "newton_restart" in claims:
        assert any(m.n_restart_newton > 10 and m.naccpt > 0 for m in models)
    if "log_overflow" in claims:
        assert (ref["n_log"] > case.opts["max_log"]).any() and (ref["n_log"] <= case.opts["max_log"]).any()
    if "dense_fits" in claims:   # every segment of every trajectory is compared
        assert 3 < ref["n_seg"].max() <= case.opts["max_log"] and len(set(ref["n_seg"].tolist())) >= 2
    if "wrong_partition" in claims:
        assert list(ref["status"]) == [M.STEP_TOO_SMALL if b % 2 else M.SUCCESS for b in range(64)]
    if "ragged_end" in claims:
        assert np.ndim(case.t1) == 1 and case.t1[:64].max() > 4.0 * case.t1[:64].min()
    if "terminal_event" in claims:
        assert (ref["status"] == 1).all() and (ref["n_event_hits"][0] == 1).all() and len(set(ref["t_events"][0, 0].tolist())) >= 32
    if case.opts.get("t_eval") is not None:
        assert len(set(ref["n_filled"].tolist())) >= 2 or case.family != "bdf"   # ragged ends: the grids are cut at different points
        assert ref["n_filled"].max() < len(case.opts["t_eval"])                  # a point outside the span is never emitted


@pytest.mark.parametrize("case", [c for c in CASES if c.slots], ids=[c.name for c in CASES if c.slots])
def test_the_slot_count_cases_are_balanced_enough_for_the_factor_the_gpu_test_asserts(case):
    ref, _ = C.reference(case)
    assert (ref["status"] == 0).all()
    assert ref["nstep"].max() <= 2.0 * ref["nstep"].mean()
    assert {c.family for c in CASES if c.slots} == {"radau", "radau_dae", "bdf"}


def test_the_comparison_sees_a_single_bit_a_signed_zero_and_a_nan():
    case = C.by_name("radau_vdp_dense")
    ref, _ = C.reference(case)
    idx = np.arange(2 * case.B0 + 5) % case.B0
    got = {k: v[..., idx].copy() for k, v in ref.items()}
    C.compare(got, ref, idx)
    for k, where in (("y_end", (1, 70)), ("h_next", (69,)), ("seg_cont", (2, 3, 133)), ("nfev", (4,))):
        bad = {m: v.copy() for m, v in got.items()}
        if bad[k].dtype.kind == "f":
            bad[k][where] = np.nextafter(bad[k][where], np.inf)
        else:
            bad[k][where] += 1
        with pytest.raises(AssertionError):
            C.compare(bad, ref, idx)
    zero = {m: v.copy() for m, v in got.items()}
    zero["y_end"][0, idx == 3] = 0.0
    ref0 = {m: v.copy() for m, v in ref.items()}
    ref0["y_end"][0, 3] = -0.0
    with pytest.raises(AssertionError):
        C.compare(zero, ref0, idx)
    nan = {m: v.copy() for m, v in got.items()}
    nan["y_end"][0, idx == 3] = np.nan
    ref0["y_end"][0, 3] = np.nan
    C.compare(nan, ref0, idx)
    # per-trajectory grids: the CSR records of a tiled batch are the base block repeated; one wrong sample is seen
    rag = C.by_name("radau_vdp_ragged")
    rref, _ = C.reference(rag)
    offs = np.concatenate([[0], np.cumsum(rref["csr_sizes"][idx])])
    block = lambda v: np.concatenate([v] * 2 + [v[:int(np.cumsum(rref["csr_sizes"])[4])]])
    rgot = {k: v[..., idx].copy() for k, v in rref.items() if not k.startswith("csr_")}
    rgot.update(eval_offsets=offs, y_eval=block(rref["csr_y"]), eval_idx=block(rref["csr_idx"]))
    assert len(rgot["y_eval"]) == offs[-1]
    C.compare(rgot, rref, idx)
    rgot["y_eval"][int(offs[70]), 1] += 1e-9
    with pytest.raises(AssertionError):
        C.compare(rgot, rref, idx)
    # a slot past a trajectory's segment count is never written and never compared
    past = {m: v.copy() for m, v in got.items()}
    past["seg_h"][int(ref["n_seg"][1]), 1] = 123.0
    C.compare(past, ref, idx)
