"""The thread-per-trajectory stiff kernels (BDF for n <= 8, Radau IIA(5) for n <= 8, Radau with mass matrices and DAE index
sets; built-in and hiprtc right-hand sides) at every wave density the launch loop can choose, BIT FOR BIT against the
references the suite trusts: the C oracle (strict and FMA builds) for BDF, tests/radau_model.py and
tests/radau_dae_model.py for Radau.  No tolerance anywhere: status, t_end, h_next, y_end, the six counters and every
recorded output, NaN equal to NaN, signed zeros distinguished (tests/wave_density_cases.py: compare()).

Why.  enqueue_round (ivp_capi.cpp) launches these kernels with thin waves, lpw = min(64, max(1, ceil(lanes / cus)))
trajectories per wavefront, so on a device with 256 CUs every batch of up to 256 trajectories -- every other GPU test of
these kernels but one -- steps with ONE active lane per wavefront, and a wavefront is full only from 63 cus + 1 = 16 129
trajectories on.  Lane-divergent Newton and elimination loops, per-lane pivot rows, rejected / restarted / retiring lanes
beside running ones, compact_append on partly filled waves whose lpw changes from round to round, and the BDF build for
two waves per SIMD (`*_occ2`, chosen above 4 * 64 * cus running trajectories) first appear with more than one lane per
wave.  tests/test_wave_density_cases_cpu.py checks, on the references, that the first 64 entries of every base batch do
diverge in these ways.

Two ways in:

1. Through the real policy, in this process, no environment variable: every base batch (B0 = 67 for Radau, 130 for BDF)
   tiled to B trajectories, trajectory b taking the inputs of base trajectory b mod B0, with
     B = 2 cus - 3      two lanes per wave (cus < B <= 2 cus), the last wave ragged,
     B = 63 cus + 1     full waves,
     B = 256 cus + 1    (two BDF cases, strict and FMA) more than one wave per SIMD: the occ2 build runs the first rounds and
                        the ordinary build takes over as the active set shrinks.
   Every copy must equal its base reference row.

2. Pinned through the knobs, which the library reads once per process: children (tests/helpers/wave_density_dump.py) run
   every base batch with IVP_TUNE_BDF_LPW = 1, 2, 7 and 64 (67 = 9 * 7 + 4 and 130 = 18 * 7 + 4: a ragged last wave), and
   the BDF batches with IVP_TUNE_BDF_OCC2 = 1 at LPW = 64 and at the automatic density, where the whole solve runs in the
   occ2 build.  At most four children at a time, each under its own `timeout`; a child that exits non-zero fails the module
   at once with its stderr; nothing is retried.

That a density took effect shows in stats["lane_attempt_slots"]: every wave adds 64 times the `it` of its slowest lane per
launch (chunk_kernel_body, rk_global.h), and `it` counts the calls of the attempt body (any_chunk_body):
  Radau   a_b = nstep_b + the attempts that end in a singular E1 or E2 before the step is counted
              = nstep + n_restart_real + n_restart_complex of the model (radau_attempt counts the step after the
              factorisations; every other restart, rejection and exit happens in an attempt that was counted),
  BDF     a_b = nstep_b, plus one for a trajectory retired by bdf_attempt's entry checks (status 2 or 3) and none for one
              that retires inside its last step (status 0 or 1),
  and a_b = 0 for a zero-length interval, which retires in the init kernel.
With LPW = 1 the count is exactly 64 sum_b a_b; with LPW = 64 it is at most 64 ceil(B0 / 64) max_b a_b (the trajectory
with the most attempts runs in every launch, so the launches' slowest lanes add up to its attempts).  For a base batch
with max nstep <= 2 mean nstep (asserted here and in the CPU test) that is, at B0 = 67,
slots(1) / slots(64) >= 67 mean / (2 max) >= 67 / 4 > 16, and at B0 = 130 (three waves) 130 / 6 > 21; asserted: a factor
of at least 8, and a strict decrease across LPW = 1, 2, 7, 64.

Measured on an MI355X: the module takes 42 s -- 20 s for the six children (the slowest 16.1 s; see CHILD_TIMEOUT), the rest
in process, where a case costs 0.1 .. 0.3 s per batch size and up to 4.7 s when it compiles a hiprtc module for n = 8 first.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import wave_density_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tests", "helpers", "wave_density_dump.py")
ALL = C.all_cases()
BDF = C.cases("bdf")
# measured on an MI355X: the slowest children (IVP_TUNE_BDF_LPW = 2, 7 or 64 with all three families: the torch import, 8 hiprtc
# modules, 27 solves) take 16.1 s of wall time each with four children side by side, the BDF-only ones 3.5 s; the timeout is
# three times the slowest, rounded up
CHILD_TIMEOUT = 49
# the children: tag -> (environment, families)
CHILDREN = {f"lpw{v}": (dict(IVP_TUNE_BDF_LPW=str(v)), "radau,radau_dae,bdf") for v in (1, 2, 7, 64)}
CHILDREN["occ2_lpw64"] = (dict(IVP_TUNE_BDF_OCC2="1", IVP_TUNE_BDF_LPW="64"), "bdf")
CHILDREN["occ2_auto"] = (dict(IVP_TUNE_BDF_OCC2="1"), "bdf")


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _no_knobs():
    set_ = sorted(k for k in os.environ if k.startswith("IVP_TUNE_"))
    assert not set_, f"the launch policy under test is the default one, but {set_} are set"


# ---- 1. the real policy ---------------------------------------------------------------------------------------------------
def _tiled(case, B, chunk):
    idx = np.arange(B) % case.B0
    ref, _ = C.reference(case)
    t = time.time()
    got, _ = C.run(case, B, chunk=chunk)
    dt = time.time() - t
    C.compare(got, ref, idx, f"{case.name}, B = {B}, chunk_attempts = {chunk}")
    print(f"[wave density] {case.name} ({case.kernel_family}) B = {B} chunk = {chunk}: solve {dt:.2f} s, with the comparison {time.time() - t:.2f} s")


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_two_lanes_per_wave_through_the_launch_policy(case):
    cus = _cus()
    B = 2 * cus - 3
    _no_knobs()
    assert cus < B <= 2 * cus and (B + cus - 1) // cus == 2
    for chunk in case.chunks:
        _tiled(case, B, chunk)


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_full_waves_through_the_launch_policy(case):
    cus = _cus()
    B = 63 * cus + 1
    _no_knobs()
    assert B > 63 * cus and min(64, (B + cus - 1) // cus) == 64
    for chunk in case.chunks:
        _tiled(case, B, chunk)


OCC2 = [c for c in BDF if c.occ2_tile]


@pytest.mark.parametrize("case", OCC2, ids=[c.name for c in OCC2])
def test_more_than_one_wave_per_simd_starts_in_the_occ2_build(case):
    """strict and FMA: above 4 * 64 * cus running trajectories pend_launch takes ivp_launch_bdf_*_occ2; the ragged end
    times retire half the batch within the first rounds, after which the ordinary build runs"""
    cus = _cus()
    B = 4 * 64 * cus + 1
    _no_knobs()
    assert B > 4 * 64 * cus and {c.fma for c in OCC2} == {False, True}
    ref, _ = C.reference(case)
    assert np.median(ref["nstep"]) < 0.8 * ref["nstep"].max()   # the active set does shrink below the threshold while work is left
    _tiled(case, B, 0)


# ---- 2. pinned densities ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def children(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wave_density")
    pending = list(CHILDREN.items())
    running, res = [], {}

    def start():
        tag, (knobs, families) = pending.pop(0)
        env = {k: v for k, v in os.environ.items() if not k.startswith("IVP_TUNE_")}
        env.update(knobs)
        out = str(tmp / f"{tag}.npz")
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, HELPER, out, families]
        running.append((tag, out, time.time(), subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))

    while pending or running:
        while pending and len(running) < 4:
            start()
        tag, out, t0, proc = running.pop(0)
        so, se = proc.communicate()
        if proc.returncode != 0:   # at once: nothing more is started, nothing is retried
            for _, _, _, p in running:
                p.kill()
                p.communicate()
            pytest.fail(f"child {tag} ended with status {proc.returncode}\n{so[-1000:]}\n{se[-4000:]}", pytrace=False)
        res[tag] = dict(np.load(out))
        print(f"[wave density] child {tag}: {time.time() - t0:.1f} s of wall time, {float(res[tag]['seconds']):.1f} s in the helper")
    return res


def _child(children, tag, case):
    pre = case.name + "."
    return {k[len(pre):]: v for k, v in children[tag].items() if k.startswith(pre)}


def _attempts(case):
    """(lower bound, upper bound) of sum_b a_b and max_b a_b from the reference: the relation in the module docstring"""
    ref, models = C.reference(case)
    if case.family == "bdf":
        extra = ~np.isin(ref["status"], (0, 1))
        return int(ref["nstep"].sum()), int((ref["nstep"] + extra).sum()), int((ref["nstep"] + extra).max())
    a = np.array([C.attempts_of_model(m) for m in models])
    return int(a.sum()), int(a.sum()), int(a.max())


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_every_pinned_density_gives_the_references_bits(children, case):
    ref, _ = C.reference(case)
    idx = np.arange(case.B0)
    tags = [t for t, (_, fam) in CHILDREN.items() if case.family in fam.split(",")]
    assert len(tags) == (6 if case.family == "bdf" else 4)
    for tag in tags:
        C.compare(_child(children, tag, case), ref, idx, f"{case.name}, child {tag}")
    # ... and so with each other, in every member a run returns (the reference may carry fewer)
    first = _child(children, tags[0], case)
    for tag in tags[1:]:
        other = _child(children, tag, case)
        assert set(other) == set(first)
        C.compare(other, {k: v for k, v in first.items() if k in ref}, idx, f"{case.name}, child {tag} against {tags[0]}")
    # the density took effect: the slot counts of the module docstring
    lo, hi, amax = _attempts(case)
    slots = {t: int(_child(children, t, case)["slots"]) for t in tags}
    print(f"[wave density] {case.name} ({case.kernel_family}) lane_attempt_slots {slots}; 64 sum a_b = {64 * lo}" + ("" if hi == lo else f" .. {64 * hi}"))
    waves = (case.B0 + 63) // 64
    assert 64 * lo <= slots["lpw1"] <= 64 * hi
    assert 0 < slots["lpw64"] <= 64 * waves * amax
    assert slots["lpw1"] >= slots["lpw2"] >= slots["lpw64"] and slots["lpw1"] >= slots["lpw7"] >= slots["lpw64"]
    if case.family == "bdf":   # the occ2 build changes no count: full waves, and the automatic single lane per wave
        assert 0 < slots["occ2_lpw64"] <= 64 * waves * amax
        assert slots["occ2_auto"] == slots["lpw1"]
    if case.slots:
        assert (ref["status"] == 0).all() and ref["nstep"].max() <= 2.0 * ref["nstep"].mean()
        assert slots["lpw1"] > slots["lpw2"] > slots["lpw7"] > slots["lpw64"]
        assert slots["lpw1"] >= 8 * slots["lpw64"]


def test_every_kernel_family_carries_the_slot_count_check():
    assert {c.family for c in ALL if c.slots} == {"radau", "radau_dae", "bdf"}
