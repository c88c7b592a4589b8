"""The deferred in-band guard of the DOPRI5 / DOP853 attempts (ivp_amd/csrc/rk_core.h: IvpInbandAcc), on the CPU.

1. Sufficiency: the folded predicate (two unsigned bounds on the high dwords of r^2, a running minimum of the frexp exponents
   of the four factors, the coefficients once per chunk) must never hold where the per-call definition it replaces
   (ivp_sq_inband on s1, s2; ivp_num_inband on the six products) does not.  2^20 seeded states plus every triple of edge
   values: zeros of both signs, denormals, inf, NaN, the ends of every band +-1 ulp, mu in {0, 1, 2^-60}.
2. The redo path: tests/helpers/inband_redo_main.cpp, a stand-alone program, built as is and with the decision forced to
   "out of band" -- identical bytes for whole DOPRI5 and DOP853 solves of 16 trajectories in every output flavour -- and
   built and run with the host's address and undefined-behaviour sanitizers.
3. The committed late-stage state still has an attempt whose first stage is in band and a later stage is not."""
import os
import subprocess

import numpy as np
import pytest

from tests import inband_deferred_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
REDO_SRC = os.path.join(HERE, "helpers", "inband_redo_main.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return C.build_host(tmp_path_factory.mktemp("inband_host"))


def test_folded_guard_is_sufficient_for_the_per_call_guard(host):
    guards, _ = host
    x, y, z, mu = C.operand_states()
    assert x.size >= 1 << 20
    per_call, folded = guards(x, y, z, mu)
    bad = np.flatnonzero(folded & ~per_call)
    assert bad.size == 0, [(x[i].hex(), y[i].hex(), z[i].hex(), mu[i].hex()) for i in bad[:5]]
    # the draw reaches both answers of both guards, and states the old guard accepts and the new one gives up
    assert per_call.sum() > x.size // 10 and (~per_call).sum() > x.size // 10
    assert folded.sum() > x.size // 10 and (per_call & ~folded).sum() > 0


def test_folded_guard_holds_on_ordinary_states(host):
    guards, _ = host
    per_call, folded = guards(*C.ordinary_states())
    assert per_call.all() and folded.all()


def test_folded_guard_at_the_band_ends(host):
    guards, _ = host
    p2 = lambda e: np.ldexp(1.0, e)
    up, dn = lambda v: np.nextafter(v, np.inf), lambda v: np.nextafter(v, 0.0)
    # mu = 0: a = x, s1 = x^2 (y = z = 0), the products are x, 0; b = x - 1 is of order 1 unless x is
    cases = [  # (x, y, z, mu, folded)
        (p2(-100), 0.0, 0.0, 0.0, True), (dn(p2(-100)), 0.0, 0.0, 0.0, False),        # s1 = 2^-200 is the lower end
        (0.5, p2(99), 0.0, 0.0, True), (0.5, p2(100), 0.0, 0.0, False),               # s < 2^200 (the per-call guard allows =)
        (0.5, p2(-541), 0.0, 0.0, True), (0.5, dn(p2(-541)), 0.0, 0.0, False),        # frexp exponent -540 is |f| >= 2^-541
        (0.5, 0.25, -0.0, 0.0, True), (0.5, 0.25, 5e-324, 0.0, False),
        (0.5, 0.25, 0.0, 1.0, True), (0.5, 0.25, 0.0, p2(-60), False), (0.5, 0.25, 0.0, p2(-51), True),
        (0.5, 0.25, 0.0, dn(p2(-51)), False), (0.5, 0.25, 0.0, np.nan, False), (0.5, 0.25, 0.0, np.inf, False),
        (np.nan, 0.25, 0.0, 0.0, False), (np.inf, 0.25, 0.0, 0.0, False), (0.5, -np.inf, 0.0, 0.0, False),
    ]
    arr = np.array([c[:4] for c in cases], dtype=np.float64).T
    per_call, folded = guards(*arr)
    assert folded.tolist() == [c[4] for c in cases], list(zip(folded.tolist(), cases))
    assert not (folded & ~per_call).any()


def test_late_stage_state_has_a_first_stage_in_band_and_a_later_one_out(host):
    _, trace = host
    y0, mu, g = C.late_stage_state()
    for method in ("DOPRI5", "DOP853"):
        ok = trace(y0, mu, g["t1"], method)
        late = [i for i in range(len(ok)) if ok[i, 0] and not ok[i].all()]
        assert late == g["late_attempts"][method], (method, late)
        assert ok.all(axis=1).sum() > len(ok) // 2      # and most of its attempts stay on the helpers


def _build(out, extra):
    return subprocess.Popen(["g++"] + C.HOST_FLAGS + extra + [REDO_SRC, "-o", out])


def test_redo_path_is_a_pure_recomputation_and_clean_under_sanitizers(tmp_path):
    a, b, s = (str(tmp_path / n) for n in ("redo_asis", "redo_forced", "redo_forced_san"))
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    jobs = [_build(a, ["-O2"]), _build(b, ["-O2", "-DIVP_INBAND_FORCE_REDO"]), _build(s, san + ["-DIVP_INBAND_FORCE_REDO"])]
    assert [j.wait() for j in jobs] == [0, 0, 0]
    outs = {}
    for exe in (a, b, s):
        r = subprocess.run([exe, exe + ".bin"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert ("every stage block redone" in r.stdout) == (exe != a)
        outs[exe] = open(exe + ".bin", "rb").read()
        # 2 chunk lengths x (4 DOPRI5 + 5 DOP853 flavours); trajectories finish, run out of steps and stall at a collision
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("method")]
        assert len(lines) == 18 and all(" 3" in ln.split("status")[1] and " 0" in ln.split("status")[1] for ln in lines)
    assert len(outs[a]) > 1_000_000
    assert outs[a] == outs[b], "a redone stage block changed a result"
    assert outs[s] == outs[a]
