"""Balanced bulk rounds on the GPU (ivp_amd/csrc/ivp_balance.h, balanced_chunk_kernel_t in rk_global.h, enqueue_round in
ivp_capi.cpp): results never depend on how attempts are cut into launches, so every solve must equal, bit for bit, the same
solve with IVP_TUNE_BALANCE=0 (windowed launches) and the oracle's -- end states, status words and all counters, and for the
logged solve every record.

IVP_TUNE_BALANCE_SLOTS makes the launch loop plan as if the device had 4 (5) wave slots, so a few hundred trajectories take
every path; IVP_TUNE_COOP_CAP_LANES = 256 keeps the bulk path down to 32 trajectories.  The knobs are read once per process:
each (slots, balance) setting is one child process (tests/helpers/balance_dump.py) that runs all its cases; the four children
run side by side, once per module.

Shapes, on 4 slots (windows, hence plans, exist for 256..409, 512..614 and 768..819 list entries):
  443          7 blocks, ragged last block -- the last wave-round would be 87 % full: no window, the plan must decline
  5 * 64       just above the slot count: L = 6 launches of q = 40
  15 * 64 + 1  just below four slot-fulls: 94 % full, the plan must decline
  601          10 blocks, ragged (25 entries): two balanced rounds (every trajectory needs more than the 256 attempts of a
               round and its pair), the second one through the compacted list
  mixed 800    zero-length intervals, a block that dies in its first piece, trajectories that retire mid-round; DOPRI5
               rounds start from 800 and 368 entries, both balanced
and on 5 slots 443 entries (7 blocks, ragged): a window, and a plan.  CR3BP, DOPRI5 strict and FMA, DOP853 strict; the
logged solve (flavour 2) at every uniform size."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import balance_cases as C
from tests.common import oracle_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tests", "helpers", "balance_dump.py")
SETTINGS = {4: ([443, 5 * 64, 15 * 64 + 1, 601], 800), 5: ([443], 0)}
# (slots, size): does a balanced plan exist for the solve's FIRST round?  (ivp_balance_plan, restated in the docstring)
FIRST_ROUND_BALANCED = {(4, 443): False, (4, 320): True, (4, 961): False, (4, 601): True, (4, "mixed800"): True, (5, 443): True}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("balance")
    jobs = {}
    for slots, (sizes, mixed) in SETTINGS.items():
        for bal in (1, 0):
            out = str(tmp / f"s{slots}_b{bal}.npz")
            env = dict(os.environ, IVP_TUNE_BALANCE=str(bal), IVP_TUNE_BALANCE_SLOTS=str(slots), IVP_TUNE_COOP_CAP_LANES="256", IVP_TRACE_LAUNCHES="1")
            for k in ("IVP_TUNE_WINDOW", "IVP_TUNE_LAUNCHES_PER_POLL", "IVP_TUNE_BULK_CHUNK"):
                env.pop(k, None)
            cmd = [sys.executable, HELPER, out, ",".join(map(str, sizes))] + ([str(mixed)] if mixed else [])
            jobs[(slots, bal)] = (subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), out)
    res = {}
    for key, (proc, out) in jobs.items():
        so, se = proc.communicate(timeout=300)
        assert proc.returncode == 0, (key, so[-1000:], se[-3000:])
        trace, cur = {}, None
        for ln in se.splitlines():
            if ln.startswith("case "):
                cur = ln[5:].strip()
                trace[cur] = []
            elif ln.startswith("ivp launch") and cur is not None:
                trace[cur].append(ln.split())
        print(key, [ln for ln in se.splitlines() if ln.startswith("at ")][-1:], "last case started")
        res[key] = (dict(np.load(out)), trace)
    return res


_oracle_cache = {}


def oracle(size, method, fma):
    key = (size, method, fma)
    if key not in _oracle_cache:
        y0, p, t0, t1 = C.mixed_batch(int(size[5:])) if isinstance(size, str) else C.batch(size)
        _oracle_cache[key] = oracle_batch("cr3bp", y0, p, t0, t1, threads=16, fma=fma, **C.opts(method))
    return _oracle_cache[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


CASES = [(s, b) for s, (sizes, mixed) in SETTINGS.items() for b in sizes + ([f"mixed{mixed}"] if mixed else [])]


@pytest.mark.parametrize("method,fma", C.MODES, ids=[f"{m}-{'fma' if f else 'strict'}" for m, f in C.MODES])
@pytest.mark.parametrize("slots,size", CASES, ids=[f"slots{s}-{b}" for s, b in CASES])
def test_balanced_rounds_change_nothing(runs, slots, size, method, fma):
    (bal, tr_bal), (win, tr_win) = runs[(slots, 1)], runs[(slots, 0)]
    nm = C.name(size, method, fma)
    ref = oracle(size, method, fma)
    for k in C.KEYS:
        assert same_bits(bal[f"{nm}.{k}"], win[f"{nm}.{k}"]), f"{nm}.{k}: balanced rounds differ from windows"
        want = np.asarray(ref[k])
        got = bal[f"{nm}.{k}"]
        assert same_bits(got.astype(want.dtype) if got.dtype.kind in "iu" else got, want), f"{nm}.{k}: differs from the oracle"
    # the path that was meant to run did run: "bal" lines in the launch trace of the first round, none with IVP_TUNE_BALANCE=0
    kinds = [ln[3] for ln in tr_bal[nm]]
    assert (kinds[0] == "bal") == FIRST_ROUND_BALANCED[(slots, size)], kinds
    assert "bal" not in [ln[3] for ln in tr_win[nm]]
    if size in (601, "mixed800") and method == "DOPRI5":
        # two balanced rounds (601: 601 entries each; mixed: 800, then 368), each followed by its (bulk, cooperative) pair;
        # the oracle's attempt counts say how many trajectories the second round starts from
        assert int((np.asarray(ref["nstep"]) > 256).sum()) == (601 if size == 601 else 368)
        starts = [i for i, k in enumerate(kinds) if k == "bal" and (i == 0 or kinds[i - 1] != "bal")]
        assert len(starts) == 2, kinds
        assert kinds[starts[1] - 2:starts[1]] == ["bulk", "coop"], kinds


@pytest.mark.parametrize("slots,size", [(s, b) for s, b in CASES if not isinstance(b, str)], ids=[f"slots{s}-{b}" for s, b in CASES if not isinstance(b, str)])
def test_balanced_rounds_with_the_one_pass_step_log(runs, slots, size):
    (bal, tr_bal), (win, _) = runs[(slots, 1)], runs[(slots, 0)]
    nm = f"{size}.logged"
    for k in C.KEYS + ("log_offsets", "t_log", "y_log", "passes"):
        assert same_bits(bal[f"{nm}.{k}"], win[f"{nm}.{k}"]), f"{nm}.{k}: balanced rounds differ from windows"
    assert int(bal[f"{nm}.passes"]) == 1            # the page pool did not run dry: one integration
    assert ([ln[3] for ln in tr_bal[nm]][0] == "bal") == FIRST_ROUND_BALANCED[(slots, size)]
    y0, p, t0, _ = C.batch(size)
    off, tl, yl = bal[f"{nm}.log_offsets"], bal[f"{nm}.t_log"], bal[f"{nm}.y_log"]
    assert int(off[-1]) == len(tl)
    for j in range(size):                           # every record of every trajectory
        s = O.solve_ivp("cr3bp", t0, C.T1_LOGGED, y0[:, j], params=p[:, j], detpow=True, **C.opts("DOPRI5"))
        assert same_bits(tl[off[j]:off[j + 1]], s.t) and same_bits(yl[off[j]:off[j + 1]], s.y), j
