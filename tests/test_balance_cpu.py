"""Balanced bulk rounds (ivp_amd/csrc/ivp_balance.h) on the CPU: the schedule is a pure integer function, so everything the
kernel and the launch loop rely on is proven here before any kernel runs.

1. The plan: tests/helpers/balance_plan_main.cpp sweeps nb in 1..6000 blocks (full and with a one-entry last block), S in
   {1, 2, 3, 4, 7, 1024} wave slots, R in {64, 192, 256} attempts per round and chunk in {16, 64}.  For every applicable plan:
   every block receives exactly R attempts over the round, no block appears in two workgroups of one launch, no workgroup
   exceeds the quota q, only the trailing workgroup of a launch is short, a block's "last piece" is the one in its highest
   launch; plans that do not apply are reported as such (against the rules restated independently); BASELINE C2 gives
   L = 5, q = 59, 5087 segments.
2. The host emulation: tests/helpers/balance_emul_main.cpp drives 443 CR3BP trajectories (7 blocks, the last ragged; intervals
   of zero length, blocks that die early) through the kernel bodies with the balanced schedule on 5, 4, 2 and 1 wave slots
   and with the plain schedule: bit-identical end states, counters and step logs, in both arithmetic modes.

Both programs are stand-alone, host only, and built with -fsanitize=address,undefined."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
FP = ["-march=x86-64-v3", "-fno-fast-math", "-ffp-contract=off", "-Wno-unknown-pragmas"]


def test_plan_sweep(tmp_path):
    exe = str(tmp_path / "balance_plan")
    subprocess.run(["g++"] + SAN + [os.path.join(HERE, "helpers", "balance_plan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1].split()
    # "balance plan: A applicable, D not applicable, 0 failures": both kinds occur, and every case of the sweep was looked at
    applicable, declined, failures = int(last[2]), int(last[4]), int(last[-2])
    assert failures == 0 and applicable > 10_000 and declined > 10_000
    assert applicable + declined == 2 * 6000 * 6 * 3 * 2


def test_host_emulation_of_the_balanced_schedule_is_bit_identical(tmp_path):
    src = os.path.join(HERE, "helpers", "balance_emul_main.cpp")
    exes = {fast: str(tmp_path / f"balance_emul_{fast}") for fast in (0, 1)}
    jobs = [subprocess.Popen(["g++"] + SAN + FP + [f"-DIVP_FAST={fast}", src, "-o", exe]) for fast, exe in exes.items()]
    assert [j.wait() for j in jobs] == [0, 0]
    for fast, exe in exes.items():
        r = subprocess.run([exe], capture_output=True, text=True)
        print(r.stdout[-3000:])
        assert r.returncode == 0, (fast, r.stdout[-3000:], r.stderr[-3000:])
        lines = [ln for ln in r.stdout.splitlines() if "balanced rounds" in ln]
        # 3 solves (DOPRI5 end state, DOPRI5 step log, DOP853 end state) x 4 slot counts, each with at least one balanced round
        assert len(lines) == 12 and all(ln.endswith("bit-identical") and " 0 balanced" not in ln for ln in lines), lines
        assert r.stdout.strip().splitlines()[-1] == "0 failures"
