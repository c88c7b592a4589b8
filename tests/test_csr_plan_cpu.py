"""The range planner of the CSR logs' filling solve (ivp_amd/csrc/ivp_csr_plan.h) on the CPU: which trajectories share one
bounded staging block is a pure integer function, so it is proven here before any kernel runs.

tests/helpers/csr_plan_main.cpp sweeps B in 1..200 trajectories, needs that are all 0, all 1, small, small with one large
outlier and a mix of those, slot sizes of 8, 56, 264 and 4096 bytes, and budgets from one byte (below one slot) to twice the
block of the whole batch.  For every case: the ranges tile [0, B) in order without gap or overlap; a range's depth is
max(its largest need, 1); a range of more than one trajectory fits the budget; a range is maximal (one more trajectory
would not fit).  These four determine the greedy plan uniquely.

The program is stand-alone, host only, and built with -fsanitize=address,undefined."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_range_plan_sweep(tmp_path):
    exe = str(tmp_path / "csr_plan")
    subprocess.run(["g++"] + SAN + [os.path.join(HERE, "helpers", "csr_plan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1].replace(",", "").split()
    # "csr plan: C cases, R ranges, S split, W whole, O one-per-trajectory, 0 failures": every case of the sweep was looked
    # at, and batches in one range, in several and in one range per trajectory all occur
    cases, ranges, split, whole, singles, failures = (int(last[i]) for i in (2, 4, 6, 8, 10, 12))
    assert failures == 0 and cases == 200 * 5 * 4 * 11
    assert split > 10_000 and whole > 10_000 and singles > 1_000 and ranges > cases
