#!/usr/bin/env python3
"""What the always-multiplied mass matrix costs on the group Radau kernels at n = 64: lin_matrix(64) of
tests/test_gpu_radau_group.py (y' = A y in component form, jac_col) through ``DeviceIVP(..., mass_col=True)`` with M = I
against the plain call on the same batch -- the same steps, bit for bit; the mass form reads M from LDS in the assembly and
in every mass-contribution sum and keeps one workgroup per CU either way.  For the record, not a gate.  The method of
tools/time_radau_dense64.py: one warm-up solve per form, then REPS interleaved repeats (mass, plain, mass, plain, ...);
prints one JSON line per batch size with the median and the min / max of each form.
  python tools/time_radau_group_mass.py > radau_group_mass.jsonl"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ivp_amd  # noqa: E402
from tests import radau_group_dae_problems as P  # noqa: E402
from tests import test_gpu_radau_group as G  # noqa: E402

N, RTOL, ATOL, T1, REPS = 64, 1e-6, 1e-8, 0.1, 7


def main():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    src = G.lin_source(G.lin_matrix(N), True)
    plain_prob = ivp_amd.DeviceIVP(src, N, jac=True)
    mass_prob = ivp_amd.DeviceIVP(src + P.identity_mass_source(), N, jac=True, mass_col=True)
    opt = ivp_amd.Options(rtol=RTOL, atol=ATOL)
    for B in (256, 4096):
        y0 = torch.as_tensor(1.0 + 0.5 * rng.standard_normal((N, B)), device=dev)
        mass = lambda out=None: ivp_amd.Radau().solve_batch(mass_prob, 0.0, T1, y0, None, opt, out=out)
        plain = lambda out=None: ivp_amd.Radau().solve_batch(plain_prob, 0.0, T1, y0, None, opt, out=out)
        res = {"mass": mass(), "plain": plain()}   # warm-up: code objects, buffers
        torch.cuda.synchronize()
        ms = {"mass": [], "plain": []}
        for _ in range(REPS):
            for name, fn in (("mass", mass), ("plain", plain)):
                t = time.perf_counter()
                res[name] = fn(res[name])
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t) * 1e3)
        row = {"problem": "lin_matrix(64), M = I", "B": B, "rtol": RTOL, "atol": ATOL, "t1": T1, "reps": REPS}
        for name in ("mass", "plain"):
            r = res[name]
            row.update({f"{name}_ms_median": statistics.median(ms[name]), f"{name}_ms_min": min(ms[name]), f"{name}_ms_max": max(ms[name]),
                        f"{name}_accepted": int(r.naccpt.sum().item()), f"{name}_nlu": int(r.nlu.sum().item()),
                        f"{name}_nfev": int(r.nfev.sum().item()), f"{name}_all_success": bool((r.status == 0).all().item())})
        row["mass_over_plain"] = row["mass_ms_median"] / row["plain_ms_median"]
        row["y_end_bit_identical"] = bool(torch.equal(res["mass"].y_end, res["plain"].y_end))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
