#!/usr/bin/env python3
"""Radau IIA(5) (radau_group.h: factors in LDS) against BDF on the built-in dense 64-state system, end-state flavour, the
same rtol / atol: batches of 256 and 4096 trajectories.  For the record, not a gate.  One warm-up solve per (method, batch),
then REPS interleaved repeats (Radau, BDF, Radau, BDF, ...); prints one JSON line per batch size with the median and the
min / max of each method, the accepted-step counts and the refactorisation counts.
  python tools/time_radau_dense64.py > radau_dense64.jsonl"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ivp_amd  # noqa: E402

RTOL, ATOL, T1, REPS = 1e-6, 1e-9, 0.6, 7


def main():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    for B in (256, 4096):
        y0 = torch.as_tensor(1.0 + 0.5 * rng.standard_normal((64, B)), device=dev)
        k = torch.as_tensor(np.full((1, B), 3.0) * (1.0 + 0.2 * rng.uniform(-1, 1, (1, B))), device=dev)
        prob = ivp_amd.Dense64()
        radau = lambda out=None: ivp_amd.Radau().solve_batch(prob, 0.0, T1, y0, k, ivp_amd.Options(rtol=RTOL, atol=ATOL), out=out)
        bdf = lambda out=None: ivp_amd.solve_ivp_batch(prob, 0.0, T1, y0, k, ivp_amd.Options(method="BDF", rtol=RTOL, atol=ATOL), out=out)
        res = {"radau": radau(), "bdf": bdf()}   # warm-up: code objects, buffers
        torch.cuda.synchronize()
        ms = {"radau": [], "bdf": []}
        for _ in range(REPS):
            for name, fn in (("radau", radau), ("bdf", bdf)):
                t = time.perf_counter()
                res[name] = fn(res[name])
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t) * 1e3)
        row = {"problem": "dense64", "B": B, "rtol": RTOL, "atol": ATOL, "t1": T1, "reps": REPS}
        for name in ("radau", "bdf"):
            r = res[name]
            row.update({f"{name}_ms_median": statistics.median(ms[name]), f"{name}_ms_min": min(ms[name]), f"{name}_ms_max": max(ms[name]),
                        f"{name}_accepted": int(r.naccpt.sum().item()), f"{name}_nlu": int(r.nlu.sum().item()),
                        f"{name}_nfev": int(r.nfev.sum().item()), f"{name}_all_success": bool((r.status == 0).all().item())})
        row["max_abs_diff_y_end"] = float((res["radau"].y_end - res["bdf"].y_end).abs().max().item())
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
