#!/usr/bin/env python3
"""Radau IIA(5) in its wide form (64 < n <= 512, radau_group.h) beside BDF on the problem the form exists for: the
method-of-lines heat equation on 256 interior points, compiled in component form with jac_col, B = 256 and B = 4096
trajectories with distinct diffusivities, the same rtol / atol for both methods (BDF in dense n x n storage).  Also the time
hiprtc takes to build the Radau module of an n = 512 problem (first solve minus second solve on one trajectory).
For the record, not a gate: nothing depends on the outcome.  The method of tools/time_radau_group_mass.py: one warm-up solve
per method, then REPS interleaved repeats (radau, bdf, radau, bdf, ...); medians with min / max.
  python tools/bench_radau_wide.py --out radau_wide.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ivp_amd  # noqa: E402

N, RTOL, ATOL, T1, REPS = 256, 1e-6, 1e-8, 0.05, 7


def heat_source(n):
    return ("__device__ double ode_comp(int i, double t, const double* y, const double* p) {\n"
            f"  const double left = i > 0 ? y[i - 1] : 0.0, right = i < {n - 1} ? y[i + 1] : 0.0;\n"
            "  return p[0] * (left - 2.0 * y[i] + right);\n}\n"
            "__device__ void jac_col(int col, double t, const double* y, double* column, const double* p) {\n"
            "  if (col > 0) column[col - 1] = p[0];\n"
            "  column[col] = -2.0 * p[0];\n"
            f"  if (col < {n - 1}) column[col + 1] = p[0];\n}}\n")


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="256,4096")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    x = np.arange(1, N + 1) / (N + 1.0)
    prob = ivp_amd.DeviceIVP(heat_source(N), N, params=[1.0], jac=True)
    o_radau = ivp_amd.Options(rtol=RTOL, atol=ATOL)
    o_bdf = ivp_amd.Options(method="BDF", rtol=RTOL, atol=ATOL)
    rows = []
    for B in (int(v) for v in args.batches.split(",")):
        kappa = (N + 1) ** 2 * (0.5 + np.arange(B) / B)   # kappa / dx^2 from 0.5 to 1.5
        y0 = np.sin(np.pi * x)[:, None] + 0.25 * np.sin(5 * np.pi * x)[:, None] * np.linspace(0.0, 1.0, B)[None, :]
        y0, par = torch.as_tensor(y0, device=dev), torch.as_tensor(kappa[None, :].copy(), device=dev)
        radau = lambda out=None: ivp_amd.Radau().solve_batch(prob, 0.0, T1, y0, par, o_radau, out=out)
        bdf = lambda out=None: ivp_amd.solve_ivp_batch(prob, 0.0, T1, y0, par, o_bdf, out=out)
        res = {"radau": radau(), "bdf": bdf()}   # warm-up: code objects, buffers
        ms = {"radau": [], "bdf": []}
        for _ in range(REPS):
            for name, fn in (("radau", radau), ("bdf", bdf)):
                res[name], dt = timed(lambda: fn(res[name]))
                ms[name].append(dt)
        row = {"problem": f"heat equation, n = {N}, jac_col", "B": B, "rtol": RTOL, "atol": ATOL, "t1": T1, "reps": REPS}
        for name in ("radau", "bdf"):
            r = res[name]
            row.update({f"{name}_ms_median": statistics.median(ms[name]), f"{name}_ms_min": min(ms[name]), f"{name}_ms_max": max(ms[name]),
                        f"{name}_accepted": int(r.naccpt.sum().item()), f"{name}_nlu": int(r.nlu.sum().item()), f"{name}_njev": int(r.njev.sum().item()),
                        f"{name}_nfev": int(r.nfev.sum().item()), f"{name}_all_success": bool((r.status == 0).all().item())})
        lam1 = kappa * (2.0 - 2.0 * np.cos(np.pi / (N + 1)))
        lam5 = kappa * (2.0 - 2.0 * np.cos(5 * np.pi / (N + 1)))
        exact = np.exp(-lam1 * T1)[None, :] * np.sin(np.pi * x)[:, None] + \
            0.25 * np.linspace(0.0, 1.0, B)[None, :] * np.exp(-lam5 * T1)[None, :] * np.sin(5 * np.pi * x)[:, None]
        for name in ("radau", "bdf"):
            row[f"{name}_max_error_vs_eigenmodes"] = float(np.abs(res[name].y_end.cpu().numpy() - exact).max())
        row["radau_over_bdf"] = row["radau_ms_median"] / row["bdf_ms_median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    # the hiprtc build of the n = 512 Radau module: the first solve builds it, the second runs it
    p512 = ivp_amd.DeviceIVP(heat_source(512), 512, params=[1.0], jac=True)
    y512 = torch.as_tensor(np.sin(np.pi * np.arange(1, 513) / 513.0)[:, None].copy(), device=dev)
    k512 = torch.as_tensor(np.array([[513.0 ** 2]]), device=dev)
    solve512 = lambda: ivp_amd.Radau().solve_batch(p512, 0.0, 1e-3, y512, k512, o_radau)
    _, first = timed(solve512)
    r2, second = timed(solve512)
    build = {"n": 512, "first_solve_ms": first, "second_solve_ms": second, "hiprtc_build_ms": first - second,
             "second_solve_success": bool((r2.status == 0).all().item()), "jit_cache": bool(os.environ.get("IVP_JIT_CACHE_DIR"))}
    print(json.dumps(build), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"heat256": rows, "radau_module_n512": build}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
