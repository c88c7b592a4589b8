#!/usr/bin/env python3
"""Times the CSR dense output (solve_ivp_batch_dense / ivp_batch_solve_dense_device) on BASELINE C2 beside the bounded
[max_log] dense solve of the same batch and the end-state solve, and the device evaluation (ivp_dense_eval_device) of C2's
segments at 256 shared query times per trajectory.  Meant to run under `rocprofv3 --kernel-trace --stats` too (the
evaluation kernel's own time); writes a JSON record stamped with the kernel-source hash.

  python tools/time_dense.py [--fp strict|fma] [--solves K] [--evals R] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivp_amd  # noqa: E402
from ivp_amd import workloads as W  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_sha import kernel_sources_sha256  # noqa: E402


def timed(fn, k):
    ts = []
    r = None
    for _ in range(k):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return r, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fp", default="strict", choices=["strict", "fma"])
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    f = ivp_amd.CR3BP()
    y0, p, t0, t1 = W.cr3bp_batch(a.batch)
    fp = ivp_amd.FpMode.FMA if a.fp == "fma" else ivp_amd.FpMode.STRICT
    o = dict(method="DOPRI5", rtol=1e-6, atol=1e-9, fp_mode=fp)
    y0d, pd = torch.as_tensor(y0, device=dev), torch.as_tensor(p, device=dev)
    B, n = y0.shape[1], y0.shape[0]
    nc = 5 * n
    solve = lambda opts: ivp_amd.solve_ivp_batch(f, t0, t1, y0d, pd, ivp_amd.Options(**opts))
    solve(o)   # warm-up (first launch, context scratch)
    _, t_end = timed(lambda: solve(o), a.solves)
    d, t_csr = timed(lambda: ivp_amd.solve_ivp_batch_dense(f, t0, t1, y0d, pd, ivp_amd.Options(**o)), a.solves)
    ns = d.n_seg.cpu().numpy().astype(np.int64)
    ml = int(ns.max())
    bounded = dict(o, dense_output=True, max_log=ml)
    solve(bounded)
    b, t_bounded = timed(lambda: solve(bounded), a.solves)
    assert np.array_equal(b.n_seg.cpu().numpy().astype(np.int64), ns)
    del b
    torch.cuda.empty_cache()
    # ---- evaluation: 256 shared query times per trajectory over the whole span ----
    grid = torch.linspace(0.0, float(t1), 256, dtype=torch.float64, device=dev)
    y, found = d.dense(grid)
    assert int((found == 1).sum()) == 256 * B
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_eval = []
    for _ in range(a.evals):
        ev0.record()
        d.dense(grid)
        ev1.record()
        torch.cuda.synchronize()
        t_eval.append(ev0.elapsed_time(ev1))
    nq = 256 * B
    alg = nq * 8 * (nc + 1 + n)            # per query: the segment's coefficients + t + y
    alg_full = nq * 8 * (nc + 3 + n)       # ... + the segment's xold and h
    med = lambda v: float(np.median(v))
    rec = {
        "what": "C2 (100k CR3BP DOPRI5 rtol 1e-6): CSR dense solve vs the bounded [max_log] dense solve vs the end-state solve "
                "(wall ms per solve, host-synchronised); device evaluation at 256 shared query times per trajectory "
                "(torch-event ms per call incl. allocation of y / found)",
        "fp_mode": a.fp, "B": B, "segments": int(ns.sum()), "max_n_seg": ml, "mean_n_seg": float(ns.mean()),
        "end_state_ms": t_end, "bounded_dense_ms": t_bounded, "csr_dense_ms": t_csr,
        "csr_over_bounded": med(t_csr) / med(t_bounded), "csr_over_end_state": med(t_csr) / med(t_end),
        "csr_passes": d.dense_info["passes"], "csr_bytes": d.dense_info["bytes"], "csr_staging_bytes": d.dense_info["staging_bytes"],
        "bounded_bytes": ml * (nc + 2) * 8 * B,
        "eval_queries": nq, "eval_ms": t_eval, "eval_alg_bytes": alg, "eval_alg_tbps": alg / (med(t_eval) * 1e-3) / 1e12,
        "eval_alg_bytes_with_xold_h": alg_full,
        "kernel_sources_sha256": kernel_sources_sha256(),
    }
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
