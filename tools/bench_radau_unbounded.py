#!/usr/bin/env python3
"""What the unbounded forms of the direct Radau call cost: BASELINE C5's batch (10 000 stiff Van der Pol oscillators,
mu ~ 1000, t in [0, 3000], rtol 1e-4, atol 1e-6 -- bench.py's C5 leg) through ivp_amd.Radau.

  end            Radau.solve_batch                       the end state and the counters
  bounded_log    ... Options(max_log = the largest count) the [max_log][B] step log one has to size for the worst trajectory
  logged         Radau.solve_batch_logged                the CSR step log from one integration (page pool + gather)
  bounded_dense  ... Options(dense_output, max_log)      the [max_log][4 n + 2][B] segment block
  dense_csr      Radau.solve_batch_dense                 the CSR segment log (max_log = 1: counting solve + filling solve)
  dense_csr_fit  ... with max_log = the largest count    (every run fits the counting solve's block: one integration)

The legs alternate in ONE process, `--repeats` (default 7) timed solves each after one warm-up; reported per leg: median /
min / max wall ms, the spread, passes, records or segments and the bytes of the result.  Then four such batches one after
the other and through BatchPipeline(streams = 4).map(radau = ...), the same way.

  python tools/bench_radau_unbounded.py --out profiles/r12_radau_unbounded.json [--parent parent.json]
  python tools/bench_radau_unbounded.py --end-only --root <built checkout of the parent commit> --out parent.json

`--end-only` times the `end` leg alone (all the parent commit can do; `--root` imports ivp_amd from it); `--parent` merges
such a file and records ONE check with the spread of the PARENT's repeats as the margin: the blocking end-state path has
not moved.  Everything else is informational.  Exit status 1 if the forms differ from each other (statuses, records, end states) or the check fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HERE = os.path.dirname(os.path.abspath(__file__))
if "--root" in sys.argv:   # before ivp_amd is imported
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ivp_amd  # noqa: E402
from ivp_amd import workloads  # noqa: E402
from ivp_amd.pipeline import BatchPipeline  # noqa: E402
from kernel_sha import kernel_sources_sha256  # noqa: E402

RTOL, ATOL = 1e-4, 1e-6   # bench.py WORKLOADS["c5"]


def stats(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "spread_ms": float(np.max(ts) - np.min(ts)),
            "ms": [round(float(t), 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="JSON of an --end-only run with the parent commit's library")
    ap.add_argument("--end-only", action="store_true")
    ap.add_argument("--root", default=None, help="checkout to import ivp_amd from (default: this one)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=10_000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    y0, mu, t0, t1 = workloads.vdp_stiff_batch(a.batch)
    yd, pd = torch.as_tensor(y0, device=dev), torch.as_tensor(mu, device=dev)
    f, rad = ivp_amd.VanDerPol(), ivp_amd.Radau()
    O = lambda **kw: ivp_amd.Options(rtol=RTOL, atol=ATOL, **kw)
    out = {"tool": "tools/bench_radau_unbounded.py", "kernel_sources_sha256": kernel_sources_sha256(os.path.abspath(ROOT)), "repeats": a.repeats,
           "library": "checkout given with --root" if a.root else "in-tree", "device": torch.cuda.get_device_name(0),
           "workload": f"C5 through Radau: {a.batch} stiff Van der Pol, t in [0, 3000], rtol {RTOL}, atol {ATOL}", "results": {}}
    legs = {"end": lambda: rad.solve_batch(f, t0, t1, yd, pd, O())}
    if not a.end_only:
        first = rad.solve_batch_logged(f, t0, t1, yd, pd, O())
        most = int(first.n_log.max().item())
        out["records"] = {"total": int(first.log_offsets[-1].item()), "largest": most, "smallest": int(first.n_log.min().item())}
        legs["bounded_log"] = lambda: rad.solve_batch(f, t0, t1, yd, pd, O(max_log=most))
        legs["logged"] = lambda: rad.solve_batch_logged(f, t0, t1, yd, pd, O())
        legs["bounded_dense"] = lambda: rad.solve_batch(f, t0, t1, yd, pd, O(dense_output=True, max_log=most))
        legs["dense_csr"] = lambda: rad.solve_batch_dense(f, t0, t1, yd, pd, O(max_log=1))
        legs["dense_csr_fit"] = lambda: rad.solve_batch_dense(f, t0, t1, yd, pd, O(max_log=most))

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    res, ts = {}, {k: [] for k in legs}
    for k, fn in legs.items():   # warm-up: sizes the scratch and the pool
        _, res[k] = timed(fn)
    for _ in range(a.repeats):   # interleaved rounds
        for k, fn in legs.items():
            res[k] = None        # one block of the bounded forms at a time
            t, res[k] = timed(fn)
            ts[k].append(t)
        print(", ".join(f"{k} {ts[k][-1]:.1f} ms" for k in legs), file=sys.stderr, flush=True)
    ok = True
    for k in legs:
        r, e = res[k], stats(ts[k])
        e["status_not_success"] = int((r.status != 0).sum().item())   # informational: C5 has trajectories that end in a status under BDF too
        e["accepted"] = int(r.naccpt.sum().item())
        ok = ok and bool(torch.equal(r.status, res["end"].status))
        n, B = 2, a.batch
        if k == "bounded_log":
            e.update(max_log=most, records=int(r.n_log.sum().item()), bytes=most * (n + 1) * 8 * B)
        elif k == "logged":
            e.update(passes=r.log_info["passes"], records=r.log_info["records"], bytes=r.log_info["records"] * (n + 1) * 8,
                     pool_bytes=r.log_info["pool_bytes"], pool_used_bytes=r.log_info["pool_used_bytes"])
        elif k == "bounded_dense":
            e.update(max_log=most, segments=int(r.n_seg.sum().item()), bytes=most * (4 * n + 2) * 8 * B + most * (n + 1) * 8 * B)
        elif k.startswith("dense_csr"):
            e.update(passes=r.dense_info["passes"], segments=r.dense_info["segments"], bytes=r.dense_info["bytes"], staging_bytes=r.dense_info["staging_bytes"])
        out["results"][k] = e
    same = True
    if not a.end_only:   # the forms agree with each other (the tests hold them to the model)
        lg, bl = res["logged"], res["bounded_log"]
        b = int(torch.argmax(lg.n_log).item())
        lo, hi = int(lg.log_offsets[b].item()), int(lg.log_offsets[b + 1].item())
        same = bool(torch.equal(lg.t_log[lo:hi], bl.t_log[:hi - lo, b])) and bool(torch.equal(lg.n_log.to(torch.int64), bl.n_log.to(torch.int64)))
        same = same and bool(torch.equal(res["dense_csr"].seg_cont, res["dense_csr_fit"].seg_cont)) and bool(torch.equal(lg.y_end, res["end"].y_end))
        out["forms_agree"] = same
        # ---- four batches: one after the other, and four in flight ----
        batches = [dict(t0=t0, t1=t1, y0=yd, params=pd) for _ in range(4)]
        pipe = BatchPipeline(streams=4)
        four = {"serial": lambda: [rad.solve_batch(f, t0, t1, yd, pd, O()) for _ in range(4)],
                "pipeline_streams4": lambda: pipe.map(f, batches, O(), radau=rad)}
        ts4 = {k: [] for k in four}
        r4 = {}
        for k, fn in four.items():
            _, r4[k] = timed(fn)
        for _ in range(a.repeats):
            for k, fn in four.items():
                t, r4[k] = timed(fn)
                ts4[k].append(t)
            print(", ".join(f"{k} {ts4[k][-1]:.1f} ms" for k in four), file=sys.stderr, flush=True)
        out["four_batches"] = {k: stats(ts4[k]) for k in four}
        out["four_batches"]["bit_identical"] = all(bool(torch.equal(x.y_end, y.y_end)) for x, y in zip(r4["serial"], r4["pipeline_streams4"]))
        out["four_batches"]["ratio_serial_over_pipeline"] = out["four_batches"]["serial"]["ms_median"] / out["four_batches"]["pipeline_streams4"]["ms_median"]
        same = same and out["four_batches"]["bit_identical"]
    failed = False
    if a.parent and not a.end_only:
        parent = json.load(open(a.parent))
        pe, e = parent["results"]["end"], out["results"]["end"]
        out["parent"] = {"library": parent.get("library"), "kernel_sources_sha256": parent.get("kernel_sources_sha256"), "end": pe}
        moved = e["ms_median"] - pe["ms_median"]
        out["check"] = {"margin_ms": pe["spread_ms"], "end_moved_ms": moved, "end_unmoved": abs(moved) <= pe["spread_ms"],
                        "same_accepted_steps": e["accepted"] == pe["accepted"]}
        failed = not (out["check"]["end_unmoved"] and out["check"]["same_accepted_steps"])
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 1 if (failed or not ok or not same) else 0


if __name__ == "__main__":
    sys.exit(main())
