#!/usr/bin/env python3
"""What event functions cost on the direct Radau call: BASELINE C5's batch (10 000 stiff Van der Pol oscillators, mu ~ 1000,
t in [0, 3000], rtol 1e-4, atol 1e-6 -- bench.py's C5 leg, as in tools/bench_radau_unbounded.py) with the event y[0] = 0.

  end           Radau.solve_batch, built-in VanDerPol       the end state and the counters (the leg of the one check)
  end_jit       Radau.solve_batch, the compiled snippet     the same batch without events, the kernels the event legs derive from
  events_1pass  Radau.solve_batch_events, max_events = most every run fits the counting solve's block: one integration
  events_2pass  Radau.solve_batch_events, max_events = 0    count only, then the filling solve

The legs alternate in ONE process, `--repeats` (default 7) timed solves each after one warm-up; reported per leg: median /
min / max wall ms, the spread, passes, records and bytes.  No target is set for the event legs.

  python tools/bench_radau_events.py --out profiles/r13_radau_events.json [--parent parent.json]
  python tools/bench_radau_events.py --end-only --root <built checkout of the parent commit> --out parent.json

`--end-only` times the `end` leg alone (all the parent commit can do; `--root` imports ivp_amd from it, in a process of its
own); `--parent` merges such a file and records the ONE check, with the spread of the PARENT's repeats as the margin: the
end-state Radau solve without events has not moved.  Both spreads are recorded.  Exit status 1 if the event legs differ from
each other or from the event-free end state, or the check fails."""
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
from kernel_sha import kernel_sources_sha256  # noqa: E402

RTOL, ATOL = 1e-4, 1e-6   # bench.py WORKLOADS["c5"]
ODE = ("__device__ void ode(double t, const double* y, double* d, const double* p) {\n"
       "  d[0] = y[1];\n  d[1] = p[0] * (1.0 - y[0] * y[0]) * y[1] - y[0];\n}\n")   # RhsVdp's operations, unfused
EVENTS = "__device__ void events(double t, const double* y, double* g, const double* p) { g[0] = y[0]; }\n"


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
    rad = ivp_amd.Radau()
    O = lambda **kw: ivp_amd.Options(rtol=RTOL, atol=ATOL, **kw)
    out = {"tool": "tools/bench_radau_events.py", "kernel_sources_sha256": kernel_sources_sha256(os.path.abspath(ROOT)), "repeats": a.repeats,
           "library": "checkout given with --root" if a.root else "in-tree", "device": torch.cuda.get_device_name(0),
           "workload": f"C5 through Radau: {a.batch} stiff Van der Pol, t in [0, 3000], rtol {RTOL}, atol {ATOL}; event y[0] = 0", "results": {}}
    legs = {"end": lambda: rad.solve_batch(ivp_amd.VanDerPol(), t0, t1, yd, pd, O())}
    if not a.end_only:
        p0 = (float(np.asarray(mu).reshape(-1)[0]),)
        f_plain = ivp_amd.DeviceIVP(ODE, 2, params=p0)
        f_ev = ivp_amd.DeviceIVP(ODE + EVENTS, 2, params=p0, events=[ivp_amd.EventConfig()])
        first = rad.solve_batch_events(f_ev, t0, t1, yd, pd, O(max_events=0))
        most = int(first.n_event_hits.max().item())
        out["records"] = {"total": first.event_info["total"], "largest": most, "smallest": int(first.n_event_hits.min().item())}
        legs["end_jit"] = lambda: rad.solve_batch(f_plain, t0, t1, yd, pd, O())
        legs["events_1pass"] = lambda: rad.solve_batch_events(f_ev, t0, t1, yd, pd, O(max_events=max(most, 1)))
        legs["events_2pass"] = lambda: rad.solve_batch_events(f_ev, t0, t1, yd, pd, O(max_events=0))

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    res, ts = {}, {k: [] for k in legs}
    for k, fn in legs.items():   # warm-up: compiles the modules, sizes the scratch
        _, res[k] = timed(fn)
    for _ in range(a.repeats):   # interleaved rounds
        for k, fn in legs.items():
            t, res[k] = timed(fn)
            ts[k].append(t)
        print(", ".join(f"{k} {ts[k][-1]:.1f} ms" for k in legs), file=sys.stderr, flush=True)
    for k in legs:
        r, e = res[k], stats(ts[k])
        e["status_not_success"] = int((r.status != 0).sum().item())
        e["accepted"] = int(r.naccpt.sum().item())
        if k.startswith("events"):
            e.update(passes=r.event_info["passes"], records=r.event_info["total"], bytes=r.event_info["total"] * (2 + 1) * 8,
                     staging_bytes=r.event_info["staging_bytes"])
        out["results"][k] = e
    same = True
    if not a.end_only:
        one, two, ej = res["events_1pass"], res["events_2pass"], res["end_jit"]
        same = one.event_info["passes"] == 1 and two.event_info["passes"] == 2
        same = same and all(bool(torch.equal(getattr(one, k), getattr(two, k))) for k in ("event_offsets", "t_events_csr", "y_events_csr", "y_end", "status"))
        same = same and bool(torch.equal(one.y_end, ej.y_end)) and bool(torch.equal(one.naccpt, ej.naccpt))   # a non-terminal event does not steer the integration
        out["forms_agree"] = same
        ev, pl = out["results"]["events_1pass"]["ms_median"], out["results"]["end_jit"]["ms_median"]
        out["events_over_event_free"] = {"one_pass": ev / pl, "two_pass": out["results"]["events_2pass"]["ms_median"] / pl}
    failed = False
    if a.parent and not a.end_only:
        parent = json.load(open(a.parent))
        pe, e = parent["results"]["end"], out["results"]["end"]
        out["parent"] = {"library": parent.get("library"), "kernel_sources_sha256": parent.get("kernel_sources_sha256"), "end": pe}
        moved = e["ms_median"] - pe["ms_median"]
        out["check"] = {"margin_ms": pe["spread_ms"], "spread_ms_here": e["spread_ms"], "end_moved_ms": moved, "end_unmoved": abs(moved) <= pe["spread_ms"],
                        "same_accepted_steps": e["accepted"] == pe["accepted"]}
        failed = not (out["check"]["end_unmoved"] and out["check"]["same_accepted_steps"])
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 1 if (failed or not same) else 0


if __name__ == "__main__":
    sys.exit(main())
