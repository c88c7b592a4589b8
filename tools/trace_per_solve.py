#!/usr/bin/env python3
"""Per-solve kernel times from a rocprofv3 --kernel-trace CSV of bench.py.

Usage: trace_per_solve.py <kernel_trace.csv> <tag> [warmup_solves]
A solve starts with its init_kernel dispatch; the durations of the thread-per-trajectory stepping kernel (chunk_kernel_t) and of
the lane-cooperative one (coop_chunk_kernel) are summed per solve.  Prints one JSON line: the per-solve values in microseconds
(warm-up solves dropped) with their median, quartiles, minimum and maximum."""
import csv, json, statistics, sys

src, tag = sys.argv[1:3]
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rows = sorted(csv.DictReader(open(src)), key=lambda r: int(r["Start_Timestamp"]))
solves, cur = [], None
for r in rows:
    k = r["Kernel_Name"]
    if "init_kernel" in k:
        cur = {"bulk": 0.0, "coop": 0.0, "init": 0.0}
        solves.append(cur)
    if cur is None:
        continue
    d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    if "init_kernel" in k:
        cur["init"] += d
    elif "coop_chunk_kernel" in k:
        cur["coop"] += d
    elif "chunk_kernel_t" in k:
        cur["bulk"] += d
solves = [s for s in solves[warm:] if s["bulk"] > 0.0 or s["coop"] > 0.0]   # an init launch with no stepping behind it is no solve
out = {"tag": tag, "solves": len(solves)}
for key in ("bulk", "coop", "init"):
    v = [s[key] for s in solves]
    q = statistics.quantiles(v, n=4)
    out[key + "_us"] = {"median": statistics.median(v), "q1": q[0], "q3": q[2], "min": min(v), "max": max(v), "mean": statistics.fmean(v),
                        "values": [round(x, 1) for x in v]}
print(json.dumps(out))
