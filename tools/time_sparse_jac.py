#!/usr/bin/env python3
"""What `jac_sparsity` is worth: BDF solves of two method-of-lines systems with the dense forward-difference Jacobian
(n + 1 right-hand sides per evaluation) and with the grouped one (n_groups + 1), as one trajectory and as a batch.

  tri256      y_i' = k (y_{i-1} - 2 y_i + y_{i+1}) - a y_i^3, n = 256, tridiagonal: 3 groups
  medazko400  the 400-state Medazko system of examples/scipy_style_front_end.py: 4 groups

Dense and sparse solves alternate in ONE process, `--repeats` (default 7) timed solves each after one warm-up; reported
per leg: median / min / max wall ms, the spread (max - min) of the dense repeats = the margin of every comparison below,
njev and nlu (summed over the batch; equal in both legs, the results are bit-identical), and the time one Jacobian
evaluation saves, (dense - sparse) / (Jacobian evaluations per trajectory).

  python tools/time_sparse_jac.py --out profiles/r07_sparse_jac.json [--parent parent.json]
  python tools/time_sparse_jac.py --dense-only --root <built checkout of the parent commit> --out parent.json

`--dense-only` times the solves WITHOUT a pattern (all an older checkout can do; `--root` imports ivp_amd from it);
`--parent` merges such a file and checks that the dense path has not moved by more than the margin -- the spread of the
PARENT's repeats -- and that the sparse solve is no slower than the dense one by the same margin at n = 256.  The checks are recorded under "checks"; the exit status is 1 if one fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if "--root" in sys.argv:   # before ivp_amd is imported
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ivp_amd  # noqa: E402
from kernel_sha import kernel_sources_sha256  # noqa: E402

TRI = """
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{
    const double ym = i > 0 ? y[i - 1] : 0.0, yp = i < 255 ? y[i + 1] : 0.0;
    return p[0] * ((ym - 2.0 * y[i]) + yp) - p[1] * ((y[i] * y[i]) * y[i]);
}
"""

MEDAZKO = r"""
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{
    const int n = 200;
    const double k = 100.0, c = 4.0, d = 1.0 / n;
    const double phi = t <= 5 ? 2.0 : 0.0;
    auto ext = [&](int m) { return m == 0 ? phi : (m == 1 ? 0.0 : (m == 2 * n + 2 ? y[2 * n - 2] : y[m - 2])); };
    const int j = i / 2 + 1;
    if (i & 1) return -k * ext(2 * j + 1) * ext(2 * j);
    const double s = j * d - 1.0;
    const double alpha = 2 * s * s * s / (c * c), beta = s * s * s * s / (c * c);
    return alpha * (ext(2 * j + 2) - ext(2 * j - 2)) / (2 * d) + beta * (ext(2 * j - 2) - 2 * ext(2 * j) + ext(2 * j + 2)) / (d * d)
           - k * ext(2 * j) * ext(2 * j + 1);
}
"""


def tri_pattern(n):
    i, j = np.indices((n, n))
    return (np.abs(i - j) <= 1).astype(np.int8)


def medazko_pattern(n):
    pat = np.zeros((2 * n, 2 * n), dtype=np.int8)
    for j in range(n):
        e, o = 2 * j, 2 * j + 1
        for c in (e - 2, e, e + 2, o):
            if 0 <= c < 2 * n:
                pat[e, c] = 1
        pat[o, o] = pat[o, e] = 1
    return pat


def systems(t1_medazko):
    rng = np.random.default_rng(11)

    def tri_inputs(B):
        x = np.linspace(0.0, 1.0, 258)[1:-1]
        y0 = 1.0 + 0.5 * np.sin(np.pi * x)[:, None] + 0.05 * rng.standard_normal((256, B))
        p = np.stack([4000.0 * (1.0 + 0.1 * rng.uniform(-1, 1, B)), 50.0 * (1.0 + 0.1 * rng.uniform(-1, 1, B))])
        return y0, p

    def medazko_inputs(B):
        y0 = np.zeros((400, B))
        y0[1::2] = 1.0 + 0.01 * rng.uniform(-1, 1, (200, B))
        return y0, None

    return {
        "tri256": dict(source=TRI, n=256, params=(1.0, 1.0), pattern=tri_pattern(256), inputs=tri_inputs, t1=0.05,
                       opts=dict(method="BDF", rtol=1e-5, atol=1e-8)),
        "medazko400": dict(source=MEDAZKO, n=400, params=(), pattern=medazko_pattern(200), inputs=medazko_inputs, t1=t1_medazko,
                           opts=dict(method="BDF", rtol=1e-3, atol=1e-6)),
    }


def timed(f, t1, yd, pd, o, r):
    t = time.perf_counter()
    r = ivp_amd.solve_ivp_batch(f, 0.0, t1, yd, pd, o, out=r)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def summary(ts, r):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "spread_ms": float(np.max(ts) - np.min(ts)),
            "ms": [round(float(t), 4) for t in ts], "njev": int(r.njev.sum().item()), "nlu": int(r.nlu.sum().item()),
            "nfev": int(r.nfev.sum().item()), "accepted": int(r.naccpt.sum().item()), "ok": bool((r.status == 0).all().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="JSON of a --dense-only run with the parent commit's library")
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--root", default=None, help="checkout to import ivp_amd from (default: this one)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--t1-medazko", type=float, default=20.0)
    ap.add_argument("--systems", default="tri256,medazko400")
    a = ap.parse_args()
    out = {"tool": "tools/time_sparse_jac.py", "kernel_sources_sha256": kernel_sources_sha256(), "repeats": a.repeats,
           "library": "checkout given with --root" if a.root else "in-tree", "device": torch.cuda.get_device_name(0), "results": {}}
    for name, s in systems(a.t1_medazko).items():
        if name not in a.systems.split(","):
            continue
        o = ivp_amd.Options(**s["opts"])
        legs = {"dense": ivp_amd.DeviceIVP(s["source"], n=s["n"], params=s["params"])}
        if not a.dense_only:
            legs["sparse"] = ivp_amd.DeviceIVP(s["source"], n=s["n"], params=s["params"], jac_sparsity=s["pattern"])
            out.setdefault("n_groups", {})[name] = ivp_amd.api.jac_sparsity_groups(s["pattern"], s["n"])[1]
        for B in (1, a.batch):
            y0, p = s["inputs"](B)
            yd = torch.as_tensor(y0, device="cuda:0")
            pd = None if p is None else torch.as_tensor(p, device="cuda:0")
            res, ts = {}, {k: [] for k in legs}
            for k, f in legs.items():   # warm-up: compiles the module, sizes the scratch
                _, res[k] = timed(f, s["t1"], yd, pd, o, None)
            for _ in range(a.repeats):   # interleaved rounds
                for k, f in legs.items():
                    t, res[k] = timed(f, s["t1"], yd, pd, o, res[k])
                    ts[k].append(t)
                print(f"{name} B={B}: " + ", ".join(f"{k} {ts[k][-1]:.2f} ms" for k in legs), file=sys.stderr, flush=True)
            entry = {k: summary(ts[k], res[k]) for k in legs}
            entry["t1"] = s["t1"]
            if "sparse" in legs:
                entry["bit_identical"] = bool(torch.equal(res["dense"].y_end, res["sparse"].y_end)) and entry["dense"]["njev"] == entry["sparse"]["njev"]
                d, sp = entry["dense"]["ms_median"], entry["sparse"]["ms_median"]
                entry["speedup"] = d / sp
                entry["saved_us_per_jacobian"] = (d - sp) * 1e3 / (entry["dense"]["njev"] / B)
            out["results"][f"{name}_B{B}"] = entry
    if a.parent and not a.dense_only:
        parent = json.load(open(a.parent))
        out["parent"] = {"library": parent.get("library"), "kernel_sources_sha256": parent.get("kernel_sources_sha256"), "results": {}}
        out["checks"] = {}
        for key, e in out["results"].items():
            pe = parent["results"].get(key)
            if pe is None:
                continue
            out["parent"]["results"][key] = pe["dense"]
            margin = pe["dense"]["spread_ms"]
            out["checks"][key] = {"margin_ms": margin,
                                  "dense_moved_ms": e["dense"]["ms_median"] - pe["dense"]["ms_median"],
                                  "dense_unmoved": abs(e["dense"]["ms_median"] - pe["dense"]["ms_median"]) <= margin,
                                  "sparse_minus_dense_ms": e["sparse"]["ms_median"] - e["dense"]["ms_median"],
                                  "sparse_not_slower": e["sparse"]["ms_median"] <= e["dense"]["ms_median"] + margin}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    failed = [k for k, c in out.get("checks", {}).items() if not (c["dense_unmoved"] and (c["sparse_not_slower"] or not k.startswith("tri256")))]
    ok = all(e[leg]["ok"] for e in out["results"].values() for leg in ("dense", "sparse") if leg in e)
    return 1 if (failed or not ok) else 0


if __name__ == "__main__":
    sys.exit(main())
