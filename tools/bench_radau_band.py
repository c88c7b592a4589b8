#!/usr/bin/env python3
"""Radau IIA(5) in band storage against the dense Radau call on the same source, on one device.

  speed     the tridiagonal system y_i' = k (y_{i-1} - 2 y_i + y_{i+1}) / 2 - a y_i^3 at n = 65, 256, 512 and the ml = mu = 8
            system at n = 100, with B = 1 and B = 2000 trajectories: `dense` = Radau.solve_batch on the source compiled without
            a pattern (forward differences, 4 n^2 doubles per trajectory), `banded` = Radau.solve_batch_banded on the source
            compiled with the pattern and jac_storage="banded".  rtol 1e-2, atol 1e-4, first_step 4e-3, t in [0, 0.012]: about
            three steps, so that the dense leg at n = 512, B = 2000 stays a matter of seconds.  End state only.
            The two legs of a point alternate in ONE process, `--repeats` (default 7) timed solves each after one warm-up;
            reported: median / min / max wall ms, the ratio dense / banded, the matrix bytes per trajectory of both, and whether
            the two end states are bit-equal.
  capacity  the largest B at n = 512 for which each call's per-trajectory buffers fit the device's free memory, from the sizes
            (nothing is allocated to find out).
  --dense-only [--root <built checkout>]   the dense leg alone at n = 64 and n = 256 (B = 2000): what the parent commit can
            run too, in a process of its own; `--parent <that JSON>` merges it and records the check "the dense call has not
            moved", with the spread of the PARENT's repeats as the margin.

  python tools/bench_radau_band.py --out profiles/r18_radau_band.json [--parent parent.json]"""
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
import ivp_amd  # noqa: E402

RTOL, ATOL, H0, T1 = 1e-2, 1e-4, 4e-3, 0.012
POINTS = [(65, 1), (256, 1), (512, 1), (100, 8)]   # (n, half bandwidth)
BATCHES = [1, 2000]


def source(n, w):
    return f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{{
    double s = 0.0;
    for (int d = 1; d <= {w}; ++d) {{
        const double ym = i - d >= 0 ? y[i - d] : 0.0, yp = i + d < {n} ? y[i + d] : 0.0;
        s += (1.0 / (double)(1 << d)) * ((ym - 2.0 * y[i]) + yp);
    }}
    return p[0] * s - p[1] * ((y[i] * y[i]) * y[i]);
}}
"""


def pattern(n, w):
    i, j = np.indices((n, n))
    return (np.abs(i - j) <= w).astype(np.int8)


def inputs(n, B, dev):
    rng = np.random.default_rng(n + B)
    y0 = 0.5 + rng.uniform(size=(n, B))
    params = np.stack([100.0 * (1.0 + rng.uniform(size=B)), 5.0 + 10.0 * rng.uniform(size=B)])
    return torch.as_tensor(y0, device=dev), torch.as_tensor(params, device=dev)


def stats(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "spread_ms": float(np.max(ts) - np.min(ts)),
            "ms": [round(float(t), 3) for t in ts]}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def per_trajectory_bytes(n, ml, mu, banded):
    """what submit reserves per trajectory for a Radau solve: the matrix block, cont + h_acc + err_acc, two pivot rows, and
    the state-sized vectors (y, k1)"""
    mat = ((ml + mu + 1) + 3 * (2 * ml + mu + 1)) * n * 8 if banded else 4 * n * n * 8
    return {"matrices": mat, "total": mat + (4 * n + 2) * 8 + 2 * n * 4 + 2 * n * 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="JSON of a --dense-only run with the parent commit's library")
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--root", default=None, help="checkout to import ivp_amd from (default: this one)")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rad = ivp_amd.Radau()
    opt = ivp_amd.Options(rtol=RTOL, atol=ATOL, first_step=H0)
    out = {"tool": "tools/bench_radau_band.py", "repeats": a.repeats, "library": "checkout given with --root" if a.root else "in-tree",
           "device": torch.cuda.get_device_name(0), "setup": {"rtol": RTOL, "atol": ATOL, "first_step": H0, "t1": T1}, "results": {}}

    def run_point(name, legs):
        res, ts = {}, {k: [] for k in legs}
        for k, fn in legs.items():   # warm-up: compiles the modules, sizes the buffers
            _, res[k] = timed(fn)
        for _ in range(a.repeats):   # interleaved rounds
            for k, fn in legs.items():
                t, res[k] = timed(fn)
                ts[k].append(t)
        e = {k: stats(ts[k]) for k in legs}
        for k in legs:
            e[k]["status_not_success"] = int((res[k].status != 0).sum().item())
            e[k]["accepted"] = int(res[k].naccpt.sum().item())
        print(name, ", ".join(f"{k} {e[k]['ms_median']:.2f} ms" for k in legs), file=sys.stderr, flush=True)
        return e, res

    failed = False
    if a.dense_only:
        for n in (64, 256):
            f = ivp_amd.DeviceIVP(source(n, 1), n=n, params=(1.0, 1.0))
            y0, params = inputs(n, 2000, dev)
            e, _ = run_point(f"dense n={n}", {"dense": lambda: rad.solve_batch(f, 0.0, T1, y0, params, opt)})
            out["results"][f"dense_n{n}_B2000"] = e["dense"]
    else:
        for n, w in POINTS:
            fd = ivp_amd.DeviceIVP(source(n, w), n=n, params=(1.0, 1.0))
            fb = ivp_amd.DeviceIVP(source(n, w), n=n, params=(1.0, 1.0), jac_sparsity=pattern(n, w), jac_storage="banded")
            for B in BATCHES:
                y0, params = inputs(n, B, dev)
                e, res = run_point(f"n={n} w={w} B={B}", {"dense": lambda: rad.solve_batch(fd, 0.0, T1, y0, params, opt),
                                                           "banded": lambda: rad.solve_batch_banded(fb, 0.0, T1, y0, params, opt)})
                same = all(bool(torch.equal(getattr(res["dense"], k), getattr(res["banded"], k)))
                           for k in ("y_end", "t_end", "h_next", "status", "nfev", "njev", "nlu", "nstep", "naccpt", "nrejct"))
                failed = failed or not same
                out["results"][f"n{n}_ml{w}_mu{w}_B{B}"] = {
                    "dense": e["dense"], "banded": e["banded"], "dense_over_banded": e["dense"]["ms_median"] / e["banded"]["ms_median"],
                    "bit_equal": same, "bytes_per_trajectory": {"dense": per_trajectory_bytes(n, w, w, False), "banded": per_trajectory_bytes(n, w, w, True)}}
        free_b, total_b = torch.cuda.mem_get_info()
        cap = {k: per_trajectory_bytes(512, 1, 1, k == "banded") for k in ("dense", "banded")}
        out["capacity_n512"] = {"device_free_bytes": int(free_b), "device_total_bytes": int(total_b),
                                "largest_B": {k: int(free_b // v["total"]) for k, v in cap.items()}, "bytes_per_trajectory": cap,
                                "note": "from the sizes of the per-trajectory buffers; nothing was allocated to find out"}
        for n in (64, 256):   # the dense legs the parent can run too
            f = ivp_amd.DeviceIVP(source(n, 1), n=n, params=(1.0, 1.0))
            y0, params = inputs(n, 2000, dev)
            e, _ = run_point(f"dense n={n}", {"dense": lambda: rad.solve_batch(f, 0.0, T1, y0, params, opt)})
            out["results"][f"dense_n{n}_B2000"] = e["dense"]
        if a.parent:
            parent = json.load(open(a.parent))
            out["parent"] = {"library": parent.get("library"), "results": parent["results"]}
            out["check"] = {}
            for k, pe in parent["results"].items():
                e = out["results"][k]
                moved = e["ms_median"] - pe["ms_median"]
                ok = moved <= pe["spread_ms"] and e["accepted"] == pe["accepted"]
                out["check"][k] = {"margin_ms": pe["spread_ms"], "spread_ms_here": e["spread_ms"], "moved_ms": moved, "not_slower": moved <= pe["spread_ms"],
                                   "same_accepted_steps": e["accepted"] == pe["accepted"]}
                failed = failed or not ok
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
