#!/usr/bin/env python3
"""What banded Jacobian storage (`jac_storage="banded"`, bdf_band.h) is worth: BDF solves of the two method-of-lines
systems of tools/time_sparse_jac.py with the declared pattern and dense n x n storage, and with the same pattern and band
storage, as one trajectory and as a batch.

  tri256      y_i' = k (y_{i-1} - 2 y_i + y_{i+1}) - a y_i^3, n = 256, (ml, mu) = (1, 1)
  medazko400  the 400-state Medazko system, (ml, mu) = (2, 2)

Dense-with-pattern and banded solves alternate in ONE process, `--repeats` (default 7) timed solves each after one
warm-up; reported per leg: median / min / max wall ms, the spread of the repeats, nlu / njev (equal in both legs: the
results are checked bit-identical here), the ratio dense / banded, the time one refactorisation-plus-its-solves saves
((dense - banded) / factorisations per trajectory) and the bytes of BDF work space (J + factors, all trajectories).

  python tools/time_banded_lu.py --out profiles/r08_banded_lu.json [--parent parent.json]
  python tools/time_banded_lu.py --dense-only --root <built checkout of the parent commit> --out parent.json

`--dense-only` times the dense-with-pattern leg alone (all the parent commit can do; `--root` imports ivp_amd from it);
`--parent` merges such a file and records two checks per leg, both with the spread of the PARENT's seven repeats as the
margin: the dense path has not moved, and banded is not slower than dense-with-pattern.  Exit status 1 if a solve failed,
the results differ, or a check fails."""
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
from kernel_sha import kernel_sources_sha256  # noqa: E402
from time_sparse_jac import systems  # noqa: E402  (the same four legs)

FIELDS = ("y_end", "t_end", "h_next", "status", "nfev", "nstep", "naccpt", "nrejct", "njev", "nlu")


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
    out = {"tool": "tools/time_banded_lu.py", "kernel_sources_sha256": kernel_sources_sha256(os.path.abspath(ROOT)), "repeats": a.repeats,
           "library": "checkout given with --root" if a.root else "in-tree", "device": torch.cuda.get_device_name(0), "results": {}}
    for name, s in systems(a.t1_medazko).items():
        if name not in a.systems.split(","):
            continue
        o = ivp_amd.Options(**s["opts"])
        n = s["n"]
        legs = {"dense": ivp_amd.DeviceIVP(s["source"], n=n, params=s["params"], jac_sparsity=s["pattern"])}
        layout = {"dense": {"banded": False, "ml": 0, "mu": 0, "jac_doubles": n * n, "lu_doubles": n * n}}
        if not a.dense_only:
            legs["banded"] = ivp_amd.DeviceIVP(s["source"], n=n, params=s["params"], jac_sparsity=s["pattern"], jac_storage="banded")
            layout = {k: f.jac_layout for k, f in legs.items()}
            out.setdefault("bandwidth", {})[name] = list(ivp_amd.api.jac_bandwidth(s["pattern"], n))
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
            for k in legs:
                entry[k]["work_space_bytes"] = 8 * (layout[k]["jac_doubles"] + layout[k]["lu_doubles"]) * B
            entry["t1"] = s["t1"]
            if "banded" in legs:
                entry["bit_identical"] = all(bool(torch.equal(getattr(res["dense"], k), getattr(res["banded"], k))) for k in FIELDS)
                d, b = entry["dense"]["ms_median"], entry["banded"]["ms_median"]
                entry["ratio_dense_over_banded"] = d / b
                entry["saved_us_per_factorisation"] = (d - b) * 1e3 / (entry["dense"]["nlu"] / B)
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
                                  "banded_minus_dense_ms": e["banded"]["ms_median"] - e["dense"]["ms_median"],
                                  "banded_not_slower": e["banded"]["ms_median"] <= e["dense"]["ms_median"] + margin}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    failed = [k for k, c in out.get("checks", {}).items() if not (c["dense_unmoved"] and c["banded_not_slower"])]
    ok = all(e[leg]["ok"] for e in out["results"].values() for leg in ("dense", "banded") if leg in e)
    same = all(e.get("bit_identical", True) for e in out["results"].values())
    return 1 if (failed or not ok or not same) else 0


if __name__ == "__main__":
    sys.exit(main())
