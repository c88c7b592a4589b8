#!/usr/bin/env python3
"""Helper of tests/test_gpu_context_lifecycle.py: DOP853 solves with Options.t_eval -- the case the library may hand to the
deferred sampling kernels (flavour 3) -- with every output written to an .npz.  Which path runs comes from the environment
(IVP_TUNE_DEFER_EVAL is read once per process by the library, IVP_DEFER_EVAL_BYTES per call), hence a process of its own;
IVP_TRACE_LAUNCHES=1 makes the library say on stderr when it enqueues the deferred sample kernel (Options.profile = 1).
  python tests/helpers/teval_dump.py OUT.npz"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import ivp_amd  # noqa: E402
from ivp_amd import workloads as W  # noqa: E402

out = sys.argv[1]
dev = torch.device("cuda:0")
KEYS = ("y_end", "t_end", "h_next", "status", "nfev", "nstep", "naccpt", "nrejct", "y_eval", "eval_idx", "n_filled", "eval_offsets")
res = {}


def solve(name, f, y0, p, t0, t1, **extra):
    o = ivp_amd.Options(method="DOP853", rtol=1e-8, atol=1e-10, profile=1, **extra)
    t1d = torch.as_tensor(t1, device=dev) if np.ndim(t1) else t1
    r = ivp_amd.solve_ivp_batch(f, t0, t1d, torch.as_tensor(y0, device=dev), torch.as_tensor(p, device=dev), o)
    torch.cuda.synchronize()
    for k in KEYS:
        v = getattr(r, k, None)
        if v is not None:
            res[f"{name}.{k}"] = v.cpu().numpy()


# one grid of 65 points shared by both batches: the Van der Pol intervals end at 50 .. 60, the CR3BP ones at 17.07 (the points
# behind a trajectory's end are not sampled)
GRID = list(np.linspace(0.0, 60.0, 65))
y0, p, t0, t1 = W.vdp_batch(3000)
t1 = np.minimum(t1, 60.0)
solve("vdp", ivp_amd.VanDerPol(), y0, p, t0, t1, t_eval=GRID)
y0, p, t0, t1 = W.cr3bp_batch(500)
solve("cr3bp", ivp_amd.CR3BP(), y0, p, t0, t1, t_eval=GRID)
# one grid per trajectory: lengths 0 .. 40 (an empty one included), each over its own interval
y0, p, t0, t1 = W.vdp_batch(64)
t1 = np.minimum(t1, 60.0)
lengths = np.random.default_rng(64).permutation(np.arange(64) % 41)
grids = [np.linspace(0.0, t1[b], int(m)) for b, m in enumerate(lengths)]
solve("ragged", ivp_amd.VanDerPol(), y0, p, t0, t1, t_eval_per_trajectory=grids)
np.savez(out, **res)
print("ok", int(res["vdp.n_filled"].min()), int(res["cr3bp.n_filled"].min()), int(res["ragged.n_filled"].sum()))
