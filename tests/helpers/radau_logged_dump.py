#!/usr/bin/env python3
"""Helper of tests/test_gpu_radau_unbounded.py: B exponential decays (k = 0.5 + 0.75 b, y0 = 1, t in [0, 2]) through
Radau.solve_batch_logged with Options.profile = 1, the CSR log, the end state, the counters, stats["lane_attempt_slots"] and
log_info["passes"] written to an .npz.  How many trajectories a wavefront carries -- the columns of a page -- comes from
IVP_TUNE_BDF_LPW, which the library reads once per process: hence a process of its own.
  python tests/helpers/radau_logged_dump.py OUT.npz B"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import ivp_amd  # noqa: E402

out, B = sys.argv[1], int(sys.argv[2])
dev = torch.device("cuda:0")
k = torch.as_tensor(np.array([[0.5 + 0.75 * b for b in range(B)]]), device=dev)
y0 = torch.ones((1, B), dtype=torch.float64, device=dev)
r = ivp_amd.Radau().solve_batch_logged(ivp_amd.ExponentialDecay(), 0.0, 2.0, y0, k, ivp_amd.Options(rtol=1e-6, atol=1e-8, profile=True))
res = {m: getattr(r, m).cpu().numpy() for m in ("log_offsets", "t_log", "y_log", "n_log", "y_end", "t_end", "h_next", "status", "nfev", "njev",
                                                "nlu", "nstep", "naccpt", "nrejct")}
res["slots"] = np.array(r.stats["lane_attempt_slots"], dtype=np.int64)
res["passes"] = np.array(r.log_info["passes"], dtype=np.int64)
np.savez(out, **res)
print("ok", B, int(res["slots"]))
