#!/usr/bin/env python3
"""Helper of tests/test_gpu_balance.py: CR3BP solves whose bulk phase may run as balanced rounds (ivp_amd/csrc/ivp_balance.h),
with every output written to an .npz.  Which launch schedule runs comes from the environment -- IVP_TUNE_BALANCE,
IVP_TUNE_BALANCE_SLOTS and IVP_TUNE_COOP_CAP_LANES are read once per process by the library -- hence a process of its own;
with IVP_TRACE_LAUNCHES=1 the library prints one line per stepping launch on stderr (Options.profile = 1), behind a
"case NAME" line printed here.
  python tests/helpers/balance_dump.py OUT.npz B[,B...] [MIXED_B]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import ivp_amd  # noqa: E402
from tests import balance_cases as C  # noqa: E402

out = sys.argv[1]
sizes = [int(v) for v in sys.argv[2].split(",")]
mixed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
dev = torch.device("cuda:0")
res = {}
T0 = time.time()


def put(name, r, keys):
    for k in keys:
        v = getattr(r, k, None)
        if v is not None:
            res[f"{name}.{k}"] = v.cpu().numpy()


def solve(name, y0, p, t0, t1, method, fma):
    sys.stderr.write(f"case {name}\n")   # (elapsed time on a line of its own: the test reads the name only)
    sys.stderr.write(f"at {time.time() - T0:.1f} s\n")
    sys.stderr.flush()
    o = ivp_amd.Options(fp_mode=ivp_amd.FpMode.FAST if fma else ivp_amd.FpMode.STRICT, profile=1, **C.opts(method))
    t1d = torch.as_tensor(t1, device=dev) if np.ndim(t1) else t1
    r = ivp_amd.solve_ivp_batch(ivp_amd.CR3BP(), t0, t1d, torch.as_tensor(y0, device=dev), torch.as_tensor(p, device=dev), o)
    torch.cuda.synchronize()
    put(name, r, C.KEYS)


def solve_logged(name, y0, p, t0, t1):
    sys.stderr.write(f"case {name}\n")   # (elapsed time on a line of its own: the test reads the name only)
    sys.stderr.write(f"at {time.time() - T0:.1f} s\n")
    sys.stderr.flush()
    o = ivp_amd.Options(profile=1, **C.opts("DOPRI5"))
    r = ivp_amd.solve_ivp_batch_logged(ivp_amd.CR3BP(), t0, t1, torch.as_tensor(y0, device=dev), torch.as_tensor(p, device=dev), o)
    torch.cuda.synchronize()
    put(name, r, C.KEYS + ("log_offsets", "t_log", "y_log"))
    res[f"{name}.passes"] = np.asarray(r.log_info["passes"])


for B in sizes:
    y0, p, t0, t1 = C.batch(B)
    for method, fma in C.MODES:
        solve(C.name(B, method, fma), y0, p, t0, t1, method, fma)
    solve_logged(f"{B}.logged", y0, p, t0, C.T1_LOGGED)
if mixed:
    y0, p, t0, t1 = C.mixed_batch(mixed)
    for method, fma in C.MODES:
        solve(C.name(f"mixed{mixed}", method, fma), y0, p, t0, t1, method, fma)
np.savez(out, **res)
print("ok", len(res))
