#!/usr/bin/env python3
"""Helper of tests/test_gpu_wave_density.py: the base batches of tests/wave_density_cases.py, each solved once with
Options.profile = 1, every output written to an .npz as NAME.MEMBER, with NAME.slots (stats["lane_attempt_slots"]),
NAME.launches and NAME.seconds beside them.  How many trajectories a wavefront of the thread-per-trajectory stiff kernels
carries, and which BDF build runs, comes from the environment -- IVP_TUNE_BDF_LPW and IVP_TUNE_BDF_OCC2 are read once per
process by the library -- hence a process of its own.
  python tests/helpers/wave_density_dump.py OUT.npz FAMILY[,FAMILY...]        (radau, radau_dae, bdf)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import wave_density_cases as C  # noqa: E402

out = sys.argv[1]
res = {}
T0 = time.time()
for family in sys.argv[2].split(","):
    for case in C.cases(family):
        sys.stderr.write(f"case {case.name} at {time.time() - T0:.1f} s\n")
        sys.stderr.flush()
        t = time.time()
        got, stats = C.run(case, profile=1)
        for k, v in got.items():
            res[f"{case.name}.{k}"] = v
        res[f"{case.name}.slots"] = np.array(stats["lane_attempt_slots"], dtype=np.int64)
        res[f"{case.name}.launches"] = np.array(stats["launches"], dtype=np.int64)
        res[f"{case.name}.seconds"] = np.array(time.time() - t)
res["seconds"] = np.array(time.time() - T0)
np.savez(out, **res)
print("ok", len(res), f"{time.time() - T0:.1f} s")
