"""bench.py: a plain run prints the headline alone, and --dump-outputs writes what its timed path computed.  bench.py sets
OpenMP variables when it is imported, so it runs in child processes here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_ENV = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


def test_dump_outputs_samples_a_large_batch_to_64_mb(tmp_path):
    script = (
        "import sys, numpy as np, bench\n"
        "B = 1_000_000\n"
        "rng = np.random.default_rng(3)\n"
        "arrays = {'y_end': rng.standard_normal((8, B)), 'status': np.arange(B, dtype=np.int32), 'nstep': np.arange(B, dtype=np.int64)}\n"
        "bench.dump_outputs(sys.argv[1], arrays)\n"
        "bench.dump_outputs(sys.argv[2], arrays)\n"
        "np.save(sys.argv[1] + '_y_end_full.npy', arrays['y_end'])\n")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    r = subprocess.run([sys.executable, "-c", script, a, b], capture_output=True, text=True, timeout=300, env=CHILD_ENV, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) == ["nstep.npy", "sample_index.npy", "status.npy", "y_end.npy"]
    assert sum(os.path.getsize(os.path.join(a, f)) for f in files) <= 64_000_000
    got = {f[:-4]: np.load(os.path.join(a, f)) for f in files}
    assert all(v.dtype == np.float64 for v in got.values())
    for f in files:                                  # the same fixed sample every time
        assert np.array_equal(got[f[:-4]], np.load(os.path.join(b, f))), f
    idx = got["sample_index"].astype(np.int64)
    assert len(idx) > 500_000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(got["status"], idx) and np.array_equal(got["nstep"], idx)
    assert np.array_equal(got["y_end"], np.load(a + "_y_end_full.npy")[:, idx])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    import torch
    import ivp_amd
    from ivp_amd import workloads as W

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=CHILD_ENV, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["unit"] == "steps/s" and res["all_success"]
    assert not {"roofline", "cpu_baseline", "fma_fp_mode", "pipelined", "outputs"} & set(res)   # secondary figures: --full only
    # the headline batch (C2: 100k CR3BP, DOPRI5, rtol 1e-6, atol 1e-9) solved here directly gives the same bits
    y0, p, t0, t1 = W.cr3bp_batch(100_000)
    dev = torch.device("cuda:0")
    ref = ivp_amd.solve_ivp_batch(ivp_amd.CR3BP(), t0, t1, torch.as_tensor(y0, device=dev), torch.as_tensor(p, device=dev),
                                  ivp_amd.Options(method="DOPRI5", rtol=1e-6, atol=1e-9))
    names = [n for n in ("y_end", "t_end", "h_next", "status", "nfev", "nstep", "naccpt", "nrejct", "njev", "nlu")
             if getattr(ref, n) is not None]
    assert len(names) >= 8 and sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in names)
    for n in names:
        got = np.load(os.path.join(tmp_path, n + ".npy"))
        assert got.dtype == np.float64
        assert np.array_equal(got, getattr(ref, n).cpu().numpy().astype(np.float64)), n
    assert int(np.load(os.path.join(tmp_path, "naccpt.npy")).sum()) == res["accepted_steps_per_batch"]
