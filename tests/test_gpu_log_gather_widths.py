"""The one-pass accepted-step log (page pool + log_gather.hip) at the state widths no other logged test runs.

The gather kernel keeps a whole column group of a page in LDS per wavefront: 32 slots x 8 columns x (n + 1) doubles, four
wavefronts per workgroup -- 65 536 B of dynamic LDS at n = 7 and 73 728 B at n = 8, plus 1 KB static, which is more than
the 64 KB a workgroup gets on every part before gfx950.  The built-in problems stop at n = 6 and start again at n = 64, so
these widths need a hiprtc system.  n = 1 and n = 5 are the odd record lengths (2 and 6 doubles) no logged test uses.

ivp_log_gather sizes the workgroup (4, 2 or 1 wavefronts, else the tiled single-wave path) from the device's
sharedMemPerBlock.  gfx950 has 160 KB of LDS per workgroup, so n = 7 and n = 8 are expected to keep four wavefronts there --
the launch the library made before it looked at the limit; test_workgroup_of_the_gather_follows_the_lds_limit prints the
limit and the choice (pytest -s) and holds the one to the other.  NOT MEASURED when this was written: no MI355X run of this file, with or without the limit check,
could be made (see the commit message); whether the four-wave launch at n = 7 / n = 8 works on the device is what the
first run of this file says.  The 2-, 1-wave and tiled choices are what a 64 KB or partitioned device would get; they are
covered by reasoning only (the kernel reads its wave count from blockDim, the tiled path is the one n > 8 takes).

Three mechanisms that share neither pages nor gather must agree bit for bit: the one-pass log, the counted two-pass CSR
log (count solve + scan + fill solve) and the bounded [max_log] log of solve_ivp_batch re-laid in CSR order on the host.
B = 130: two full waves and a ragged 2-lane tail, hence a last column group of 2; per-trajectory end times in [0.2, 6] make
the counts differ widely.  At rtol 1e-7 alone the longest trajectory takes 21 (n = 1), 51 (n = 5), 63 (n = 7) and 66 (n = 8)
records (the CPU oracle's counts): the rates of this system are too slow for the step-size controller to fill three pages at
every width, n = 1 (y' = -0.4 y) least of all.  Options.max_step = 0.05 is therefore part of the solve: at least 20 records
per unit of time, about 120 for the longest trajectories and 5 for the shortest, at every width -- more than two 32-slot
pages for some trajectories and less than one for others, which is what the n_log.max() > 64 assertion is there to ensure."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import ivp_amd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = 130


def linear_ring_source(n):
    """dydx[i] = -(0.5 + 0.25 i) y[i] + 0.1 y[(i + 1) % n], written out for the given n"""
    rows = " ".join(f"dydx[{i}] = -{0.5 + 0.25 * i!r} * y[{i}] + 0.1 * y[{(i + 1) % n}];" for i in range(n))
    return "__device__ void ode(double x, const double* y, double* dydx, const double* p) { " + rows + " }"


def ring_inputs(n, batch=B, seed=20261017):
    rng = np.random.default_rng(seed + n)
    y0 = 1.0 + 0.5 * rng.standard_normal((n, batch))
    t1 = rng.uniform(0.2, 6.0, batch)
    return y0, t1


RING_OPTIONS = dict(method="DOPRI5", rtol=1e-7, atol=1e-10, max_step=0.05)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n", [7, 8, 1, 5])
def test_one_pass_log_equals_two_pass_and_bounded_log(n):
    ctx = ivp_amd.Context(0)   # fresh: no learnt pool size, the default 256 MB pool cannot run dry here
    try:
        f = ivp_amd.DeviceIVP(linear_ring_source(n), n, ctx=ctx)
        y0, t1 = ring_inputs(n)
        y0d, t1d = torch.as_tensor(y0, device=DEV), torch.as_tensor(t1, device=DEV)
        opt = dict(RING_OPTIONS)
        one = ivp_amd.solve_ivp_batch_logged(f, 0.0, t1d, y0d, None, ivp_amd.Options(**opt), ctx)
        assert one.log_info["passes"] == 1, one.log_info
        two = ivp_amd.solve_ivp_batch_logged(f, 0.0, t1d, y0d, None, ivp_amd.Options(**opt), ctx, two_pass=True)
        cnt = one.n_log.cpu().numpy().astype(np.int64)
        print(f"n = {n}: records {int(cnt.sum())}, n_log min {int(cnt.min())} max {int(cnt.max())}")
        assert int(cnt.max()) > 64                                   # the multi-page path is really taken
        off = one.log_offsets.cpu().numpy()
        assert off[0] == 0 and np.array_equal(np.diff(off), cnt) and int(off[-1]) == one.t_log.shape[0] == one.log_info["records"]
        assert np.array_equal(off, two.log_offsets.cpu().numpy())
        assert np.array_equal(cnt, two.n_log.cpu().numpy().astype(np.int64))
        assert np.array_equal(_bits(one.t_log), _bits(two.t_log))
        assert np.array_equal(_bits(one.y_log), _bits(two.y_log))
        # third mechanism: the bounded [max_log][B] log, re-laid in CSR order on the host
        ml = int(cnt.max())
        bnd = ivp_amd.solve_ivp_batch(f, 0.0, t1d, y0d, None, ivp_amd.Options(max_log=ml, **opt), ctx)
        assert np.array_equal(bnd.n_log.cpu().numpy().astype(np.int64), cnt)
        kk = np.concatenate([np.arange(c) for c in cnt])
        bb = np.repeat(np.arange(B), cnt)
        assert np.array_equal(_bits(one.t_log), _bits(bnd.t_log.cpu().numpy()[kk, bb]))
        assert np.array_equal(_bits(one.y_log), _bits(bnd.y_log.cpu().numpy()[kk, :, bb]))
        for k in ("y_end", "t_end", "h_next"):
            assert np.array_equal(_bits(getattr(one, k)), _bits(getattr(bnd, k))), k
        for k in ("status", "nfev", "naccpt", "nrejct"):
            assert torch.equal(getattr(one, k), getattr(bnd, k)), k
        # every trajectory's log starts at t0 with y0 and ends with its own end state: the records are where they belong
        t, y = one.t_log.cpu().numpy(), one.y_log.cpu().numpy()
        assert not t[off[:-1]].any() and np.array_equal(y[off[:-1]], y0.T)
        assert np.array_equal(_bits(t[off[1:] - 1]), _bits(one.t_end)) and np.array_equal(_bits(y[off[1:] - 1].T), _bits(one.y_end))
        assert np.abs(t[off[1:] - 1] - t1).max() <= 4.0 * np.spacing(6.0)     # t_end = x + h of the last step: t1 up to a rounding
    finally:
        ctx.close()


_TRACE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, ivp_amd
from tests.test_gpu_log_gather_widths import RING_OPTIONS, linear_ring_source, ring_inputs
print("sharedMemPerBlock", torch.cuda.get_device_properties(0).shared_memory_per_block)
for n in (7, 8):
    y0, t1 = ring_inputs(n, 64)
    dev = torch.device("cuda:0")
    f = ivp_amd.DeviceIVP(linear_ring_source(n), n)
    r = ivp_amd.solve_ivp_batch_logged(f, 0.0, torch.as_tensor(t1, device=dev), torch.as_tensor(y0, device=dev), None,
                                       ivp_amd.Options(profile=1, **RING_OPTIONS))
    assert r.log_info["passes"] == 1
"""


def test_workgroup_of_the_gather_follows_the_lds_limit(tmp_path):
    """IVP_TRACE_LAUNCHES is read once per process, hence a child.  The gather's workgroup at n = 7 and n = 8 is the largest
    of 4, 2, 1 wavefronts whose whole column groups (32 slots x 8 columns x (n + 1) doubles each) fit the device's LDS per
    workgroup next to the kernel's 1 KB of static LDS; the limit the library used is the device's sharedMemPerBlock."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "trace_gather.py"
    script.write_text(_TRACE)
    r = subprocess.run([sys.executable, str(script), root], env=dict(os.environ, IVP_TRACE_LAUNCHES="1"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    limit = int(re.search(r"sharedMemPerBlock (\d+)", r.stdout).group(1))
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("ivp launch gather")]
    print(f"sharedMemPerBlock {limit}")
    print("\n".join(lines))
    assert len(lines) == 2, r.stderr[-2000:]
    for ln, n in zip(lines, (7, 8)):
        m = re.match(r"ivp launch gather  n = (\d+), (\d+) wave\(s\) per workgroup, LDS limit (\d+) B", ln)
        assert m, ln
        want = next((w for w in (4, 2, 1) if 32 * 8 * (n + 1) * 8 * w + 1024 <= limit), 0)
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (n, want, limit), ln
