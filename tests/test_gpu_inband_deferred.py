"""The deferred in-band guard of the DOPRI5 / DOP853 attempts (ivp_amd/csrc/rk_core.h: IvpInbandAcc) on the MI355X.

Integration: 72 CR3BP trajectories -- one full thread-per-trajectory wave plus one lane-cooperative wave -- holding, in both
parts, the trajectories that leave the band (z = 1e-200, a denormal coordinate, at rest 1e-31 from the first primary) and
the committed state with attempts whose first stage is in band and a later stage is not (tests/golden): every kernel variant
(lean, resident, lane-cooperative, the default hand-over), DOPRI5 and DOP853, one attempt per launch (the sticky "stay on the
plain operators" flag never carries over) and 64 (it does), bit for bit against the oracle.

Predicates: the device's per-call and folded guards against their host restatements on the operand sets of
tests/test_inband_deferred_cpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import inband_deferred_cases as C
from tests.common import assert_bitexact, gpu_batch, oracle_batch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def batch():
    y0, p, t0, t1 = C.batch72()
    ref = {m: oracle_batch("cr3bp", y0, p, t0, t1, method=m, rtol=1e-6, atol=1e-9, max_steps=3000) for m in ("DOPRI5", "DOP853")}
    return y0, p, t0, t1, ref


@pytest.fixture(scope="module")
def batch_late_only():
    y0, p, t0, t1 = C.batch72_late_only()
    ref = {m: oracle_batch("cr3bp", y0, p, t0, t1, method=m, rtol=1e-6, atol=1e-9, max_steps=3000) for m in ("DOPRI5", "DOP853")}
    return y0, p, t0, t1, ref


@pytest.mark.parametrize("chunk", [1, 64])
@pytest.mark.parametrize("method", ["DOPRI5", "DOP853"])
@pytest.mark.parametrize("variant", [1, 2, 3, 0], ids=["lean", "resident", "cooperative", "default"])
def test_a_wave_whose_only_out_of_band_lane_leaves_late_in_an_attempt(batch_late_only, variant, method, chunk):
    """Every other lane of both waves stays in band for the whole run, so the redo is decided by stages after the first."""
    y0, p, t0, t1, ref = batch_late_only
    got = gpu_batch("cr3bp", y0, p, t0, t1, variant=variant, chunk=chunk, method=method, rtol=1e-6, atol=1e-9, max_steps=3000)
    assert_bitexact(got, ref[method], f"{method} variant {variant} chunk {chunk}: ")
    assert (np.asarray(got["status"]) == 0).all()


@pytest.mark.parametrize("chunk", [1, 64])
@pytest.mark.parametrize("method", ["DOPRI5", "DOP853"])
@pytest.mark.parametrize("variant", [1, 2, 3, 0], ids=["lean", "resident", "cooperative", "default"])
def test_trajectories_leaving_the_band_late_in_an_attempt_stay_bitexact(batch, variant, method, chunk):
    y0, p, t0, t1, ref = batch
    got = gpu_batch("cr3bp", y0, p, t0, t1, variant=variant, chunk=chunk, method=method, rtol=1e-6, atol=1e-9, max_steps=3000)
    assert_bitexact(got, ref[method], f"{method} variant {variant} chunk {chunk}: ")
    # the batch does what it is for: ordinary trajectories finish, the collision course stalls
    st = np.asarray(got["status"])
    assert (st == 0).sum() >= 60 and (st != 0).any()


def test_device_guards_match_their_host_restatements(tmp_path):
    guards, _ = C.build_host(tmp_path)
    so = str(tmp_path / "libinband_deferred_probe.so")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-Wno-unused-function", os.path.join(HERE, "helpers", "inband_deferred_probe.hip"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.inband_guards_device.restype = ctypes.c_int
    lib.inband_guards_device.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int]
    x, y, z, mu = C.operand_states()
    dev = torch.device("cuda:0")
    t = [torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (x, y, z, mu)]
    out = [torch.empty(x.size, dtype=torch.int32, device=dev) for _ in range(2)]
    assert lib.inband_guards_device(*[v.data_ptr() for v in t + out], x.size) == 0
    per_call_d, folded_d = (v.cpu().numpy().astype(bool) for v in out)
    per_call_h, folded_h = guards(x, y, z, mu)
    for name, d, h in (("per call", per_call_d, per_call_h), ("folded", folded_d, folded_h)):
        bad = np.flatnonzero(d != h)
        assert bad.size == 0, (name, [(x[i].hex(), y[i].hex(), z[i].hex(), mu[i].hex(), bool(d[i])) for i in bad[:5]])
    assert not (folded_d & ~per_call_d).any()
    # the accumulator over several calls, as an attempt's stage block folds them: out of band as soon as ANY call is, the
    # later ones included.  Sequences of six calls: all ordinary; one call out of band at each position in turn
    # (a factor below 2^-541, r^2 above 2^200, a denormal); and random sequences against the host's per-call answers.
    lib.inband_fold_seq_device.restype = ctypes.c_int
    lib.inband_fold_seq_device.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    calls = 6
    ox, oy, oz, omu = (v[:calls * 64] for v in C.ordinary_states())
    seqs = [np.stack([ox, oy, oz, omu])]
    for bad_xyz in ((0.5, 0.25, 1e-170), (0.5, 2.0 ** 101, 0.0), (0.5, 5e-324, 0.0)):
        for pos in range(calls):
            q = np.stack([ox[:calls], oy[:calls], oz[:calls], omu[:calls]]).copy()
            q[:3, pos] = bad_xyz
            seqs.append(q)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, x.size, calls * 4096)
    rnd = np.stack([x[idx], y[idx], z[idx], np.repeat(mu[idx[::calls]], calls)])
    seqs.append(rnd)
    sx, sy, sz, smu = np.concatenate(seqs, axis=1)
    n_seq = sx.size // calls
    _, single = guards(sx, sy, sz, smu)
    want = single.reshape(n_seq, calls).all(axis=1)
    ts = [torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (sx, sy, sz, smu)]
    got = torch.empty(n_seq, dtype=torch.int32, device=dev)
    assert lib.inband_fold_seq_device(*[v.data_ptr() for v in ts], calls, got.data_ptr(), n_seq) == 0
    got = got.cpu().numpy().astype(bool)
    assert got[:64].all() and not got[64:64 + 3 * calls].any()
    assert np.array_equal(got, want) and want[64 + 3 * calls:].any() and not want[64 + 3 * calls:].all()
