"""The in-range IEEE division and square root of ivp_amd/csrc/rk_core.h (ivp_recip_inband / ivp_div_inband /
ivp_sqrt_inband and their range predicates) against the hardware `/` and sqrt() on the MI355X, bit for bit.

The helpers are the compiler's own instruction sequences without the scale steps, which are no-ops on the guarded
range; the strict RhsCr3bp takes them when the whole wave is in range.  Operands: random
within the bands and at their edges, +-0 / +-inf / NaN numerators, and values just outside the bands, which the
predicates must reject.  The integration case puts trajectories that leave the band (a tiny out-of-plane offset, a
denormal coordinate, a collision course) into ordinary C2 waves and compares every kernel variant with the oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from ivp_amd import workloads as W
from tests.common import assert_bitexact, gpu_batch, oracle_batch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("inband") / "libinband_probe.so")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-Wno-unused-function", os.path.join(HERE, "helpers", "inband_probe.hip"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.inband_probe.restype = ctypes.c_int
    lib.inband_probe.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_int]

    def run(n, d, x):
        dev = torch.device("cuda:0")
        t = [torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=dev) for v in (n, d, x)]
        out = [torch.empty(len(n), dtype=torch.float64, device=dev) for _ in range(4)]
        pred = torch.empty(len(n), dtype=torch.int32, device=dev)
        assert lib.inband_probe(*[v.data_ptr() for v in t + out + [pred]], len(n)) == 0
        return [v.cpu().numpy() for v in out] + [pred.cpu().numpy()]
    return run


def _rand(rng, k, e_lo, e_hi):
    """k doubles with uniformly random exponent in [e_lo, e_hi), random mantissa and sign"""
    mant = rng.uniform(1.0, 2.0, k)
    return np.ldexp(mant, rng.integers(e_lo, e_hi, k)) * rng.choice([-1.0, 1.0], k)


def _num_inband(n):
    m = np.abs(n)
    return (m == 0) | np.isnan(m) | np.isinf(m) | ((m >= 2.0 ** -601) & (m < 2.0 ** 423))


def _sq_inband(x):
    return (x >= 2.0 ** -200) & (x <= 2.0 ** 200)


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def test_inband_division_and_sqrt_are_the_hardware_operations(probe):
    rng = np.random.default_rng(20261016)
    K = 1 << 20
    edges_n = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** -601, -(2.0 ** -601), np.nextafter(2.0 ** 423, 0.0),
                        -np.nextafter(2.0 ** 423, 0.0), 1.0, -1.0, 1e-17, 0.0121505856])
    edges_d = np.array([2.0 ** -300, -(2.0 ** -300), 2.0 ** 300, -(2.0 ** 300), 1.0, 3.0, 1e-90, 1e90])
    n = _rand(rng, K, -601, 423)
    d = _rand(rng, K, -300, 300)
    n[:len(edges_n) * len(edges_d)] = np.repeat(edges_n, len(edges_d))
    d[:len(edges_n) * len(edges_d)] = np.tile(edges_d, len(edges_n))
    n[-K // 8:] = rng.choice([0.0, -0.0], K // 8)                                  # the planar orbits' z = 0 numerators
    x = np.abs(_rand(rng, K, -767, 1024))
    x[:6] = [2.0 ** -767, np.finfo(np.float64).max, 2.0 ** -200, 2.0 ** 200, 1.0, 2.0]
    q_hw, q_fast, s_hw, s_fast, pred = probe(n, d, x)
    assert np.array_equal(pred & 1, _num_inband(n).astype(np.int32))
    assert np.array_equal((pred >> 1) & 1, _sq_inband(x).astype(np.int32))
    bad = np.flatnonzero(_bits(q_hw) != _bits(q_fast))
    assert bad.size == 0, [(n[i], d[i], q_hw[i], q_fast[i]) for i in bad[:5]]
    bad = np.flatnonzero(_bits(s_hw) != _bits(s_fast))
    assert bad.size == 0, [(x[i], s_hw[i], s_fast[i]) for i in bad[:5]]
    # the reciprocal is shared: r^3 of a guarded r^2 stays inside [2^-300, 2^300]
    s = np.abs(_rand(rng, 4096, -200, 200))
    s[:2] = [2.0 ** -200, 2.0 ** 200]
    r3 = np.sqrt(s) ** 3
    assert (r3 >= 2.0 ** -300).all() and (r3 <= 2.0 ** 300).all()


def test_out_of_band_operands_are_rejected(probe):
    tiny = np.array([2.0 ** -602, np.nextafter(2.0 ** -601, 0.0), 2.0 ** -1000, 5e-324, -5e-324, 2.0 ** -1022, 1e-200, 2.0 ** 423,
                     -(2.0 ** 423), 2.0 ** 1000, np.finfo(np.float64).max])
    sq = np.array([np.nextafter(2.0 ** -200, 0.0), np.nextafter(2.0 ** 200, np.inf), 0.0, -0.0, -1.0, np.inf, np.nan, 5e-324,
                   1e-70, 1e70])
    k = max(len(tiny), len(sq))
    n = np.resize(tiny, k)
    x = np.resize(sq, k)
    _, _, _, _, pred = probe(n, np.ones(k), x)
    assert not (pred & 1).any()
    assert not ((pred >> 1) & 1).any()


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_c2_trajectories_leaving_the_band_stay_bitexact(variant):
    y0, p, t0, t1 = W.cr3bp_batch(256)
    y0 = np.array(y0, dtype=np.float64, copy=True)
    mu = float(np.asarray(p)[0, 140])
    y0[2, 3] = 1e-200                     # out-of-plane offset: numerators far below 2^-601 for the whole run
    y0[5, 3] = 0.0
    y0[1, 70] = 5e-324                    # a denormal coordinate at the start
    y0[:, 140] = [-mu, 1e-31, 0.0, 0.0, 0.0, 0.0]        # at rest next to the first primary: r^2 far below 2^-200
    o = dict(method="DOPRI5", rtol=1e-6, atol=1e-9, max_steps=3000)
    ref = oracle_batch("cr3bp", y0, p, t0, t1, **o)
    got = gpu_batch("cr3bp", y0, p, t0, t1, variant=variant, **o)
    assert_bitexact(got, ref, f"variant {variant}: ")
