"""Shared inputs of tests/test_inband_deferred_cpu.py and tests/test_gpu_inband_deferred.py: the operand sets on which
the folded guard of the strict CR3BP right-hand side (ivp_inband_fold / ivp_inband_ok / ivp_inband_seed in
ivp_amd/csrc/rk_core.h) is compared with the per-call one, the host restatement of both (tests/helpers/inband_guard_host.cpp,
built with g++ into a directory the caller names), and the 72-trajectory batch of the integration cases."""
import ctypes
import json
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "inband_late_stage_state.json")
HOST_FLAGS = ["-std=c++17", "-march=x86-64-v3", "-fno-fast-math", "-ffp-contract=off", "-Wno-unknown-pragmas", "-DIVP_FAST=0"]
MU_EM = 0.0121505856


def _pow2(e):
    return np.ldexp(1.0, e)


def edge_values():
    """Zeros of both signs, denormals, inf, NaN and the ends of every band of the proof, each with its two neighbours."""
    out = [0.0, -0.0, 5e-324, -5e-324, _pow2(-1022), np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, np.finfo(np.float64).max]
    for e in (-100, 100, -541, -540, -601, -600, 422, 423, -51, 60, -767):
        v = _pow2(e)
        out += [np.nextafter(v, 0.0), v, np.nextafter(v, np.inf), -v]
    return np.array(out)


def operand_states(k=1 << 20, seed=20261019):
    """(x, y, z, mu), each [k + edges]: what one call of the right-hand side sees.  Every coordinate draws its own category:
    ordinary magnitudes (z often exactly 0), exponents over the whole double range, exponents around the factor bound
    2^-541, around the |w| <= 2^100 / >= 2^-100 ends of the r^2 band, around the old numerator bound 2^-601, and specials."""
    rng = np.random.default_rng(seed)

    def coord(n, zero_share):
        cat = rng.integers(0, 8, n)
        mant = rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
        e = np.select([cat <= 1, cat == 2, cat == 3, cat == 4, cat == 5, cat == 6],
                      [rng.integers(-10, 2, n), rng.integers(-1074, 1024, n), rng.integers(-546, -536, n),
                       rng.choice([-1, 1], n) * rng.integers(96, 104, n), rng.integers(-610, -590, n), rng.integers(-60, 70, n)], 0)
        v = np.ldexp(mant, e)
        special = rng.choice(np.array([0.0, -0.0, 5e-324, np.inf, -np.inf, np.nan, 1e-310]), n)
        v = np.where(cat == 7, special, v)
        return np.where(rng.random(n) < zero_share, 0.0, v)

    x, y, z = coord(k, 0.0), coord(k, 0.05), coord(k, 0.3)
    mu = np.select([rng.random(k) < 0.5, rng.random(k) < 0.5], [np.full(k, MU_EM), rng.uniform(0.0, 0.5, k)], coord(k, 0.1))
    pick = rng.random(k) < 0.06
    mu[pick] = rng.choice(np.array([0.0, 1.0, _pow2(-60)]), int(pick.sum()))
    # the edges: every triple of edge values for (x, y, z) with mu in {0, 1, 2^-60, Earth-Moon}; with mu = 0 the offset a is x itself
    ev = edge_values()
    ex, ey, ez, em = np.meshgrid(ev, ev, ev, np.array([0.0, 1.0, _pow2(-60), MU_EM]), indexing="ij")
    return (np.concatenate([x, ex.ravel()]), np.concatenate([y, ey.ravel()]), np.concatenate([z, ez.ravel()]),
            np.concatenate([mu, em.ravel()]))


def ordinary_states(k=4096, seed=7):
    """States of the size the benchmark integrates: the folded guard must hold on all of them."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, k)
    y = rng.uniform(-1.5, 1.5, k)
    z = np.where(rng.random(k) < 0.5, 0.0, rng.uniform(-0.2, 0.2, k))
    return x, y, z, np.full(k, MU_EM)


def build_host(tmpdir):
    """g++ build of tests/helpers/inband_guard_host.cpp; returns (guards(x, y, z, mu) -> (per_call, folded), trace(...))."""
    so = os.path.join(str(tmpdir), "libinband_guard_host.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + HOST_FLAGS + [os.path.join(HERE, "helpers", "inband_guard_host.cpp"), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    lib.inband_guards.restype = None
    lib.inband_guards.argtypes = [dp, dp, dp, dp, ip, ip, ctypes.c_long]
    lib.inband_trace.restype = ctypes.c_int
    lib.inband_trace.argtypes = [dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ip, ip]

    def guards(x, y, z, mu):
        arrs = [np.ascontiguousarray(v, dtype=np.float64) for v in (x, y, z, mu)]
        n = arrs[0].size
        per_call, folded = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        lib.inband_guards(*[v.ctypes.data_as(dp) for v in arrs], per_call.ctypes.data_as(ip), folded.ctypes.data_as(ip), n)
        return per_call.astype(bool), folded.astype(bool)

    def trace(y0, mu, t1, method, rtol=1e-6, atol=1e-9, max_attempts=400):
        y0 = np.ascontiguousarray(y0, dtype=np.float64)
        ok = np.full((max_attempts, 12), -1, dtype=np.int32)
        ns = ctypes.c_int(0)
        n = lib.inband_trace(y0.ctypes.data_as(dp), float(mu), float(t1), {"DOPRI5": 1, "DOP853": 2}[method], rtol, atol, max_attempts,
                             ok.ctypes.data_as(ip), ctypes.byref(ns))
        return ok[:n, :ns.value].astype(bool)

    return guards, trace


def late_stage_state():
    """The committed initial state whose attempts include one with the first stage in band and a later stage out of it."""
    with open(GOLDEN) as f:
        g = json.load(f)
    return np.array([float.fromhex(v) for v in g["y0_hex"]]), float.fromhex(g["mu_hex"]), g


def batch72():
    """72 trajectories: one full thread-per-trajectory wave plus one lane-cooperative wave's worth.  In both parts: the
    trajectories that leave the band (tests/test_gpu_inband_div_sqrt.py) and the late-stage state of tests/golden."""
    from ivp_amd import workloads as W
    y0, p, t0, t1 = W.cr3bp_batch(72)
    y0 = np.array(y0, dtype=np.float64, copy=True)
    p = np.array(p, dtype=np.float64, copy=True)
    late, late_mu, _ = late_stage_state()
    for base in (0, 64):
        mu = float(p[0, base + 5])
        y0[2, base + 1] = 1e-200                     # out-of-plane offset: a factor far below 2^-541 for the whole run
        y0[5, base + 1] = 0.0
        y0[1, base + 3] = 5e-324                     # a denormal coordinate at the start
        y0[:, base + 5] = [-mu, 1e-31, 0.0, 0.0, 0.0, 0.0]   # at rest next to the first primary: r^2 far below 2^-200
        y0[:, base + 6] = late
        p[0, base + 6] = late_mu
    return y0, p, t0, t1


def batch72_late_only():
    """72 ordinary trajectories and, in each part, the late-stage state as the ONLY lane that ever leaves the band: its wave's
    decision then depends on a stage after the first (in batch72 the z = 1e-200 lane fails every wave from the first stage on)."""
    from ivp_amd import workloads as W
    y0, p, t0, t1 = W.cr3bp_batch(72)
    y0 = np.array(y0, dtype=np.float64, copy=True)
    p = np.array(p, dtype=np.float64, copy=True)
    late, late_mu, _ = late_stage_state()
    for base in (0, 64):
        y0[:, base + 6] = late
        p[0, base + 6] = late_mu
    return y0, p, t0, t1
