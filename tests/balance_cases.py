"""The batches of tests/test_gpu_balance.py, shared by the test (which asks the oracle) and by its child processes
(tests/helpers/balance_dump.py, which ask the GPU)."""
import numpy as np

from ivp_amd import workloads as W

KEYS = ("y_end", "t_end", "h_next", "status", "nfev", "nstep", "naccpt", "nrejct")
# (method, FMA arithmetic)
MODES = (("DOPRI5", False), ("DOPRI5", True), ("DOP853", False))
T1 = 2.0 * W.ARENSTORF_PERIOD          # ~400 DOPRI5 attempts: three rounds of 192
T1_LOGGED = W.ARENSTORF_PERIOD


def opts(method):
    # a step budget: at two periods a few of the perturbed orbits pass so close to a primary that they need millions of
    # steps; they end with NeedLargerNMax after 1000 (one more status word to compare) instead of a minute in a lone wave
    return dict(method=method, rtol=1e-6, atol=1e-9, max_steps=1000)


def name(B, method, fma):
    return f"{B}.{method}.{'fma' if fma else 'strict'}"


def batch(B):
    y0, p, t0, _ = W.cr3bp_batch(B)
    return y0, p, t0, T1


def mixed_batch(B):
    """Intervals of zero length (those trajectories retire in the init kernel), of a twentieth of a period (they retire in the
    first pieces of the first round), and of one to three periods (they retire in the middle of later rounds); the second block
    of 64 list entries has only the first two kinds, so the whole block is dead after its first piece."""
    y0, p, t0, _ = W.cr3bp_batch(B)
    j = np.arange(B)
    t1 = W.ARENSTORF_PERIOD * np.choose(j % 6, [0.0, 0.05, 1.0, 2.0, 3.0, 3.0])
    blk = (j >= 64) & (j < 128)
    t1[blk] = np.where(j[blk] % 2, 0.0, 0.05 * W.ARENSTORF_PERIOD)
    return y0, p, t0, t1
