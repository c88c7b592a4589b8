"""One generated system per state width for the wave-per-trajectory RK kernels (rk_group.h, 8 < n <= 512), with its numpy twin.

The group kernels are templates over the group width G (16, 32 or 64 lanes per trajectory) and the lane slice
C = ceil(n / G), the number of components a lane owns: every per-lane array has C elements and every SoA access goes through
`lane + G c`, guarded by `i < n`.  A ring couples component i to i - 1 and i + 1 with wrap-around, so lane 0 reads the last
component of the ragged top slot and the owner of that component reads lane 0's; the per-component decay rate
a_i = 0.125 (i % 11) makes any two components of a slot (and any two neighbouring slots: 64 % 11 = 9) distinguishable.

    y_i' = p0 ((y_{i-1} - 2 y_i) + y_{i+1}) - a_i y_i

User code is compiled with -ffp-contract=off in both arithmetic modes, so the numpy twin (same association) serves the strict
oracle (detpow=True) and the FMA oracle (fma=True) alike.  Used by tests/test_group_cases_cpu.py (the references meet the
conditions that make them worth comparing with) and tests/test_gpu_group_slices.py (the kernels equal them bit for bit)."""
import functools

import numpy as np

from oracle import oracle as O

# C = 2, 2, 3, 3, 5, 5, 6, 7, 8, 8, 8.  One lane in the top slot (n = 64 (C - 1) + 1) at C = 2, 3, 5, 7, 8 (65, 129, 257, 385,
# 449), one lane short of a full slot at C = 6, 8 (383, 511), a full top slot at C = 2, 3, 5, 8 (128, 192, 320, 512).  C = 4 is
# the built-in 256-cell heat equation's (tests/test_gpu_large_n.py), C = 1 is SMALL's.
WIDE = [65, 128, 129, 192, 257, 320, 383, 385, 449, 511, 512]
# G = 16 | 32 | 64 on both sides of each switch (n <= 16, n <= 32)
SMALL = [9, 16, 17, 32, 33]
NARROW_METHODS = [17, 65, 192, 449, 512]          # the widths RK23 and RK4 run at
OUTPUT_WIDTHS = [129, 320, 449, 512]              # the widths the output paths run at
EVENT_WIDTHS = [129, 512]

TOL = {"RK23": (1e-5, 1e-8), "DOPRI5": (1e-7, 1e-9), "DOP853": (1e-9, 1e-11)}
COUPLINGS = (3.0, 40.0, 40.0, 40.0, 150.0, 40.0)
B_WIDE, B_SMALL = 6, 11                           # 11 trajectories of n <= 32: wavefronts of 4 or 2 groups that diverge
CHUNK = 7


def method_options(method):
    """Options of the reference's field names for one method (RK4 is fixed-step: first_step is its step)"""
    if method == "RK4":
        return dict(method="RK4", first_step=0.01)
    return dict(method=method, rtol=TOL[method][0], atol=TOL[method][1])


def batch_size(n):
    return B_SMALL if n <= 32 else B_WIDE


def end_state_pairs():
    """every (n, method) whose end state and counters the GPU file compares"""
    pairs = [(n, m) for n in WIDE + SMALL for m in ("DOPRI5", "DOP853")]
    return pairs + [(n, m) for n in NARROW_METHODS for m in ("RK23", "RK4")]


def ring(n):
    """(src, fun, events_src, events_fun): the device snippet in component form, its numpy twin, the two event functions
    as a device snippet (whole-state signature) and their twin"""
    src = r'''
#define RING_N %d   // not N: the snippet shares a translation unit with the integrator headers
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{
    const int l = i > 0 ? i - 1 : RING_N - 1, r = i < RING_N - 1 ? i + 1 : 0;
    const double a = 0.125 * (double)(i %% 11);
    return p[0] * ((y[l] - 2.0 * y[i]) + y[r]) - a * y[i];
}
''' % n
    events_src = r'''
__device__ void events(double t, const double* y, double* g, const double* p)
{
    g[0] = y[0] - y[RING_N - 1];     // across the ragged top slot
    g[1] = y[RING_N / 2];
}
'''
    a = 0.125 * (np.arange(n) % 11).astype(np.float64)

    def fun(t, y, p):
        return p[0] * ((np.roll(y, 1) - 2.0 * y) + np.roll(y, -1)) - a * y

    def events_fun(t, y, p):
        return [y[0] - y[n - 1], y[n // 2]]

    return src, fun, events_src, events_fun


def batch(n, seed=0, B=B_WIDE, backward=True):
    """(y0 [n, B], p [1, B], t0, t1 [B]): random states, couplings 3 (slow: long steps), 40 (steps rejected at the
    tolerances above) and 150 (stability-limited), end times in [1, 2]; trajectory 2 runs backward (the ring then grows:
    its end time is short) and trajectory 3 has a zero-length interval.  backward=False keeps trajectory 2 forward: RK4's
    first_step is its signed step, so one first_step = 0.01 for the batch is an invalid step size for a backward run
    (rk4.rs:81-87)."""
    rng = np.random.default_rng(1000 * seed + n)
    y0 = rng.standard_normal((n, B))
    p = np.array([[COUPLINGS[b % len(COUPLINGS)] for b in range(B)]])
    t1 = rng.uniform(1.0, 2.0, B)
    if backward:
        t1[2] = -0.05 * t1[2]
    t1[3] = 0.0
    return y0, p, 0.0, t1


def method_batch(n, method, seed=0):
    """the batch one method runs at width n"""
    return batch(n, seed, batch_size(n), backward=method != "RK4")


@functools.lru_cache(maxsize=None)
def references(n, method, fma, seed=0, dense=False, t_eval=None):
    """the oracle's solve_ivp of every trajectory of batch(n, seed): strict (portable pow) or FMA build; shared by the tests
    of one process and never modified"""
    _, fun, _, _ = ring(n)
    y0, p, t0, t1 = method_batch(n, method, seed)
    kw = dict(method_options(method))
    if dense:
        kw["dense_output"] = True
    if t_eval is not None:
        kw["t_eval"] = list(t_eval)
    mode = dict(fma=True) if fma else dict(detpow=True)
    return [O.solve_ivp(fun, t0, float(t1[b]), list(y0[:, b]), params=[float(p[0, b])], **mode, **kw) for b in range(y0.shape[1])]


# ---- the event case: two event functions; the first ends the trajectory at its 2nd occurrence (the ring is dissipative, so
# no component oscillates: two sign changes of y[0] - y[n - 1] is what several trajectories of a random batch show), the
# second counts in the negative direction only ----
EVENT_DIRECTION, EVENT_TERMINAL = [0, -1], [2, 0]
EVENT_T1 = 2.0


def event_batch(n, seed=0):
    """(y0, p, t0, t1) of the event case: the batch above over one common interval, forward only"""
    y0, p, t0, _ = batch(n, seed, B_WIDE)
    return y0, p, t0, np.full(y0.shape[1], EVENT_T1)


@functools.lru_cache(maxsize=None)
def event_references(n, method, fma, seed=0):
    _, fun, _, ev = ring(n)
    y0, p, t0, t1 = event_batch(n, seed)
    mode = dict(fma=True) if fma else dict(detpow=True)
    return [O.solve_ivp(fun, t0, float(t1[b]), list(y0[:, b]), params=[float(p[0, b])], events=ev, n_events=2,
                        event_direction=EVENT_DIRECTION, event_terminal=EVENT_TERMINAL, **mode, **method_options(method))
            for b in range(y0.shape[1])]
