"""Trajectories that FAIL (status 2 / 3 / 4) or carry a non-finite state, next to healthy ones: the batches, the
per-trajectory reference helpers and the CPU half of the checks.  tests/test_gpu_failure_paths.py runs the same batches
through libivp_hip.so on every kernel shape.

The bar is DESIGN section 5's: the strict kernel bodies (here: the host emulation of rk_core.h / bdf_core.h) equal
liboracle_detpow bit for bit -- y_end, t_end, h_next, status and every counter of every trajectory, failing ones
included, NaN equal to NaN.  No tolerance anywhere in this file.

Every test asserts on the ORACLE's result that the batch took the branch it is named after, so a change that makes the
input stop failing fails the test instead of passing it quietly.

RK23 never returns from the reference with a NaN error estimate (documented deviation 1): the oracle is never called on
an RK23 batch with a non-finite lane.  There the bad lanes must end with status 3 and the healthy lanes equal an oracle
run of the healthy lanes alone.  RK4 has no error estimate: a non-finite state travels to the end with status 0, which
is what the oracle reports and what is asserted.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests.common import KEYS_INT, assert_bitexact, emul_batch, oracle_batch

NAN, INF = np.nan, np.inf
OK, MAXSTEPS, TOOSMALL, STIFF = 0, 2, 3, 4


# ---- helpers ---------------------------------------------------------------------------------------------------------

def poison(y0, lanes):
    """lanes: (trajectory, component, value); component -1 is the last one"""
    y0 = np.array(y0, dtype=np.float64)
    for b, c, v in lanes:
        y0[c, b] = v
    return y0


def take(res, idx):
    """the trajectories idx of a result dict (arrays whose last axis is the batch)"""
    B = len(res["status"])
    return {k: (np.asarray(v)[..., idx] if isinstance(v, np.ndarray) and v.ndim and v.shape[-1] == B else v) for k, v in res.items()}


def per_trajectory(fun, y0, params, t0, t1, *, jac=None, fma=False, **opts):
    """One oracle solve_ivp() call per trajectory (Python callables or a built-in name), in the result shape of
    oracle_batch.  The end state and end time are the last step record: solve_ivp's record mode stores the start point
    and every accepted step, so this holds for a trajectory that fails before its first accepted step as well
    (test_per_trajectory_helper_equals_the_batch_entry_point_on_failing_lanes)."""
    n, B = y0.shape
    t0, t1 = np.broadcast_to(np.asarray(t0, float), B), np.broadcast_to(np.asarray(t1, float), B)
    res = {"y_end": np.zeros((n, B)), "t_end": np.zeros(B), "h_next": np.zeros(B), "status": np.zeros(B, np.int32)}
    for k in KEYS_INT[1:]:
        res[k] = np.zeros(B, np.uint64)
    sols = []
    for b in range(B):
        extra = {} if params is None else {"params": [float(v) for v in params[:, b]]}
        if jac is not None:
            extra["jac"] = jac
        s = O.solve_ivp(fun, float(t0[b]), float(t1[b]), [float(v) for v in y0[:, b]], detpow=True, fma=fma, **extra, **opts)
        res["y_end"][:, b], res["t_end"][b], res["h_next"][b], res["status"][b] = s.y[-1], s.t[-1], s.h_next, s.status
        for k in KEYS_INT[1:]:
            res[k][b] = getattr(s, k)
        sols.append(s)
    res["solutions"] = sols
    return res


def assert_rk23_rule(got, y0, healthy_ref, bad):
    """RK23 with non-finite lanes: status 3 on the bad lanes, the rest equal the oracle run of the healthy lanes alone"""
    good = np.ones(y0.shape[1], bool)
    good[list(bad)] = False
    assert (np.asarray(got["status"])[list(bad)] == TOOSMALL).all(), got["status"]
    assert_bitexact(take(got, good), healthy_ref, "RK23 healthy lanes: ")


# ---- section 1a: thread-per-trajectory batches (n <= 8), B = 70 = one full wavefront and a partial one ----------------------

BAD70 = ((0, 0, NAN), (63, -1, INF), (64, -1, NAN), (69, 0, -INF))
LONG70 = (5, 40, 66)


def thread_batch(rhs, method):
    """-> (y0, params, t0, t1, options, statuses the oracle must report side by side)"""
    B = 70
    rng = np.random.default_rng(5)
    p = None
    if rhs == "sho":
        y0 = np.stack([np.cos(rng.uniform(0, 1, B)), np.sin(rng.uniform(0, 1, B))])
        t1 = rng.uniform(0.5, 3.0, B)
        t1[list(LONG70)] = 40.0
        # the step cap makes the long lanes need 4000 steps; the NaN lanes need 459 (DOPRI5) .. 1016 (BDF) attempts to underflow
        o = dict(method=method, rtol=1e-6, atol=1e-9, max_steps=1200, max_step=0.01)
        want = {OK, MAXSTEPS, TOOSMALL}
        if method == "RK4":
            o, want = dict(method=method, first_step=0.02, max_steps=200), {OK, MAXSTEPS}
    elif rhs == "robertson":
        y0 = np.tile(np.array([[1.0], [0.0], [0.0]]), (1, B))
        y0[0] *= 1.0 + 0.01 * np.arange(B)
        t1 = rng.uniform(0.05, 0.3, B)
        t1[list(LONG70)] = 40.0
        t1[[7, 33]] = 0.8
        o = dict(method=method, rtol=1e-6, atol=1e-9, max_steps=1200)
        want = {OK, MAXSTEPS, TOOSMALL} if method == "DOPRI5" else {OK, TOOSMALL, STIFF}   # DOP853's detector fires at step 1017
        if method == "BDF":
            t1[list(LONG70)] = 1e9
            o.update(rtol=1e-9, max_steps=1100)
            want = {OK, MAXSTEPS, TOOSMALL}
        if method == "RK4":
            o, want = dict(method=method, first_step=2e-4, max_steps=2000), {OK, MAXSTEPS}
    else:   # vdp with the stiff-vdp parameter ladder: ProbablyStiff beside everything else
        assert rhs == "vdp" and method in ("DOPRI5", "DOP853")
        y0 = np.tile(np.array([[2.0], [0.0]]), (1, B))
        y0[0] *= 1.0 + 0.001 * np.arange(B)
        p = np.tile(np.array([[1.0, 5.0, 50.0, 200.0, 500.0, 1000.0, 2000.0]]), (1, 10))
        t1 = np.full(B, 40.0)
        t1[::3] = rng.uniform(1.0, 5.0, len(t1[::3]))
        t1[[7, 35]] = 4000.0          # mu = 1: not stiff, far more than max_steps steps
        o = dict(method=method, rtol=1e-4, atol=1e-6, max_steps=1500)
        want = {OK, MAXSTEPS, TOOSMALL, STIFF}
    return poison(y0, BAD70), p, 0.0, t1, o, want


THREAD_SHAPES = [(r, m) for r in ("sho", "robertson") for m in ("DOPRI5", "DOP853", "RK4", "BDF")] + [("vdp", "DOPRI5"), ("vdp", "DOP853")]
_cache = {}


def thread_reference(rhs, method):
    """the oracle's result of thread_batch(rhs, method), computed once per process and never modified"""
    key = (rhs, method)
    if key not in _cache:
        y0, p, t0, t1, o, want = thread_batch(rhs, method)
        r = oracle_batch(rhs, y0, p, t0, t1, **o)
        check_thread_reference(r, method, want, (7, 35) if rhs == "vdp" else LONG70)
        _cache[key] = r
    return _cache[key]


def check_thread_reference(r, method, want, long):
    """the batch took the branches it is built for"""
    st = r["status"]
    assert set(int(s) for s in st) == want, (sorted(set(st)), want)
    bad = [b for b, _, _ in BAD70]
    if method == "RK4":
        assert (st[bad] == OK).all() and not np.isfinite(r["y_end"][:, bad]).all(axis=0).any()
    else:
        assert (st[bad] == TOOSMALL).all() and (r["naccpt"][bad] == 0).all()
        assert np.isin(st[list(long)], (MAXSTEPS, STIFF)).all()
    assert len(set(int(v) for v in r["nstep"][st == OK])) > 5      # ragged: the finishing lanes retire at different times


@pytest.mark.parametrize("chunk", [100000, 7])
@pytest.mark.parametrize("rhs,method", THREAD_SHAPES)
def test_mixed_status_batch_in_the_host_emulation(rhs, method, chunk):
    y0, p, t0, t1, o, want = thread_batch(rhs, method)
    ref = thread_reference(rhs, method)
    got = emul_batch(rhs, y0, p, t0, t1, chunk=chunk, **o)
    assert_bitexact(got, ref, f"{rhs} {method} chunk={chunk}: ")
    # the FMA arithmetic mode against the oracle's FMA build
    ref = oracle_batch(rhs, y0, p, t0, t1, fma=True, **o)
    bad = [b for b, _, _ in BAD70]
    assert (ref["status"][bad] == (OK if method == "RK4" else TOOSMALL)).all() and set(int(v) for v in ref["status"]) == want
    assert_bitexact(emul_batch(rhs, y0, p, t0, t1, chunk=chunk, fast=True, **o), ref, f"{rhs} {method} fma chunk={chunk}: ")


@pytest.mark.parametrize("rhs", ["sho", "robertson"])
def test_rk23_mixed_status_batch_in_the_host_emulation(rhs):
    y0, p, t0, t1, o, _ = thread_batch(rhs, "DOPRI5")
    o = dict(o, method="RK23", rtol=1e-4, atol=1e-7)
    bad = [b for b, _, _ in BAD70]
    good = np.ones(70, bool)
    good[bad] = False
    ref = oracle_batch(rhs, y0[:, good], p, t0, t1[good], **o)
    assert MAXSTEPS in ref["status"] and OK in ref["status"]
    for chunk in (100000, 7):
        assert_rk23_rule(emul_batch(rhs, y0, p, t0, t1, chunk=chunk, **o), y0, ref, bad)


def test_bdf_branch_signatures_of_the_sho_batch():
    """The Newton-failure halving chain down to StepSizeTooSmall, and the non-finite initial state that fails before
    its first step: the counter signatures of both on the oracle (bdf.rs:325-328, 383-395)."""
    r = thread_reference("sho", "BDF")
    for b in (0, 64):      # NaN component: every attempt rejected, one LU and one Jacobian per attempt, h halves to the denormals
        assert r["status"][b] == TOOSMALL and r["naccpt"][b] == 0
        assert r["nstep"][b] == r["nrejct"][b] == r["nlu"][b] > 1000 and r["njev"][b] == r["nstep"][b] + 1
        assert 0.0 < r["h_next"][b] < 1e-300
    for b in (63, 69):     # infinite component: the initial step size is not finite
        assert r["status"][b] == TOOSMALL
        assert (r["nstep"][b], r["nlu"][b], r["njev"][b], r["h_next"][b]) == (0, 0, 1, 0.0)


def test_per_trajectory_helper_equals_the_batch_entry_point_on_failing_lanes():
    for method in ("DOPRI5", "BDF"):
        y0, p, t0, t1, o, _ = thread_batch("sho", method)
        idx = [0, 1, 5, 63, 64, 69]
        one = per_trajectory("sho", y0[:, idx], None, t0, t1[idx], **o)
        assert_bitexact(one, take(thread_reference("sho", method), idx), "solve_ivp vs batch: ")
        assert len(one["solutions"][3].t) == 1      # the trajectory that failed before its first step: the start record alone


# ---- section 1b: the systems of the other kernel shapes (inputs only; the kernels are GPU-only) --------------------------

def coop_batch(rhs, method, B, where):
    """sho / lorenz / cr3bp use 2 / 3 / 6 of a group's 8 lanes.  Bad groups: first of its wave (0), last of its wave (7),
    first of the partly filled last wave (64), last trajectory (B - 1).  where = 0: the NaN sits in component 0 and the
    inf in the last component; where = -1: the other way round."""
    from ivp_amd import workloads as W
    rng = np.random.default_rng(40 + B)
    p = None
    if rhs == "sho":
        y0 = np.stack([np.cos(rng.uniform(0, 1, B)), np.sin(rng.uniform(0, 1, B))])
        t1, long_t = rng.uniform(0.5, 3.0, B), 40.0
        o = dict(rtol=1e-6, atol=1e-9, max_steps=800, max_step=0.01)
    elif rhs == "lorenz":
        y0 = 1.0 + 0.1 * rng.standard_normal((3, B))
        p = np.repeat(np.array([[10.0], [28.0], [8.0 / 3.0]]), B, axis=1) * (1.0 + 0.01 * rng.standard_normal((3, B)))
        t1, long_t = rng.uniform(0.2, 1.0, B), 60.0
        o = dict(rtol=1e-8, atol=1e-10, max_steps=800)
    else:
        y0, p, _, _ = W.cr3bp_batch(B)
        t1, long_t = rng.uniform(0.5, 3.0, B), 1000.0
        o = dict(rtol=1e-9, atol=1e-12, max_steps=800)
    bad = sorted({0, min(7, B - 1), B - 1} | ({64} if B > 64 else set()))
    lanes = [(b, (where if k % 2 == 0 else -1 - where), (NAN if k % 2 == 0 else INF)) for k, b in enumerate(bad)]
    long = [b for b in (3, 8, 33) if b < B and b not in bad]
    t1[long] = long_t
    return poison(y0, lanes), p, 0.0, t1, dict(method=method, **o), bad, long


def ring_source(K, events=False):
    src = r'''
    #define K %d
    __device__ double ode_comp(int i, double t, const double* y, const double* p)
    {   // K masses on a ring: y[0..K) positions, y[K..2K) velocities
        if (i < K) return y[K + i];
        const int k = i - K, l = (k + K - 1) %% K, r = (k + 1) %% K;
        return p[0] * (y[l] - 2.0 * y[k] + y[r]);
    }
    ''' % K
    if events:
        src += "__device__ void events(double t, const double* y, double* g, const double* p) { g[0] = y[0] - y[K / 2]; }\n"
    return src


def ring_fun(K):
    left, right = (np.arange(K) + K - 1) % K, (np.arange(K) + 1) % K

    def ring(t, y, p):      # the snippet's association: p0 * ((y[l] - 2 y[k]) + y[r])
        d = np.empty(2 * K)
        d[:K] = y[K:]
        q = y[:K]
        d[K:] = p[0] * (q[left] - 2.0 * q + q[right])
        return d
    return ring


def ring_batch(K, method, pos):
    """n = 2K states, B = 11 (n = 12: two full wavefronts of four groups and one of three).  The NaN trajectory sits at
    group position `pos` of the first wavefront, the inf trajectory in the partly filled last one."""
    n, B = 2 * K, 11
    rng = np.random.default_rng(10 + K)
    y0 = rng.standard_normal((n, B))
    par = rng.uniform(1.0, 4.0, (1, B))
    t1 = rng.uniform(1.0, 3.0, B)
    tol = dict(RK23=(1e-5, 1e-8), DOPRI5=(1e-7, 1e-9), DOP853=(1e-9, 1e-11), BDF=(1e-5, 1e-8))[method]
    bad = [pos, 8 + pos % 3]
    long = [b for b in (5, 6) if b not in bad]
    t1[long] = 400.0
    y0 = poison(y0, [(bad[0], (0 if pos % 2 == 0 else -1), NAN), (bad[1], K, INF)])
    # max_steps above the NaN chains (DOPRI5 ~460, DOP853 ~680, BDF ~1020 attempts), below what the long horizon needs
    o = dict(method=method, rtol=tol[0], atol=tol[1], max_steps=1100 if method == "BDF" else 700, max_step=0.05)
    return y0, par, 0.0, t1, o, bad, long


def decay100_batch(method, B=6):
    rng = np.random.default_rng(3)
    y0 = poison(rng.uniform(-2.0, 2.0, (100, B)), [(1, 0, NAN), (3, 99, NAN), (4, 50, INF)])
    t1 = rng.uniform(0.5, 2.0, B)
    t1[2] = 400.0
    o = dict(method=method, rtol=1e-5, atol=1e-8, max_steps=1100 if method == "BDF" else 700, max_step=0.1)
    if method == "RK23":
        o.update(rtol=1e-4, atol=1e-7)
    return y0, None, 0.0, t1, o, [1, 3, 4], [2]


def heat256_batch(method, B=8):
    rng = np.random.default_rng(5)
    x = np.arange(1, 257) / 257.0
    y0 = np.sin(np.pi * x[:, None] * rng.integers(1, 6, B)[None, :]) + 0.1 * rng.standard_normal((256, B))
    kappa = rng.uniform(20.0, 100.0, (1, B))
    kappa[0, [2, 6]] = 4000.0
    t1 = rng.uniform(0.02, 0.1, B)
    t1[[2, 6]] = 20.0
    y0 = poison(y0, [(1, 128, NAN), (5, 255, INF)])
    o = dict(method=method, rtol=1e-4, atol=1e-7)
    if method == "RK23":      # no stiffness detector (127 000 steps to t = 20): the kappa = 4000 members end at max_steps instead
        o["max_steps"] = 2000
    return y0, kappa, 0.0, t1, o, [1, 5], [2, 6]


def dense64_batch(B=5):
    rng = np.random.default_rng(12)
    y0 = poison(1.0 + 0.5 * rng.standard_normal((64, B)), [(1, 63, NAN), (3, 0, INF)])
    k = np.full((1, B), 3.0) * (1.0 + 0.2 * rng.uniform(-1, 1, (1, B)))
    return y0, k, 0.0, 0.6, dict(method="BDF", rtol=1e-6, atol=1e-9), [1, 3], []


def check_group_reference(r, bad, long, long_status=MAXSTEPS):
    st = np.asarray(r["status"])
    assert (st[bad] == TOOSMALL).all() and (np.asarray(r["naccpt"])[bad] == 0).all(), st
    assert (st[long] == long_status).all(), st
    rest = [b for b in range(len(st)) if b not in bad and b not in long]
    assert (st[rest] == OK).all(), st


@pytest.mark.parametrize("method", ["DOPRI5", "DOP853"])
@pytest.mark.parametrize("rhs", ["sho", "lorenz", "cr3bp"])
def test_cooperative_batches_take_their_branches_and_pass_the_host_emulation(rhs, method):
    """rk_coop.h is GPU-only; the batches it is given are checked here on the oracle and on the per-lane bodies"""
    for B in (1, 9, 65):
        for where in (0, -1):
            y0, p, t0, t1, o, bad, long = coop_batch(rhs, method, B, where)
            ref = oracle_batch(rhs, y0, p, t0, t1, **o)
            check_group_reference(ref, bad, long)
            assert_bitexact(emul_batch(rhs, y0, p, t0, t1, chunk=5, **o), ref, f"{rhs} {method} B={B}: ")


@pytest.mark.parametrize("method", ["DOPRI5", "BDF"])
def test_ring_batch_takes_its_branches_on_the_oracle(method):
    y0, par, t0, t1, o, bad, long = ring_batch(6, method, 2)
    r = per_trajectory(ring_fun(6), y0, par, t0, t1, **o)
    check_group_reference(r, bad, long)
    if method == "BDF":      # the NaN trajectory: one failed LU-and-Newton attempt per halving; the inf one never factorises
        assert r["nlu"][bad[0]] == r["nrejct"][bad[0]] > 1000 and r["nlu"][bad[1]] == 0


@pytest.mark.parametrize("method", ["DOPRI5", "DOP853", "BDF"])
def test_large_system_batches_take_their_branches_on_the_oracle(method):
    y0, p, t0, t1, o, bad, long = decay100_batch(method)
    check_group_reference(oracle_batch("linear_decay100", y0, p, t0, t1, **o), bad, long)
    if method != "BDF":
        y0, p, t0, t1, o, bad, long = heat256_batch(method)
        check_group_reference(oracle_batch("heat1d256", y0, p, t0, t1, **o), bad, long, STIFF)
    else:
        y0, p, t0, t1, o, bad, long = dense64_batch()
        check_group_reference(oracle_batch("dense64", y0, p, t0, t1, **o), bad, long)


def test_counter_signatures_of_linear_decay100_bdf():
    """linear_decay100, BDF, rtol 1e-5 / atol 1e-8, t in [0, 2]: the NaN trajectory ends with status 3 after 1024 rejected
    steps and 4097 evaluations, the healthy ones with status 0 after 37 steps."""
    rng = np.random.default_rng(3)
    y0 = poison(rng.uniform(-2.0, 2.0, (100, 3)), [(1, 0, NAN)])
    r = oracle_batch("linear_decay100", y0, None, 0.0, 2.0, method="BDF", rtol=1e-5, atol=1e-8)
    assert (int(r["status"][1]), int(r["nrejct"][1]), int(r["nfev"][1])) == (TOOSMALL, 1024, 4097)
    assert list(r["status"][[0, 2]]) == [OK, OK] and list(r["nstep"][[0, 2]]) == [37, 37]


# ---- section 2: the singular-matrix branch of BDF ----------------------------------------------------------------------

H0 = 1.185 * 2.0 ** -4          # first attempt: order 1, c = h0 / alpha_1 = h0 / 1.185 = 2^-4, so 1 - 16 c == 0 exactly
LAM_NEXT = float(np.nextafter(16.0, 17.0))
SING_OPTS = dict(method="BDF", rtol=1e-6, atol=1e-9, first_step=H0)


def sing_comp(n):
    return min(3, n - 1)


def sing_fun(n):
    s = sing_comp(n)

    def fun(t, y, p):
        d = [-float(v) for v in y]
        d[s] = float(p[0]) * float(y[s])
        return d

    def jac(t, y, p):
        j = [[0.0] * n for _ in range(n)]
        for i in range(n):
            j[i][i] = -1.0
        j[0][0] = float(p[1])       # -1 for every healthy trajectory (the exact entry); NaN in the NaN-Jacobian case
        j[s][s] = float(p[0])
        return j
    return fun, jac


def sing_source(n):
    s = sing_comp(n)
    if n <= 8:
        return f"""
__device__ void ode(double t, const double* y, double* d, const double* p)
{{
    for (int i = 0; i < {n}; ++i) d[i] = -y[i];
    d[{s}] = p[0] * y[{s}];
}}
__device__ void jac(double t, const double* y, double* j, const double* p)
{{
    for (int i = 0; i < {n}; ++i) j[i * {n} + i] = -1.0;
    j[0] = p[1];
    j[{s} * {n} + {s}] = p[0];
}}
"""
    return f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p) {{ return i == {s} ? p[0] * y[i] : -y[i]; }}
__device__ void jac_col(int col, double t, const double* y, double* column, const double* p)
{{
    column[col] = col == {s} ? p[0] : (col == 0 ? p[1] : -1.0);
}}
"""


def sing_batch(n, B=7):
    """lambda = 16 (LU failure on the first attempt) beside 15 and nextafter(16) (Newton failure there) in one wavefront"""
    rng = np.random.default_rng(n)
    y0 = 1.0 + 0.2 * rng.standard_normal((n, B))
    lam = np.array([16.0, 15.0, LAM_NEXT, 16.0, 15.0, 16.0, LAM_NEXT])[:B]
    par = np.stack([lam, np.full(B, -1.0)])
    return y0, par, 0.0, 0.5


def check_singular_reference(first, full, par):
    """first: the oracle's result with max_steps = 1; full: to the end"""
    assert H0 / 1.185 == 2.0 ** -4
    n = np.asarray(full["y_end"]).shape[0]
    for b in range(par.shape[1]):
        sig = tuple(int(first[k][b]) for k in ("status", "nstep", "nrejct", "nlu", "njev", "nfev"))
        if par[0, b] == 16.0:
            assert sig == (MAXSTEPS, 1, 1, 1, 1, 1), sig          # no Newton evaluation at all: the LU-failure branch
            assert first["h_next"][b] == H0 / 2.0
        elif par[0, b] == LAM_NEXT:                               # one ulp off: factorised, and the Newton iteration ran
            assert sig[:4] == (MAXSTEPS, 1, 1, 1) and sig[5] >= 3, sig
            if n == 12:
                assert sig == (MAXSTEPS, 1, 1, 1, 1, 3), sig      # n = 12: one Jacobian, two Newton evaluations
    assert (np.asarray(full["status"]) == OK).all() and (np.asarray(full["nrejct"]) > 0).all()


@pytest.mark.parametrize("fma", [False, True], ids=["strict", "fma"])
@pytest.mark.parametrize("n", [3, 12])
def test_singular_first_attempt_takes_the_lu_failure_branch_on_the_oracle(n, fma):
    fun, jac = sing_fun(n)
    y0, par, t0, t1 = sing_batch(n)
    first = per_trajectory(fun, y0, par, t0, t1, jac=jac, fma=fma, max_steps=1, **SING_OPTS)
    full = per_trajectory(fun, y0, par, t0, t1, jac=jac, fma=fma, **SING_OPTS)
    check_singular_reference(first, full, par)
    if n == 12 and not fma:      # lambda = 16 at n = 12 goes on to finish with 72 accepted, 5 rejected steps and 18 LU
        assert any((int(full["naccpt"][b]), int(full["nrejct"][b]), int(full["nlu"][b])) == (72, 5, 18) for b in (0, 3, 5))


def nan_jac_batch(n, B=5):
    y0, par, t0, t1 = sing_batch(n, B)
    par[0] = 15.0
    par[1, 2] = NAN
    return y0, par, t0, t1


def check_nan_jac_reference(r):
    """NaN in J[0][0]: the pivot search of column 0 sees a NaN diagonal; every attempt fails and the step halves away"""
    st = np.asarray(r["status"])
    assert st[2] == TOOSMALL and r["naccpt"][2] == 0 and r["nlu"][2] > 1000, (st, r["nlu"])
    assert (np.delete(st, 2) == OK).all()


def test_nan_jacobian_entry_returns_through_step_halving_on_the_oracle():
    fun, jac = sing_fun(12)
    y0, par, t0, t1 = nan_jac_batch(12)
    check_nan_jac_reference(per_trajectory(fun, y0, par, t0, t1, jac=jac, **SING_OPTS))


# ---- section 3: output paths of a trajectory that fails part-way (n = 2 in the host emulation) ----------------------------

OUT_IDX = (0, 1, 5, 17, 40, 62, 63, 64, 66, 69)     # bad lanes, long lanes and some that finish
T_EVAL = np.concatenate([[-0.5], np.linspace(0.0, 14.0, 29), [45.0]])


def sho_out_options(method):
    y0, p, t0, t1, o, _ = thread_batch("sho", method)
    return y0, t1, o


def check_bounded_outputs(got, sols, idx, t_eval=None, dense=False, events=False):
    """t_eval samples / step log / dense segments / event records of the trajectories idx against the oracle Solutions"""
    seen = set()
    for b, s in zip(idx, sols):
        seen.add(int(s.status))
        assert int(got["status"][b]) == s.status and int(got["nfev"][b]) == s.nfev and int(got["naccpt"][b]) == s.naccpt, b
        if t_eval is not None:
            m = int(got["n_filled"][b])
            assert m == len(s.t), (b, m, len(s.t))
            assert np.array_equal(t_eval[got["eval_idx"][:m, b]], s.t)
            assert np.array_equal(got["y_eval"][:m, :, b], s.y, equal_nan=True), b
        else:
            m = int(got["n_log"][b])
            assert m == len(s.t), (b, m, len(s.t))
            assert np.array_equal(got["t_log"][:m, b], s.t) and np.array_equal(got["y_log"][:m, :, b], s.y, equal_nan=True), b
            if s.status == MAXSTEPS:
                assert m == s.naccpt + 1          # exactly its accepted steps (and the start record)
        if dense:
            ns = int(got["n_seg"][b])
            assert ns == (0 if s.seg_h is None else len(s.seg_h)), (b, ns)
            if ns:
                assert np.array_equal(got["seg_xold"][:ns, b], s.seg_xold) and np.array_equal(got["seg_h"][:ns, b], s.seg_h)
                assert np.array_equal(got["seg_cont"][:ns, :, b], s.seg_cont, equal_nan=True), b
        if events:
            for i in range(len(s.t_events)):
                m = int(got["n_ev"][i, b])
                assert m == len(s.t_events[i]), (b, i, m)
                assert np.array_equal(got["t_events"][i, :m, b], s.t_events[i])
                assert np.array_equal(got["y_events"][i, :m, :, b], s.y_events[i]), (b, i)
    assert {OK, MAXSTEPS, TOOSMALL} <= seen, seen


def sho_solutions(method, idx, **kw):
    y0, t1, o = sho_out_options(method)
    rhs = "sho_ev" if "event_direction" in kw else "sho"
    return [O.solve_ivp(rhs, 0.0, float(t1[b]), y0[:, b], detpow=True, **o, **kw) for b in idx]


@pytest.mark.parametrize("method", ["DOPRI5", "DOP853", "BDF"])
def test_bounded_outputs_of_failing_lanes_in_the_host_emulation(method):
    y0, t1, o = sho_out_options(method)
    g = emul_batch("sho", y0, None, 0.0, t1, chunk=7, t_eval=T_EVAL, **o)
    assert ("def_rec" in g) == (method == "DOP853")          # DOP853: the deferred sampling bodies took the samples
    check_bounded_outputs(g, sho_solutions(method, OUT_IDX, t_eval=T_EVAL), OUT_IDX, t_eval=T_EVAL)
    g = emul_batch("sho", y0, None, 0.0, t1, chunk=7, max_log=1300, dense_output=True, **o)
    check_bounded_outputs(g, sho_solutions(method, OUT_IDX, dense_output=True), OUT_IDX, dense=True)
    ev = dict(event_direction=[0], event_terminal=[0])
    g = emul_batch("sho_ev", y0, None, 0.0, t1, chunk=7, max_log=1300, max_events=16, **ev, **o)
    sols = sho_solutions(method, OUT_IDX, **ev)
    assert ("evd_rec" in g) == (method != "BDF")             # explicit methods, no terminal event: deferred root refinement
    check_bounded_outputs(g, sols, OUT_IDX, events=True)
    assert max(len(s.t_events[0]) for s in sols) >= 3 and len(sols[0].t_events[0]) == 0
