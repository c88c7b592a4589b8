"""The Radau IIA(5) kernel bodies (radau_init_body / radau_chunk_body / radau_attempt of ivp_amd/csrc/radau_core.h), run on
the CPU by tests/host_emul with the GPU launch loop's init -> chunk -> chunk schedule, against the CPU model
tests/radau_model.py, BIT FOR BIT: status, t_end, h_next, y_end and the six counters of every trajectory and every recorded
output, with the same() rule of tests/test_gpu_radau.py (NaN equals NaN, signed zeros distinguished).  No tolerance anywhere.

Every test that claims a branch asserts on the MODEL's counters that the input takes it.  The degenerate and NaN intervals
have no model: they are solve_ivp's own early return, and are held to what the emulator gives for DOPRI5 on the same input
(that path is pinned to the oracle by tests/test_differential_random_cpu.py and tests/test_failure_paths_cpu.py)."""
import math
import time

import numpy as np
import pytest

from tests import radau_model as M
from tests.host_emul import emul as E

UNBOUNDED = 0xFFFFFFFF
COUNTERS = ("nfev", "njev", "nlu", "nstep", "naccpt", "nrejct")
RT, AT = 1e-6, 1e-8
CR3BP_MU = 0.012277471
CR3BP_Y0 = [0.994, 0.0, 0.0, 0.0, -2.0015851063790825, 0.0]


def same(a, b):
    a, b = float(a), float(b)
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def same_vec(a, b):
    return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))


def lin_matrix(n):
    """The dense test matrix of tests/test_gpu_radau.py's 8 x 8 system at width n: a negative diagonal, 200 below it in every
    odd row (a one-way coupling inside each pair: once U1 / h + 1 < 200 it is the pivot of its column in E1 and in E2),
    entries of 1e-3 .. 7e-3 everywhere else."""
    a = [[1e-3 * (1 + ((3 * i + 5 * j) % 7)) for j in range(n)] for i in range(n)]
    for i in range(n):
        a[i][i] = -1.0 - 0.25 * i
        if i % 2:
            a[i][i - 1] = 200.0
    return a


def problem(name, par=None):
    """-> (emulator rhs name, parameter column or None, model f, model jac or None)"""
    if name == "decay":
        return "decay", [par], M.rhs_decay(par), None
    if name == "sho":
        return "sho", None, M.rhs_sho, None
    if name == "vdp":
        return "vdp", [par], M.rhs_vdp(par), None
    if name == "vdp_eps":
        return "vdp_eps", [par], M.rhs_vdp_eps(par), None
    if name == "lorenz":
        return "lorenz", list(par), M.rhs_lorenz(*par), None
    if name == "robertson":
        return "robertson", None, M.rhs_robertson, None
    if name == "robertson_jac":
        return "robertson_jac", None, M.rhs_robertson, M.jac_robertson
    if name == "cr3bp":
        return "cr3bp", [CR3BP_MU], M.rhs_cr3bp(CR3BP_MU), None
    if name.startswith("lin"):   # "lin4", "lin4_jac": par is the matrix
        flat = [v for row in par for v in row]
        return name, flat, M.rhs_dense_linear(par), (M.jac_dense_linear(par) if name.endswith("_jac") else None)
    raise KeyError(name)


def run_emul(name, pars, y0s, t0, t1, chunk, rtol=RT, atol=AT, radau=None, **kw):
    """One emulator batch: trajectory b has parameters pars[b] (problem()'s `par`) and initial state y0s[b]."""
    cols = [problem(name, p)[1] for p in pars]
    rhs = problem(name, pars[0])[0]
    params = None if cols[0] is None else np.array(cols, dtype=np.float64).T.copy()
    y0 = np.array(y0s, dtype=np.float64).T.copy()
    return E.solve_batch(rhs, y0, params, t0, t1, method="RADAU", rtol=rtol, atol=atol, chunk=chunk, radau=radau, **kw)


def run_model(name, par, y0, t0, t1, rtol=RT, atol=AT, radau=None, **kw):
    _, _, f, jac = problem(name, par)
    return M.solve(f, t0, t1, list(y0), rtol, atol, settings=M.Settings(**(radau or {})), jac=jac, **kw)


def check_end(res, b, m, tag):
    got = dict(status=int(res["status"][b]), **{k: int(res[k][b]) for k in COUNTERS})
    want = dict(status=m.status, **{k: getattr(m, k) for k in COUNTERS})
    assert got == want, (tag, got, want)
    assert same(res["t_end"][b], m.t_end), (tag, "t_end", float(res["t_end"][b]), m.t_end)
    assert same(res["h_next"][b], m.h_next), (tag, "h_next", float(res["h_next"][b]), m.h_next)
    assert same_vec(res["y_end"][:, b], m.y_end), (tag, "y_end", list(res["y_end"][:, b]), m.y_end)


def check_outputs(res, b, m, tag, t_eval=False, log=0, dense=False):
    if t_eval:
        k = int(res["n_filled"][b])
        assert k == len(m.t) and [int(v) for v in res["eval_idx"][:k, b]] == m.eval_idx, (tag, k, len(m.t))
        for q in range(k):
            assert same_vec(res["y_eval"][q, :, b], m.y[q]), (tag, "t_eval sample", q)
    if log:
        assert int(res["n_log"][b]) == len(m.t), (tag, int(res["n_log"][b]), len(m.t))   # the count runs on past the capacity
        for q in range(min(log, len(m.t))):
            assert same(res["t_log"][q, b], m.t[q]) and same_vec(res["y_log"][q, :, b], m.y[q]), (tag, "log record", q)
    if dense:
        assert int(res["n_seg"][b]) == len(m.segs) == m.naccpt, (tag, int(res["n_seg"][b]), len(m.segs))
        for q, (cont, xold, h) in enumerate(m.segs[:log]):
            assert same(res["seg_xold"][q, b], xold) and same(res["seg_h"][q, b], h) and same_vec(res["seg_cont"][q, :, b], cont), (tag, "segment", q)


def both(name, pars, y0s, t0, t1, chunks=(1, 7, UNBOUNDED), rtol=RT, atol=AT, radau=None, t_eval=None, max_log=0, dense_output=False, **kw):
    """Models once, the emulator at every chunk length; returns the models."""
    mkw = dict(kw)
    if t_eval is not None:
        mkw["t_eval"] = list(t_eval)
    if dense_output:
        mkw["dense_output"] = True
    models = [run_model(name, p, y, t0, t1, rtol, atol, radau, **mkw) for p, y in zip(pars, y0s)]
    for chunk in chunks:
        res = run_emul(name, pars, y0s, t0, t1, chunk, rtol, atol, radau, t_eval=t_eval, max_log=max_log, dense_output=dense_output, **kw)
        for b, m in enumerate(models):
            tag = f"{name} trajectory {b} chunk {chunk}"
            check_end(res, b, m, tag)
            check_outputs(res, b, m, tag, t_eval is not None, max_log if t_eval is None else 0, dense_output)
    return models


def vdp_eps_batch(B, seed=2024):
    rng = np.random.default_rng(seed)
    eps = np.exp(rng.uniform(np.log(5e-4), np.log(2e-3), 67))
    y0 = np.stack([2.0 + 0.1 * rng.standard_normal(67), 0.1 * rng.standard_normal(67)])
    return [float(v) for v in eps[:B]], [[float(v) for v in y0[:, b]] for b in range(B)]


# ---- 1. the random differential sweep -----------------------------------------------------------------------------------

N_RANDOM = 1600   # about half a minute; the count is printed
NAMES = ["decay", "sho", "vdp", "vdp_eps", "lorenz", "robertson", "robertson_jac", "cr3bp",
         "lin4", "lin4_jac", "lin5", "lin5_jac", "lin7", "lin7_jac", "lin8", "lin8_jac"]
SMALL_PRIMES = [2, 3, 5, 7, 11, 13]


def random_case(seed):
    """Every draw is a valid input: nothing is filtered afterwards.  Integrating a stiff problem backwards follows its
    fastest growing mode, so those spans are short, and every case carries a max_steps (1500, or in a tenth of the cases a
    small one that ends the run in NeedLargerNMax) as part of its input."""
    r = np.random.default_rng(90_000 + seed)
    name = NAMES[seed % len(NAMES)]   # every problem comes up
    backward = bool(r.random() < 0.4)
    B = 1 + int(r.integers(0, 2))
    par, span, y0f = None, 1.0, None
    if name == "decay":
        par, span, y0f = float(r.uniform(0.1, 30.0)), float(r.uniform(0.2, 2.0)), lambda: r.uniform(0.5, 2.0, 1)
    elif name == "sho":
        span, y0f = float(r.uniform(0.5, 6.0)), lambda: r.standard_normal(2)
    elif name == "vdp":
        par, span, y0f = float(r.uniform(0.5, 3.0)), float(r.uniform(0.5, 1.5 if backward else 5.0)), lambda: r.uniform(-2.0, 2.0, 2)
    elif name == "vdp_eps":
        par = float(np.exp(r.uniform(np.log(5e-4), np.log(2e-2))))
        span = float(r.uniform(2.0, 20.0)) * par if backward else float(r.uniform(0.3, 2.0))
        y0f = lambda: np.array([2.0, 0.0]) + 0.1 * r.standard_normal(2)
    elif name == "lorenz":
        par, span = (10.0, 28.0 * float(r.uniform(0.8, 1.1)), 8.0 / 3.0), float(r.uniform(0.1, 0.4 if backward else 1.0))
        y0f = lambda: 1.0 + r.standard_normal(3)
    elif name.startswith("robertson"):
        span = 1e-4 * float(r.uniform(0.5, 5.0)) if backward else float(10.0 ** r.uniform(0.0, 4.0))
        y0f = lambda: np.array([1.0, 0.0, 0.0]) + np.array([0.0, 1e-5, 1e-2]) * r.uniform(0.0, 1.0, 3)
    elif name == "cr3bp":
        span, y0f = float(r.uniform(0.1, 0.5)), lambda: np.array(CR3BP_Y0) + 1e-3 * r.standard_normal(6)
    else:
        n = int(name[3])
        par, span, y0f = lin_matrix(n), float(r.uniform(0.5, 3.0)), lambda: r.uniform(-2.0, 2.0, n)
    t0 = float(r.uniform(-1.0, 1.0)) if name in ("sho", "decay") else 0.0
    t1 = t0 - span if backward else t0 + span
    y0s = [[float(v) for v in y0f()] for _ in range(B)]
    e = float(r.uniform(3.0, 9.0))
    rtol = float(10.0 ** -e)
    atol = float(rtol * 10.0 ** -r.uniform(0.0, 3.0))
    kw = dict(max_steps=1500 if r.random() < 0.9 else int(r.integers(1, 60)))
    if r.random() < 0.4:
        kw["first_step"] = float(span * 10.0 ** r.uniform(-4.0, -0.7))
    radau = dict(newton_maxiter=int(r.integers(2, 16)), predictive=bool(r.random() < 0.5))
    out = int(r.integers(0, 4))   # end state, t_eval, step log, step log + dense segments
    if out == 1:
        te = np.sort(r.uniform(min(t0, t1) - 0.1 * span, max(t0, t1) + 0.1 * span, int(r.integers(1, 9))))
        te = np.concatenate([[min(t0, t1)], te, [max(t0, t1)]])
        kw["t_eval"] = [float(v) for v in (te[::-1] if backward else te)]
    elif out >= 2:
        kw["max_log"] = int(r.integers(3, 40))
        kw["dense_output"] = out == 3
    chunks = (1, int(SMALL_PRIMES[r.integers(len(SMALL_PRIMES))]), UNBOUNDED)
    return dict(name=name, pars=[par] * B, y0s=y0s, t0=t0, t1=t1, chunks=chunks, rtol=rtol, atol=atol, radau=radau, **kw)


def test_random_differential_sweep():
    t = time.time()
    stats = dict(status={}, restarts=0, dyth=0, reuse=0, rejected=0, trajectories=0, backward=0)
    for seed in range(N_RANDOM):
        c = random_case(seed)
        for m in both(**c):
            stats["status"][m.status] = stats["status"].get(m.status, 0) + 1
            stats["restarts"] += m.n_restart
            stats["dyth"] += m.n_dyth
            stats["reuse"] += m.n_reuse
            stats["rejected"] += m.nrejct
            stats["trajectories"] += 1
            stats["backward"] += c["t1"] < c["t0"]
    print(f"random sweep: {N_RANDOM} cases x 3 chunk lengths, {stats['trajectories']} trajectories each, {time.time() - t:.1f} s; {stats}")
    assert len({random_case(s)["name"] for s in range(N_RANDOM)}) == len(NAMES)
    # the sweep is not all easy sailing: it holds Newton restarts, dyth exits, reused factors, rejections and both directions
    assert stats["status"].get(M.NEED_LARGER_NMAX, 0) > 0 and stats["status"].get(M.SUCCESS, 0) > N_RANDOM // 2
    assert stats["restarts"] > 0 and stats["dyth"] > 0 and stats["reuse"] > 0 and stats["rejected"] > 0 and stats["backward"] > 0


# ---- 2. restarts --------------------------------------------------------------------------------------------------------

def test_newton_maxiter_1_ends_in_singular_matrix_after_exactly_5_restarts():
    eps, y0s = vdp_eps_batch(3)
    models = both("vdp_eps", eps, y0s, 0.0, 2.0, radau=dict(newton_maxiter=1))
    for m in models:
        assert m.status == M.SINGULAR_MATRIX == 5 and m.n_restart == 5 and m.n_restart_newton == 6 and m.naccpt == 0
        assert m.n_restart_real == m.n_restart_complex == m.n_restart_theta == 0
        assert m.h_next == 1e-6 * 0.5 ** 5


def test_newton_maxiter_2_restarts_hundreds_of_times_across_launch_boundaries():
    """At chunk length 1 every restart is followed by a launch boundary, so h, reject, call_decomp and singular_count (flag
    bits 8..10) cross it hundreds of times.  The solve succeeds only because the count is reset by every accepted step: a
    count that is not reset ends in SingularMatrix after the fifth restart.  (A count that is LOST at a boundary shows in the
    newton_maxiter = 1 test above, whose fifth restart must still end the solve at chunk length 1.)"""
    eps, y0s = vdp_eps_batch(2)
    models = both("vdp_eps", eps, y0s, 0.0, 2.0, chunks=(1, 3, UNBOUNDED), radau=dict(newton_maxiter=2))
    for m in models:
        print("newton_maxiter = 2:", m.status, m.n_restart, m.nstep, m.naccpt)
        assert m.n_restart_newton > 100 and m.n_restart_newton == m.n_restart + (m.status == M.SINGULAR_MATRIX)
        assert m.naccpt > 0


def test_real_zero_pivot_on_the_first_factorisation():
    """y' = k y with k = U1 / first_step, computed in double: E1 = U1 / h - J is exactly zero.  The Jacobian is the forward
    difference (f(y + d) - f(y)) / d with d = 2^-26 max(|y|, 1): for y0 in {0, 2^-26, -2^-27} both products are exact, so
    J == k to the bit."""
    h = 0.01
    k = M.U1 / h
    y0s = [[0.0], [2.0 ** -26], [-(2.0 ** -27)]]
    models = both("decay", [-k] * 3, y0s, 0.0, 0.05, first_step=h)   # RhsDecay is y' = -p y
    for m in models:
        assert m.n_restart_real == 1 and m.n_restart == 1 and m.n_restart_complex == m.n_restart_newton == 0
        assert m.status == M.SUCCESS and m.h_tried[0] == 0.5 * h


def test_complex_zero_pivot_on_the_first_factorisation():
    """The rotation J = [[a, -b], [b, a]] with a = ALPH / h, b = BETA / h: E2 = [[i b, b], [-b, i b]], whose second pivot is
    i b - b (1 / (i b)) b = 0 when b (1 / b^2) b rounds to 1; h = 2^-6 is a step for which it does (asserted)."""
    h = 2.0 ** -6
    a, b = M.ALPH / h, M.BETA / h
    J = [[a, -b], [b, a]]
    models = both("lin2_jac", [J, J], [[1.0, 0.0], [0.3, -0.7]], 0.0, 4.0 * h, first_step=h)
    for m in models:
        assert m.n_restart_complex == 1 and m.n_restart == 1 and m.n_restart_real == m.n_restart_newton == 0
        assert m.h_tried[0] == 0.5 * h


def test_purely_imaginary_multiplier_in_the_complex_elimination():
    h = 2.0 ** -10
    J = [[0.0, 1.0], [-1e5, M.ALPH / h]]
    models = both("lin2_jac", [J, J], [[1.0, 0.0], [0.5, 0.25]], 0.0, 8.0 * h, first_step=h)
    for m in models:
        assert "imag" in m.cases, m.cases
        assert ("complex", 0, 1) in m.pivots


# ---- 3. step bounds -----------------------------------------------------------------------------------------------------

def test_max_step_bounds_every_logged_step():
    hmax = 0.02
    free = run_model("sho", None, [1.0, 0.0], 0.0, 1.0)
    assert max(abs(b - a) for a, b in zip(free.t, free.t[1:])) > 2 * hmax   # unbounded, the steps grow past it
    models = both("sho", [None, None], [[1.0, 0.0], [0.3, -0.7]], 0.0, 1.0, max_step=hmax, max_log=80)
    for m in models:
        steps = [abs(b - a) for a, b in zip(m.t, m.t[1:])]
        assert len(m.t) <= 80 and max(steps) <= hmax * (1 + 1e-12) and sum(s > 0.99 * hmax for s in steps) > 20
        assert max(abs(v) for v in m.h_tried) == hmax


def test_min_step_with_max_step_on_stiff_van_der_pol():
    eps, y0s = vdp_eps_batch(2)
    free = [run_model("vdp_eps", e, y, 0.0, 2.0) for e, y in zip(eps, y0s)]
    models = both("vdp_eps", eps, y0s, 0.0, 2.0, min_step=1e-3, max_step=0.02)
    for m, f in zip(models, free):
        assert min(f.h_tried) < 1e-3 and max(f.h_tried) > 0.02          # both clamps bind on this problem
        assert m.h_tried.count(1e-3) > 0 and m.h_tried.count(0.02) > 0
        assert (m.nstep, m.t_end, m.y_end) != (f.nstep, f.t_end, f.y_end)


def test_first_step_larger_than_max_step_is_clamped():
    for t1, sign in ((1.0, 1.0), (-1.0, -1.0)):
        models = both("sho", [None], [[1.0, 0.0]], 0.0, t1, first_step=0.5, max_step=0.01)
        assert models[0].h_tried[0] == sign * 0.01 and models[0].status == M.SUCCESS


# ---- 4. per-component tolerances ------------------------------------------------------------------------------------------

def test_vector_tolerances_and_the_same_vectors_reversed():
    """newton_tol derives from rtol[0] alone and scal[i] from (rtol[i], atol[i]): a kernel that read the vectors in another
    order would give the reversed run's results."""
    rt, at = [1e-4, 1e-7, 1e-5], [1e-6, 1e-11, 1e-8]
    y0 = [[1.0, 0.0, 0.0]]
    fwd = both("robertson", [None], y0, 0.0, 1e3, rtol=rt, atol=at)[0]
    rev = both("robertson", [None], y0, 0.0, 1e3, rtol=rt[::-1], atol=at[::-1])[0]
    scalar = run_model("robertson", None, y0[0], 0.0, 1e3, rt[0], at[0])
    assert fwd.status == rev.status == M.SUCCESS
    assert (fwd.nstep, fwd.nfev, fwd.y_end) != (rev.nstep, rev.nfev, rev.y_end)
    assert (fwd.nstep, fwd.nfev, fwd.y_end) != (scalar.nstep, scalar.nfev, scalar.y_end)
    both("robertson_jac", [None], y0, 0.0, 1e3, rtol=rt, atol=at)


# ---- 5. outputs at N = 1, 4 and 8 ---------------------------------------------------------------------------------------

OUT_PROBLEMS = [("decay", [0.5, 300.0], [[1.0], [2.0]], 3.0),
                ("lin4", [lin_matrix(4)] * 2, [[1.0, 0.5, -0.5, 0.25], [0.1, -1.0, 2.0, 0.0]], 3.0),
                ("lin8_jac", [lin_matrix(8)] * 2, [[1.0, 0.5, -0.5, 0.25, 0.0, 1e-3, -1.0, 2.0], [0.5] * 8], 3.0)]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["n1", "n4", "n8"])
def test_t_eval_log_and_dense_segments(which):
    """At N = 8 a dense segment is 32 doubles per trajectory, the widest indexing of seg_cont."""
    name, pars, y0s, t1 = OUT_PROBLEMS[which]
    grid = [0.0, 0.1, 0.1 + 1e-13, 0.7, 1.5, t1, t1 + 0.5]
    models = both(name, pars, y0s, 0.0, t1, chunks=(1, 5, UNBOUNDED), t_eval=grid)
    assert all(len(m.t) == 6 for m in models)
    models = both(name, pars, y0s, 0.0, t1, chunks=(1, 5, UNBOUNDED), max_log=12)
    assert any(len(m.t) > 12 for m in models)                                  # the log overflows, the count runs on
    nseg = max(len(m.t) for m in models) + 1
    models = both(name, pars, y0s, 0.0, t1, chunks=(1, 5, UNBOUNDED), max_log=nseg, dense_output=True)
    assert all(len(m.segs) == m.naccpt > 3 for m in models)
    if name.startswith("lin"):
        assert all(any(p[0] == "real" for p in m.pivots) and any(p[0] == "complex" for p in m.pivots) for m in models)


# ---- 6. every state width on the host -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lin4", "lin4_jac", "lin5", "lin5_jac", "lin7", "lin7_jac", "lin8", "lin8_jac"])
def test_state_widths_4_5_7_8_exchange_rows_in_both_factorisations(name):
    n = int(name[3])
    y0 = [1.0, 0.5, -0.5, 0.25, 0.0, 1e-3, -1.0, 2.0][:n]
    models = both(name, [lin_matrix(n)] * 2, [y0, [v + 1e-3 * (i + 1) for i, v in enumerate(y0)]], 0.0, 5.0, rtol=1e-4, atol=1e-6)
    for m in models:
        assert m.status == M.SUCCESS
        assert any(p[0] == "real" for p in m.pivots) and any(p[0] == "complex" for p in m.pivots)


# ---- 7. degenerate and NaN intervals ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, pars, y0s", [("decay", [0.5, 2.0], [[1.0], [2.0]]), ("sho", [None, None], [[1.0, 0.0], [0.3, -0.7]]),
                                             ("lin8", [lin_matrix(8)] * 2, [[1.0] * 8, [0.5] * 8])], ids=["n1", "n2", "n8"])
@pytest.mark.parametrize("kind", ["equal", "1e-16", "nan"])
@pytest.mark.parametrize("out", ["end", "t_eval", "log", "dense"])
def test_degenerate_and_nan_intervals_are_the_early_return_of_solve_ivp(name, pars, y0s, kind, out):
    t0 = 0.25
    t1 = {"equal": t0, "1e-16": t0 + 1e-16, "nan": float("nan")}[kind]
    assert kind != "1e-16" or (t1 != t0 and abs(t1 - t0) < 1e-15)
    kw = {"end": {}, "t_eval": dict(t_eval=[t0 - 1.0, t0 - 5e-13, t0, t0 + 5e-13, t0 + 2e-12, t0 + 1.0]), "log": dict(max_log=4),
          "dense": dict(max_log=4, dense_output=True)}[out]
    cols = [problem(name, p)[1] for p in pars]
    rhs = problem(name, pars[0])[0]
    params = None if cols[0] is None else np.array(cols, dtype=np.float64).T.copy()
    y0 = np.array(y0s, dtype=np.float64).T.copy()
    n = y0.shape[0]
    ref = E.solve_batch(rhs, y0, params, t0, t1, method="DOPRI5", rtol=RT, atol=AT, chunk=64, **kw)
    for chunk in (1, UNBOUNDED):
        got = E.solve_batch(rhs, y0, params, t0, t1, method="RADAU", rtol=RT, atol=AT, chunk=chunk, **kw)
        assert got["chunks"] == 0                                  # retired by the init body: no attempt runs
        for b in range(2):
            assert int(got["status"][b]) == int(ref["status"][b]) == (3 if kind == "nan" else 0)
            assert same(got["h_next"][b], 0.0) and same(got["h_next"][b], ref["h_next"][b])
            assert same(got["t_end"][b], ref["t_end"][b]) and same_vec(got["y_end"][:, b], ref["y_end"][:, b])
            assert same_vec(got["y_end"][:, b], y0[:, b])
            for k in COUNTERS:
                assert int(got[k][b]) == int(ref[k][b]) == 0, k
            if out == "end":
                continue
            for k in ("n_filled", "n_log", "n_seg"):
                assert int(got[k][b]) == int(ref[k][b]), (k, int(got[k][b]), int(ref[k][b]))
            if out == "t_eval":
                k = int(got["n_filled"][b])
                assert k == (0 if kind == "nan" else 3)             # the grid points within 1e-12 of t0
                assert list(got["eval_idx"][:k, b]) == list(ref["eval_idx"][:k, b])
                for q in range(k):
                    assert same_vec(got["y_eval"][q, :, b], ref["y_eval"][q, :, b])
            else:
                k = int(got["n_log"][b])
                assert k == (0 if kind == "nan" else 1)
                for q in range(k):
                    assert same(got["t_log"][q, b], ref["t_log"][q, b]) and same_vec(got["y_log"][q, :, b], ref["y_log"][q, :, b])
            if out == "dense":
                k = int(got["n_seg"][b])
                assert k == (0 if kind == "nan" else 1)
                for q in range(k):   # ContinuousOutput::constant: [y, 0, 0, ..]; DOPRI5 carries 5 n coefficients, Radau 4 n
                    assert same(got["seg_xold"][q, b], ref["seg_xold"][q, b]) and same(got["seg_h"][q, b], ref["seg_h"][q, b])
                    assert same_vec(got["seg_cont"][q, :, b], ref["seg_cont"][q, :4 * n, b])
                    assert same_vec(ref["seg_cont"][q, 4 * n:, b], [0.0] * n)


def test_event_problems_are_rejected_as_the_host_rejects_them():
    with pytest.raises(AssertionError):
        E.solve_batch("sho_ev", np.array([[1.0], [0.0]]), None, 0.0, 1.0, method="RADAU", event_direction=[0], event_terminal=[0])


# ---- 8. the three linear-algebra functions on their own (the host twin of tests/test_gpu_radau_lu_probe.py) ----------------

@pytest.mark.parametrize("n", range(1, 9))
def test_lu_and_solves_on_chosen_matrices_equal_the_model(n):
    from tests import radau_lu_cases as L
    L.assert_equal_to_model(n, E.radau_lu(n, L.reference(n)))
