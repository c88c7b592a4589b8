"""`jac_sparsity` on the GPU: grouped forward differences (BdfG::fd_jac_sparse) against the dense differences and the oracle.

The claim under test (include/ivp_hip.h): a declared pattern that contains every structurally
non-zero entry of dF/dy gives the dense path's Jacobian bit for bit, so the WHOLE solve -- end state, end time, next
step, status, all six counters, t_eval samples, step log, dense segments -- equals the solve without a pattern and the
oracle's, in strict mode (oracle with detpow) and in FMA mode (the FMA oracle).  The systems are nonlinear, so the
Jacobian is re-evaluated along the way; `chunk_attempts = 7` makes J and the factors cross launch boundaries.

The right-hand sides exist twice, as device code and as numpy code with the same operations in the same order (the
user's code is compiled without contraction in both arithmetic modes, so one Python restatement serves both)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 11
RTOL, ATOL = 1e-5, 1e-8


# ---- the systems ----------------------------------------------------------------------------------------------------
def band_system(n, w):
    """y_i' = k sum_{d=1..w} 2^-d (y_{i-d} - 2 y_i + y_{i+d}) - a y_i^3, zero outside: true pattern |i - j| <= w."""
    src = f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{{
    double s = 0.0;
    for (int d = 1; d <= {w}; ++d) {{
        const double ym = i - d >= 0 ? y[i - d] : 0.0, yp = i + d < {n} ? y[i + d] : 0.0;
        s += (1.0 / (double)(1 << d)) * ((ym - 2.0 * y[i]) + yp);
    }}
    return p[0] * s - p[1] * ((y[i] * y[i]) * y[i]);
}}
"""

    def fun(t, y, p):
        y = np.asarray(y, dtype=np.float64)
        z = np.concatenate((np.zeros(w), y, np.zeros(w)))
        s = np.zeros(n)
        for d in range(1, w + 1):
            s = s + (1.0 / (1 << d)) * ((z[w - d:w - d + n] - 2.0 * y) + z[w + d:w + d + n])
        return p[0] * s - p[1] * ((y * y) * y)

    return src, fun


def band_pattern(n, w):
    i, j = np.indices((n, n))
    return (np.abs(i - j) <= w).astype(np.int8)


def laplace_system(m):
    """5-point Laplacian on an m x m grid (row-major), zero boundary, minus a y^3: not banded in the first-fit sense."""
    n = m * m
    src = f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{{
    const int r = i / {m}, c = i % {m};
    const double up = r > 0 ? y[i - {m}] : 0.0, dn = r < {m - 1} ? y[i + {m}] : 0.0;
    const double lf = c > 0 ? y[i - 1] : 0.0, rt = c < {m - 1} ? y[i + 1] : 0.0;
    return p[0] * ((((up + dn) + lf) + rt) - 4.0 * y[i]) - p[1] * ((y[i] * y[i]) * y[i]);
}}
"""

    def fun(t, y, p):
        y = np.asarray(y, dtype=np.float64)
        g = np.zeros((m + 2, m + 2))
        g[1:-1, 1:-1] = y.reshape(m, m)
        lap = (((g[:-2, 1:-1] + g[2:, 1:-1]) + g[1:-1, :-2]) + g[1:-1, 2:]) - 4.0 * g[1:-1, 1:-1]
        return p[0] * lap.reshape(n) - p[1] * ((y * y) * y)

    pat = np.zeros((n, n), dtype=np.int8)
    for i in range(n):
        r, c = divmod(i, m)
        pat[i, i] = 1
        for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
            if 0 <= rr < m and 0 <= cc < m:
                pat[i, rr * m + cc] = 1
    return src, fun, pat


def arrow_system(n):
    """y_0' = -k y_0 + (k / n) sum_{j >= 1} y_j y_j;  y_i' = k (y_0 - (1 + i / n) y_i) - a y_i^3: dense row 0, dense column 0."""
    src = f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{{
    if (i == 0) {{
        double s = 0.0;
        for (int j = 1; j < {n}; ++j) s += y[j] * y[j];
        return (p[0] * {1.0 / n!r}) * s - p[0] * y[0];
    }}
    return p[0] * (y[0] - (1.0 + (double)i * {1.0 / n!r}) * y[i]) - p[1] * ((y[i] * y[i]) * y[i]);
}}
"""

    def fun(t, y, p):
        y = np.asarray(y, dtype=np.float64)
        s = 0.0
        for j in range(1, n):
            s += float(y[j]) * float(y[j])
        out = p[0] * (y[0] - (1.0 + np.arange(n) * (1.0 / n)) * y) - p[1] * ((y * y) * y)
        out[0] = (p[0] * (1.0 / n)) * s - p[0] * y[0]
        return out

    pat = np.eye(n, dtype=np.int8)
    pat[0, :] = 1
    pat[:, 0] = 1
    return src, fun, pat


def batch_inputs(n, seed):
    rng = np.random.default_rng(seed)
    y0 = 0.5 + rng.uniform(size=(n, B))
    params = np.stack([40.0 * (1.0 + 4.0 * rng.uniform(size=B)), 5.0 + 20.0 * rng.uniform(size=B)])   # k, a per trajectory
    t1 = 0.02 + 0.05 * rng.uniform(size=B)                                                              # ragged ends
    return y0, params, t1


CASES = {
    "tri12": lambda: (*band_system(12, 1), band_pattern(12, 1), 12, 3),        # G = 16, four trajectories per wave
    "tri24": lambda: (*band_system(24, 1), band_pattern(24, 1), 24, 3),        # G = 32
    "tri40": lambda: (*band_system(40, 1), band_pattern(40, 1), 40, 3),        # a whole wave
    "tri65": lambda: (*band_system(65, 1), band_pattern(65, 1), 65, 3),        # two components in one lane, ragged last chunk
    "tri130": lambda: (*band_system(130, 1), band_pattern(130, 1), 130, 3),
    "band4_40": lambda: (*band_system(40, 4), band_pattern(40, 4), 40, 9),     # 9 groups: one more than a sweep holds
    "band8_100": lambda: (*band_system(100, 8), band_pattern(100, 8), 100, 17),
    "laplace5x5": lambda: (*laplace_system(5), 25, None),                      # non-banded, non-trivial first-fit
    "arrow20": lambda: (*arrow_system(20), 20, 20),                            # n groups
    "full20": lambda: (*band_system(20, 1), np.ones((20, 20), dtype=np.int8), 20, 20),   # the dense work with the sparse code
    "tri24_as_penta": lambda: (*band_system(24, 1), band_pattern(24, 2), 24, 5),         # strict superset of the true pattern
}

_ORACLE = {}   # (case, fma) -> per-trajectory oracle solutions, computed once


def oracle_solutions(case, fun, y0, params, t1, te, fma):
    from oracle import oracle as O
    key = (case, fma)
    if key not in _ORACLE:
        mode = dict(fma=True) if fma else dict(detpow=True)
        sols = []
        for b in range(B):
            common = dict(params=list(params[:, b]), method="BDF", rtol=RTOL, atol=ATOL, **mode)
            sols.append((O.solve_ivp(fun, 0.0, float(t1[b]), list(y0[:, b]), dense_output=True, **common),
                         O.solve_ivp(fun, 0.0, float(t1[b]), list(y0[:, b]), t_eval=te, **common)))
        _ORACLE[key] = sols
    return _ORACLE[key]


FIELDS = ("y_end", "t_end", "h_next", "status", "nfev", "nstep", "naccpt", "nrejct", "njev", "nlu")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()


def gpu_runs(f, y0, params, t1, te, fma, chunk=7):
    """The two solves that cover every output: one with a t_eval grid, one with the step log and dense segments."""
    import ivp_amd
    mode = ivp_amd.FpMode.FMA if fma else ivp_amd.FpMode.STRICT
    o = dict(method="BDF", rtol=RTOL, atol=ATOL, chunk_attempts=chunk, fp_mode=mode)
    sampled = ivp_amd.solve_ivp_batch(f, 0.0, t1, y0, params, ivp_amd.Options(t_eval=te, **o))
    logged = ivp_amd.solve_ivp_batch(f, 0.0, t1, y0, params, ivp_amd.Options(dense_output=True, max_log=256, **o))
    return sampled, logged


def assert_runs_equal(got, want, what):
    for (g, w), names in zip(zip(got, want), (FIELDS + ("y_eval", "eval_idx", "n_filled"),
                                              FIELDS + ("t_log", "y_log", "n_log", "seg_cont", "seg_xold", "seg_h", "n_seg"))):
        for k in names:
            assert same_bits(np.asarray(getattr(g, k)), np.asarray(getattr(w, k))), f"{what}: {k} differs"


def assert_equals_oracle(got, sols, te, what):
    sampled, logged = got
    for b, (s_log, s_eval) in enumerate(sols):
        for r, s in ((logged, s_log), (sampled, s_eval)):
            tag = f"{what} trajectory {b}"
            assert int(r.status[b]) == int(s.status), tag
            assert (int(r.nfev[b]), int(r.njev[b]), int(r.nlu[b]), int(r.nstep[b]), int(r.naccpt[b]), int(r.nrejct[b])) == \
                   (s.nfev, s.njev, s.nlu, s.nstep, s.naccpt, s.nrejct), tag
            assert same_bits(np.asarray(r.h_next)[b], np.float64(s.h_next)), tag
        assert same_bits(np.asarray(logged.y_end)[:, b], s_log.y[-1]) and same_bits(np.asarray(logged.t_end)[b], s_log.t[-1]), f"{what} {b}: end state"
        m = int(logged.n_log[b])
        assert m == len(s_log.t) and m <= 256, (what, b, m)
        assert same_bits(np.asarray(logged.t_log)[:m, b], s_log.t) and same_bits(np.asarray(logged.y_log)[:m, :, b], s_log.y), f"{what} {b}: step log"
        ns = int(logged.n_seg[b])
        assert ns == len(s_log.seg_h), (what, b, ns)
        assert same_bits(np.asarray(logged.seg_xold)[:ns, b], s_log.seg_xold) and same_bits(np.asarray(logged.seg_h)[:ns, b], s_log.seg_h), f"{what} {b}: segments"
        assert same_bits(np.asarray(logged.seg_cont)[:ns, :, b], s_log.seg_cont), f"{what} {b}: segment coefficients"
        m = int(sampled.n_filled[b])
        assert m == len(s_eval.t), (what, b, m)
        assert same_bits(te[np.asarray(sampled.eval_idx)[:m, b]], s_eval.t) and same_bits(np.asarray(sampled.y_eval)[:m, :, b], s_eval.y), f"{what} {b}: samples"


@pytest.mark.parametrize("fma", [False, True], ids=["strict", "fma"])
@pytest.mark.parametrize("case", list(CASES))
def test_sparse_differences_equal_dense_differences_and_the_oracle(case, fma):
    import ivp_amd
    from ivp_amd import api
    src, fun, pattern, n, want_groups = CASES[case]()
    if want_groups is not None:
        assert api.jac_sparsity_groups(pattern, n)[1] == want_groups
    else:
        assert 3 < api.jac_sparsity_groups(pattern, n)[1] < n
    y0, params, t1 = batch_inputs(n, seed=n + len(case))
    te = np.linspace(0.0, 0.07, 9)
    dense = gpu_runs(ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0)), y0, params, t1, te, fma)
    sparse = gpu_runs(ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=pattern), y0, params, t1, te, fma)
    assert (np.asarray(dense[0].status) == 0).all()
    assert int(np.asarray(dense[0].njev).min()) > 1, "the Jacobian must be re-evaluated for this case to test anything"
    assert_runs_equal(sparse, dense, f"{case}: sparse vs dense")
    assert_equals_oracle(sparse, oracle_solutions(case, fun, y0, params, t1, te, fma), te, f"{case}: sparse vs oracle")
    assert_equals_oracle(dense, oracle_solutions(case, fun, y0, params, t1, te, fma), te, f"{case}: dense vs oracle")


def test_a_given_jac_col_wins_over_the_pattern():
    import ivp_amd
    n = 24
    src, _ = band_system(n, 1)
    src += f"""
__device__ void jac_col(int col, double t, const double* y, double* column, const double* p)
{{
    if (col > 0) column[col - 1] = p[0] * 0.5;
    column[col] = p[0] * 0.5 * -2.0 - p[1] * 3.0 * y[col] * y[col];
    if (col + 1 < {n}) column[col + 1] = p[0] * 0.5;
}}
"""
    y0, params, t1 = batch_inputs(n, seed=5)
    te = np.linspace(0.0, 0.07, 9)
    own = gpu_runs(ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac=True), y0, params, t1, te, False)
    # a pattern that would give a DIFFERENT matrix if it were used: diagonal only
    both = gpu_runs(ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac=True, jac_sparsity=np.eye(n)), y0, params, t1, te, False)
    assert (np.asarray(own[0].status) == 0).all()
    assert_runs_equal(both, own, "jac_col with and without a pattern")


def test_under_declared_pattern_is_deterministic_and_still_converges():
    """Tridiagonal system declared diagonal: one group, every column perturbed at once, so the differences alias (the
    diagonal absorbs the neighbours' contributions).  No equality with the dense path is claimed: the Newton matrix is
    approximate.  What must hold: the solve does not depend on how it is cut into launches, and since BDF accepts a step
    only after its Newton iteration converged on the TRUE right-hand side, the end state is within the requested
    tolerance of a DOP853 solve at rtol 1e-12 of the same system.

    The horizon: a step-size controller bounds the LOCAL error per step by the tolerance; the end state is within the
    tolerance where earlier local errors have been damped away, i.e. for a dissipative system past its transient.  The
    slowest mode of k * tridiag(1/2, -1, 1/2) decays at k (1 - cos(pi / (n + 1))) (the cubic term only adds damping), so
    every trajectory runs for three time constants of that mode, t1 = 3 / (k (1 - cos(pi / (n + 1)))): ragged, 2-8 time
    units.  (On the first 2-7 % of that horizon, still inside the transient, dense-Jacobian BDF and the under-declared
    solve both sit at 2.1-2.2 x the bound against the same reference.)"""
    import ivp_amd
    n = 24
    src, _ = band_system(n, 1)
    y0, params, _ = batch_inputs(n, seed=9)
    t1 = 3.0 / (params[0] * (1.0 - np.cos(np.pi / (n + 1))))
    rtol, atol = 1e-4, 1e-7
    f = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=np.eye(n))
    runs = [ivp_amd.solve_ivp_batch(f, 0.0, t1, y0, params, ivp_amd.Options(method="BDF", rtol=rtol, atol=atol, chunk_attempts=c))
            for c in (3, 7, 0)]
    assert (np.asarray(runs[0].status) == 0).all()
    for r in runs[1:]:
        for k in FIELDS:
            assert same_bits(np.asarray(getattr(r, k)), np.asarray(getattr(runs[0], k))), k
    ref = ivp_amd.solve_ivp_batch(ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0)), 0.0, t1, y0, params,
                                  ivp_amd.Options(method="DOP853", rtol=1e-12, atol=1e-14))
    assert (np.asarray(ref.status) == 0).all()
    err = np.abs(np.asarray(runs[0].y_end) - np.asarray(ref.y_end))
    bound = atol + rtol * np.abs(np.asarray(ref.y_end))
    print("under-declared pattern: max err / (atol + rtol |y|) =", float((err / bound).max()))
    assert (err <= bound).all(), float((err / bound).max())


def test_non_finite_right_hand_side_retires_with_a_failure_status():
    """Outside the bit-equality claim (dense differencing puts NaN into rows the sparse form leaves 0): a trajectory whose
    right-hand side is NaN must still retire, with a failure status, and must not disturb its neighbours in the wave."""
    import ivp_amd
    n = 12
    src, _ = band_system(n, 1)
    y0, params, t1 = batch_inputs(n, seed=3)
    params[1, 4] = np.nan
    f = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=band_pattern(n, 1))
    r = ivp_amd.solve_ivp_batch(f, 0.0, t1, y0, params, ivp_amd.Options(method="BDF", rtol=RTOL, atol=ATOL, chunk_attempts=7))
    status = np.asarray(r.status)
    assert int(status[4]) not in (int(ivp_amd.Status.Success), -1), status
    ok = np.arange(B) != 4
    assert (status[ok] == 0).all() and np.isfinite(np.asarray(r.y_end)[:, ok]).all()
    g = ivp_amd.solve_ivp_batch(ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0)), 0.0, t1, y0, params,
                                ivp_amd.Options(method="BDF", rtol=RTOL, atol=ATOL, chunk_attempts=7))
    assert same_bits(np.asarray(r.y_end)[:, ok], np.asarray(g.y_end)[:, ok])


# ---- the SciPy-style front end -----------------------------------------------------------------------------------------
TRI40 = """
for (int i = 0; i < 40; ++i) {
    const double ym = i > 0 ? y[i - 1] : 0.0, yp = i < 39 ? y[i + 1] : 0.0;
    dydx[i] = p[0] * ((ym - 2.0 * y[i]) + yp) - p[1] * ((y[i] * y[i]) * y[i]);
}
"""


def _same_result(a, b):
    return (same_bits(a.t, b.t) and same_bits(a.y, b.y) and (a.nfev, a.njev, a.nlu, a.status) == (b.nfev, b.njev, b.nlu, b.status))


def test_pyfront_forwards_the_pattern_for_bdf_and_ignores_it_for_explicit_methods():
    sp = pytest.importorskip("scipy.sparse")
    from ivp_amd.pyfront import solve_ivp
    n = 40
    y0 = 0.5 + np.random.default_rng(1).uniform(size=n)
    kw = dict(args=(60.0, 8.0), rtol=1e-5, atol=1e-8)
    plain = solve_ivp(TRI40, (0.0, 0.05), y0, method="BDF", **kw)
    assert plain.success and plain.njev > 1
    for pattern in (band_pattern(n, 1), sp.csr_matrix(band_pattern(n, 1).astype(float))):
        res = solve_ivp(TRI40, (0.0, 0.05), y0, method="BDF", jac_sparsity=pattern, **kw)
        assert res.success and _same_result(res, plain)
    explicit = solve_ivp(TRI40, (0.0, 0.01), y0, method="RK45", **kw)
    # explicit methods never call jac: the pattern is accepted and unused, even a malformed one is never looked at
    assert _same_result(solve_ivp(TRI40, (0.0, 0.01), y0, method="RK45", jac_sparsity=band_pattern(n, 1), **kw), explicit)
    with pytest.raises(NotImplementedError):
        solve_ivp("dydx[0] = -y[0]; dydx[1] = y[0];", (0, 1), [1.0, 0.0], method="BDF", jac_sparsity=np.eye(2))


def medazko_pattern(n):
    """dF/dy of the Medazko system (tests/test_helpers.py:54-79): concentration rows 2j see their neighbours 2j -+ 2, themselves
    and the partner 2j + 1; partner rows 2j + 1 see themselves and 2j.  Returned as a scipy COO matrix like the reference's."""
    import scipy.sparse as sp
    rows, cols = [], []
    for j in range(n):
        e, o = 2 * j, 2 * j + 1
        for c in (e - 2, e, e + 2, o):
            if 0 <= c < 2 * n:
                rows.append(e); cols.append(c)
        rows += [o, o]
        cols += [o, e]
    return sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(2 * n, 2 * n))


def api_groups(n):
    from ivp_amd import api
    return api.jac_sparsity_groups(medazko_pattern(n), 2 * n)[1]


def test_integration_sparse_difference_BDF_with_the_pattern():   # test_stiff.py:148-165, test_ivp.py:245-265, the BDF leg
    pytest.importorskip("scipy.sparse")
    from numpy.testing import assert_, assert_allclose, assert_equal
    from ivp_amd.pyfront import solve_ivp
    from tests.test_pyfront_suite import MEDAZKO
    n = 200
    t_span = [0, 20]
    y0 = np.zeros(2 * n)
    y0[1::2] = 1
    res = solve_ivp(MEDAZKO, t_span, y0, method="BDF", jac_sparsity=medazko_pattern(n))
    assert_equal(res.t[0], t_span[0])
    assert_(res.t_events is None)
    assert_(res.y_events is None)
    assert_(res.success)
    assert_equal(res.status, 0)
    assert_allclose(res.y[78, -1], 0.233994e-3, rtol=1e-2)
    assert_allclose(res.y[79, -1], 0, atol=1e-3)
    assert_allclose(res.y[148, -1], 0.359561e-3, rtol=1e-2)
    assert_allclose(res.y[149, -1], 0, atol=1e-3)
    assert_allclose(res.y[198, -1], 0.117374129e-3, rtol=1e-2)
    assert_allclose(res.y[199, -1], 0.6190807e-5, atol=1e-3)
    assert_allclose(res.y[238, -1], 0, atol=1e-3)
    assert_allclose(res.y[239, -1], 0.9999997, rtol=1e-2)
    assert api_groups(n) == 4   # four evaluations of the right-hand side per Jacobian instead of 401
