"""Banded Jacobian storage on the GPU (`jac_storage="banded"`, ivp_amd/csrc/bdf_band.h) against the dense storage with the
same pattern and against the oracle.

The claim under test (include/ivp_hip.h): for a finite right-hand side and a pattern that contains
every structurally non-zero entry, the banded solve -- end state, end time, next step, status, all six counters, t_eval
samples, step log, dense segments -- equals the dense solve with that pattern and the oracle bit for bit, in strict and
in FMA mode, for any chunk length and for either residency of the factors (LDS, global memory).  `chunk_attempts = 7`
makes J and the factors cross launch boundaries.  The helpers and systems are those of tests/test_gpu_jac_sparsity.py."""
import numpy as np
import pytest

from tests.test_gpu_jac_sparsity import (ATOL, B, CASES, FIELDS, RTOL, TRI40, assert_equals_oracle, assert_runs_equal, band_pattern,
                                         band_system, batch_inputs, gpu_runs, medazko_pattern, oracle_solutions, same_bits)

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = -100
TE = np.linspace(0.0, 0.07, 9)


def asym_system(n):
    """y_i' = k (0.25 y_{i-2} + 0.5 y_{i-1} - 2 y_i + 0.5 y_{i+1}) - a y_i^3, zero outside: (ml, mu) = (2, 1)."""
    src = f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{{
    const double y2 = i >= 2 ? y[i - 2] : 0.0, y1 = i >= 1 ? y[i - 1] : 0.0, yp = i + 1 < {n} ? y[i + 1] : 0.0;
    const double s = ((0.25 * y2 + 0.5 * y1) - 2.0 * y[i]) + 0.5 * yp;
    return p[0] * s - p[1] * ((y[i] * y[i]) * y[i]);
}}
"""

    def fun(t, y, p):
        y = np.asarray(y, dtype=np.float64)
        z = np.concatenate((np.zeros(2), y, np.zeros(1)))
        s = ((0.25 * z[0:n] + 0.5 * z[1:n + 1]) - 2.0 * y) + 0.5 * z[3:n + 3]
        return p[0] * s - p[1] * ((y * y) * y)

    i, j = np.indices((n, n))
    return src, fun, ((i - j <= 2) & (j - i <= 1)).astype(np.int8)


def pivot_system(n):
    """y_i' = -k y_i + 1.5 k y_{i-1} - a y_i^3: (I - cJ) has 1 + c k (+ the cubic term) on the diagonal and -1.5 c k below it."""
    src = f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{{
    const double ym = i >= 1 ? y[i - 1] : 0.0;
    return (1.5 * p[0] * ym - p[0] * y[i]) - p[1] * ((y[i] * y[i]) * y[i]);
}}
"""

    def fun(t, y, p):
        y = np.asarray(y, dtype=np.float64)
        ym = np.concatenate((np.zeros(1), y[:-1]))
        return (1.5 * p[0] * ym - p[0] * y) - p[1] * ((y * y) * y)

    i, j = np.indices((n, n))
    return src, fun, ((i - j <= 1) & (j <= i)).astype(np.int8)


# name -> (source, numpy restatement, pattern, n, (ml, mu), trajectories)
BANDED_CASES = {
    **{k: (lambda k=k, bw=bw: (*CASES[k]()[:4], bw, B))
       for k, bw in (("tri12", (1, 1)), ("tri24", (1, 1)), ("tri40", (1, 1)), ("tri65", (1, 1)), ("tri130", (1, 1)),
                     ("band4_40", (4, 4)), ("band8_100", (8, 8)), ("tri24_as_penta", (2, 2)))},
    "asym40": lambda: (*asym_system(40), 40, (2, 1), B),
    "tri512": lambda: (*band_system(512, 1), band_pattern(512, 1), 512, (1, 1), 3),     # band factors in LDS where dense could never be
    "band8_512": lambda: (*band_system(512, 8), band_pattern(512, 8), 512, (8, 8), 3),  # over the LDS budget: the global form by itself
}

_ORACLE3 = {}


def oracle_for(case, fun, y0, params, t1, te, fma, **extra):
    """oracle_solutions for any batch size and extra options (the shared helper is fixed to B trajectories)"""
    if y0.shape[1] == B and not extra:
        return oracle_solutions(case, fun, y0, params, t1, te, fma)   # same inputs as tests/test_gpu_jac_sparsity.py: one cache
    from oracle import oracle as O
    key = (case, fma)
    if key not in _ORACLE3:
        mode = dict(fma=True) if fma else dict(detpow=True)
        sols = []
        for b in range(y0.shape[1]):
            common = dict(params=list(params[:, b]), method="BDF", rtol=RTOL, atol=ATOL, **mode, **extra)
            sols.append((O.solve_ivp(fun, 0.0, float(t1[b]), list(y0[:, b]), dense_output=True, **common),
                         O.solve_ivp(fun, 0.0, float(t1[b]), list(y0[:, b]), t_eval=te, **common)))
        _ORACLE3[key] = sols
    return _ORACLE3[key]


def runs(f, y0, params, t1, te, fma, chunk=7, max_log=256, **extra):
    """gpu_runs with extra options (variant, first_step)"""
    import ivp_amd
    if not extra:
        return gpu_runs(f, y0, params, t1, te, fma, chunk)
    mode = ivp_amd.FpMode.FMA if fma else ivp_amd.FpMode.STRICT
    o = dict(method="BDF", rtol=RTOL, atol=ATOL, chunk_attempts=chunk, fp_mode=mode, **extra)
    return (ivp_amd.solve_ivp_batch(f, 0.0, t1, y0, params, ivp_amd.Options(t_eval=te, **o)),
            ivp_amd.solve_ivp_batch(f, 0.0, t1, y0, params, ivp_amd.Options(dense_output=True, max_log=max_log, **o)))


def inputs(n, nb, seed):
    y0, params, t1 = batch_inputs(n, seed)
    return np.ascontiguousarray(y0[:, :nb]), np.ascontiguousarray(params[:, :nb]), np.ascontiguousarray(t1[:nb])


@pytest.mark.parametrize("fma", [False, True], ids=["strict", "fma"])
@pytest.mark.parametrize("case", list(BANDED_CASES))
def test_banded_equals_dense_with_the_pattern_and_the_oracle(case, fma):
    import ivp_amd
    from ivp_amd import api
    src, fun, pattern, n, bw, nb = BANDED_CASES[case]()
    assert api.jac_bandwidth(pattern, n) == bw
    y0, params, t1 = inputs(n, nb, seed=n + len(case))
    dense = gpu_runs(ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=pattern), y0, params, t1, TE, fma)
    f = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=pattern, jac_storage="banded")
    ml, mu = bw
    assert f.jac_layout == {"banded": True, "ml": ml, "mu": mu, "jac_doubles": (ml + mu + 1) * n, "lu_doubles": (2 * ml + mu + 1) * n}
    banded = gpu_runs(f, y0, params, t1, TE, fma)
    assert (np.asarray(dense[0].status) == 0).all()
    assert int(np.asarray(dense[0].njev).min()) > 1 and int(np.asarray(dense[0].nlu).min()) > 1
    assert_runs_equal(banded, dense, f"{case}: banded vs dense")
    sols = oracle_for(case, fun, y0, params, t1, TE, fma)
    assert_equals_oracle(banded, sols, TE, f"{case}: banded vs oracle")
    assert_equals_oracle(dense, sols, TE, f"{case}: dense vs oracle")


@pytest.mark.parametrize("fma", [False, True], ids=["strict", "fma"])
def test_row_exchanges_inside_a_real_solve(fma):
    """first_step = 0.5: the first factorisation has c = 0.5 / 1.185 (BDF1: alpha = 1 - kappa_1 = 1.185), and with
    1.5 c k > 1 + c k (+ the cubic term's share of the diagonal) the sub-diagonal entry of EVERY column beats the
    diagonal: the pivot search exchanges rows throughout that factorisation."""
    import ivp_amd
    n = 24
    src, fun, pattern = pivot_system(n)
    y0, params, t1 = batch_inputs(n, seed=77)
    params[1] = 0.01 * (1.0 + np.arange(B))          # a: small, the linear part decides the pivots
    t1 = 1.0 + 0.1 * np.arange(B)                   # beyond first_step: no last-step clamp before the first factorisation
    c = 0.5 / 1.185
    k, a = params
    assert (1.5 * c * k > 1.0 + c * k).all()
    assert (1.5 * c * k > 1.0 + c * k + 3.0 * a * c * (y0 * y0).max(axis=0)).all()
    extra = dict(first_step=0.5, max_log=512)   # up to 275 dense-output segments per trajectory (the step log stays below 256)
    dense = runs(ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=pattern), y0, params, t1, TE, fma, **extra)
    f = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=pattern, jac_storage="banded")
    assert (f.jac_layout["ml"], f.jac_layout["mu"]) == (1, 0)
    banded = runs(f, y0, params, t1, TE, fma, **extra)
    assert (np.asarray(dense[0].status) == 0).all()
    assert_runs_equal(banded, dense, "pivoting: banded vs dense")
    sols = oracle_for("pivot24", fun, y0, params, t1, TE, fma, first_step=0.5)
    assert_equals_oracle(banded, sols, TE, "pivoting: banded vs oracle")
    assert_equals_oracle(dense, sols, TE, "pivoting: dense vs oracle")


@pytest.mark.parametrize("case", ["tri40", "band4_40", "tri130"])
def test_global_memory_factors_give_the_bits_of_the_lds_form(case):
    import ivp_amd
    src, fun, pattern, n, bw, nb = BANDED_CASES[case]()
    y0, params, t1 = inputs(n, nb, seed=n + len(case))
    f = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=pattern, jac_storage="banded")
    lds = gpu_runs(f, y0, params, t1, TE, False)
    glob = runs(f, y0, params, t1, TE, False, variant=1)
    assert (np.asarray(lds[0].status) == 0).all()
    assert_runs_equal(glob, lds, f"{case}: variant 1 vs variant 0")
    forced = runs(f, y0, params, t1, TE, False, variant=2)
    assert_runs_equal(forced, lds, f"{case}: variant 2 vs variant 0")


def test_layout_and_validation():
    import ivp_amd
    n = 40
    src, _ = band_system(n, 1)
    dense = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=band_pattern(n, 1))
    assert dense.jac_layout == {"banded": False, "ml": 0, "mu": 0, "jac_doubles": n * n, "lu_doubles": n * n}
    plain = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0))
    assert plain.jac_layout == {"banded": False, "ml": 0, "mu": 0, "jac_doubles": n * n, "lu_doubles": n * n}
    band = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=band_pattern(n, 4), jac_storage="banded")
    assert band.jac_layout == {"banded": True, "ml": 4, "mu": 4, "jac_doubles": 9 * n, "lu_doubles": 13 * n}

    # the three rejections of ivp_rhs_compile_sparse, at the C entry point (the Python layer refuses jac=True earlier)
    import ctypes as C
    from ivp_amd import api
    ctx = api.default_context()
    i32p = C.POINTER(C.c_int32)

    def compile_rc(source, nn, flags, pattern):
        cp, ri = api.sparsity_csc(pattern, nn)
        h = C.c_void_p()
        rc = ctx.lib.ivp_rhs_compile_sparse(ctx.handle, source.encode(), nn, 2, 0, flags, cp.ctypes.data_as(i32p), ri.ctypes.data_as(i32p), C.byref(h))
        return rc, ctx.last_error()

    jac_src = src + "__device__ void jac_col(int col, double t, const double* y, double* column, const double* p) { column[col] = -1.0; }\n"
    rc, msg = compile_rc(jac_src, n, 1 | 2, band_pattern(n, 1))
    assert rc == BAD_ARGUMENT and "HAS_JAC" in msg, msg
    small = "__device__ void ode(double x, const double* y, double* d, const double* p) { for (int i = 0; i < 8; ++i) d[i] = -y[i]; }"
    rc, msg = compile_rc(small, 8, 2, band_pattern(8, 1))
    assert rc == BAD_ARGUMENT and msg, msg
    arrow = np.eye(20, dtype=np.int8)
    arrow[0, :] = 1
    arrow[:, 0] = 1
    rc, msg = compile_rc(band_system(20, 1)[0], 20, 2, arrow)
    assert rc == BAD_ARGUMENT and "wide" in msg, msg
    with pytest.raises(ivp_amd.ConfigError) as e:
        ivp_amd.DeviceIVP(band_system(20, 1)[0], n=20, params=(1.0, 1.0), jac_sparsity=arrow, jac_storage="banded")
    assert e.value.code == BAD_ARGUMENT
    with pytest.raises(ivp_amd.ConfigError) as e:   # 2 ml + mu + 1 = n exactly
        ivp_amd.DeviceIVP(band_system(13, 1)[0], n=13, params=(1.0, 1.0), jac_sparsity=band_pattern(13, 4), jac_storage="banded")
    assert e.value.code == BAD_ARGUMENT


def test_non_finite_right_hand_side_retires_with_a_failure_status():
    """Outside the bit-equality claim; the lane must still retire with a failure status, and its neighbours in the wave
    (n = 12: four trajectories per wavefront) must equal the dense solve bit for bit."""
    import ivp_amd
    n = 12
    src, _ = band_system(n, 1)
    y0, params, t1 = batch_inputs(n, seed=3)
    params[1, 4] = np.nan
    o = ivp_amd.Options(method="BDF", rtol=RTOL, atol=ATOL, chunk_attempts=7)
    f = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=band_pattern(n, 1), jac_storage="banded")
    r = ivp_amd.solve_ivp_batch(f, 0.0, t1, y0, params, o)
    status = np.asarray(r.status)
    assert int(status[4]) not in (int(ivp_amd.Status.Success), -1), status
    ok = np.arange(B) != 4
    assert (status[ok] == 0).all() and np.isfinite(np.asarray(r.y_end)[:, ok]).all()
    g = ivp_amd.solve_ivp_batch(ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=band_pattern(n, 1)), 0.0, t1, y0, params, o)
    for k in FIELDS:
        assert same_bits(np.asarray(getattr(r, k))[..., ok], np.asarray(getattr(g, k))[..., ok]), k


def _same_result(a, b):
    return (same_bits(a.t, b.t) and same_bits(a.y, b.y) and (a.nfev, a.njev, a.nlu, a.status) == (b.nfev, b.njev, b.nlu, b.status))


def test_pyfront_forwards_the_storage_for_bdf():
    from ivp_amd.pyfront import solve_ivp
    n = 40
    y0 = 0.5 + np.random.default_rng(1).uniform(size=n)
    kw = dict(args=(60.0, 8.0), rtol=1e-5, atol=1e-8)
    plain = solve_ivp(TRI40, (0.0, 0.05), y0, method="BDF", **kw)
    assert plain.success and plain.njev > 1
    res = solve_ivp(TRI40, (0.0, 0.05), y0, method="BDF", jac_sparsity=band_pattern(n, 1), jac_storage="banded", **kw)
    assert res.success and _same_result(res, plain)
    # explicit methods never call jac: pattern and storage are accepted and unused
    explicit = solve_ivp(TRI40, (0.0, 0.01), y0, method="RK45", **kw)
    assert _same_result(solve_ivp(TRI40, (0.0, 0.01), y0, method="RK45", jac_sparsity=band_pattern(n, 1), jac_storage="banded", **kw), explicit)


def test_medazko_golden_values_with_banded_storage():   # test_stiff.py:148-165
    pytest.importorskip("scipy.sparse")
    from numpy.testing import assert_, assert_allclose, assert_equal
    from ivp_amd import api
    from ivp_amd.pyfront import solve_ivp
    from tests.test_pyfront_suite import MEDAZKO
    n = 200
    t_span = [0, 20]
    y0 = np.zeros(2 * n)
    y0[1::2] = 1
    assert api.jac_bandwidth(medazko_pattern(n), 2 * n) == (2, 2)
    res = solve_ivp(MEDAZKO, t_span, y0, method="BDF", jac_sparsity=medazko_pattern(n), jac_storage="banded")
    assert_equal(res.t[0], t_span[0])
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


def test_chunk_lengths_and_work_space_resizing_on_one_context():
    """One context: a dense problem, then a banded one (smaller blocks in the same buffers), then a dense one of larger n
    (the buffers grow) -- and the banded problem again.  Every solve equals its own fresh-order result for every chunk length."""
    import ivp_amd
    src40, _ = band_system(40, 1)
    src65, _ = band_system(65, 1)
    in40, in65 = inputs(40, B, seed=41), inputs(65, B, seed=66)
    dense40 = ivp_amd.DeviceIVP(src40, n=40, params=(1.0, 1.0), jac_sparsity=band_pattern(40, 1))
    band40 = ivp_amd.DeviceIVP(src40, n=40, params=(1.0, 1.0), jac_sparsity=band_pattern(40, 1), jac_storage="banded")
    dense65 = ivp_amd.DeviceIVP(src65, n=65, params=(1.0, 1.0), jac_sparsity=band_pattern(65, 1))
    want40 = gpu_runs(dense40, *in40, TE, False, chunk=7)
    for chunk in (3, 7, 0):
        a = gpu_runs(dense40, *in40, TE, False, chunk=chunk)
        b = gpu_runs(band40, *in40, TE, False, chunk=chunk)
        c = gpu_runs(dense65, *in65, TE, False, chunk=chunk)
        d = gpu_runs(band40, *in40, TE, False, chunk=chunk)
        assert (np.asarray(c[0].status) == 0).all()
        assert_runs_equal(a, want40, f"chunk {chunk}: dense")
        assert_runs_equal(b, want40, f"chunk {chunk}: banded after dense")
        assert_runs_equal(d, want40, f"chunk {chunk}: banded after a larger dense problem")
        if chunk == 3:
            want65 = c
        assert_runs_equal(c, want65, f"chunk {chunk}: dense n = 65 after banded")
