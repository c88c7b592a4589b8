"""Radau IIA(5) without a GPU: the CPU model (tests/radau_model.py, the yardstick of tests/test_gpu_radau.py) against
outside truths, and the host validation of the direct-call entry points.

The model is judged here against things that are not the kernels: SciPy's Radau at rtol = atol = 1e-10
(tests/golden/scipy_stiff_truth.json), the analytic harmonic oscillator, the collocation identities of the dense output
and numpy's linear algebra.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from ivp_amd import _lib
from tests import radau_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = json.load(open(os.path.join(ROOT, "tests", "golden", "scipy_stiff_truth.json")))["truth"]


# ---- 1. the model against SciPy's Radau (libm powers, as the reference computes them) ---------------------------------

def test_model_stiff_vdp_against_scipy_truth():
    """The bounds of the BDF pins for the same problems and tolerances (tests/test_gpu_reference_pins.py:246-248)."""
    r = M.solve(M.rhs_vdp_eps(1e-3), 0.0, 2.0, [2.0, 0.0], 1e-6, 1e-8, libm=True)
    print("eps = 1e-3:", r.status, r.y_end, np.abs(np.array(r.y_end) - TRUTH["vdp_eps1e-3_t2"]).max())
    assert r.status == M.SUCCESS
    assert np.abs(np.array(r.y_end) - TRUTH["vdp_eps1e-3_t2"]).max() < 1e-4
    assert r.n_reuse > 0 and r.nrejct > 0   # the factor-reuse branch and ordinary rejections are on this problem's path


def test_model_vdp_mu1000_against_scipy_truth():
    r = M.solve(M.rhs_vdp(1000.0), 0.0, 3000.0, [2.0, 0.0], 1e-4, 1e-6, libm=True)
    print("mu = 1000:", r.status, r.y_end, np.abs(np.array(r.y_end) - TRUTH["vdp_mu1000_t3000"]).max())
    assert r.status == M.SUCCESS
    assert np.abs(np.array(r.y_end) - TRUTH["vdp_mu1000_t3000"]).max() < 1e-2
    assert r.n_dyth > 0   # the Newton loop's dyth >= 1 exit


# ---- 2. SHO, one period (tests/accuracy.rs) ---------------------------------------------------------------------------

def test_model_sho_one_period():
    r = M.solve(M.rhs_sho, 0.0, 2.0 * math.pi, [1.0, 0.0], 1e-6, 1e-8, libm=True)
    assert r.status == M.SUCCESS
    assert abs(r.y_end[0] - 1.0) < 1e-5 and abs(r.y_end[1]) < 1e-5


# ---- 3. interpolate ---------------------------------------------------------------------------------------------------

def test_model_interpolate_reproduces_the_collocation_values():
    """On an accepted step the dense polynomial is the Newton form through (s, value) = (0, y1), (c2 - 1, y0 + z2),
    (c1 - 1, y0 + z1), (-1, y0) with s = (t - (xold + h)) / h: interpolate returns the step's end point at xold + h and the
    three collocation values y0 + z_i at xold + c_i h.
    Tolerance.  Each coefficient comes from the z_i through at most three subtractions / divisions (relative error <= 3 eps
    each, the differences of the z_i are the data), the four-term Horner form adds one multiply and one add per level
    (<= 2 eps of the partial result per level, 3 levels), and y1 = y0 + z3 is rounded once: <= 16 eps (|y1| + |c1| + |c2|
    + |c3|) in all, taken as 32 eps for the constants' own rounding (C1, C2, C1M1, C2M1 are stored to 16 digits).  The
    abscissa xold + c_i h is rounded too: s is off by <= 4 eps max|x| / |h|, which moves the value by <= |p'(s)| times
    that, |p'| <= |c1| + 2 |c2| + 3 |c3| on [-1, 0]."""
    eps = np.finfo(float).eps
    r = M.solve(M.rhs_vdp_eps(1e-3), 0.0, 2.0, [2.0, 0.0], 1e-6, 1e-8, dense_output=True, libm=True)
    assert len(r.segs) == r.naccpt == len(r.stages)
    for k in (0, 1, 7, len(r.segs) // 2, len(r.segs) - 1):
        cont, xold, h = r.segs[k]
        y0, z1, z2, z3 = r.stages[k]
        n = len(y0)
        ds = 4 * eps * max(abs(xold), abs(xold + h)) / abs(h)
        end = M.interpolate(xold + h, cont, xold, h)
        for i in range(n):
            scale = abs(cont[i]) + abs(cont[n + i]) + abs(cont[2 * n + i]) + abs(cont[3 * n + i])
            slope = abs(cont[n + i]) + 2 * abs(cont[2 * n + i]) + 3 * abs(cont[3 * n + i])
            tol = 32 * eps * scale + slope * ds
            assert abs(end[i] - r.y[k + 1][i]) <= tol, (k, i)
            for ci, z in ((M.C1, z1), (M.C2, z2), (1.0, z3)):
                got = M.interpolate(xold + ci * h, cont, xold, h)[i]
                assert abs(got - (y0[i] + z[i])) <= tol, (k, i, ci, got - (y0[i] + z[i]), tol)


def test_model_dense_coefficients_are_the_divided_differences_of_the_stage_increments():
    """cont[n..4n) against the definition (radau.rs:697-705) on hand-made increments: the polynomial passes through
    (c_i - 1, z_i - z3) for the three stages."""
    z1, z2, z3, y1 = 0.3, -0.7, 1.1, 5.0
    ak = (z1 - z2) / M.C1MC2
    c1_ = (z2 - z3) / M.C2M1
    c2_ = (ak - c1_) / M.C1M1
    c3_ = c2_ - (ak - z1 / M.C1) / M.C2
    cont = [y1, c1_, c2_, c3_]
    for ci, zi in ((M.C1, z1), (M.C2, z2), (1.0, z3)):
        got = M.interpolate(10.0 + ci * 0.5, cont, 10.0, 0.5)[0]
        assert abs(got - (y1 - z3 + zi)) < 1e-13, (ci, got)
    assert abs(M.interpolate(10.0, cont, 10.0, 0.5)[0] - (y1 - z3)) < 1e-13


# ---- 4. host validation without a device ------------------------------------------------------------------------------

def _check(prob=None, opt=None, rad=None, radau=True, B=4):
    lib = _lib.load()
    p = _lib.ProblemT()
    p.rhs_id, p.n, p.n_params = prob or (10, 2, 1)   # StiffVanDerPol
    o = _lib.OptionsT()
    lib.ivp_options_default(C.byref(o))
    for k, v in (opt or {}).items():
        setattr(o, k, v)
    s = _lib.RadauSettingsT()
    lib.ivp_radau_settings_default(C.byref(s))
    for k, v in (rad or {}).items():
        setattr(s, k, v)
    msg = C.create_string_buffer(512)
    if radau:
        rc = lib.ivp_radau_check(C.byref(p), B, C.byref(o), C.byref(s), msg, 512)
    else:
        rc = lib.ivp_options_check(C.byref(p), B, C.byref(o), msg, 512)
    return rc, msg.value.decode()


def test_radau_settings_default_are_the_reference_struct_defaults():
    """RADAU::default(), radau.rs:68-90."""
    lib = _lib.load()
    s = _lib.RadauSettingsT()
    s.reserved = 77
    lib.ivp_radau_settings_default(C.byref(s))
    assert (s.uround, s.safety_factor, s.scale_min, s.scale_max, s.newton_maxiter, s.has_newton_tol, s.predictive, s.reserved) == \
           (2.3e-16, 0.9, 0.2, 8.0, 7, 0, 1, 0)
    assert C.sizeof(_lib.RadauSettingsT) == 56


def test_valid_settings_pass_and_method_is_ignored():
    assert _check()[0] == 0
    for m in (0, 4, 5, 99):
        assert _check(opt={"method": m})[0] == 0
    assert _check(rad={"newton_maxiter": 15, "has_newton_tol": 1, "newton_tol": 1e-3, "predictive": 0})[0] == 0
    assert _check(prob=(15, 3, 0))[0] == 0   # RobertsonJac


@pytest.mark.parametrize("rad, opt, code", [
    ({"uround": 1e-36}, {}, -2), ({"uround": 1.0}, {}, -2),                       # OutOfRange, radau.rs:143-151
    ({"safety_factor": 1e-4}, {}, -2), ({"safety_factor": 1.0}, {}, -2),          # OutOfRange, radau.rs:153-161
    ({"scale_min": 0.0}, {}, -6), ({"scale_min": 8.0}, {}, -6), ({"scale_max": float("nan")}, {}, -6),   # InvalidScaleFactors
    ({"newton_maxiter": 0}, {}, -1),                                              # MustBePositive, radau.rs:179-185
    ({"newton_maxiter": 16}, {}, -2),                                             # the device's bound
    ({}, {"has_first_step": 1, "first_step": 0.0}, -5),                           # InvalidStepSize, radau.rs:256-261
    ({}, {"rtol": -1e-6}, -3), ({}, {"atol": -1.0}, -3),                          # NegativeTolerance
])
def test_config_errors_map_to_their_codes(rad, opt, code):
    rc, msg = _check(rad=rad, opt=opt)
    assert rc == code, msg
    assert msg


def test_tolerance_vector_length_is_checked():
    v = (C.c_double * 3)(1e-6, 1e-6, 1e-6)
    rc, msg = _check(opt={"rtol_vec": C.cast(v, C.POINTER(C.c_double)), "rtol_vec_len": 3})
    assert rc == -4, msg


@pytest.mark.parametrize("prob, opt, word", [
    ((100, 100, 0), {}, "n = 100"),                   # LinearDecay100: n > 8
    ((11, 2, 0), {}, "event"),                        # SHO with an event function
    ((10, 2, 1), {"fp_mode": 1}, "FMA"),
    ((10, 2, 1), {"variant": 3}, "variant"),
])
def test_not_yet_rejections_are_bad_argument_with_a_message(prob, opt, word):
    rc, msg = _check(prob=prob, opt=opt)
    assert rc == -100
    assert "not yet" in msg and word in msg, msg


def test_radau_through_the_solve_ivp_entry_points_is_still_unsupported():
    rc, msg = _check(opt={"method": 4}, radau=False)
    assert rc == -101 and "RADAU" in msg
    assert _check(opt={"method": 5}, radau=False)[0] == 0
    lib = _lib.load()   # and with no context nothing is validated at all
    assert lib.ivp_radau_solve(None, None, 1, None, None, None, 1, None, 1, None, None, None) == -100


# ---- 5. the model's complex LU against numpy --------------------------------------------------------------------------

def _solve_complex(A, b):
    n = len(b)
    ar = [[float(A[i, j].real) for j in range(n)] for i in range(n)]
    ai = [[float(A[i, j].imag) for j in range(n)] for i in range(n)]
    ip, piv, cases = [0] * n, [], set()
    ok = M.lu_decomp_complex(ar, ai, ip, piv, cases)
    if not ok:
        return None, piv, cases
    br, bi = [float(v.real) for v in b], [float(v.imag) for v in b]
    M.lin_solve_complex(ar, ai, br, bi, ip)
    return np.array(br) + 1j * np.array(bi), piv, cases


@pytest.mark.parametrize("n", range(1, 9))
def test_model_complex_lu_against_numpy(n):
    """Partial pivoting is backward stable up to the growth factor: |x - x_ref| / |x_ref| <= c n eps cond(A); c = 64
    leaves room for the growth of an 8 x 8 random matrix and for numpy's own error."""
    rng = np.random.default_rng(100 + n)
    for _ in range(5):
        A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        x, _, _ = _solve_complex(A, b)
        ref = np.linalg.solve(A, b)
        bound = 64 * n * np.finfo(float).eps * np.linalg.cond(A)
        assert np.abs(x - ref).max() <= bound * np.abs(ref).max(), (n, np.abs(x - ref).max(), bound)


def test_model_complex_lu_exchanges_rows_and_takes_all_three_multiplier_cases():
    A = np.array([[1e-3, 2.0, 1j], [4.0 + 1j, 1.0, 3j], [1.0, 2j, 5.0]], dtype=complex)   # column 0: row 1 is the pivot;
    # its row holds a real (1.0) and an imaginary (3j) multiplier, the second elimination step a general one
    b = np.array([1.0, 2.0 - 1j, 0.5j])
    x, piv, cases = _solve_complex(A, b)
    assert ("complex", 0, 1) in piv
    assert np.abs(x - np.linalg.solve(A, b)).max() <= 64 * 3 * np.finfo(float).eps * np.linalg.cond(A) * np.abs(x).max()
    assert cases == {"real", "imag", "general"}
    # first maximum wins: two rows of equal |re| + |im| in column 0 keep the upper one
    _, piv, _ = _solve_complex(np.array([[1.0 + 1j, 1.0], [2.0, 3.0]], dtype=complex), np.array([1.0, 1.0], dtype=complex))
    assert piv == []


def test_model_lu_reports_singular_matrices():
    assert _solve_complex(np.array([[1.0 + 1j, 2.0], [2.0 + 2j, 4.0]], dtype=complex), np.array([1.0, 1.0], dtype=complex))[0] is None
    assert _solve_complex(np.zeros((1, 1), dtype=complex), np.array([1.0 + 0j]))[0] is None
    assert _solve_complex(np.zeros((3, 3), dtype=complex), np.ones(3, dtype=complex))[0] is None
    a = [[1.0, 2.0], [2.0, 4.0]]
    assert not M.lu_decomp(a, [0, 0])
    a = [[0.0, 1.0], [1.0, 0.0]]
    ip = [0, 0]
    assert M.lu_decomp(a, ip) and ip[0] == 1
    b = [3.0, 5.0]
    M.lin_solve(a, b, ip)
    assert b == [5.0, 3.0]


def test_model_identity_mass_products_keep_the_sign_of_zero():
    """Quirk 5 of the restatement: sum -= 0.0 * f over the identity's zeros from +0.0 gives 0.0 - f[i], which is +0.0 for
    f[i] = +0.0 where -f[i] would be -0.0; the model multiplies the zeros out, so it has this by construction."""
    s = 0.0
    for mij, f in ((0.0, 3.0), (1.0, 0.0), (0.0, -2.0)):
        s -= mij * f
    assert math.copysign(1.0, s) == 1.0 and math.copysign(1.0, -0.0) == -1.0


# ---- 6. the model's real and complex solves against mpmath ------------------------------------------------------------

def test_model_lu_backward_error_against_mpmath():
    """The fixed-seed systems of tests/radau_lu_cases.py (67 per N = 1..8: the set the device probe of
    tests/test_gpu_radau_lu_probe.py is held to, bit for bit), every one the model factorises: the normwise backward error
    |A x - b| / (|A| |x|) in the infinity norm, with the residual formed by mpmath at 50 digits from the float64 data.

    Measured: 3.1911975778961213e-16 at most over the real systems (lu_decomp / lin_solve; N = 8, a kernel-form matrix
    fac1 I - J) and 3.485266890995033e-16 over the complex ones (lu_decomp_complex / lin_solve_complex; N = 6, a kernel-form
    matrix).  The bound is 4 x the measured value: the model's arithmetic is IEEE float64 one operation at a time and so is
    deterministic, the margin is for a different numpy drawing the matrices.  The number is the model's against mpmath, not
    the kernel's; the device inherits it through bit equality."""
    import mpmath as mp
    from tests import radau_lu_cases as L
    worst, worstc = 0.0, 0.0
    with mp.workdps(50):
        for n in range(1, 9):
            for r in L.reference(n):
                if r["ok"]:
                    A, x, b = mp.matrix(r["a"].tolist()), mp.matrix([float(v) for v in r["x"]]), mp.matrix([float(v) for v in r["b"]])
                    worst = max(worst, float(mp.norm(A * x - b, mp.inf) / (mp.mnorm(A, mp.inf) * mp.norm(x, mp.inf))))
                if r["okc"]:
                    A = mp.matrix([[mp.mpc(float(r["ar"][i][j]), float(r["ai"][i][j])) for j in range(n)] for i in range(n)])
                    x = mp.matrix([mp.mpc(float(u), float(v)) for u, v in zip(r["xr"], r["xi"])])
                    b = mp.matrix([mp.mpc(float(u), float(v)) for u, v in zip(r["br"], r["bi"])])
                    worstc = max(worstc, float(mp.norm(A * x - b, mp.inf) / (mp.mnorm(A, mp.inf) * mp.norm(x, mp.inf))))
    print(f"largest backward error: real {worst!r}, complex {worstc!r}")
    assert worst <= 4 * 3.1911975778961213e-16 and worstc <= 4 * 3.485266890995033e-16
    assert worst > 0.0 and worstc > 0.0
