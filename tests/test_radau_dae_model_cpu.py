"""tests/radau_dae_model.py, the yardstick of the Radau DAE tests, against what it must agree with before anything is held to it:

  * tests/radau_model.py BIT FOR BIT on ODE problems, with the mass matrix omitted and with the identity given -- among them
    runs with rejected steps, first-step rejections, `h *= 0.5` restarts and the Newton `dyth` exit, so the `hhfac`
    bookkeeping the DAE model adds is shown inert when no index-2/3 variable reads it;
  * independent truth on M y' = f problems: closed forms, Robertson's ODE form through radau_model, and the pendulum in
    its angle form integrated with RK4 at 20 000 steps.  Every bound is 10x the model's own error, measured with the
    deterministic power (the default); the measured value stands next to each bound;
  * the reference's partition rules (radau.rs:210-246), and the index-2 pendulum with the pure-ODE partition, which does not
    end in Success: the index sets are observable.
"""
import math

import numpy as np
import pytest

from tests import radau_dae_model as D
from tests import radau_model as M

COUNTERS = ("nfev", "njev", "nlu", "nstep", "naccpt", "nrejct")


def same(a, b):
    a, b = float(a), float(b)
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def identity(n):
    return [[1.0 if r == c else 0.0 for c in range(n)] for r in range(n)]


def assert_same_run(a, b, tag):
    assert a.status == b.status and all(getattr(a, k) == getattr(b, k) for k in COUNTERS), (tag, [(getattr(a, k), getattr(b, k)) for k in COUNTERS])
    assert same(a.t_end, b.t_end) and same(a.h_next, b.h_next), tag
    assert all(same(u, v) for u, v in zip(a.y_end, b.y_end)), tag
    assert len(a.t) == len(b.t) and all(same(u, v) for u, v in zip(a.t, b.t)), tag
    assert all(same(u, v) for ya, yb in zip(a.y, b.y) for u, v in zip(ya, yb)), tag
    assert len(a.segs) == len(b.segs), tag
    for (ca, xa, ha), (cb, xb, hb) in zip(a.segs, b.segs):
        assert same(xa, xb) and same(ha, hb) and all(same(u, v) for u, v in zip(ca, cb)), tag
    assert a.h_tried == b.h_tried and a.newton_counts == b.newton_counts, tag


ODE_CASES = {
    # name: (f, jac, t0, t1, y0, rtol, atol, kwargs, settings)
    "decay": (M.rhs_decay(2.0), None, 0.0, 3.0, [1.0], 1e-6, 1e-8, {}, {}),
    "sho_backward": (M.rhs_sho, None, 1.0, -2.0, [1.0, 0.0], 1e-6, 1e-8, {}, {}),
    "vdp_eps": (M.rhs_vdp_eps(1e-3), None, 0.0, 2.0, [2.0, 0.0], 1e-6, 1e-8, {"dense_output": True}, {}),
    "vdp_mu_1000": (M.rhs_vdp(1000.0), None, 0.0, 100.0, [2.0, 0.0], 1e-6, 1e-8, {}, {}),
    "robertson_jac": (M.rhs_robertson, M.jac_robertson, 0.0, 40.0, [1.0, 0.0, 0.0], 1e-6, 1e-10, {"t_eval": [0.0, 0.4, 4.0, 40.0]}, {}),
    "lorenz_first_step": (M.rhs_lorenz(10.0, 28.0, 8.0 / 3.0), None, 0.0, 1.0, [1.0, 1.0, 1.0], [1e-6, 1e-5, 1e-7], [1e-8, 1e-9, 1e-7],
                          {"first_step": 0.5}, {}),
    "vdp_eps_newton_2": (M.rhs_vdp_eps(1e-3), None, 0.0, 2.0, [2.0, 0.0], 1e-6, 1e-8, {}, {"newton_maxiter": 2}),
    "vdp_eps_no_predictive": (M.rhs_vdp_eps(1e-3), None, 0.0, 2.0, [2.0, 0.0], 1e-6, 1e-8, {}, {"predictive": False}),
}


@pytest.fixture(scope="module")
def ode_runs():
    out = {}
    for name, (f, jac, t0, t1, y0, rt, at, kw, st) in ODE_CASES.items():
        base = M.solve(f, t0, t1, list(y0), rt, at, settings=M.Settings(**st), jac=jac, **kw)
        plain = D.solve(f, t0, t1, list(y0), rt, at, settings=M.Settings(**st), jac=jac, **kw)
        ident = D.solve(f, t0, t1, list(y0), rt, at, settings=M.Settings(**st), jac=jac, mass=identity(len(y0)), **kw)
        out[name] = (base, plain, ident)
    return out


@pytest.mark.parametrize("name", sorted(ODE_CASES))
def test_the_dae_model_is_radau_model_bit_for_bit_without_a_mass_matrix_and_with_the_identity(ode_runs, name):
    base, plain, ident = ode_runs[name]
    assert_same_run(base, plain, name + " (mass omitted)")
    assert_same_run(base, ident, name + " (identity given)")


def test_the_ode_cases_take_the_paths_that_assign_hhfac(ode_runs):
    """every assignment of hhfac is reached by one of the runs above: the three `h *= 0.5` restarts that exist without a
    singular matrix (Newton out of iterations, theta >= 0.99), the dyth exit, a first-step rejection, an ordinary rejection,
    both accepted-step paths (the reuse `continue` among them)"""
    runs = {k: v[0] for k, v in ode_runs.items()}
    assert any(r.n_dyth > 0 for r in runs.values())
    assert any(r.nrejct > r.n_dyth for r in runs.values())
    assert any(r.n_first_reject > 0 for r in runs.values())
    assert any(r.n_restart_newton > 0 for r in runs.values())
    assert any(r.n_restart_theta > 0 for r in runs.values())
    assert any(r.n_reuse > 0 for r in runs.values())
    # ... and the DAE model saw a different hhfac on each of them
    hh = set()
    for _, plain, _ in ode_runs.values():
        hh.update(plain.hhfacs)
    assert {0.5, 0.1} <= hh and len(hh) > 20


# ---- independent truth ------------------------------------------------------------------------------------------------------

def max_err(got, want):
    return max(abs(u - v) for u, v in zip(got, want))


def pendulum_truth(t1, steps=20000):
    """p = (cos phi, sin phi), phi'' = -cos phi from phi = phi' = 0: classical RK4 -> (p1, p2, v1, v2, lam)"""
    f = lambda s: np.array([s[1], -math.cos(s[0])])
    s = np.array([0.0, 0.0])
    h = t1 / steps
    for _ in range(steps):
        k1 = f(s)
        k2 = f(s + 0.5 * h * k1)
        k3 = f(s + 0.5 * h * k2)
        k4 = f(s + h * k3)
        s = s + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    phi, om = float(s[0]), float(s[1])
    return [math.cos(phi), math.sin(phi), -om * math.sin(phi), om * math.cos(phi), om * om - math.sin(phi)]


@pytest.fixture(scope="module")
def pend_truth():
    return pendulum_truth(2.0)


def test_robertson_as_an_index_1_dae_equals_its_ode_form():
    ode = M.solve(M.rhs_robertson, 0.0, 40.0, [1.0, 0.0, 0.0], 1e-6, 1e-10)
    dae = D.solve(D.rhs_robertson_dae, 0.0, 40.0, [1.0, 0.0, 0.0], 1e-6, 1e-10, mass=D.MASS_ROBERTSON)
    assert dae.status == M.SUCCESS and (dae.naccpt, dae.nrejct) == (ode.naccpt, ode.nrejct) == (48, 2)
    err = max_err(dae.y_end, ode.y_end)
    print("robertson dae - ode:", err)
    assert err <= 1.43e-13   # 10 x the measured 1.43e-14


def test_the_algebraic_equation_with_zero_mass():
    r = D.solve(D.rhs_algebraic, 0.0, 2.0, [1.0], 1e-6, 1e-8, mass=[[0.0]])
    assert r.status == M.SUCCESS and r.naccpt == 8
    err = abs(r.y_end[0] - math.cos(2.0))
    print("algebraic:", err)
    assert err <= 5.6e-16   # 10 x the measured 5.6e-17 (half an ulp of the result)


def test_a_scalar_mass():
    r = D.solve(D.rhs_scaled_decay, 0.0, 2.0, [1.0], 1e-6, 1e-8, mass=[[2.0]])
    assert r.status == M.SUCCESS
    err = abs(r.y_end[0] - math.exp(-1.0))
    print("2 y' = -y:", err)
    assert err <= 1.29e-7   # 10 x the measured 1.29e-8


def test_a_dense_non_singular_mass():
    """M y' = -M y with M = [[2, 1], [1, 2]]: y = y0 exp(-t)"""
    f = lambda x, y: [-(2.0 * y[0] + y[1]), -(y[0] + 2.0 * y[1])]
    r = D.solve(f, 0.0, 2.0, [1.0, -0.5], 1e-6, 1e-8, mass=[[2.0, 1.0], [1.0, 2.0]])
    assert r.status == M.SUCCESS
    err = max_err(r.y_end, [math.exp(-2.0), -0.5 * math.exp(-2.0)])
    print("dense M:", err)
    assert err <= 1.12e-7   # 10 x the measured 1.12e-8


def test_the_semi_explicit_index_1_system():
    """y1' = -y1 + y2, 0 = y2 - sin t, y(0) = 0: y1 = (sin t - cos t + exp(-t)) / 2"""
    r = D.solve(D.rhs_semi_explicit, 0.0, 2.0, [0.0, 0.0], 1e-6, 1e-8, mass=[[1.0, 0.0], [0.0, 0.0]])
    assert r.status == M.SUCCESS
    err = max_err(r.y_end, [0.5 * (math.sin(2.0) - math.cos(2.0) + math.exp(-2.0)), math.sin(2.0)])
    print("semi-explicit:", err)
    assert err <= 3.56e-7   # 10 x the measured 3.56e-8


Y0_PEND = [1.0, 0.0, 0.0, 0.0, 0.0]


def test_the_pendulum_in_index_2_form(pend_truth):
    r = D.solve(D.rhs_pendulum_index2, 0.0, 2.0, Y0_PEND, 1e-6, 1e-6, mass=D.MASS_PENDULUM, nind1=4, nind2=1, nind3=0)
    assert r.status == M.SUCCESS and r.naccpt == 24
    e_pv, e_lam = max_err(r.y_end[:4], pend_truth[:4]), abs(r.y_end[4] - pend_truth[4])
    print("pendulum index 2: p, v", e_pv, "lam", e_lam)
    assert e_pv <= 4.93e-6    # 10 x the measured 4.93e-7
    assert e_lam <= 8.47e-6   # 10 x the measured 8.47e-7


def test_the_pendulum_in_index_3_form(pend_truth):
    r = D.solve(D.rhs_pendulum_index3, 0.0, 2.0, Y0_PEND, 1e-6, 1e-6, mass=D.MASS_PENDULUM, nind1=2, nind2=2, nind3=1, first_step=1e-3)
    assert r.status == M.SUCCESS and r.naccpt == 34
    e_p, e_v, e_lam = max_err(r.y_end[:2], pend_truth[:2]), max_err(r.y_end[2:4], pend_truth[2:4]), abs(r.y_end[4] - pend_truth[4])
    print("pendulum index 3: p", e_p, "v", e_v, "lam", e_lam)
    assert e_p <= 8.2e-6      # 10 x the measured 8.2e-7
    assert e_v <= 1.72e-4     # 10 x the measured 1.72e-5
    assert e_lam <= 1.87e-2   # 10 x the measured 1.87e-3


@pytest.mark.parametrize("tol", [1e-4, 1e-6])
def test_index_2_with_the_pure_ode_partition_does_not_succeed(tol):
    r = D.solve(D.rhs_pendulum_index2, 0.0, 2.0, Y0_PEND, tol, tol, mass=D.MASS_PENDULUM, nind1=5, nind2=0, nind3=0)
    assert r.status == M.STEP_TOO_SMALL
    ok = D.solve(D.rhs_pendulum_index2, 0.0, 2.0, Y0_PEND, tol, tol, mass=D.MASS_PENDULUM, nind2=1)   # nind1 inferred
    assert ok.status == M.SUCCESS


def test_the_index_3_pendulum_restarts_at_tolerance_1e_4():
    r = D.solve(D.rhs_pendulum_index3, 0.0, 2.0, Y0_PEND, 1e-4, 1e-4, mass=D.MASS_PENDULUM, nind1=2, nind2=2, nind3=1, first_step=1e-3)
    assert r.status == M.SUCCESS and r.n_restart == 1


def test_partition_rules():
    assert D.partition(5) == (5, 0, 0)
    assert D.partition(5, None, 1, None) == (4, 1, 0)
    assert D.partition(5, None, 2, 1) == (2, 2, 1)
    assert D.partition(5, None, 2, 3) == (0, 2, 3)
    assert D.partition(5, 2, 2, 1) == (2, 2, 1)
    assert D.partition(5, 5, None, None) == (5, 0, 0)
    for bad in ((None, 3, 3), (4, None, None), (5, 1, None), (2, 2, 2), (None, -1, None), (-1, 3, 3)):
        with pytest.raises(D.InvalidDAEPartition):
            D.partition(5, *bad)
