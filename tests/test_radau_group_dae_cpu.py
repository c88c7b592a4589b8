"""Radau IIA(5) for M y' = f at 8 < n <= 64 (``DeviceIVP(..., mass_col=True)`` / IVP_RHS_HAS_MASS_COL), the part that needs
no device: the constant and the refusals of the front end, which come before anything is compiled, and the soundness IN THE
MODEL (tests/radau_dae_model.py) of the stacked pendulum problems tests/test_gpu_radau_group_dae.py runs on the device.

The stacked problems are k uncoupled planar pendulums in one state vector, index-1 variables first.  Each pendulum starts
on the orbit of tests/test_radau_dae_model_cpu.py's `pendulum_truth` (released at rest at angle 0) but at its own time
tau_q, hence its own angle (tests/radau_group_dae_problems.py: `orbit` and the phases); at the end it is held against
pendulum_truth(tau_q + t1) with the bounds that file uses for the single pendulum at the same tolerance (1e-6)."""
import os
import re

import pytest

import ivp_amd
from ivp_amd import api
from tests import radau_dae_model as D
from tests import radau_group_dae_problems as P
from tests import radau_model as M
from tests.test_radau_dae_model_cpu import max_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "__device__ double ode_comp(int i, double x, const double* y, const double* p) { return -y[i]; }\n" + P.identity_mass_source()


def test_the_flag_is_16_in_the_header_and_in_python():
    hdr = open(os.path.join(ROOT, "include", "ivp_hip.h")).read()
    assert re.search(r"^#define\s+IVP_RHS_HAS_MASS_COL\s+16u\s*$", hdr, re.M)
    assert re.search(r"^#define\s+IVP_RHS_HAS_MASS\s+4u\s*$", hdr, re.M)
    assert api.RHS_HAS_MASS_COL == 16 and api.RHS_HAS_MASS == 4


@pytest.mark.parametrize("n, kw, word", [
    (8, {}, "8 < n <= 64"),
    (5, {}, "mass=True"),
    (65, {}, "8 < n <= 64"),
    (10, {"events": [ivp_amd.EventConfig()]}, "events"),
    (10, {"mass": True}, "mass=True"),          # mass=True keeps its own check, n <= 8, which comes first
    (5, {"mass": True}, "one mass hook"),
    (10, {"jac_sparsity": ([0] * 11, [])}, "jac_sparsity"),
    (10, {"jac_sparsity": ([0] * 11, []), "jac_storage": "banded"}, "banded"),
])
def test_mass_col_is_refused_with_a_value_error_before_anything_is_compiled(n, kw, word, monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("the refusal must come before a context is asked for")
    monkeypatch.setattr(api, "default_context", no_context)
    with pytest.raises(ValueError) as e:
        ivp_amd.DeviceIVP(SRC, n, mass_col=True, **kw)
    assert word in str(e.value)


def test_mass_true_is_still_refused_beyond_n_8(monkeypatch):
    monkeypatch.setattr(api, "default_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("no context")))
    with pytest.raises(ValueError) as e:
        ivp_amd.DeviceIVP(SRC, 9, mass=True)
    assert "n <= 8" in str(e.value)


# ---- the stacked pendulums in the model -------------------------------------------------------------------------------------

@pytest.mark.parametrize("taus", [P.TAUS_INDEX2_K2, P.TAUS_INDEX2_K4], ids=["n10", "n20"])
def test_stacked_pendulums_in_index_2_form(taus):
    k = len(taus)
    y0 = P.pend2_state([P.orbit(tau) for tau in taus])
    r = D.solve(P.pend2_rhs(k), 0.0, 2.0, y0, 1e-6, 1e-6, mass=P.pend_mass(k), nind1=4 * k, nind2=k, nind3=0)
    assert r.status == M.SUCCESS
    for q, got in enumerate(P.pend2_split(k, r.y_end)):
        want = P.orbit(taus[q] + 2.0)
        e_pv, e_lam = max_err(got[:4], want[:4]), abs(got[4] - want[4])
        print("stacked index 2, pendulum", q, "of", k, ": p, v", e_pv, "lam", e_lam)
        assert e_pv <= 4.93e-6    # the single pendulum's bounds at this tolerance (tests/test_radau_dae_model_cpu.py)
        assert e_lam <= 8.47e-6


def test_stacked_pendulums_in_index_3_form():
    taus = P.TAUS_INDEX3_K2
    k = len(taus)
    y0 = P.pend3_state([P.orbit(tau) for tau in taus])
    r = D.solve(P.pend3_rhs(k), 0.0, 2.0, y0, 1e-6, 1e-6, mass=P.pend_mass(k), nind1=2 * k, nind2=2 * k, nind3=k, first_step=1e-3)
    assert r.status == M.SUCCESS
    for q, got in enumerate(P.pend3_split(k, r.y_end)):
        want = P.orbit(taus[q] + 2.0)
        e_p, e_v, e_lam = max_err(got[:2], want[:2]), max_err(got[2:4], want[2:4]), abs(got[4] - want[4])
        print("stacked index 3, pendulum", q, ": p", e_p, "v", e_v, "lam", e_lam)
        assert e_p <= 8.2e-6      # the single pendulum's bounds at this tolerance
        assert e_v <= 1.72e-4
        assert e_lam <= 1.87e-2


def test_the_stacked_index_3_pendulums_released_at_rest_restart_at_tolerance_1e_4():
    """the restart case of tests/test_gpu_radau_group_dae.py (the orbit phases above take none at any tolerance tried)"""
    k = 2
    y0 = P.pend3_state([P.pend_at_rest(0.1), P.pend_at_rest(0.2)])
    r = D.solve(P.pend3_rhs(k), 0.0, 2.0, y0, 1e-4, 1e-4, mass=P.pend_mass(k), nind1=2 * k, nind2=2 * k, nind3=k, first_step=1e-3)
    assert r.status == M.SUCCESS and r.n_restart == 1
    for got in P.pend3_split(k, r.y_end):   # still on the circle, to the tolerance's order
        assert abs(got[0] * got[0] + got[1] * got[1] - 1.0) < 1e-3


def test_stacked_pendulums_at_rest_fail_under_the_pure_ode_partition_unless_the_constraints_are_index_1():
    """the mixed batch of tests/test_gpu_radau_group_dae.py: p[0] selects the constraint per trajectory"""
    k = 2
    y0 = P.pend2_state([P.pend_at_rest(0.1), P.pend_at_rest(0.4)])
    bad = D.solve(P.pend2_rhs(k, select=1.0), 0.0, 2.0, y0, 1e-6, 1e-6, mass=P.pend_mass(k), nind1=5 * k, nind2=0, nind3=0)
    good = D.solve(P.pend2_rhs(k, select=0.0), 0.0, 2.0, y0, 1e-6, 1e-6, mass=P.pend_mass(k), nind1=5 * k, nind2=0, nind3=0)
    assert bad.status == M.STEP_TOO_SMALL and good.status == M.SUCCESS


def test_one_stacked_pendulum_state_equals_the_single_pendulum_bit_for_bit():
    """k = 1 of the stacked forms is the 5-state pendulum of tests/radau_dae_model.py: same operations, same results"""
    y0 = [1.0, 0.0, 0.0, 0.0, 0.0]
    a = D.solve(P.pend2_rhs(1), 0.0, 2.0, y0, 1e-6, 1e-6, mass=P.pend_mass(1), nind1=4, nind2=1, nind3=0)
    b = D.solve(D.rhs_pendulum_index2, 0.0, 2.0, y0, 1e-6, 1e-6, mass=D.MASS_PENDULUM, nind1=4, nind2=1, nind3=0)
    assert a.y_end == b.y_end and (a.nstep, a.nfev, a.naccpt, a.nrejct) == (b.nstep, b.nfev, b.naccpt, b.nrejct)
    a = D.solve(P.pend3_rhs(1), 0.0, 2.0, y0, 1e-6, 1e-6, mass=P.pend_mass(1), nind1=2, nind2=2, nind3=1, first_step=1e-3)
    b = D.solve(D.rhs_pendulum_index3, 0.0, 2.0, y0, 1e-6, 1e-6, mass=D.MASS_PENDULUM, nind1=2, nind2=2, nind3=1, first_step=1e-3)
    assert a.y_end == b.y_end and (a.nstep, a.nfev, a.naccpt, a.nrejct) == (b.nstep, b.nfev, b.naccpt, b.nrejct)


def test_identity_mass_at_n_9_equals_radau_model_bit_for_bit():
    n = 9
    a = [[1e-3 * (1 + ((3 * i + 5 * j) % 7)) for j in range(n)] for i in range(n)]
    for i in range(n):
        a[i][i] = -1.0 - 0.25 * i
        if i % 2:
            a[i][i - 1] = 200.0
    y0 = [1.0, 0.5, -0.5, 0.25, 0.0, 1e-3, -1.0, 2.0, 1.0]
    plain = M.solve(M.rhs_dense_linear(a), 0.0, 0.5, list(y0), 1e-6, 1e-8)
    ident = D.solve(M.rhs_dense_linear(a), 0.0, 0.5, list(y0), 1e-6, 1e-8, mass=P.identity(n))
    assert plain.status == ident.status == M.SUCCESS and plain.njev > 1
    for k in ("t_end", "h_next", "nfev", "njev", "nlu", "nstep", "naccpt", "nrejct"):
        assert getattr(plain, k) == getattr(ident, k), k
    assert [v.hex() for v in plain.y_end] == [v.hex() for v in ident.y_end]
    assert len(plain.t) == len(ident.t) and all([v.hex() for v in p] == [v.hex() for v in q] for p, q in zip(plain.y, ident.y))
