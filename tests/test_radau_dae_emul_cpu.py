"""The Radau kernel bodies of ivp_amd/csrc/radau_core.h for problems WITH A MASS MATRIX (HasMass: M y' = f and the DAE index
sets), run on the CPU by tests/host_emul_dae with the GPU launch loop's init -> chunk -> chunk schedule, against
tests/radau_dae_model.py BIT FOR BIT: status, t_end, h_next, y_end and the six counters of every trajectory, and every
recorded output.  No tolerance anywhere, no GPU.

Chunk lengths 1, 7 and unbounded: `scal`, `hhfac` and M cross a launch boundary after every attempt, in the middle of
rejection sequences (each test that claims one asserts it on the model's counters)."""
import math

import numpy as np
import pytest

from tests import radau_dae_model as D
from tests import radau_model as M
from tests.host_emul_dae import emul_dae as E

UNBOUNDED = 0xFFFFFFFF
CHUNKS = (1, 7, UNBOUNDED)
COUNTERS = ("nfev", "njev", "nlu", "nstep", "naccpt", "nrejct")
RT, AT = 1e-6, 1e-8
Y0_PEND = [1.0, 0.0, 0.0, 0.0, 0.0]


def same(a, b):
    a, b = float(a), float(b)
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def same_vec(a, b):
    return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))


# ---- the functors of emul_dae.cpp, restated ---------------------------------------------------------------------------------
def f_scalar(p1):
    return lambda x, y: [M.fdiv(p1, 1.0 + x * x) - y[0]]


def f_semi(x, y):
    return [-y[0] + y[1], y[1] - M.fdiv(x, 1.0 + x * x)]


def lin_matrix(n):
    """tests/test_radau_emul_cpu.py's dense test matrix"""
    a = [[1e-3 * (1 + ((3 * i + 5 * j) % 7)) for j in range(n)] for i in range(n)]
    for i in range(n):
        a[i][i] = -1.0 - 0.25 * i
        if i % 2:
            a[i][i - 1] = 200.0
    return a


def full_mass(n):
    """a full, well-conditioned mass matrix: a growing diagonal, entries of 0.01 .. 0.05 (both signs) everywhere else"""
    return [[(1.0 + 0.125 * r) if r == c else (0.01 * (1 + (r + 2 * c) % 5)) * (-1.0 if (r + c) % 3 == 0 else 1.0) for c in range(n)]
            for r in range(n)]


def flat(m):
    return [v for row in m for v in row]


def check(res, b, m, tag, t_eval=False, log=0, dense=False):
    got = dict(status=int(res["status"][b]), **{k: int(res[k][b]) for k in COUNTERS})
    want = dict(status=m.status, **{k: getattr(m, k) for k in COUNTERS})
    assert got == want, (tag, got, want)
    assert same(res["t_end"][b], m.t_end), (tag, "t_end", float(res["t_end"][b]), m.t_end)
    assert same(res["h_next"][b], m.h_next), (tag, "h_next", float(res["h_next"][b]), m.h_next)
    assert same_vec(res["y_end"][:, b], m.y_end), (tag, "y_end", list(res["y_end"][:, b]), m.y_end)
    if t_eval:
        k = int(res["n_filled"][b])
        assert k == len(m.t) and [int(v) for v in res["eval_idx"][:k, b]] == m.eval_idx, (tag, k, len(m.t))
        for q in range(k):
            assert same_vec(res["y_eval"][q, :, b], m.y[q]), (tag, "t_eval sample", q)
    if log:
        assert int(res["n_log"][b]) == len(m.t), (tag, int(res["n_log"][b]), len(m.t))
        for q in range(min(log, len(m.t))):
            assert same(res["t_log"][q, b], m.t[q]) and same_vec(res["y_log"][q, :, b], m.y[q]), (tag, "log record", q)
    if dense:
        assert int(res["n_seg"][b]) == len(m.segs) == m.naccpt, (tag, int(res["n_seg"][b]), len(m.segs))
        for q, (cont, xold, h) in enumerate(m.segs[:log]):
            assert same(res["seg_xold"][q, b], xold) and same(res["seg_h"][q, b], h) and same_vec(res["seg_cont"][q, :, b], cont), (tag, "segment", q)


def both(rhs, fs, masses, y0s, t0, t1, params=None, rtol=RT, atol=AT, nind=(None, None, None), chunks=CHUNKS, t_eval=None, max_log=0,
         dense_output=False, radau=None, **kw):
    """Trajectory b: model right-hand side fs[b], mass matrix masses[b], initial state y0s[b], parameter column params[b].
    The models once, the kernel body at every chunk length; returns the models."""
    n = len(y0s[0])
    _, i2, i3 = D.partition(n, *nind)
    mkw = dict(kw)
    if t_eval is not None:
        mkw["t_eval"] = list(t_eval)
    if dense_output:
        mkw["dense_output"] = True
    models = [D.solve(f, t0, t1, list(y0), rtol, atol, settings=M.Settings(**(radau or {})), mass=ms, nind1=nind[0], nind2=nind[1],
                      nind3=nind[2], **mkw) for f, ms, y0 in zip(fs, masses, y0s)]
    par = None if params is None else np.array(params, dtype=np.float64).T.copy()
    y0 = np.array(y0s, dtype=np.float64).T.copy()
    for chunk in chunks:
        res = E.solve_batch(rhs, y0, par, t0, t1, rtol=rtol, atol=atol, nind2=i2, nind3=i3, chunk=chunk, t_eval=t_eval, max_log=max_log,
                            dense_output=dense_output, radau=radau, **kw)
        for b, m in enumerate(models):
            tag = f"{rhs} trajectory {b} chunk {chunk}"
            assert same_vec(res["mass"][:, b], flat(masses[b])), (tag, "the persistent mass matrix")
            check(res, b, m, tag, t_eval is not None, max_log if t_eval is None else 0, dense_output)
    return models


# ---- n = 1 ------------------------------------------------------------------------------------------------------------------
def test_n1_algebraic_equation_and_a_mass_per_trajectory():
    p0 = [0.0, 2.0, 0.5, -0.0, 1.0]
    ms = both("scalar", [f_scalar(1.0)] * 5, [[[v]] for v in p0], [[1.0]] * 5, 0.0, 2.0, params=[[v, 1.0] for v in p0])
    assert all(m.status == M.SUCCESS for m in ms)
    assert len({tuple(m.y_end) for m in ms[:3]}) == 3   # the mass is read per trajectory


# ---- n = 2 ------------------------------------------------------------------------------------------------------------------
SEMI = [[1.0, 0.0], [0.0, 0.0]]
DENSE2 = [[2.0, 1.0], [1.0, 2.0]]


def test_n2_semi_explicit_and_dense_mass_forward_with_dense_segments():
    ms = both("semi", [f_semi, f_semi], [SEMI, DENSE2], [[0.0, 0.0], [1.0, -0.5]], 0.0, 2.0, params=[flat(SEMI), flat(DENSE2)],
              max_log=64, dense_output=True)
    assert all(m.status == M.SUCCESS for m in ms) and any(m.nrejct > 0 for m in ms)


def test_n2_backward_integration():
    ms = both("semi", [f_semi, f_semi], [SEMI, DENSE2], [[0.3, 0.4], [1.0, -0.5]], 2.0, 0.0, params=[flat(SEMI), flat(DENSE2)])
    assert all(m.status == M.SUCCESS and m.t_end == 0.0 for m in ms)


# ---- n = 3 ------------------------------------------------------------------------------------------------------------------
def test_n3_robertson_dae_with_per_component_tolerances_and_t_eval():
    grid = [0.0, 1e-3, 0.4, 4.0, 39.0, 40.0]
    ms = both("robertson", [D.rhs_robertson_dae], [D.MASS_ROBERTSON], [[1.0, 0.0, 0.0]], 0.0, 40.0, rtol=[1e-6, 1e-5, 1e-6],
              atol=[1e-10, 1e-12, 1e-9], t_eval=grid)
    assert ms[0].status == M.SUCCESS and ms[0].nrejct > 0 and len(ms[0].t) == len(grid)


# ---- n = 5: the index sets ----------------------------------------------------------------------------------------------------
def test_n5_pendulum_index_2_rejections_cross_every_launch_boundary():
    """tolerance 1e-4: 14 rejections, 7 of them the Newton dyth exit -- at chunk length 1 every one of them is followed by a
    launch boundary, so the accumulated divisions of scal and the hhfac of the rejection travel through memory"""
    ms = both("pendulum2", [D.rhs_pendulum_index2] * 2, [D.MASS_PENDULUM] * 2, [Y0_PEND, [0.8, 0.6, 0.0, 0.0, -0.6]], 0.0, 2.0, rtol=1e-4,
              atol=1e-4, nind=(4, 1, 0), max_log=16)
    assert all(m.status == M.SUCCESS for m in ms)
    assert ms[0].n_dyth >= 5 and ms[0].nrejct - ms[0].n_dyth >= 5
    assert len(ms[0].t) > 16   # the bounded log overflows: the count runs on


def test_n5_pendulum_index_2_at_tolerance_1e_6_with_the_inferred_partition():
    ms = both("pendulum2", [D.rhs_pendulum_index2], [D.MASS_PENDULUM], [Y0_PEND], 0.0, 2.0, rtol=1e-6, atol=1e-6, nind=(None, 1, None))
    assert ms[0].status == M.SUCCESS and ms[0].naccpt == 24


def test_n5_pendulum_index_3_restart():
    """the index-3 pendulum's `h *= 0.5` restart (the model shows one at tolerance 1e-4): hhfac = 0.5 is squared into scal"""
    ms = both("pendulum3", [D.rhs_pendulum_index3], [D.MASS_PENDULUM], [Y0_PEND], 0.0, 2.0, rtol=1e-4, atol=1e-4, nind=(2, 2, 1), first_step=1e-3)
    assert ms[0].status == M.SUCCESS and ms[0].n_restart == 1 and 0.5 in ms[0].hhfacs


def test_n5_pendulum_index_3_at_tolerance_1e_6():
    ms = both("pendulum3", [D.rhs_pendulum_index3], [D.MASS_PENDULUM], [Y0_PEND], 0.0, 2.0, rtol=1e-6, atol=1e-6, nind=(2, 2, 1), first_step=1e-3)
    assert ms[0].status == M.SUCCESS and ms[0].naccpt == 34


@pytest.mark.parametrize("tol", [1e-4, 1e-6])
def test_n5_wrong_partition_ends_in_step_size_too_small(tol):
    ms = both("pendulum2", [D.rhs_pendulum_index2], [D.MASS_PENDULUM], [Y0_PEND], 0.0, 2.0, rtol=tol, atol=tol, nind=(5, 0, 0))
    assert ms[0].status == M.STEP_TOO_SMALL


# ---- M y' = A y at every width ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_dense_linear_system_with_a_full_mass_matrix(n):
    a, ms_ = lin_matrix(n), full_mass(n)
    y0s = [[1.0 + 0.25 * i for i in range(n)], [(-1.0) ** i * (0.5 + 0.125 * i) for i in range(n)]]
    ms = both(f"lin{n}", [M.rhs_dense_linear(a)] * 2, [ms_] * 2, y0s, 0.0, 1.5, params=[flat(a) + flat(ms_)] * 2, max_log=8)
    assert all(m.status == M.SUCCESS for m in ms)
    if n == 8:
        assert ms[0].pivots, "rows are exchanged in the factorisations"


def test_identity_mass_gives_the_bits_of_the_plain_radau_model():
    a = lin_matrix(5)
    ident = [[1.0 if r == c else 0.0 for c in range(5)] for r in range(5)]
    y0 = [1.0 + 0.25 * i for i in range(5)]
    ms = both("lin5", [M.rhs_dense_linear(a)], [ident], [y0], 0.0, 1.5, params=[flat(a) + flat(ident)])
    plain = M.solve(M.rhs_dense_linear(a), 0.0, 1.5, y0, RT, AT)
    assert same_vec(ms[0].y_end, plain.y_end) and ms[0].nfev == plain.nfev and same(ms[0].h_next, plain.h_next)


def test_zero_mass_with_a_singular_jacobian_runs_through_to_singular_matrix():
    """M = 0 and a Jacobian with a zero row: E1 = -J is singular at every step size, six restarts end the solve"""
    a = [[-1.0, 0.5, 0.0], [0.0, 0.0, 0.0], [0.25, 0.0, -2.0]]
    zero = [[0.0] * 3 for _ in range(3)]
    ms = both("lin3", [M.rhs_dense_linear(a)], [zero], [[1.0, 2.0, 3.0]], 0.0, 1.0, params=[flat(a) + flat(zero)])
    assert ms[0].status == M.SINGULAR_MATRIX and ms[0].n_restart_real == 6 and ms[0].nstep == 0 and ms[0].nlu == 6


# ---- the early exits still define M -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t1", [1.0, float("nan")])
def test_degenerate_and_nan_intervals_write_the_mass_matrix(t1):
    par = np.array([flat(SEMI), flat(DENSE2)], dtype=np.float64).T.copy()
    res = E.solve_batch("semi", np.array([[0.0, 1.0], [0.0, -0.5]]), par, 1.0, t1, chunk=7)
    assert [int(v) for v in res["status"]] == ([0, 0] if t1 == 1.0 else [3, 3])
    assert same_vec(res["mass"][:, 0], flat(SEMI)) and same_vec(res["mass"][:, 1], flat(DENSE2))
    assert int(res["chunks"]) == 0
