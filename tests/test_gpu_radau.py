"""Radau IIA(5) on the device (ivp_amd.Radau -> ivp_radau_solve*() -> radau_core.h) against the CPU model
tests/radau_model.py, BIT FOR BIT: status, t_end, y_end, h_next and the six counters of every trajectory, and every
recorded output.  No tolerance anywhere except the two comparisons with the SciPy truth, which carry the bounds of the BDF
pins for the same problems.

The model is judged on its own in tests/test_radau_cpu.py.  Every test that claims a branch asserts on the MODEL's
counters that the inputs take it.  Model runs are cached per input and shared between tests.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import Options, Radau
from tests import radau_model as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = json.load(open(os.path.join(ROOT, "tests", "golden", "scipy_stiff_truth.json")))["truth"]
MEMBERS = ("status", "t_end", "h_next", "nfev", "njev", "nlu", "nstep", "naccpt", "nrejct")
RT, AT = 1e-6, 1e-8

_CACHE = {}


def model(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def same(a, b):
    """bit equality of two floats, NaN equal to NaN"""
    a, b = float(a), float(b)
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def same_vec(a, b):
    return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))


def gpu_row(r, b):
    d = {k: (float(_np(getattr(r, k))[b]) if k in ("t_end", "h_next") else int(_np(getattr(r, k))[b])) for k in MEMBERS}
    d["y_end"] = [float(v) for v in _np(r.y_end)[:, b]]
    return d


def model_row(m):
    d = {k: getattr(m, k) for k in MEMBERS}
    d["y_end"] = list(m.y_end)
    return d


def assert_rows(r, models, what=""):
    bad = []
    for b, m in enumerate(models):
        g, w = gpu_row(r, b), model_row(m)
        ok = all(g[k] == w[k] for k in MEMBERS if k not in ("t_end", "h_next")) and same(g["t_end"], w["t_end"]) and \
            same(g["h_next"], w["h_next"]) and same_vec(g["y_end"], w["y_end"])
        if not ok:
            bad.append((b, g, w))
    assert not bad, f"{what}: {len(bad)} of {len(models)} trajectories differ from the model; first: {bad[0]}"


# ---- inputs -----------------------------------------------------------------------------------------------------------

def vdp_eps_batch(B=67, seed=2024):
    rng = np.random.default_rng(seed)
    eps = np.exp(rng.uniform(np.log(5e-4), np.log(2e-3), B))
    y0 = np.stack([2.0 + 0.1 * rng.standard_normal(B), 0.1 * rng.standard_normal(B)])
    return y0, eps[None, :].copy()


def vdp_eps_models(B, **kw):
    y0, eps = vdp_eps_batch()
    key = tuple(sorted((k, repr(v)) for k, v in kw.items()))
    return [model(("vdp_eps", b, key), lambda b=b: M.solve(M.rhs_vdp_eps(float(eps[0, b])), 0.0, 2.0, [float(v) for v in y0[:, b]], RT, AT, **kw))
            for b in range(B)]


OPT = Options(rtol=RT, atol=AT)


# ---- 1. one wave plus a tail ------------------------------------------------------------------------------------------
# (of trajectories, not of lanes: the launch loop spreads a batch this small over the CUs, ONE trajectory per wavefront --
# lpw = ceil(67 / cus) = 1 on an MI355X -- so neither this test nor any other in this file has two trajectories in one
# wavefront.  tests/test_gpu_wave_density.py runs these inputs with 2, 7 and 64 trajectories per wavefront.)

def test_one_wave_plus_a_tail_of_stiff_van_der_pol():
    y0, eps = vdp_eps_batch()
    models = vdp_eps_models(67)
    assert any(m.n_reuse > 0 for m in models) and any(m.nrejct > 0 for m in models)
    assert len({tuple(m.newton_counts[:40]) for m in models}) > 1   # Newton iteration counts differ between the trajectories
    r = Radau().solve_batch(ivp_amd.StiffVanDerPol(), 0.0, 2.0, y0, eps, OPT)
    assert_rows(r, models, "stiff VdP, B = 67")
    assert all(m.status == 0 for m in models)


# ---- 2. the Newton loop's dyth >= 1 exit ------------------------------------------------------------------------------

def test_newton_exit_path_on_van_der_pol_mu_1000():
    y0 = np.array([[2.0, 2.0 + 1e-3, 2.0 - 1e-3, 1.99, 2.01], [0.0, 1e-3, -1e-3, 0.0, 0.01]])
    mu = np.full((1, 5), 1000.0)
    models = [model(("vdp1000", b), lambda b=b: M.solve(M.rhs_vdp(1000.0), 0.0, 3000.0, [float(v) for v in y0[:, b]], 1e-4, 1e-6)) for b in range(5)]
    assert all(m.n_dyth > 0 for m in models)
    r = Radau().solve_batch(ivp_amd.VanDerPol(), 0.0, 3000.0, y0, mu, Options(rtol=1e-4, atol=1e-6))
    assert_rows(r, models, "VdP mu = 1000")
    assert np.abs(_np(r.y_end)[:, 0] - TRUTH["vdp_mu1000_t3000"]).max() < 1e-2


# ---- 3. every N that gets instantiated --------------------------------------------------------------------------------

def test_n1_exponential_decay():
    k = np.array([[0.5, 2.0, 300.0]])
    models = [M.solve(M.rhs_decay(float(k[0, b])), 0.0, 3.0, [1.0], RT, AT) for b in range(3)]
    r = Radau().solve_batch(ivp_amd.ExponentialDecay(), 0.0, 3.0, np.ones((1, 3)), k, OPT)
    assert_rows(r, models, "decay")


@pytest.mark.parametrize("analytic", [False, True])
def test_n3_robertson_with_forward_differences_and_with_the_analytic_jacobian(analytic):
    m = M.solve(M.rhs_robertson, 0.0, 1e5, [1.0, 0.0, 0.0], RT, AT, jac=M.jac_robertson if analytic else None)
    f = ivp_amd.RobertsonJac() if analytic else ivp_amd.Robertson()
    r = Radau().solve_batch(f, 0.0, 1e5, np.array([[1.0], [0.0], [0.0]]), None, OPT)
    assert_rows(r, [m], "Robertson")
    assert m.status == 0 and m.njev > 1
    # the difference quotients' right-hand sides are not in nfev: both Jacobians count 1 + 3 per Newton pass + 1 per
    # accepted step + 1 per refinement
    assert m.nfev == 1 + 3 * sum(m.newton_counts) + m.naccpt + m.n_refine


def test_n6_cr3bp():
    rng = np.random.default_rng(6)
    y0 = np.array([0.994, 0.0, 0.0, 0.0, -2.0015851063790825, 0.0])[:, None] + 1e-3 * rng.standard_normal((6, 4))
    mu = ivp_amd.CR3BP().mu
    models = [M.solve(M.rhs_cr3bp(mu), 0.0, 0.5, [float(v) for v in y0[:, b]], RT, AT) for b in range(4)]
    r = Radau().solve_batch(ivp_amd.CR3BP(), 0.0, 0.5, y0, None, OPT)
    assert_rows(r, models, "CR3BP")


def _a8():
    """A fixed dense 8 x 8 matrix: a negative diagonal, 200 at (1, 0), (3, 2), (5, 4), (7, 6) (one-way couplings inside four
    pairs: the eigenvalues stay near the diagonal, the solution is smooth and the steps grow), entries of 1e-3 .. 7e-3
    everywhere else.  Once U1 / h + 1 < 200 the coupling is the pivot of its column in E1, and likewise in E2."""
    a = [[1e-3 * (1 + ((3 * i + 5 * j) % 7)) for j in range(8)] for i in range(8)]
    for i in range(8):
        a[i][i] = -1.0 - 0.25 * i
        if i % 2:
            a[i][i - 1] = 200.0
    return a


def _a8_source(with_jac):
    a = _a8()
    lit = lambda v: float(v).hex()
    src = "__device__ void ode(double x, const double* y, double* d, const double* p) {\n"
    for i in range(8):
        src += f"  d[{i}] = " + " + ".join(f"{lit(a[i][j])} * y[{j}]" for j in range(8)) + ";\n"
    src += "}\n"
    if with_jac:
        src += "__device__ void jac(double x, const double* y, double* j, const double* p) {\n"
        src += "".join(f"  j[{i * 8 + k}] = {lit(a[i][k])};\n" for i in range(8) for k in range(8)) + "}\n"
    return src


@pytest.mark.parametrize("with_jac", [True, False])
def test_n8_hiprtc_linear_system_exchanges_rows_in_both_factorisations(with_jac):
    a = _a8()

    def f(x, y):
        out = []
        for i in range(8):
            s = a[i][0] * y[0]
            for j in range(1, 8):
                s = s + a[i][j] * y[j]
            out.append(s)
        return out

    def jac(x, y, J):
        for i in range(8):
            for j in range(8):
                J[i][j] = a[i][j]

    y0 = [1.0, 0.5, -0.5, 0.25, 0.0, 1e-3, -1.0, 2.0]
    m = M.solve(f, 0.0, 5.0, y0, 1e-4, 1e-6, jac=jac if with_jac else None)
    assert any(p[0] == "real" for p in m.pivots) and any(p[0] == "complex" for p in m.pivots)
    prob = ivp_amd.DeviceIVP(_a8_source(with_jac), 8, jac=with_jac)
    r = Radau().solve_batch(prob, 0.0, 5.0, np.array(y0)[:, None], None, Options(rtol=1e-4, atol=1e-6))
    assert_rows(r, [m], "8 x 8 linear system")
    assert m.status == 0


# ---- 4. backward integration ------------------------------------------------------------------------------------------

def test_backward_integration():
    y0 = np.array([[1.0, 0.3], [0.0, -0.7]])
    models = [M.solve(M.rhs_sho, 1.0, -2.0, [float(v) for v in y0[:, b]], RT, AT) for b in range(2)]
    r = Radau().solve_batch(ivp_amd.SHO(), 1.0, -2.0, y0, None, OPT)
    assert_rows(r, models, "SHO backwards")
    assert all(m.status == 0 and m.t_end == -2.0 and m.h_next < 0.0 for m in models)


# ---- 5. chunk-length invariance (the persisted state) -----------------------------------------------------------------

@pytest.mark.parametrize("chunk", [1, 7, 0])
def test_chunk_length_does_not_change_a_bit(chunk):
    y0, eps = vdp_eps_batch()
    y0, eps = np.ascontiguousarray(y0[:, :16]), np.ascontiguousarray(eps[:, :16])
    models = vdp_eps_models(16)
    r = Radau().solve_batch(ivp_amd.StiffVanDerPol(), 0.0, 2.0, torch.as_tensor(y0, device=DEV), torch.as_tensor(eps, device=DEV),
                            Options(rtol=RT, atol=AT, chunk_attempts=chunk))
    assert_rows(r, models, f"chunk_attempts = {chunk}")


# ---- 6. outputs -------------------------------------------------------------------------------------------------------

def _out_problems():
    y0s = np.array([[1.0, 0.5, -0.3, 2.0, 0.0], [0.0, 0.5, 0.9, -1.0, 1.0]])
    y0v, epsv = vdp_eps_batch()
    return [("sho", ivp_amd.SHO(), None, y0s, lambda b: M.rhs_sho, 3.0),
            ("vdp", ivp_amd.StiffVanDerPol(), np.ascontiguousarray(epsv[:, :5]), np.ascontiguousarray(y0v[:, :5]),
             lambda b: M.rhs_vdp_eps(float(epsv[0, b])), 2.0)]


@pytest.mark.parametrize("which", [0, 1])
def test_shared_t_eval_grid(which):
    name, f, p, y0, rhs, t1 = _out_problems()[which]
    grid = [0.0, 0.1, 0.1 + 1e-13, 0.7, 1.5, t1, t1 + 0.5]   # t0, a pair closer than the tolerance, t1, a point outside
    models = [M.solve(rhs(b), 0.0, t1, [float(v) for v in y0[:, b]], RT, AT, t_eval=grid) for b in range(5)]
    r = Radau().solve_batch(f, 0.0, t1, y0, p, Options(rtol=RT, atol=AT, t_eval=grid))
    assert_rows(r, models, name)
    for b, m in enumerate(models):
        k = int(r.n_filled[b])
        assert k == len(m.t) == 6 and list(r.eval_idx[:k, b]) == m.eval_idx
        for q in range(k):
            assert same_vec(r.y_eval[q, :, b], m.y[q]), (b, q)


def test_per_trajectory_ragged_t_eval_grids():
    name, f, p, y0, rhs, t1 = _out_problems()[1]
    grids = [np.linspace(0.0, t1, 3 + 2 * b) if b != 2 else np.zeros(0) for b in range(5)]
    models = [M.solve(rhs(b), 0.0, t1, [float(v) for v in y0[:, b]], RT, AT, t_eval=list(grids[b])) for b in range(5)]
    r = Radau().solve_batch(f, 0.0, t1, y0, p, Options(rtol=RT, atol=AT, t_eval_per_trajectory=grids))
    assert_rows(r, models, name)
    for b, m in enumerate(models):
        idx, y = r.eval_of(b)
        assert list(idx) == m.eval_idx and len(y) == len(m.y)
        for q in range(len(y)):
            assert same_vec(y[q], m.y[q]), (b, q)


@pytest.mark.parametrize("which", [0, 1])
def test_bounded_step_log_with_one_trajectory_that_overflows(which):
    name, f, p, y0, rhs, t1 = _out_problems()[which]
    t1s = np.array([t1, 0.05 * t1, t1, t1, 0.05 * t1])   # two short trajectories fit, three overflow
    models = [M.solve(rhs(b), 0.0, float(t1s[b]), [float(v) for v in y0[:, b]], RT, AT) for b in range(5)]
    ml = max(len(models[1].t), len(models[4].t)) + 2
    assert any(len(m.t) > ml for m in models) and any(len(m.t) <= ml for m in models)
    r = Radau().solve_batch(f, 0.0, t1s, y0, p, Options(rtol=RT, atol=AT, max_log=ml))
    assert_rows(r, models, name)
    for b, m in enumerate(models):
        assert int(r.n_log[b]) == len(m.t)                       # the count runs on past the capacity
        for q in range(min(ml, len(m.t))):
            assert same(r.t_log[q, b], m.t[q]) and same_vec(r.y_log[q, :, b], m.y[q]), (b, q)


def _find_segment(segs, t, extrapolate):
    """ContinuousOutput::find_segment / find_segment_extrapolate (cont.rs:104-153) on the model's segments"""
    tol = 1e-12
    for cont, xold, h in segs:
        lo, hi = min(xold, xold + h), max(xold, xold + h)
        if lo - tol <= t <= hi + tol:
            return (cont, xold, h), 1
    if extrapolate and segs:
        first, last = segs[0], segs[-1]
        if t < min(first[1], first[1] + first[2]):
            return first, 2
        if t > max(last[1], last[1] + last[2]):
            return last, 2
    return None, 0


@pytest.mark.parametrize("which", [0, 1])
def test_dense_output_segments_and_their_evaluation_on_the_device(which):
    name, f, p, y0, rhs, t1 = _out_problems()[which]
    models = [M.solve(rhs(b), 0.0, t1, [float(v) for v in y0[:, b]], RT, AT, dense_output=True) for b in range(5)]
    ml = max(len(m.segs) for m in models) + 1
    r = Radau().solve_batch(f, 0.0, t1, y0, p, Options(rtol=RT, atol=AT, dense_output=True, max_log=ml))
    assert_rows(r, models, name)
    n = y0.shape[0]
    for b, m in enumerate(models):
        assert int(r.n_seg[b]) == len(m.segs) == m.naccpt
        for q, (cont, xold, h) in enumerate(m.segs):
            assert same(r.seg_xold[q, b], xold) and same(r.seg_h[q, b], h) and same_vec(r.seg_cont[q, :, b], cont), (b, q)
    # the segments as a CSR log on the device, evaluated by ivp_dense_eval_device(method = RADAU)
    counts = np.array([int(v) for v in r.n_seg])
    off = np.zeros(6, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    cont = np.concatenate([r.seg_cont[:counts[b], :, b] for b in range(5)])
    xold = np.concatenate([r.seg_xold[:counts[b], b] for b in range(5)])
    hh = np.concatenate([r.seg_h[:counts[b], b] for b in range(5)])
    ctx = ivp_amd.default_context(0)
    dense = ivp_amd.BatchContinuousOutput(ivp_amd.Method.RADAU, n, torch.as_tensor(off, device=DEV), torch.as_tensor(np.ascontiguousarray(cont), device=DEV),
                                          torch.as_tensor(xold, device=DEV), torch.as_tensor(hh, device=DEV), ivp_amd.FpMode.STRICT, ctx)
    grid = np.array([-0.25, 0.0, 1e-7, 0.3333, 0.5 * t1, t1, t1 + 0.125])   # before the span, inside, the ends, past the span
    for extrapolate in (False, True):
        y, found = dense(grid, extrapolate=extrapolate)
        y, found = _np(y), _np(found)
        for b, m in enumerate(models):
            for q, t in enumerate(grid):
                seg, kind = _find_segment(m.segs, float(t), extrapolate)
                assert int(found[q, b]) == kind, (b, q, extrapolate)
                if kind == 0:
                    assert np.isnan(y[q, :, b]).all()
                else:
                    assert same_vec(y[q, :, b], M.interpolate(float(t), *seg)), (b, q, extrapolate)
        assert (found[0] == (2 if extrapolate else 0)).all() and (found[-1] == (2 if extrapolate else 0)).all() and (found[3] == 1).all()
    # ... and the host ContinuousOutput built from one trajectory's segments
    co = ivp_amd.ContinuousOutput(ivp_amd.Method.RADAU, n, r.seg_cont[:counts[0], :, 0], r.seg_xold[:counts[0], 0], r.seg_h[:counts[0], 0])
    assert same_vec(co.evaluate(0.3333), M.interpolate(0.3333, *_find_segment(models[0].segs, 0.3333, False)[0]))


# ---- 7. failing and non-finite trajectories ---------------------------------------------------------------------------

def test_max_steps_gives_need_larger_nmax_with_the_models_step_count():
    y0, eps = vdp_eps_batch()
    y0, eps = np.ascontiguousarray(y0[:, :3]), np.ascontiguousarray(eps[:, :3])
    models = vdp_eps_models(3, max_steps=10)
    assert all(m.status == M.NEED_LARGER_NMAX and m.nstep == 11 for m in models)
    r = Radau().solve_batch(ivp_amd.StiffVanDerPol(), 0.0, 2.0, y0, eps, Options(rtol=RT, atol=AT, max_steps=10))
    assert_rows(r, models, "max_steps = 10")


def test_first_step_zero_is_invalid_step_size():
    with pytest.raises(ivp_amd.ConfigError) as e:
        Radau().solve_batch(ivp_amd.SHO(), 0.0, 1.0, np.array([[1.0], [0.0]]), None, Options(rtol=RT, atol=AT, first_step=0.0))
    assert e.value.code == -5


def test_first_step_is_taken_and_enforced_in_the_step_log():
    m = M.solve(M.rhs_sho, 0.0, 1.0, [1.0, 0.0], RT, AT, first_step=1e-3)
    s = Radau().solve(ivp_amd.SHO(), 0.0, 1.0, [1.0, 0.0], Options(rtol=RT, atol=AT, first_step=1e-3))
    assert same_vec(s.t, m.t) and all(same_vec(a, b) for a, b in zip(s.y, m.y)) and len(s.y) == len(m.y)
    assert m.t[1] == 1e-3 and (s.nfev, s.nstep, int(s.status)) == (m.nfev, m.nstep, m.status)


def test_finite_time_blow_up_ends_in_the_models_status():
    """y' = y^2, y(0) = 1 has its pole at t = 1: an ordinary numerical failure that ends in a status."""
    m = M.solve(lambda x, y: [y[0] * y[0]], 0.0, 2.0, [1.0], RT, AT)
    assert m.status != M.SUCCESS and m.t_end < 1.0 + 1e-6
    prob = ivp_amd.DeviceIVP("__device__ void ode(double x, const double* y, double* d, const double* p) { d[0] = y[0] * y[0]; }", 1)
    r = Radau().solve_batch(prob, 0.0, 2.0, np.ones((1, 1)), None, OPT)
    assert_rows(r, [m], "y' = y^2")


def test_nan_right_hand_side_in_one_lane_leaves_the_other_63_untouched():
    """At B = 64 the device runs one trajectory per wavefront (lpw = ceil(64 / cus) = 1), so the 63 are the NaN trajectory's
    neighbours in the batch and in the state arrays, not in its wavefront; tests/test_gpu_wave_density.py (radau_mixed) puts
    a NaN right-hand side into a full wavefront."""
    rng = np.random.default_rng(64)
    eps = np.exp(rng.uniform(np.log(2e-2), np.log(5e-2), 64))[None, :]
    y0 = np.stack([2.0 + 0.1 * rng.standard_normal(64), 0.1 * rng.standard_normal(64)])
    bad = 17
    eps[0, bad] = np.nan                                  # ((1 - y0^2) y1 - y0) / NaN: the right-hand side is NaN from the first call
    o = Options(rtol=1e-4, atol=1e-6)
    mb = M.solve(M.rhs_vdp_eps(float("nan")), 0.0, 0.5, [float(v) for v in y0[:, bad]], 1e-4, 1e-6)
    assert mb.status != M.SUCCESS or any(v != v for v in mb.y_end)
    r = Radau().solve_batch(ivp_amd.StiffVanDerPol(), 0.0, 0.5, y0, eps, o)
    g, w = gpu_row(r, bad), model_row(mb)
    assert all(g[k] == w[k] for k in MEMBERS if k not in ("t_end", "h_next")) and same(g["t_end"], w["t_end"]) and \
        same(g["h_next"], w["h_next"]) and same_vec(g["y_end"], w["y_end"]), (g, w)
    keep = [b for b in range(64) if b != bad]
    solo = Radau().solve_batch(ivp_amd.StiffVanDerPol(), 0.0, 0.5, np.ascontiguousarray(y0[:, keep]), np.ascontiguousarray(eps[:, keep]), o)
    for k in MEMBERS + ("y_end",):
        a, b = _np(getattr(r, k))[..., keep], _np(getattr(solo, k))
        assert a.tobytes() == b.tobytes(), k
    assert (solo.status == 0).all()
    for b in (0, 16, 18, 63):                              # and the healthy neighbours are the model's
        m = M.solve(M.rhs_vdp_eps(float(eps[0, b])), 0.0, 0.5, [float(v) for v in y0[:, b]], 1e-4, 1e-6)
        gg, ww = gpu_row(r, b), model_row(m)
        assert gg["nstep"] == ww["nstep"] and same_vec(gg["y_end"], ww["y_end"]), b


# ---- 8. settings ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(newton_maxiter=3), dict(newton_tol=1e-3), dict(predictive=False),
                                dict(safety_factor=0.8, scale_min=0.3, scale_max=4.0), dict(newton_maxiter=15, uround=1e-15)])
def test_settings_reach_the_kernel(kw):
    y0, eps = vdp_eps_batch()
    y0, eps = np.ascontiguousarray(y0[:, :3]), np.ascontiguousarray(eps[:, :3])
    models = [M.solve(M.rhs_vdp_eps(float(eps[0, b])), 0.0, 2.0, [float(v) for v in y0[:, b]], RT, AT, settings=M.Settings(**kw)) for b in range(3)]
    base = vdp_eps_models(3)
    assert any(model_row(a) != model_row(b) for a, b in zip(models, base))   # the setting changes the run
    r = Radau(**kw).solve_batch(ivp_amd.StiffVanDerPol(), 0.0, 2.0, y0, eps, OPT)
    assert_rows(r, models, str(kw))


# ---- 9. sequences on one context --------------------------------------------------------------------------------------

def test_radau_bdf_radau_on_one_context_equals_fresh_contexts():
    y0, eps = vdp_eps_batch()
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)

    def radau(ctx, B, opts):
        return Radau().solve_batch(ivp_amd.StiffVanDerPol(), 0.0, 2.0, dev(y0[:, :B]), dev(eps[:, :B]), opts, ctx=ctx)

    def bdf(ctx):
        return ivp_amd.solve_ivp_batch(ivp_amd.StiffVanDerPol(), 0.0, 2.0, dev(y0[:, :9]), dev(eps[:, :9]), Options(method="BDF", rtol=RT, atol=AT), ctx=ctx)

    o1, o3 = OPT, Options(rtol=RT, atol=AT, dense_output=True, max_log=400)
    fresh = []
    for call in (lambda c: radau(c, 5, o1), bdf, lambda c: radau(c, 12, o3)):
        c = ivp_amd.Context(0)
        fresh.append(call(c))
    one = ivp_amd.Context(0)
    seq = [radau(one, 5, o1), bdf(one), radau(one, 12, o3)]
    for a, b in zip(seq, fresh):
        for k in MEMBERS + ("y_end", "n_seg", "seg_cont", "seg_xold", "seg_h"):
            va, vb = getattr(a, k, None), getattr(b, k, None)
            assert (va is None) == (vb is None), k
            if va is None:
                continue
            va, vb = _np(va), _np(vb)
            if k.startswith("seg_"):   # slots past a trajectory's count are never written
                ns = _np(a.n_seg)
                for t in range(va.shape[-1]):
                    assert va[:ns[t], ..., t].tobytes() == vb[:ns[t], ..., t].tobytes(), (k, t)
            else:
                assert va.tobytes() == vb.tobytes(), k
    assert_rows(seq[2], vdp_eps_models(12), "third solve of the sequence")


# ---- 10. front ends ---------------------------------------------------------------------------------------------------

VDP_SRC = "__device__ void ode(double x, const double* y, double* d, const double* p) { d[0] = y[1]; d[1] = ((1.0 - y[0] * y[0]) * y[1] - y[0]) / 1e-3; }"


def test_scipy_front_end_routes_radau_to_the_direct_call():
    grid = np.linspace(0.0, 2.0, 9)
    res = ivp_amd.pyfront.solve_ivp(VDP_SRC, (0.0, 2.0), [2.0, 0.0], method="Radau", rtol=RT, atol=AT, t_eval=grid)
    s = Radau().solve(ivp_amd.DeviceIVP(VDP_SRC, 2), 0.0, 2.0, [2.0, 0.0], Options(rtol=RT, atol=AT, t_eval=grid))
    assert res.success and res.status == 0
    assert np.asarray(res.t).tobytes() == np.asarray(s.t).tobytes() and np.asarray(res.y).tobytes() == np.ascontiguousarray(np.asarray(s.y).T).tobytes()
    assert (res.nfev, res.njev, res.nlu) == (s.nfev, s.njev, s.nlu)
    m = M.solve(M.rhs_vdp_eps(1e-3), 0.0, 2.0, [2.0, 0.0], RT, AT, t_eval=list(grid))
    assert all(same_vec(a, b) for a, b in zip(s.y, m.y)) and (s.nfev, s.njev, s.nlu, s.nstep) == (m.nfev, m.njev, m.nlu, m.nstep)
    assert np.abs(np.asarray(s.y[-1]) - TRUTH["vdp_eps1e-3_t2"]).max() < 1e-4


def test_scipy_front_end_honours_jac_for_radau():
    jac = "__device__ void jac(double x, const double* y, double* j, const double* p) { j[0] = 0.0; j[1] = 1.0; j[2] = (-2.0 * y[0] * y[1] - 1.0) / 1e-3; j[3] = (1.0 - y[0] * y[0]) / 1e-3; }"
    res = ivp_amd.pyfront.solve_ivp(VDP_SRC, (0.0, 2.0), [2.0, 0.0], method="Radau", rtol=RT, atol=AT, jac=jac)

    def mj(x, y, J):
        J[0][0], J[0][1] = 0.0, 1.0
        J[1][0], J[1][1] = (-2.0 * y[0] * y[1] - 1.0) / 1e-3, (1.0 - y[0] * y[0]) / 1e-3

    m = M.solve(M.rhs_vdp_eps(1e-3), 0.0, 2.0, [2.0, 0.0], RT, AT, jac=mj)
    assert res.success and (res.nfev, res.njev, res.nlu) == (m.nfev, m.njev, m.nlu)
    assert same_vec(np.asarray(res.y)[:, -1], m.y_end) and len(res.t) == len(m.t)


def test_options_method_radau_through_solve_ivp_batch_is_still_unsupported():
    with pytest.raises(ivp_amd.ConfigError) as e:
        ivp_amd.solve_ivp_batch(ivp_amd.SHO(), 0.0, 1.0, np.array([[1.0], [0.0]]), None, Options(method="RADAU"))
    assert e.value.code == -101


# ---- 11. the branches no whole solve above takes ------------------------------------------------------------------------
# The same inputs run on the host in tests/test_radau_emul_cpu.py; what only the device can show is the hiprtc
# instantiations, the launch loop's own bookkeeping across restarts and retired lanes, and the compiled kernels' bits.

def lin_matrix(n):
    """_a8()'s construction at width n (tests/test_radau_emul_cpu.py has the same)."""
    a = [[1e-3 * (1 + ((3 * i + 5 * j) % 7)) for j in range(n)] for i in range(n)]
    for i in range(n):
        a[i][i] = -1.0 - 0.25 * i
        if i % 2:
            a[i][i - 1] = 200.0
    return a


def lin_source(a, with_jac):
    """y' = A y with A fixed in the functor, every row summed left to right (M.rhs_dense_linear)."""
    n = len(a)
    lit = lambda v: float(v).hex()
    src = "__device__ void ode(double x, const double* y, double* d, const double* p) {\n"
    for i in range(n):
        src += f"  d[{i}] = " + " + ".join(f"{lit(a[i][j])} * y[{j}]" for j in range(n)) + ";\n"
    src += "}\n"
    if with_jac:
        src += "__device__ void jac(double x, const double* y, double* j, const double* p) {\n"
        src += "".join(f"  j[{i * n + k}] = {lit(a[i][k])};\n" for i in range(n) for k in range(n)) + "}\n"
    return src


# n = 2, the matrix in the parameters: one compiled problem serves every 2 x 2 Jacobian below
LIN2_SRC = ("__device__ void ode(double x, const double* y, double* d, const double* p) { d[0] = p[0] * y[0] + p[1] * y[1]; d[1] = p[2] * y[0] + p[3] * y[1]; }\n"
            "__device__ void jac(double x, const double* y, double* j, const double* p) { j[0] = p[0]; j[1] = p[1]; j[2] = p[2]; j[3] = p[3]; }\n")


def lin_models(a, y0s, t1, with_jac, rtol=RT, atol=AT, **kw):
    return [M.solve(M.rhs_dense_linear(a), 0.0, t1, list(y0), rtol, atol, jac=M.jac_dense_linear(a) if with_jac else None, **kw) for y0 in y0s]


def test_newton_maxiter_1_is_status_singular_matrix_after_five_restarts():
    y0, eps = vdp_eps_batch()
    y0, eps = np.ascontiguousarray(y0[:, :3]), np.ascontiguousarray(eps[:, :3])
    models = [M.solve(M.rhs_vdp_eps(float(eps[0, b])), 0.0, 2.0, [float(v) for v in y0[:, b]], RT, AT, settings=M.Settings(newton_maxiter=1)) for b in range(3)]
    assert all(m.status == M.SINGULAR_MATRIX and m.n_restart == 5 and m.n_restart_newton == 6 and m.naccpt == 0 for m in models)
    for chunk in (0, 1):
        r = Radau(newton_maxiter=1).solve_batch(ivp_amd.StiffVanDerPol(), 0.0, 2.0, y0, eps, Options(rtol=RT, atol=AT, chunk_attempts=chunk))
        assert_rows(r, models, f"newton_maxiter = 1, chunk_attempts = {chunk}")
        assert all(int(v) == ivp_amd.Status.SingularMatrix == 5 for v in _np(r.status))


def test_newton_maxiter_2_restarts_survive_every_launch_boundary():
    """chunk_attempts = 1: h, reject, call_decomp and singular_count (flag bits 8..10) cross a launch boundary after every
    one of hundreds of restarts; the solve succeeds only because every accepted step resets the count.  (A count lost at a
    boundary shows in the newton_maxiter = 1 test above at chunk_attempts = 1: its fifth restart must still end the solve.)"""
    y0, eps = vdp_eps_batch()
    y0, eps = np.ascontiguousarray(y0[:, :2]), np.ascontiguousarray(eps[:, :2])
    models = [M.solve(M.rhs_vdp_eps(float(eps[0, b])), 0.0, 2.0, [float(v) for v in y0[:, b]], RT, AT, settings=M.Settings(newton_maxiter=2)) for b in range(2)]
    assert all(m.n_restart_newton > 100 and m.naccpt > 0 for m in models)
    r = Radau(newton_maxiter=2).solve_batch(ivp_amd.StiffVanDerPol(), 0.0, 2.0, y0, eps, Options(rtol=RT, atol=AT, chunk_attempts=1))
    assert_rows(r, models, "newton_maxiter = 2, chunk_attempts = 1")


def test_real_zero_pivot_on_the_first_factorisation():
    """Built-in decay (y' = -k y) with k = -(U1 / h): E1 = U1 / h - J is exactly zero; for y0 in {0, 2^-26, -2^-27} the
    forward-difference Jacobian is exact (see tests/test_radau_emul_cpu.py)."""
    h = 0.01
    k = -(M.U1 / h)
    y0s = [0.0, 2.0 ** -26, -(2.0 ** -27)]
    models = [M.solve(M.rhs_decay(k), 0.0, 0.05, [v], RT, AT, first_step=h) for v in y0s]
    assert all(m.n_restart_real == 1 and m.n_restart == 1 and m.status == M.SUCCESS and m.h_tried[0] == 0.5 * h for m in models)
    r = Radau().solve_batch(ivp_amd.ExponentialDecay(), 0.0, 0.05, np.array([y0s]), np.full((1, 3), k), Options(rtol=RT, atol=AT, first_step=h))
    assert_rows(r, models, "real zero pivot")


def _lin2(J, y0s, t1, h):
    flat = [J[0][0], J[0][1], J[1][0], J[1][1]]
    models = lin_models(J, y0s, t1, True, first_step=h)
    prob = ivp_amd.DeviceIVP(LIN2_SRC, 2, params=flat, jac=True)
    r = Radau().solve_batch(prob, 0.0, t1, np.array(y0s).T.copy(), None, Options(rtol=RT, atol=AT, first_step=h))
    return models, r


def test_complex_zero_pivot_on_the_first_factorisation():
    """The rotation J = [[a, -b], [b, a]], a = ALPH / h, b = BETA / h: E2 = [[i b, b], [-b, i b]], second pivot exactly zero."""
    h = 2.0 ** -6
    a, b = M.ALPH / h, M.BETA / h
    models, r = _lin2([[a, -b], [b, a]], [[1.0, 0.0], [0.3, -0.7]], 4.0 * h, h)
    assert all(m.n_restart_complex == 1 and m.n_restart == 1 and m.n_restart_real == 0 and m.h_tried[0] == 0.5 * h for m in models)
    assert_rows(r, models, "complex zero pivot")


def test_purely_imaginary_multiplier_in_the_complex_elimination():
    h = 2.0 ** -10
    models, r = _lin2([[0.0, 1.0], [-1e5, M.ALPH / h]], [[1.0, 0.0], [0.5, 0.25]], 8.0 * h, h)
    assert all("imag" in m.cases and ("complex", 0, 1) in m.pivots for m in models)
    assert_rows(r, models, "imaginary multiplier")


def test_max_step_bounds_every_step():
    y0 = np.array([[1.0, 0.3], [0.0, -0.7]])
    models = [M.solve(M.rhs_sho, 0.0, 1.0, [float(v) for v in y0[:, b]], RT, AT, max_step=0.02) for b in range(2)]
    free = M.solve(M.rhs_sho, 0.0, 1.0, [1.0, 0.0], RT, AT)
    assert max(abs(v) for v in free.h_tried) > 0.04 and all(max(abs(v) for v in m.h_tried) == 0.02 for m in models)
    r = Radau().solve_batch(ivp_amd.SHO(), 0.0, 1.0, y0, None, Options(rtol=RT, atol=AT, max_step=0.02, max_log=80))
    assert_rows(r, models, "max_step")
    for b, m in enumerate(models):
        k = int(r.n_log[b])
        assert k == len(m.t) <= 80 and all(same(r.t_log[q, b], m.t[q]) for q in range(k))
        assert max(abs(float(r.t_log[q + 1, b]) - float(r.t_log[q, b])) for q in range(k - 1)) <= 0.02 * (1 + 1e-12)


def test_min_step_with_max_step():
    y0, eps = vdp_eps_batch()
    y0, eps = np.ascontiguousarray(y0[:, :2]), np.ascontiguousarray(eps[:, :2])
    models = vdp_eps_models(2, min_step=1e-3, max_step=0.02)
    free = vdp_eps_models(2)
    assert all(min(f.h_tried) < 1e-3 and max(f.h_tried) > 0.02 and m.h_tried.count(1e-3) > 0 and m.h_tried.count(0.02) > 0 for m, f in zip(models, free))
    r = Radau().solve_batch(ivp_amd.StiffVanDerPol(), 0.0, 2.0, y0, eps, Options(rtol=RT, atol=AT, min_step=1e-3, max_step=0.02))
    assert_rows(r, models, "min_step with max_step")


@pytest.mark.parametrize("t1", [1.0, -1.0])
def test_first_step_larger_than_max_step_is_clamped(t1):
    m = M.solve(M.rhs_sho, 0.0, t1, [1.0, 0.0], RT, AT, first_step=0.5, max_step=0.01)
    assert m.h_tried[0] == math.copysign(0.01, t1) and m.status == M.SUCCESS
    r = Radau().solve_batch(ivp_amd.SHO(), 0.0, t1, np.array([[1.0], [0.0]]), None, Options(rtol=RT, atol=AT, first_step=0.5, max_step=0.01))
    assert_rows(r, [m], "first_step > max_step")


@pytest.mark.parametrize("analytic", [False, True])
def test_vector_tolerances_and_the_same_vectors_reversed(analytic):
    rt, at = [1e-4, 1e-7, 1e-5], [1e-6, 1e-11, 1e-8]
    jac = M.jac_robertson if analytic else None
    fwd = M.solve(M.rhs_robertson, 0.0, 1e3, [1.0, 0.0, 0.0], rt, at, jac=jac)
    rev = M.solve(M.rhs_robertson, 0.0, 1e3, [1.0, 0.0, 0.0], rt[::-1], at[::-1], jac=jac)
    assert fwd.status == rev.status == M.SUCCESS and (fwd.nstep, fwd.nfev, fwd.y_end) != (rev.nstep, rev.nfev, rev.y_end)
    f = ivp_amd.RobertsonJac() if analytic else ivp_amd.Robertson()
    y0 = np.array([[1.0], [0.0], [0.0]])
    assert_rows(Radau().solve_batch(f, 0.0, 1e3, y0, None, Options(rtol=rt, atol=at)), [fwd], "vector tolerances")
    assert_rows(Radau().solve_batch(f, 0.0, 1e3, y0, None, Options(rtol=rt[::-1], atol=at[::-1])), [rev], "vector tolerances reversed")


@pytest.mark.parametrize("with_jac", [True, False])
@pytest.mark.parametrize("n", [4, 5, 7])
def test_state_widths_4_5_7_through_hiprtc(n, with_jac):
    a = lin_matrix(n)
    y0 = [1.0, 0.5, -0.5, 0.25, 0.0, 1e-3, -1.0, 2.0][:n]
    y0s = [y0, [v + 1e-3 * (i + 1) for i, v in enumerate(y0)]]
    models = lin_models(a, y0s, 5.0, with_jac, 1e-4, 1e-6)
    assert all(m.status == 0 and any(p[0] == "real" for p in m.pivots) and any(p[0] == "complex" for p in m.pivots) for m in models)
    prob = ivp_amd.DeviceIVP(lin_source(a, with_jac), n, jac=with_jac)
    r = Radau().solve_batch(prob, 0.0, 5.0, np.array(y0s).T.copy(), None, Options(rtol=1e-4, atol=1e-6))
    assert_rows(r, models, f"{n} x {n} linear system")


def test_t_eval_and_dense_output_at_n8_through_hiprtc():
    """A dense segment at N = 8 is 32 doubles per trajectory: the widest indexing of seg_cont."""
    a = _a8()
    y0s = [[1.0, 0.5, -0.5, 0.25, 0.0, 1e-3, -1.0, 2.0], [0.5] * 8]
    y0 = np.array(y0s).T.copy()
    prob = ivp_amd.DeviceIVP(_a8_source(True), 8, jac=True)
    grid = [0.0, 0.1, 0.1 + 1e-13, 0.7, 1.5, 3.0, 3.5]
    models = lin_models(a, y0s, 3.0, True, t_eval=grid)
    r = Radau().solve_batch(prob, 0.0, 3.0, y0, None, Options(rtol=RT, atol=AT, t_eval=grid))
    assert_rows(r, models, "n = 8, t_eval")
    for b, m in enumerate(models):
        k = int(r.n_filled[b])
        assert k == len(m.t) == 6 and list(r.eval_idx[:k, b]) == m.eval_idx
        assert all(same_vec(r.y_eval[q, :, b], m.y[q]) for q in range(k)), b
    models = lin_models(a, y0s, 3.0, True, dense_output=True)
    ml = max(len(m.segs) for m in models) + 1
    r = Radau().solve_batch(prob, 0.0, 3.0, y0, None, Options(rtol=RT, atol=AT, dense_output=True, max_log=ml))
    assert_rows(r, models, "n = 8, dense output")
    for b, m in enumerate(models):
        assert int(r.n_seg[b]) == len(m.segs) == m.naccpt > 3 and int(r.n_log[b]) == len(m.t)
        for q, (cont, xold, h) in enumerate(m.segs):
            assert same(r.seg_xold[q, b], xold) and same(r.seg_h[q, b], h) and same_vec(r.seg_cont[q, :, b], cont), (b, q)
        assert all(same(r.t_log[q, b], m.t[q]) and same_vec(r.y_log[q, :, b], m.y[q]) for q in range(len(m.t))), b


@pytest.mark.parametrize("flavour", ["end", "t_eval", "log", "dense"])
def test_degenerate_and_nan_intervals_beside_five_healthy_trajectories(flavour):
    """t1 == t0 and a NaN t1 retire in the init kernel with solve_ivp's own early return: status 0 / 3, h_next = 0, zero
    counters, the t_eval points within 1e-12 of t0, one log record, the constant dense segment.  Held to what DOPRI5 (pinned
    to the oracle) returns for the same lanes; the healthy neighbours stay the model's."""
    y0 = np.array([[1.0, 0.5, 2.0, -0.3, -1.5, 2.0, 0.0], [0.0, 0.5, 0.25, 0.9, 1.0, -1.0, 1.0]])
    t1s = np.array([3.0, 3.0, 0.0, 3.0, float("nan"), 2.0, 3.0])   # per-trajectory t1; lanes 2 and 4 are the odd ones
    odd, healthy = {2: 0, 4: 3}, [0, 1, 3, 5, 6]
    grid = [0.0, 5e-13, 0.1, 0.7, 1.5, 2.0, 3.0]
    okw = {"end": {}, "t_eval": dict(t_eval=grid), "log": dict(max_log=6), "dense": dict(max_log=6, dense_output=True)}[flavour]
    mkw = {"end": {}, "t_eval": dict(t_eval=grid), "log": {}, "dense": dict(dense_output=True)}[flavour]
    models = {b: model(("degenerate", flavour, b), lambda b=b: M.solve(M.rhs_sho, 0.0, float(t1s[b]), [float(v) for v in y0[:, b]], RT, AT, **mkw)) for b in healthy}
    r = Radau().solve_batch(ivp_amd.SHO(), 0.0, t1s, y0, None, Options(rtol=RT, atol=AT, **okw))
    d = ivp_amd.solve_ivp_batch(ivp_amd.SHO(), 0.0, t1s, y0, None, Options(method="DOPRI5", rtol=RT, atol=AT, **okw))
    for b in healthy:
        g, w = gpu_row(r, b), model_row(models[b])
        assert all(g[k] == w[k] for k in MEMBERS if k not in ("t_end", "h_next")) and same(g["t_end"], w["t_end"]) and \
            same(g["h_next"], w["h_next"]) and same_vec(g["y_end"], w["y_end"]), (b, g, w)
        m = models[b]
        if flavour == "t_eval":
            k = int(r.n_filled[b])
            assert k == len(m.t) and list(r.eval_idx[:k, b]) == m.eval_idx and all(same_vec(r.y_eval[q, :, b], m.y[q]) for q in range(k)), b
        elif flavour in ("log", "dense"):
            assert int(r.n_log[b]) == len(m.t) > 6 and all(same(r.t_log[q, b], m.t[q]) and same_vec(r.y_log[q, :, b], m.y[q]) for q in range(6)), b
    for b, status in odd.items():
        g, w = gpu_row(r, b), gpu_row(d, b)
        assert g["status"] == w["status"] == status and same(g["h_next"], 0.0) and same(g["h_next"], w["h_next"]), (b, g, w)
        assert same(g["t_end"], w["t_end"]) and same(g["t_end"], 0.0) and same_vec(g["y_end"], w["y_end"]) and same_vec(g["y_end"], y0[:, b]), (b, g, w)
        assert all(g[k] == 0 for k in ("nfev", "njev", "nlu", "nstep", "naccpt", "nrejct")) and all(w[k] == 0 for k in ("nfev", "nstep", "naccpt", "nrejct")), (b, g, w)
        if flavour == "t_eval":
            k = int(r.n_filled[b])
            assert k == int(d.n_filled[b]) == (2 if status == 0 else 0), (b, k)
            assert list(r.eval_idx[:k, b]) == list(d.eval_idx[:k, b]) and all(same_vec(r.y_eval[q, :, b], d.y_eval[q, :, b]) for q in range(k))
        elif flavour in ("log", "dense"):
            k = int(r.n_log[b])
            assert k == int(d.n_log[b]) == (1 if status == 0 else 0), (b, k)
            assert all(same(r.t_log[q, b], d.t_log[q, b]) and same_vec(r.y_log[q, :, b], d.y_log[q, :, b]) for q in range(k))
        if flavour == "dense":
            k = int(r.n_seg[b])
            assert k == int(d.n_seg[b]) == (1 if status == 0 else 0), (b, k)
            for q in range(k):   # ContinuousOutput::constant: [y, 0, 0, ..]; DOPRI5 carries 5 n coefficients, Radau 4 n
                assert same(r.seg_xold[q, b], d.seg_xold[q, b]) and same(r.seg_h[q, b], d.seg_h[q, b])
                assert same_vec(r.seg_cont[q, :, b], d.seg_cont[q, :8, b]) and same_vec(d.seg_cont[q, 8:, b], [0.0, 0.0])
