"""Radau IIA(5) in band storage on the device (ivp_amd.Radau.solve_batch_banded -> ivp_radau_solve_banded*() ->
RadauOpsBand, ivp_amd/csrc/radau_band.h) against the dense Radau call on the same source compiled WITHOUT a pattern and
against the CPU model (tests/radau_model.py through tests/radau_wide_model.py, forward differences), BIT FOR BIT: status,
t_end, y_end, h_next, all six counters, t_eval samples, step log, dense segments.  No tolerance anywhere.

The systems are band_system / band_pattern / batch_inputs of tests/test_gpu_jac_sparsity.py and asym_system / pivot_system of
tests/test_gpu_jac_banded.py: nonlinear, so the Jacobian is re-evaluated along the way.  Every test that names a branch asserts
from the model's counters or pivots that its input takes it.  Model runs are cached per input.  At n = 512 the recipe of
tests/test_gpu_radau_wide.py keeps the dense model quick: loose tolerances, a given first step, an interval of three steps.
Before the banded call existed every test here failed: Radau had no solve_batch_banded."""
import numpy as np
import pytest
import torch

import ivp_amd
from ivp_amd import Options, Radau
from tests import radau_wide_model as W
from tests import test_gpu_radau_group as G
from tests.test_gpu_jac_banded import asym_system, pivot_system
from tests.test_gpu_jac_sparsity import band_pattern, band_system, batch_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RT, AT = 1e-6, 1e-8
BAD_ARGUMENT = -100
FIELDS = ("y_end", "t_end", "h_next", "status", "nfev", "nstep", "naccpt", "nrejct", "njev", "nlu")
SAMPLED = FIELDS + ("y_eval", "eval_idx", "n_filled")
LOGGED = FIELDS + ("t_log", "y_log", "n_log", "seg_cont", "seg_xold", "seg_h", "n_seg")
MAX_LOG = 128
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def asym(n):
    src, fun, pat = asym_system(n)
    return src, fun, pat


# name -> (source, numpy restatement, pattern, n, (ml, mu), trajectories, (rtol, atol, first_step, t1 or None))
CASES = {
    "tri12": lambda: (*band_system(12, 1), band_pattern(12, 1), 12, (1, 1), 5, None),     # G = 16: four per wavefront, a second part-filled
    "tri24": lambda: (*band_system(24, 1), band_pattern(24, 1), 24, (1, 1), 2, None),     # G = 32
    "tri40": lambda: (*band_system(40, 1), band_pattern(40, 1), 40, (1, 1), 2, None),
    "asym40": lambda: (*asym(40), 40, (2, 1), 2, None),                                    # asymmetric band
    "tri65": lambda: (*band_system(65, 1), band_pattern(65, 1), 65, (1, 1), 2, None),     # C = 2, one lane in the top slot
    "band8_100": lambda: (*band_system(100, 8), band_pattern(100, 8), 100, (8, 8), 2, None),
    "band4_130": lambda: (*band_system(130, 4), band_pattern(130, 4), 130, (4, 4), 2, None),
    "tri512": lambda: (*band_system(512, 1), band_pattern(512, 1), 512, (1, 1), 2, (1e-2, 1e-4, 4e-3, [0.012, 0.006])),   # C = 8
}


def case_inputs(name):
    src, fun, pattern, n, bw, nb, setup = CASES[name]()
    y0, params, t1 = batch_inputs(n, seed=n + len(name))
    y0, params, t1 = np.ascontiguousarray(y0[:, :nb]), np.ascontiguousarray(params[:, :nb]), np.ascontiguousarray(t1[:nb])
    rt, at, fs = RT, AT, None
    if setup is not None:
        rt, at, fs, t1 = setup[0], setup[1], setup[2], np.array(setup[3])
    return src, fun, pattern, n, bw, y0, params, t1, rt, at, fs


def grid_of(t1):
    tm = float(np.max(t1))
    return [0.0, 0.2 * tm, 0.2 * tm + 1e-13, 0.5 * tm, 0.9 * tm, tm, tm + 0.5]


def models_of(name, kind, fun, y0, params, t1, rt, at, fs, **kw):
    """the CPU model of every trajectory (forward differences): kind 'dense' records the step log and the segments, 'eval' the samples"""
    extra = dict(dense_output=True) if kind == "dense" else dict(t_eval=grid_of(t1))
    if fs is not None:
        extra["first_step"] = fs
    extra.update(kw)
    key = (name, kind, repr(rt), repr(at), tuple(sorted((k, repr(v)) for k, v in extra.items())))
    return [cached(key + (b,), lambda b=b: W.solve(lambda x, y, p=params[:, b]: fun(x, y, p).tolist(), 0.0, float(t1[b]), y0[:, b].tolist(),
                                                     rt, at, **extra))
            for b in range(y0.shape[1])]


def problems(src, n, pattern):
    dense = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0))
    banded = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=pattern, jac_storage="banded")
    return dense, banded


def same_bits(a, b):
    a, b = np.ascontiguousarray(_np(a)), np.ascontiguousarray(_np(b))
    if a.dtype.kind in "iu" and b.dtype.kind in "iu":   # counters: uint64 on the host, int64 in a torch tensor
        a, b = a.astype(np.int64), b.astype(np.int64)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def assert_same(got, want, names, what):
    for k in names:
        assert same_bits(getattr(got, k), getattr(want, k)), f"{what}: {k} differs"


def assert_outputs_equal_models(sampled, logged, m_eval, m_dense, what):
    """the recorded outputs of the two full runs against the models' (the rows are G.assert_rows' business)"""
    for b, (me, md) in enumerate(zip(m_eval, m_dense)):
        k = int(_np(sampled.n_filled)[b])
        assert k == len(me.t) and list(_np(sampled.eval_idx)[:k, b]) == me.eval_idx, (what, b)
        assert all(G.same_vec(_np(sampled.y_eval)[q, :, b], me.y[q]) for q in range(k)), (what, b, "samples")
        m = int(_np(logged.n_log)[b])
        assert m == len(md.t) <= MAX_LOG, (what, b, m)
        for q in range(m):
            assert G.same(_np(logged.t_log)[q, b], md.t[q]) and G.same_vec(_np(logged.y_log)[q, :, b], md.y[q]), (what, b, q, "step log")
        assert int(_np(logged.n_seg)[b]) == len(md.segs) == md.naccpt, (what, b)
        for q, (cont, xold, h) in enumerate(md.segs):
            assert G.same(_np(logged.seg_xold)[q, b], xold) and G.same(_np(logged.seg_h)[q, b], h), (what, b, q)
            assert G.same_vec(_np(logged.seg_cont)[q, :, b], cont), (what, b, q, "segment")


# ---- 1. banded = dense call = model, every output form ---------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_banded_equals_the_dense_call_and_the_model(name):
    src, fun, pattern, n, bw, y0, params, t1, rt, at, fs = case_inputs(name)
    dense_p, band_p = problems(src, n, pattern)
    ml, mu = bw
    assert band_p.jac_layout == {"banded": True, "ml": ml, "mu": mu, "jac_doubles": (ml + mu + 1) * n, "lu_doubles": (2 * ml + mu + 1) * n}
    kw = dict(rtol=rt, atol=at) if fs is None else dict(rtol=rt, atol=at, first_step=fs)
    opts = (Options(**kw), Options(t_eval=grid_of(t1), **kw), Options(dense_output=True, max_log=MAX_LOG, **kw))
    want = [Radau().solve_batch(dense_p, 0.0, t1, y0, params, o) for o in opts]
    got = [Radau().solve_batch_banded(band_p, 0.0, t1, y0, params, o) for o in opts]
    # the dense run really iterates: the Jacobian is re-evaluated and re-factorised
    assert (np.asarray(want[2].status) == 0).all() and int(np.asarray(want[2].njev).min()) > 1 and int(np.asarray(want[2].nlu).min()) > 1
    for g, w, names, form in zip(got, want, (FIELDS, SAMPLED, LOGGED), ("end state", "t_eval", "dense_output")):
        assert_same(g, w, names, f"{name}, {form}: banded vs dense call")
    m_eval = models_of(name, "eval", fun, y0, params, t1, rt, at, fs)
    m_dense = models_of(name, "dense", fun, y0, params, t1, rt, at, fs)
    assert all(m.status == 0 and m.njev > 1 and m.nlu > 1 for m in m_dense)
    G.assert_rows(got[0], m_dense, f"{name}: end state vs model")
    G.assert_rows(got[1], m_eval, f"{name}: t_eval vs model")
    G.assert_rows(got[2], m_dense, f"{name}: dense_output vs model")
    assert_outputs_equal_models(got[1], got[2], m_eval, m_dense, name)


# ---- 2. row exchanges inside a real solve ------------------------------------------------------------------------------------

PIV_N, PIV_T1, PIV_H = 40, 0.06, 0.05
PIV_PARAMS = np.array([[400.0, 600.0], [1.0, 0.5]])   # k, a: 1.5 k = |J[i][i-1]| = 600, 900


def pivot_inputs():
    y0 = np.array([[0.5 + 0.01 * i for i in range(PIV_N)], [0.8 + 0.01 * i for i in range(PIV_N)]]).T.copy()
    return y0, PIV_PARAMS.copy(), np.array([PIV_T1, PIV_T1])


def test_row_exchanges_inside_a_solve():
    src, fun, pattern = pivot_system(PIV_N)
    y0, params, t1 = pivot_inputs()
    # |J[i][i-1]| = 1.5 k exceeds fac1 = U1 / h = 72.8 and |alphn + i betan| = 81.2 at h = 0.05 (and the diagonals k + fac1 ...)
    u1, alph, beta = 3.6378342527444957, 2.6810828736277521, 3.0504301992474105
    assert all(1.5 * k > max(u1, abs(complex(alph, beta))) / PIV_H for k in params[0])
    models = models_of("pivot40", "dense", fun, y0, params, t1, RT, AT, PIV_H)
    assert all(m.status == 0 and any(p[0] == "real" for p in m.pivots) and any(p[0] == "complex" for p in m.pivots) for m in models)
    dense_p, band_p = problems(src, PIV_N, pattern)
    o = Options(rtol=RT, atol=AT, first_step=PIV_H, dense_output=True, max_log=MAX_LOG)
    want = Radau().solve_batch(dense_p, 0.0, t1, y0, params, o)
    got = Radau().solve_batch_banded(band_p, 0.0, t1, y0, params, o)
    assert_same(got, want, LOGGED, "pivot system: banded vs dense call")
    G.assert_rows(got, models, "pivot system vs model")


# ---- 3. chunk lengths ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [1, 7, 0])
def test_chunk_length_does_not_change_a_bit(chunk):
    src, fun, pattern, n, bw, y0, params, t1, rt, at, fs = case_inputs("tri40")
    models = models_of("tri40", "dense", fun, y0, params, t1, rt, at, fs)
    assert any(m.n_reuse > 0 for m in models)   # an accepted step keeps its factors: with chunk = 1 another launch uses them
    _, band_p = problems(src, n, pattern)
    r = Radau().solve_batch_banded(band_p, 0.0, t1, y0, params, Options(rtol=rt, atol=at, chunk_attempts=chunk, dense_output=True, max_log=MAX_LOG))
    G.assert_rows(r, models, f"chunk_attempts = {chunk}")
    ref = cached("chunk_ref", lambda: r)
    assert_same(r, ref, LOGGED, f"chunk_attempts = {chunk} vs the first chunk length run")


# ---- 4. sequences on one context equal fresh contexts ------------------------------------------------------------------------

def test_a_sequence_on_one_context_equals_fresh_contexts():
    src40, _, pat40, _, _, y40, p40, t40, *_ = case_inputs("tri40")
    src65, _, pat65, _, _, y65, p65, t65, *_ = case_inputs("tri65")
    d40, b40 = problems(src40, 40, pat40)
    d65, _ = problems(src65, 65, pat65)
    o = Options(rtol=RT, atol=AT, dense_output=True, max_log=MAX_LOG)
    ob = Options(method="BDF", rtol=1e-5, atol=1e-8, dense_output=True, max_log=256)
    steps = [
        ("dense Radau n = 40", lambda c: Radau().solve_batch(d40, 0.0, t40, y40, p40, o, ctx=c), LOGGED),
        ("banded Radau n = 40", lambda c: Radau().solve_batch_banded(b40, 0.0, t40, y40, p40, o, ctx=c), LOGGED),
        ("banded BDF n = 40", lambda c: ivp_amd.solve_ivp_batch(b40, 0.0, t40, y40, p40, ob, ctx=c), LOGGED),
        ("dense Radau n = 65", lambda c: Radau().solve_batch(d65, 0.0, t65, y65, p65, o, ctx=c), LOGGED),
        ("banded Radau n = 40 again", lambda c: Radau().solve_batch_banded(b40, 0.0, t40, y40, p40, o, ctx=c), LOGGED),
    ]
    one = ivp_amd.Context(0)
    for what, run, names in steps:
        assert_same(run(one), run(ivp_amd.Context(0)), names, what + ": in sequence vs a fresh context")


# ---- 5. host-pointer call, out= reuse, one trajectory ---------------------------------------------------------------------------

def test_host_and_device_calls_out_reuse_and_one_trajectory():
    src, fun, pattern, n, bw, y0, params, t1, rt, at, fs = case_inputs("tri40")
    _, band_p = problems(src, n, pattern)
    o = Options(rtol=rt, atol=at, dense_output=True, max_log=MAX_LOG)
    host = Radau().solve_batch_banded(band_p, 0.0, t1, y0, params, o)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    on_dev = Radau().solve_batch_banded(band_p, 0.0, dev(t1), dev(y0), dev(params), o)
    assert isinstance(on_dev.y_end, torch.Tensor)
    assert_same(on_dev, host, LOGGED, "device call vs host-pointer call")
    # out= reuse: a second solve with other end times into the same buffers
    again = Radau().solve_batch_banded(band_p, 0.0, dev(0.5 * t1), dev(y0), dev(params), o, out=on_dev)
    assert again.y_end.data_ptr() == on_dev.y_end.data_ptr()
    fresh = Radau().solve_batch_banded(band_p, 0.0, 0.5 * t1, y0, params, o)
    assert_same(again, fresh, FIELDS + ("n_log", "n_seg"), "out= reuse")
    # one trajectory: column 0 of the batch
    one = ivp_amd.DeviceIVP(src, n=n, params=tuple(params[:, 0]), jac_sparsity=pattern, jac_storage="banded")
    s = Radau().solve_banded(one, 0.0, float(t1[0]), y0[:, 0], Options(rtol=rt, atol=at))
    m = int(host.n_log[0])
    assert s.status == ivp_amd.Status.Success and len(s.t) == m
    assert same_bits(s.t, host.t_log[:m, 0]) and same_bits(s.y, host.y_log[:m, :, 0])
    assert (s.nfev, s.njev, s.nlu, s.nstep, s.naccpt, s.nrejct) == tuple(int(getattr(host, k)[0]) for k in ("nfev", "njev", "nlu", "nstep", "naccpt", "nrejct"))
    assert same_bits(np.float64(s.h_next), np.float64(host.h_next[0]))


# ---- 6. a right-hand side that turns NaN ----------------------------------------------------------------------------------------

NAN_N = 24
NAN_SRC = f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{{
    const double ym = i >= 1 ? y[i - 1] : 0.0, yp = i + 1 < {NAN_N} ? y[i + 1] : 0.0;
    const double s = p[0] * ((ym - 2.0 * y[i]) + yp);
    return (i == 3 && t > p[1]) ? s + (0.0 / 0.0) * y[i] : s;
}}
"""


def test_a_right_hand_side_that_turns_nan_fails_like_the_dense_call():
    y0 = np.array([[1.0 + 0.1 * i for i in range(NAN_N)], [0.5 - 0.01 * i for i in range(NAN_N)]]).T.copy()
    params = np.array([[50.0, 50.0], [0.01, 1e9]])   # trajectory 0 turns NaN after t = 0.01, trajectory 1 never does
    dense_p = ivp_amd.DeviceIVP(NAN_SRC, n=NAN_N, params=(1.0, 1.0))
    band_p = ivp_amd.DeviceIVP(NAN_SRC, n=NAN_N, params=(1.0, 1.0), jac_sparsity=band_pattern(NAN_N, 1), jac_storage="banded")
    o = Options(rtol=RT, atol=AT, max_steps=2000)
    want = Radau().solve_batch(dense_p, 0.0, 0.05, y0, params, o)
    got = Radau().solve_batch_banded(band_p, 0.0, 0.05, y0, params, o)
    # the dense call's trajectory 0 really went non-finite (a failure status, or NaNs carried to the end), trajectory 1 did not
    assert (int(want.status[0]) != 0 or np.isnan(np.asarray(want.y_end)[:, 0]).any()) and int(want.status[1]) == 0
    assert np.isfinite(np.asarray(want.y_end)[:, 1]).all()
    assert [int(v) for v in got.status] == [int(v) for v in want.status]
    assert same_bits(np.asarray(got.y_end)[:, 1], np.asarray(want.y_end)[:, 1])   # the finite neighbour is untouched


# ---- 7. refusals that need a compiled problem ------------------------------------------------------------------------------------

def test_refusals_through_the_banded_call_and_the_old_refusal_of_the_plain_call():
    n = 40
    src, _ = band_system(n, 1)
    pattern = band_pattern(n, 1)
    y0, params, t1 = batch_inputs(n, seed=3)
    y0, params, t1 = np.ascontiguousarray(y0[:, :2]), np.ascontiguousarray(params[:, :2]), np.ascontiguousarray(t1[:2])
    o = Options(rtol=RT, atol=AT)
    nothing = "the banded Radau call needs a problem compiled with IVP_RHS_BANDED"

    def refused(prob, opt, call):
        with pytest.raises(ivp_amd.ConfigError) as e:
            call(prob, 0.0, t1, y0, params, opt)
        return e.value.code, str(e.value)

    code, msg = refused(ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0)), o, Radau().solve_batch_banded)
    assert code == BAD_ARGUMENT and nothing in msg and "nothing to do" in msg, msg
    code, msg = refused(ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=pattern), o, Radau().solve_batch_banded)
    assert code == BAD_ARGUMENT and nothing in msg and "nothing to do" in msg, msg
    band_p = ivp_amd.DeviceIVP(src, n=n, params=(1.0, 1.0), jac_sparsity=pattern, jac_storage="banded")
    code, msg = refused(band_p, Options(rtol=RT, atol=AT, fp_mode=ivp_amd.FpMode.FMA), Radau().solve_batch_banded)
    assert code == BAD_ARGUMENT and "Radau with fp_mode = FMA: not yet (strict arithmetic only)" in msg, msg
    ev = ivp_amd.DeviceIVP(src + "__device__ void events(double x, const double* y, double* g, const double* p) { g[0] = y[0] - 0.25; }\n",
                           n=n, params=(1.0, 1.0), events=[ivp_amd.EventConfig()], jac_sparsity=pattern, jac_storage="banded")
    code, msg = refused(ev, o, Radau().solve_batch_banded)
    assert code == BAD_ARGUMENT and "Radau for problems with event functions: not yet on the accelerated path" in msg, msg
    # every old entry point keeps its refusal of the banded problem
    code, msg = refused(band_p, o, Radau().solve_batch)
    assert code == BAD_ARGUMENT and "not yet" in msg and "IVP_RHS_BANDED" in msg, msg


# ---- 8. the SciPy-style front end -------------------------------------------------------------------------------------------------

def test_pyfront_takes_the_banded_call():
    from ivp_amd import pyfront
    n = 40
    src, _ = band_system(n, 1)
    pattern = band_pattern(n, 1)
    y0, params, t1 = batch_inputs(n, seed=n + len("tri40"))
    p = tuple(float(v) for v in params[:, 0])
    t_end = float(t1[0])
    r = pyfront.solve_ivp(src, (0.0, t_end), y0[:, 0], method="Radau", jac_sparsity=pattern, jac_storage="banded", args=p, rtol=RT, atol=AT)
    band_p = ivp_amd.DeviceIVP(src, n=n, params=p, jac_sparsity=pattern, jac_storage="banded")
    s = Radau().solve_banded(band_p, 0.0, t_end, y0[:, 0], Options(rtol=RT, atol=AT))
    assert r.success and r.status == 0 and s.njev > 1
    assert same_bits(r.t, np.asarray(s.t, dtype=np.float64)) and same_bits(r.y, np.ascontiguousarray(np.asarray(s.y, dtype=np.float64).T))
    assert (r.nfev, r.njev, r.nlu) == (s.nfev, s.njev, s.nlu)
