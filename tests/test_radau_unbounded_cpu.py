"""The direct Radau call in its resumable, one-pass step log and CSR dense forms -- what needs no device: the three symbols
in the library, in ivp_amd._lib, in include/ivp_hip.h and in the FFI crate; the Python argument errors raised before a
context exists; and the page sink of radau_core.h on the host (tests/host_emul), gathered and held to tests/radau_model.py
bit for bit.

On the host a "wave" is one lane, so every page of the emulator has one column: what this file pins is the slot
arithmetic (two slots per attempt, the initial callback's page of two, pages of chunk * 2 slots for short launches), the
flush on every exit of the chunk body and the counts.  Columns, groups and arenas of several pages are the device's
(tests/test_gpu_radau_unbounded.py).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ivp_amd import Options, Radau, _lib
import ivp_amd
from tests import radau_model as M
from tests import test_radau_emul_cpu as T
from tests.host_emul import emul as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ivp_radau_submit_device", "ivp_radau_solve_logged_device", "ivp_radau_solve_dense_device")
# the arguments of ivp_radau_solve_dae_device up to `out`, then what each form adds
COMMON = [("ivp_ctx_t", 1, False), ("ivp_problem_t", 1, True), ("size_t", 0, False), ("double", 1, True), ("double", 1, True),
          ("double", 1, True), ("size_t", 0, False), ("double", 1, True), ("size_t", 0, False), ("ivp_options_t", 1, True),
          ("ivp_radau_settings_t", 1, True), ("ivp_radau_dae_t", 1, True), ("ivp_batch_result_t", 1, False)]
STREAM = ("void", 1, False)
EXPECTED = {"ivp_radau_submit_device": COMMON + [STREAM],
            "ivp_radau_solve_logged_device": COMMON + [("ivp_step_log_t", 1, False), STREAM],
            "ivp_radau_solve_dense_device": COMMON + [("ivp_dense_log_t", 1, False), STREAM]}


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_the_library_exports_the_three_symbols(lib):
    for name in NEW:
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None


def test_lib_declares_them_with_the_arguments_of_the_dae_call(lib):
    dae = lib.ivp_radau_solve_dae_device.argtypes
    assert lib.ivp_radau_submit_device.argtypes == dae
    assert lib.ivp_radau_solve_logged_device.argtypes == dae[:-1] + [C.POINTER(_lib.StepLogT), C.c_void_p]
    assert lib.ivp_radau_solve_dense_device.argtypes == dae[:-1] + [C.POINTER(_lib.DenseLogT), C.c_void_p]
    assert all(getattr(lib, n).restype is C.c_int for n in NEW)


def _c_params(text, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, f"{name} is not declared in the header"
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        const = p.startswith("const ")
        body = p[6:] if const else p
        depth = body.count("*")
        base = body.replace("*", " ").split()[0]
        out.append((base, depth, const))
    return out


def _rust_params(text, name):
    m = re.search(r"pub\s+fn\s+" + name + r"\s*\(([^;]*?)\)\s*->\s*c_int\s*;", text, re.S)
    assert m, f"{name} is not declared in the FFI crate"
    names = {"f64": "double", "usize": "size_t", "c_void": "void"}
    out = []
    for p in m.group(1).split(","):
        ty = " ".join(p.split(":", 1)[1].split())
        depth = ty.count("*")
        const = ty.startswith("*const")
        base = ty.replace("*const", "").replace("*mut", "").strip()
        out.append((names.get(base, base), depth, const))
    return out


@pytest.mark.parametrize("name", NEW)
def test_header_and_ffi_crate_declare_the_same_signature(name):
    header = open(os.path.join(ROOT, "include", "ivp_hip.h")).read()
    crate = open(os.path.join(ROOT, "rust", "ivp-hip-sys", "src", "lib.rs")).read()
    assert _c_params(header, name) == EXPECTED[name]
    assert _rust_params(crate, name) == EXPECTED[name]


def test_argument_errors_that_need_no_device():
    y0 = np.array([[2.0], [0.0]])
    eps = np.array([[1e-3]])
    f = ivp_amd.StiffVanDerPol()
    with pytest.raises(ValueError, match="t_eval is None"):
        Radau().solve_batch_logged(f, 0.0, 0.5, y0, eps, Options(t_eval=[0.0, 0.5]))
    with pytest.raises(ValueError, match="t_eval is None"):
        Radau().solve_batch_logged(f, 0.0, 0.5, y0, eps, Options(t_eval_per_trajectory=[np.array([0.0, 0.5])]))
    with pytest.raises(ValueError, match="wait=False needs device arrays"):
        Radau().solve_batch(f, 0.0, 0.5, y0, eps, Options(), wait=False)


# ---- the page sink on the host ------------------------------------------------------------------------------------------

POOL = 1 << 20   # doubles: 64 sub-pools of 16 K, a trajectory of 60 records of n = 3 takes ~4 K
CASES = [("decay", [0.5, 2.0, 300.0], [[1.0]] * 3, 2.0),
         ("vdp_eps", [1e-3, 1.25e-3], [[2.0, 0.0], [1.9, 0.1]], 0.5),
         ("robertson", [None, None], [[1.0, 0.0, 0.0], [0.9, 0.0, 0.1]], 40.0)]


def _gathered(name, pars, y0s, t1, chunk, **kw):
    res = T.run_emul(name, pars, y0s, 0.0, t1, chunk, paged_log=POOL, **kw)
    assert not res["log_overflow"]
    off, t, y = E.gather_pages(res, len(y0s[0]))
    return res, off, t, y


def _hold(res, off, t, y, models, tag):
    for b, m in enumerate(models):
        T.check_end(res, b, m, (tag, b))
        lo, hi = int(off[b]), int(off[b + 1])
        assert int(res["n_log"][b]) == hi - lo == len(m.t), (tag, b, hi - lo, len(m.t))
        assert T.same_vec(t[lo:hi], m.t), (tag, b, "t")
        assert all(T.same_vec(y[lo + q], m.y[q]) for q in range(hi - lo)), (tag, b, "y")


@pytest.mark.parametrize("chunk", [1, 7, T.UNBOUNDED])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gathered_pages_equal_the_models_records(case, chunk):
    name, pars, y0s, t1 = case
    models = [T.run_model(name, p, y, 0.0, t1) for p, y in zip(pars, y0s)]
    assert all(m.status == M.SUCCESS and len(m.t) == m.naccpt + 1 for m in models)
    assert max(len(m.t) for m in models) > 16   # more than one page of 32 slots at two slots per attempt
    _hold(*_gathered(name, pars, y0s, t1, chunk), models, (name, chunk))


FIRST_STEP = {"decay": 0.5, "vdp_eps": 0.125, "robertson": 0.4}


def records_twice(m, target):
    """the model's own evidence that one callback recorded twice: t[1] is the target x0 + first_step, and no accepted step
    ends there (within SolOut's 1e-12), so it was interpolated in the callback that also recorded the step's end t[2]"""
    return len(m.t) > 2 and m.t[1] == target and m.t[2] > target and all(abs((xo + hh) - target) > 1e-12 for _, xo, hh in m.segs)


@pytest.mark.parametrize("chunk", [1, 7, T.UNBOUNDED])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_first_step_records_twice_in_one_callback(case, chunk):
    """first_step too long for the tolerance: the first attempts are rejected, the accepted steps before x0 + first_step are
    not recorded (solout.rs:392-421), and the step that crosses it records the target AND its own end: two slots of one
    attempt.  (Robertson from [1, 0, 0] ends in SingularMatrix with this first_step: the initial record alone.)"""
    name, pars, y0s, t1 = case
    h = FIRST_STEP[name]
    models = [T.run_model(name, p, y, 0.0, t1, first_step=h, dense_output=True) for p, y in zip(pars, y0s)]
    assert any(records_twice(m, h) for m in models), [(m.t[:3], m.naccpt, len(m.t)) for m in models]
    _hold(*_gathered(name, pars, y0s, t1, chunk, first_step=h), models, (name, chunk, "first_step"))


@pytest.mark.parametrize("chunk", [1, 7, T.UNBOUNDED])
def test_a_zero_length_interval_has_the_one_record_of_the_early_return(chunk):
    """solve_ivp.rs:110-145: t1 == t0 returns [t0], [y0] before the method is entered (the model has no such path)."""
    y0s = [[2.0, 0.0], [1.5, 0.25]]
    t1s = np.array([0.5, 0.0])
    m = T.run_model("vdp_eps", 1e-3, y0s[0], 0.0, 0.5)
    res = T.run_emul("vdp_eps", [1e-3, 1e-3], y0s, 0.0, t1s, chunk, paged_log=POOL)
    off, t, y = E.gather_pages(res, 2)
    _hold(res, off, t, y, [m], ("zero-length neighbour", chunk))
    assert int(res["n_log"][1]) == 1 and int(off[2] - off[1]) == 1
    assert T.same(t[off[1]], 0.0) and T.same_vec(y[off[1]], y0s[1])
    assert int(res["status"][1]) == 0 and int(res["nstep"][1]) == 0 and T.same(res["h_next"][1], 0.0)


@pytest.mark.parametrize("chunk", [1, 7, T.UNBOUNDED])
def test_a_max_steps_exit_flushes_its_page(chunk):
    pars, y0s = [1e-3, 1.25e-3], [[2.0, 0.0], [1.9, 0.1]]
    models = [T.run_model("vdp_eps", p, y, 0.0, 0.5, max_steps=10) for p, y in zip(pars, y0s)]
    assert all(m.status == M.NEED_LARGER_NMAX and m.nstep == 11 and len(m.t) > 1 for m in models)
    _hold(*_gathered("vdp_eps", pars, y0s, 0.5, chunk, max_steps=10), models, ("max_steps", chunk))


def test_a_singular_matrix_exit_flushes_its_page():
    """newton_maxiter = 2 restarts between accepted steps; newton_maxiter = 1 ends in SingularMatrix with the initial record only"""
    for it, want in ((1, M.SINGULAR_MATRIX), (2, None)):
        m = T.run_model("vdp_eps", 1e-3, [2.0, 0.0], 0.0, 0.05, radau=dict(newton_maxiter=it))
        assert want is None or (m.status == want and len(m.t) == 1)
        for chunk in (1, T.UNBOUNDED):
            _hold(*_gathered("vdp_eps", [1e-3], [[2.0, 0.0]], 0.05, chunk, radau=dict(newton_maxiter=it)), [m], ("newton_maxiter", it, chunk))
