"""The host side of the banded Radau call, without a device: the three new symbols (exported, declared in the header, the
ctypes table and the Rust -sys file with the arguments of the plain call), the ABI version, and every refusal of
ivp_radau_banded_check that needs no compiled problem.  What needs one -- a problem without a pattern, a pattern without band
storage, event functions and FMA on a banded problem -- is in tests/test_gpu_radau_banded.py."""
import ctypes as C
import inspect
import os
import re

import pytest

from ivp_amd import Radau, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ivp_radau_banded_check", "ivp_radau_solve_banded_device", "ivp_radau_solve_banded")
SHO, ROBERTSON, DENSE64, SHO_EV = (1, 2, 0), (9, 3, 0), (102, 64, 1), (11, 2, 0)
NOTHING = ("the banded Radau call needs a problem compiled with IVP_RHS_BANDED (ivp_rhs_compile_sparse): "
           "it has nothing to do for this one")


def _check(prob=SHO, opt=None, rad=None, B=4, fn="ivp_radau_banded_check"):
    lib = _lib.load()
    p = _lib.ProblemT()
    p.rhs_id, p.n, p.n_params = prob
    o = _lib.OptionsT()
    lib.ivp_options_default(C.byref(o))
    for k, v in (opt or {}).items():
        setattr(o, k, v)
    s = _lib.RadauSettingsT()
    lib.ivp_radau_settings_default(C.byref(s))
    for k, v in (rad or {}).items():
        setattr(s, k, v)
    msg = C.create_string_buffer(512)
    rc = getattr(lib, fn)(C.byref(p), B, C.byref(o), C.byref(s), msg, 512)
    return rc, msg.value.decode()


def test_symbols_exported_and_declared_everywhere():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ivp_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "ivp-hip-sys", "src", "lib.rs")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.EXPORTS
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
        assert re.search(r"pub fn " + s + r"\s*\(", rust), s
        assert s in integ, s
    assert re.search(r"#define\s+IVP_HIP_ABI_VERSION\s+5\b", hdr) and lib.ivp_abi_version() == 5   # additive: the version stays

    def c_args(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        return [a.split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]

    def rust_args(name):
        m = re.search(r"pub fn " + name + r"\s*\(([^;]*?)\)\s*->\s*c_int;", rust, re.S)
        return [a.split(":")[0].strip() for a in m.group(1).replace("\n", " ").split(",")]
    # the signatures of the plain call
    assert c_args("ivp_radau_banded_check") == c_args("ivp_radau_check")
    assert c_args("ivp_radau_solve_banded") == c_args("ivp_radau_solve")
    assert c_args("ivp_radau_solve_banded_device") == c_args("ivp_radau_solve_device")
    for s in NEW:
        assert [a.lower() for a in rust_args(s)] == [a.lower() for a in c_args(s)], s
    assert len(lib.ivp_radau_solve_banded_device.argtypes) == len(c_args("ivp_radau_solve_device"))
    assert len(lib.ivp_radau_solve_banded.argtypes) == len(c_args("ivp_radau_solve"))


@pytest.mark.parametrize("prob", [SHO, ROBERTSON, DENSE64])
def test_a_built_in_problem_has_nothing_for_this_call(prob):
    rc, msg = _check(prob)
    assert rc == -100 and msg == NOTHING, (rc, msg)
    assert _check(prob, fn="ivp_radau_check") == (0, "")   # ... and the plain call still takes it


@pytest.mark.parametrize("prob, opt, rad, code, word", [
    (SHO, {"fp_mode": 1}, None, -100, "Radau with fp_mode = FMA: not yet (strict arithmetic only)"),
    (SHO, {"variant": 3}, None, -100, "Radau with variant = 3 (lane-cooperative kernels): not yet"),
    (SHO_EV, {}, None, -100, "Radau for problems with event functions: not yet on the accelerated path"),
    ((100, 100, 0), {}, None, -100, "Radau for n = 100: not yet on the accelerated path"),
    (SHO, {}, {"newton_maxiter": 0}, -1, "newton_maxiter must be positive"),
    (SHO, {}, {"newton_maxiter": 16}, -2, "newton_maxiter = 16 outside [1, 15]"),
    (SHO, {}, {"uround": 1.0}, -2, "uround"),
    (SHO, {}, {"safety_factor": 1.0}, -2, "safety_factor"),
    (SHO, {}, {"scale_min": 9.0}, -6, "scale factors"),
    (SHO, {"rtol": -1.0}, None, -3, "negative tolerance"),
    (SHO, {"has_first_step": 1, "first_step": 0.0}, None, -5, "first_step is zero"),
])
def test_everything_the_plain_call_refuses_stays_refused_with_its_text(prob, opt, rad, code, word):
    rc, msg = _check(prob, opt=opt, rad=rad)
    assert rc == code and word in msg, (rc, msg)
    assert _check(prob, opt=opt, rad=rad, fn="ivp_radau_check") == (rc, msg)   # the same code and text as the plain call


def test_variants_0_1_2_and_opt_method_make_no_difference():
    for v in (0, 1, 2):
        assert _check(SHO, opt={"variant": v}) == (-100, NOTHING)
    for m in (0, 3, 5, 99):
        assert _check(SHO, opt={"method": m}) == (-100, NOTHING)


def test_without_a_context_or_arguments_nothing_is_touched():
    lib = _lib.load()
    assert lib.ivp_radau_solve_banded(None, None, 1, None, None, None, 1, None, 1, None, None, None) == -100
    assert lib.ivp_radau_solve_banded_device(None, None, 1, None, None, None, 1, None, 1, None, None, None, None) == -100
    assert lib.ivp_radau_banded_check(None, 1, None, None, None, 0) == -100


def test_python_front_end():
    sig = inspect.signature(Radau.solve_batch_banded)
    assert list(sig.parameters)[1:] == ["f", "t0", "t1", "y0", "params", "options", "ctx", "out"]
    assert list(inspect.signature(Radau.solve_banded).parameters)[1:] == ["f", "t0", "t1", "y0", "options", "ctx"]
