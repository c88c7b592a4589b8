"""The host side of the Radau events call, without a device: the new symbols (exported, declared in the header, the ctypes
table and the Rust -sys file with the same arguments), every refusal through ivp_radau_events_check, and the refusals of the
old entry points that stay.  What needs a compiled problem (n = 65, a mass hook with dae = NULL) is in
tests/test_gpu_radau_events.py."""
import ctypes as C
import inspect
import os
import re

import pytest

from ivp_amd import Radau, _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ivp_radau_events_check", "ivp_radau_solve_events_device", "ivp_radau_solve_events")
SHO_EV, BALL, RATIONAL_EV, SHO, ROBERTSON = (11, 2, 0), (12, 2, 2), (14, 2, 0), (1, 2, 0), (9, 3, 0)


def _check(prob=SHO_EV, opt=None, rad=None, dae=None, B=4, fn="ivp_radau_events_check"):
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
    d = None
    if dae is not None:
        d = _lib.RadauDaeT()
        for k, v in dae.items():
            setattr(d, "has_" + k, 1)
            setattr(d, k, v)
    msg = C.create_string_buffer(512)
    if fn == "ivp_radau_check":
        rc = lib.ivp_radau_check(C.byref(p), B, C.byref(o), C.byref(s), msg, 512)
    else:
        rc = getattr(lib, fn)(C.byref(p), B, C.byref(o), C.byref(s), None if d is None else C.byref(d), msg, 512)
    return rc, msg.value.decode()


def test_symbols_exported_and_declared_everywhere():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ivp_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "ivp-hip-sys", "src", "lib.rs")).read()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.EXPORTS
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
        assert re.search(r"pub fn " + s + r"\s*\(", rust), s
    assert re.search(r"#define\s+IVP_HIP_ABI_VERSION\s+5\b", hdr) and lib.ivp_abi_version() == 5   # additive: the version stays

    def c_args(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        return [a.split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]

    def rust_args(name):
        m = re.search(r"pub fn " + name + r"\s*\(([^;]*?)\)\s*->\s*c_int;", rust, re.S)
        return [a.split(":")[0].strip() for a in m.group(1).replace("\n", " ").split(",")]
    # the device form is ivp_radau_solve_dense_device with `ev` for `dense`; the host form drops the stream
    dev = c_args("ivp_radau_solve_events_device")
    assert dev == [("ev" if a == "dense" else a) for a in c_args("ivp_radau_solve_dense_device")]
    assert c_args("ivp_radau_solve_events") == dev[:-1]
    assert c_args("ivp_radau_events_check") == c_args("ivp_radau_dae_check")
    for s in NEW:
        assert [a.lower() for a in rust_args(s)] == [a.lower() for a in c_args(s)], s
    assert len(lib.ivp_radau_solve_events_device.argtypes) == len(dev) and len(lib.ivp_radau_solve_events.argtypes) == len(dev) - 1


@pytest.mark.parametrize("prob", [SHO_EV, BALL])
def test_a_problem_with_event_functions_passes_only_here(prob):
    assert _check(prob) == (0, "")
    assert _check(prob, dae={}) == (0, "")           # a given (empty) partition: the DAE rules, still a pure ODE
    for fn in ("ivp_radau_check", "ivp_radau_dae_check"):
        rc, msg = _check(prob, fn=fn)
        assert rc == -100 and msg == "Radau for problems with event functions: not yet on the accelerated path", (fn, rc, msg)


def test_a_problem_without_event_functions_is_refused_in_the_wording_of_the_event_log():
    for prob in (SHO, ROBERTSON):
        rc, msg = _check(prob)
        assert rc == -100 and msg == "the problem defines no event functions: there is no event log to deliver", (rc, msg)


@pytest.mark.parametrize("prob, opt, rad, dae, code, word", [
    (SHO_EV, {"fp_mode": 1}, None, None, -100, "Radau with fp_mode = FMA: not yet (strict arithmetic only)"),
    (SHO_EV, {"variant": 3}, None, None, -100, "Radau with variant = 3 (lane-cooperative kernels): not yet"),
    ((100, 100, 0), {}, None, None, -100, "Radau for n = 100: not yet on the accelerated path"),
    (SHO_EV, {}, None, {"nind2": 1}, -100, "index-2 / index-3 variables for a problem without a mass matrix"),
    (SHO_EV, {}, None, {"nind1": 3}, -7, "invalid DAE partition"),
    (SHO_EV, {}, {"newton_maxiter": 0}, None, -1, "newton_maxiter must be positive"),
    (SHO_EV, {}, {"uround": 1.0}, None, -2, "uround"),
    (SHO_EV, {"rtol": -1.0}, None, None, -3, "negative tolerance"),
    (SHO_EV, {"has_first_step": 1, "first_step": 0.0}, None, None, -5, "first_step is zero"),
])
def test_everything_else_stays_refused_with_its_text(prob, opt, rad, dae, code, word):
    rc, msg = _check(prob, opt=opt, rad=rad, dae=dae)
    assert rc == code and word in msg, (rc, msg)


def test_more_than_four_event_functions_need_the_vec_arrays():
    """no built-in has more than four, so the rule is exercised on the device (tests/test_gpu_radau_events.py); the check
    function applies it to what it can see: three event functions pass without the arrays"""
    assert _check(RATIONAL_EV) == (0, "")


def test_opt_method_is_ignored():
    for m in range(0, 6):
        assert _check(SHO_EV, opt={"method": m}) == (0, "")
    assert _check(SHO_EV, opt={"method": 99}) == (0, "")


def test_without_a_context_or_arguments_nothing_is_touched():
    lib = _lib.load()
    assert lib.ivp_radau_solve_events(None, None, 1, None, None, None, 1, None, 1, None, None, None, None, None) == -100
    assert lib.ivp_radau_solve_events_device(None, None, 1, None, None, None, 1, None, 1, None, None, None, None, None, None) == -100
    assert lib.ivp_radau_events_check(None, 1, None, None, None, None, 0) == -100


def test_python_front_end():
    sig = inspect.signature(Radau.solve_batch_events)
    assert list(sig.parameters) == ["self", "f", "t0", "t1", "y0", "params", "options", "ctx"]
    es = inspect.signature(api.solve_ivp_batch_events)
    assert list(es.parameters)[-2:] == ["_radau", "_radau_dae"] and es.parameters["_radau"].default is None
    doc = inspect.getdoc(inspect.getmodule(Radau))
    assert "solve_batch_events" in doc and "events in any form" not in doc
    assert "events beyond n = 64" in doc and "multi-GPU" in doc
