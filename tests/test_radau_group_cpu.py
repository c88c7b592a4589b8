"""The host side of Radau for 8 < n <= 64 (radau_group.h), without a device: what ivp_radau_check / ivp_radau_dae_check
accept and what they still refuse.  The bound of the Radau path is n <= 64 -- the three factors of a trajectory stay in
LDS -- so the built-in 64-state problem (id 102) passes and the larger built-ins (100: n = 100, 101: n = 256) do not.

What needs a compiled problem (hiprtc, through a context) -- the refusals of IVP_RHS_BANDED and jac_sparsity beyond n = 8 --
is in tests/test_gpu_radau_group.py."""
import ctypes as C

import pytest

from ivp_amd import _lib

DENSE64 = (102, 64, 1)


def _check(prob, opt=None, dae=False, B=4):
    lib = _lib.load()
    p = _lib.ProblemT()
    p.rhs_id, p.n, p.n_params = prob
    o = _lib.OptionsT()
    lib.ivp_options_default(C.byref(o))
    for k, v in (opt or {}).items():
        setattr(o, k, v)
    s = _lib.RadauSettingsT()
    lib.ivp_radau_settings_default(C.byref(s))
    msg = C.create_string_buffer(512)
    if dae:
        d = _lib.RadauDaeT()   # no count given: a pure index-1 partition
        rc = lib.ivp_radau_dae_check(C.byref(p), B, C.byref(o), C.byref(s), C.byref(d), msg, 512)
    else:
        rc = lib.ivp_radau_check(C.byref(p), B, C.byref(o), C.byref(s), msg, 512)
    return rc, msg.value.decode()


@pytest.mark.parametrize("dae", [False, True])
def test_the_built_in_64_state_problem_is_accepted(dae):
    rc, msg = _check(DENSE64, dae=dae)
    assert rc == 0, msg


@pytest.mark.parametrize("dae", [False, True])
@pytest.mark.parametrize("prob, word", [((100, 100, 0), "n = 100"), ((101, 256, 1), "n = 256")])
def test_larger_systems_are_still_refused_with_the_new_bound(prob, word, dae):
    rc, msg = _check(prob, dae=dae)
    assert rc == -100 and "not yet" in msg and word in msg and "n <= 64" in msg, (rc, msg)


@pytest.mark.parametrize("dae", [False, True])
@pytest.mark.parametrize("opt, word", [({"fp_mode": 1}, "FMA"), ({"variant": 3}, "variant")])
def test_fma_and_variant_3_are_still_refused_at_n_64(opt, word, dae):
    rc, msg = _check(DENSE64, opt=opt, dae=dae)
    assert rc == -100 and "not yet" in msg and word in msg, (rc, msg)


def test_index_2_variables_still_need_a_mass_matrix_at_n_64():
    lib = _lib.load()
    p = _lib.ProblemT()
    p.rhs_id, p.n, p.n_params = DENSE64
    o = _lib.OptionsT()
    lib.ivp_options_default(C.byref(o))
    s = _lib.RadauSettingsT()
    lib.ivp_radau_settings_default(C.byref(s))
    d = _lib.RadauDaeT()
    d.has_nind2, d.nind2 = 1, 2
    msg = C.create_string_buffer(512)
    rc = lib.ivp_radau_dae_check(C.byref(p), 4, C.byref(o), C.byref(s), C.byref(d), msg, 512)
    assert rc == -100 and "not yet" in msg.value.decode() and "mass" in msg.value.decode()


def test_the_other_checks_still_run_at_n_64():
    assert _check(DENSE64, opt={"rtol": -1e-6})[0] == -3
    assert _check(DENSE64, opt={"has_first_step": 1, "first_step": 0.0})[0] == -5
    assert _check((102, 64, 0))[0] == -100   # the dimensions must be the problem's
