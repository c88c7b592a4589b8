"""The host side of the Radau DAE call, without a device: ivp_radau_dae_check through ctypes and through a plain-C client
(tests/c_abi/radau_dae_check_main.c), the ctypes structure, the error code, and the Python front end's arguments.

What needs a compiled problem with a mass matrix (hiprtc, through a context) -- the refusals of such a problem by every
other entry point, the compile-time refusals of IVP_RHS_HAS_MASS -- is in tests/test_gpu_radau_dae.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from ivp_amd import ConfigError, Radau, _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(n1=None, n2=None, n3=None, prob=(9, 3, 0), opt=None, rad=None, dae=True, B=4):
    lib = _lib.load()
    p = _lib.ProblemT()
    p.rhs_id, p.n, p.n_params = prob   # Robertson
    o = _lib.OptionsT()
    lib.ivp_options_default(C.byref(o))
    for k, v in (opt or {}).items():
        setattr(o, k, v)
    s = _lib.RadauSettingsT()
    lib.ivp_radau_settings_default(C.byref(s))
    for k, v in (rad or {}).items():
        setattr(s, k, v)
    d = _lib.RadauDaeT()
    d.has_nind1, d.nind1 = (0, 0) if n1 is None else (1, n1)
    d.has_nind2, d.nind2 = (0, 0) if n2 is None else (1, n2)
    d.has_nind3, d.nind3 = (0, 0) if n3 is None else (1, n3)
    msg = C.create_string_buffer(512)
    rc = lib.ivp_radau_dae_check(C.byref(p), B, C.byref(o), C.byref(s), C.byref(d) if dae else None, msg, 512)
    return rc, msg.value.decode()


def test_struct_and_error_code():
    assert C.sizeof(_lib.RadauDaeT) == 32 and C.sizeof(_lib.RadauSettingsT) == 56
    assert [f[0] for f in _lib.RadauDaeT._fields_] == ["has_nind1", "nind1", "has_nind2", "nind2", "has_nind3", "nind3", "reserved"]
    assert _lib.ERRORS[-7] == "IVP_ERR_INVALID_DAE_PARTITION"
    hdr = open(os.path.join(ROOT, "include", "ivp_hip.h")).read()
    assert re.search(r"IVP_ERR_INVALID_DAE_PARTITION\s*=\s*-7", hdr) and re.search(r"#define\s+IVP_RHS_HAS_MASS\s+4u", hdr)
    assert re.search(r"#define\s+IVP_HIP_ABI_VERSION\s+5\b", hdr)   # additive: the version stays
    assert api.RHS_HAS_MASS == 4
    assert ConfigError(-7, "x").code == -7 and "IVP_ERR_INVALID_DAE_PARTITION" in str(ConfigError(-7, "x"))


@pytest.mark.parametrize("part", [(None, None, None), (3, None, None), (3, 0, 0), (None, 0, None), (None, None, 0), (None, 0, 0), (3, 0, None)])
def test_valid_partitions_of_a_problem_without_a_mass_matrix(part):
    rc, msg = _check(*part)
    assert rc == 0, msg


def test_null_dae_is_a_pure_ode_partition():
    assert _check(dae=False)[0] == 0


@pytest.mark.parametrize("part", [
    (2, None, None), (4, None, None), (0, None, None),      # nind1 given: the sum must be n
    (2, 1, 1), (3, 1, None), (1, 1, 0),
    (None, 2, 2), (None, 4, None), (None, None, 4),         # nind1 omitted: nind2 + nind3 > n
    (None, -1, None), (-1, 2, 2), (4, -1, None), (None, 2, -2),   # negative counts
    (None, 2 ** 31 - 1, 2 ** 31 - 1),
])
def test_invalid_partitions_are_code_minus_7(part):
    rc, msg = _check(*part)
    assert rc == -7 and "partition" in msg, (rc, msg)


@pytest.mark.parametrize("part", [(None, 1, None), (None, None, 1), (1, 1, 1), (0, 3, 0), (None, 1, 2)])
def test_index_2_and_3_variables_need_a_mass_matrix(part):
    rc, msg = _check(*part)
    assert rc == -100 and "not yet" in msg and "mass" in msg, (rc, msg)


def test_order_of_the_checks():
    """radau.rs: the struct's fields (:132-205), the partition (:210-246), the step size (:248-261)"""
    assert _check(2, opt={"has_first_step": 1, "first_step": 0.0})[0] == -7
    assert _check(opt={"has_first_step": 1, "first_step": 0.0})[0] == -5
    assert _check(2, rad={"newton_maxiter": 0})[0] == -1
    assert _check(2, rad={"uround": 1.0})[0] == -2
    assert _check(2, opt={"rtol": -1.0})[0] == -3


@pytest.mark.parametrize("prob, opt, word", [
    ((100, 100, 0), {}, "n = 100"),
    ((11, 2, 0), {}, "event"),
    ((9, 3, 0), {"fp_mode": 1}, "FMA"),
    ((9, 3, 0), {"variant": 3}, "variant"),
])
def test_the_refusals_of_the_plain_radau_call_apply(prob, opt, word):
    rc, msg = _check(prob=prob, opt=opt)
    assert rc == -100 and "not yet" in msg and word in msg, msg


def test_without_a_context_nothing_is_validated():
    lib = _lib.load()
    assert lib.ivp_radau_solve_dae(None, None, 1, None, None, None, 1, None, 1, None, None, None, None) == -100
    assert lib.ivp_radau_solve_dae_device(None, None, 1, None, None, None, 1, None, 1, None, None, None, None, None) == -100
    assert lib.ivp_radau_dae_check(None, 1, None, None, None, None, 0) == -100


def test_c_client(tmp_path):
    exe = str(tmp_path / "radau_dae_check")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_abi", "radau_dae_check_main.c"), "-o", exe,
                           "-L", os.path.join(ROOT, "ivp_amd"), "-livp_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "ivp_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_python_front_end_arguments():
    sig = inspect.signature(api.DeviceIVP.__init__)
    assert list(sig.parameters)[-1] == "mass" and sig.parameters["mass"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["mass"].default is False
    rs = inspect.signature(Radau.__init__)
    assert list(rs.parameters)[-3:] == ["nind1", "nind2", "nind3"] and all(rs.parameters[k].default is None for k in ("nind1", "nind2", "nind3"))
    # the DAE entry point is taken only when there is something for it to do
    assert Radau()._dae() is None and Radau()._dae(object()) is None
    d = Radau(nind2=1)._dae()
    assert (d.has_nind1, d.has_nind2, d.nind2, d.has_nind3) == (0, 1, 1, 0)
    d = Radau(nind1=4, nind2=1, nind3=0)._dae()
    assert (d.has_nind1, d.nind1, d.has_nind2, d.nind2, d.has_nind3, d.nind3) == (1, 4, 1, 1, 1, 0)

    class WithMass:
        has_mass = True
    assert Radau()._dae(WithMass()) is not None


def test_mass_with_a_sparsity_pattern_or_n_above_8_is_refused_before_anything_is_compiled():
    """a pattern takes the ivp_rhs_compile_sparse branch, which refuses the mass flag (tests/test_gpu_radau_dae.py): the front end
    must not get there and lose M silently"""
    src = "__device__ void ode(double x, const double* y, double* d, const double* p) { d[0] = -y[0]; d[1] = -y[1]; }\n" \
          "__device__ void mass(double* m, const double* p) { m[0] = 1.0; }\n"
    pattern = ([0, 1, 2], [0, 1])
    with pytest.raises(ValueError, match="jac_sparsity"):
        api.DeviceIVP(src, 2, jac_sparsity=pattern, mass=True)
    with pytest.raises(ValueError, match="jac_sparsity"):
        api.DeviceIVP(src, 2, jac_sparsity=[[1, 0], [0, 1]], mass=True)
    with pytest.raises(ValueError, match="banded"):
        api.DeviceIVP(src, 2, jac_sparsity=pattern, jac_storage="banded", mass=True)
    with pytest.raises(ValueError, match="n <= 8"):
        api.DeviceIVP(src, 9, mass=True)
