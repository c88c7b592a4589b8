"""The linear algebra of the wide Radau attempt (64 < n <= 512) on its own, on the MI355X: BdfG::lu_decomp + BdfG::lin_solve and
RadauW::lu_decomp_complex + RadauW::lin_solve_complex (ivp_amd/csrc/bdf_group.h, radau_group.h) on matrices in global memory,
one wavefront per matrix, C = ceil(n / 64) rows per lane, against the model's four functions in their numpy form
(tests/radau_wide_model.py, held to tests/radau_model.py bit for bit by tests/test_radau_wide_model_cpu.py).

n = 65 (one lane in the top slot), 129 (C = 3) and 512 (C = 8, every slot full).  The matrices are the families of
radau_wide_model.lu_families: a row exchange at every second pivot, each multiplier case, a tie between two rows (rows 2 and
n - 1: different slots), a NaN at [k][k] and a NaN elsewhere in column k, a zero pivot in the middle, a zero last diagonal
entry, and a matrix whose pivot row lies 64 rows below row k -- in a higher slot -- at every step that has one.

Claim: verdicts and every factor entry are bit-equal (a NaN equal to a NaN); the pivot rows are equal where the verdict is ok
and through the failing column otherwise; every solution component is bit-equal where the verdict is ok, and the right-hand
side of a singular matrix is untouched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import radau_wide_model as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
WIDTHS = (65, 129, 512)
_REF = {}


def reference(n):
    if n not in _REF:
        fams = W.lu_families(n)
        _REF[n] = (fams, [W.factorise_and_solve(f, W.NUMPY_FNS) for f in fams])
    return _REF[n]


def _failed_at(ref, key, n):
    """the column at which a failed factorisation stopped: the last pivot row the model wrote"""
    f = ref[key]
    zero = [k for k in range(n) if f[k, k] == 0.0] if key == "f" else [k for k in range(n) if ref["fr"][k, k] == 0.0 and ref["fi"][k, k] == 0.0]
    return zero[0] if zero else n - 1


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import torch
    so = str(tmp_path_factory.mktemp("radauwidelu") / "libradau_wide_lu_probe.so")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-Wno-unused-function", os.path.join(HERE, "helpers", "radau_wide_lu_probe.hip"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.radau_wide_lu_probe.restype = ctypes.c_int
    lib.radau_wide_lu_probe.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_int]

    def run(n, fams):
        dev = torch.device("cuda:0")
        nm = len(fams)
        cm = lambda k: torch.as_tensor(np.ascontiguousarray(np.stack([f[k].T for f in fams]).reshape(nm, n * n)), device=dev)   # column-major
        vec = lambda k: torch.as_tensor(np.ascontiguousarray(np.stack([f[k] for f in fams])), device=dev)
        a, b, ar, ai, br, bi = cm(1), vec(2), cm(3), cm(4), vec(5), vec(6)
        piv, pivc = (torch.full((nm, n), -1, dtype=torch.int32, device=dev) for _ in range(2))
        ok, okc = (torch.full((nm,), -1, dtype=torch.int32, device=dev) for _ in range(2))
        rc = lib.radau_wide_lu_probe(n, a.data_ptr(), b.data_ptr(), piv.data_ptr(), ok.data_ptr(), ar.data_ptr(), ai.data_ptr(),
                                     br.data_ptr(), bi.data_ptr(), pivc.data_ptr(), okc.data_ptr(), nm)
        assert rc == 0, rc
        host = lambda t: t.cpu().numpy()
        rm = lambda t: host(t).reshape(nm, n, n).transpose(0, 2, 1)
        return dict(f=rm(a), x=host(b), piv=host(piv), ok=host(ok), fr=rm(ar), fi=rm(ai), xr=host(br), xi=host(bi), pivc=host(pivc), okc=host(okc))
    return run


@pytest.mark.parametrize("n", WIDTHS)
def test_real_and_complex_lu_and_solves_equal_the_model(probe, n):
    fams, ref = reference(n)
    by = {r["tag"]: r for r in ref}
    # from the model alone: the set takes every branch the claim names
    assert [k for _, k, _ in by["exchange"]["swaps"]] == list(range(0, n - 1, 2)) == [k for _, k, _ in by["exchange"]["swapsc"]]
    assert by["real"]["cases"] == {"real"} and "imag" in by["imag"]["cases"] and "general" in by["general"]["cases"]
    assert by["tie"]["ip"][0] == 2 == by["tie"]["ipc"][0] and (n - 1) // 64 > 0
    assert by["nan_diagonal"]["ip"][1] == 1 == by["nan_diagonal"]["ipc"][1] and by["nan_below"]["ip"][1] != n - 2 != by["nan_below"]["ipc"][1]
    assert not by["zero_middle"]["ok"] and not by["zero_middle"]["okc"] and not by["zero_last"]["ok"] and not by["zero_last"]["okc"]
    assert by["zero_last"]["ip"][n - 2] == n - 2 and "skipped" in by["zero_last"]["cases"]
    h = by["higher_slot"]
    assert h["ok"] and h["okc"] and all(h["ip"][k] == k + 64 == h["ipc"][k] for k in range(n - 64))

    got = probe(n, fams)
    for q, (fam, r) in enumerate(zip(fams, ref)):
        tag = f"n = {n}, matrix {q} ({r['tag']})"
        assert int(got["ok"][q]) == int(r["ok"]), tag
        assert W.same_bits(got["f"][q], r["f"]), (tag, "real factors")
        upto = n - 1 if r["ok"] else min(_failed_at(r, "f", n) + 1, n - 1)
        assert [int(v) for v in got["piv"][q][:upto]] == [int(v) for v in r["ip"][:upto]], (tag, "real pivots")
        assert W.same_bits(got["x"][q], r["x"] if r["ok"] else fam[2]), (tag, "real solution" if r["ok"] else "right-hand side of a singular matrix touched")
        assert int(got["okc"][q]) == int(r["okc"]), tag
        assert W.same_bits(got["fr"][q], r["fr"]) and W.same_bits(got["fi"][q], r["fi"]), (tag, "complex factors")
        upto = n - 1 if r["okc"] else min(_failed_at(r, "fr", n) + 1, n - 1)
        assert [int(v) for v in got["pivc"][q][:upto]] == [int(v) for v in r["ipc"][:upto]], (tag, "complex pivots")
        assert W.same_bits(got["xr"][q], r["xr"] if r["okc"] else fam[5]) and W.same_bits(got["xi"][q], r["xi"] if r["okc"] else fam[6]), (tag, "complex solution")
