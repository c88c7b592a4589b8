"""The linear algebra of the group-per-trajectory Radau attempt on its own, on the MI355X: BdfG::lu_decomp + BdfG::lin_solve
and RadauG::lu_decomp_complex + RadauG::lin_solve_complex (ivp_amd/csrc/bdf_group.h, radau_group.h) with the factors in
LDS, one group of G lanes per matrix, against the CPU model's lu_decomp / lin_solve / lu_decomp_complex /
lin_solve_complex (tests/radau_model.py: src/matrix/lu.rs:37-302, src/matrix/linear.rs:55-217).

n = 9 (G = 16, seven idle lanes), 16 (a full group), 17 (G = 32), 33 and 64 (G = 64, partial and full).  The matrices are
those of tests/radau_lu_cases.py at these widths, thinned so that the model stays quick: the kernel's own E1 / E2, one matrix
per multiplier case of the complex elimination, mixed real / imaginary / general / zero entries, random matrices that are
not diagonally dominant (an exchange in almost every column), a zero column, a zero last pivot and an exact-zero complex
pivot.

Claim: verdicts and every factor entry are bit-equal; the pivot rows are equal where the verdict is ok and through the
failing column otherwise; every solution component is bit-equal where the verdict is ok, and the right-hand side of a
singular matrix is untouched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import radau_lu_cases as L
from tests import radau_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
WIDTHS = (9, 16, 17, 33, 64)


def pick(n):
    """A thinned tests/radau_lu_cases.make_set(n): every tagged matrix once, three of each repeated kind."""
    full = L.make_set(n)
    by = lambda tag: [s for s in full if s[0] == tag]
    few = 3
    out = by("kernel")[:few] + by("real") + by("imag") + by("general") + by("mix")[:few] + by("zero_complex_pivot") + \
        by("zero_column") + by("zero_last_pivot") + by("random")[:few]
    return out


_REF = {}


def reference(n):
    if n in _REF:
        return _REF[n]
    out = []
    for tag, a, b, ar, ai, br, bi in pick(n):
        f = [[float(v) for v in row] for row in a]
        ip, piv = [0] * n, []
        ok = M.lu_decomp(f, ip, piv)
        x = [float(v) for v in b]
        if ok:
            M.lin_solve(f, x, ip)
        fr = [[float(v) for v in row] for row in ar]
        fi = [[float(v) for v in row] for row in ai]
        ipc, pivc, cases = [0] * n, [], set()
        okc = M.lu_decomp_complex(fr, fi, ipc, pivc, cases)
        xr, xi = [float(v) for v in br], [float(v) for v in bi]
        if okc:
            M.lin_solve_complex(fr, fi, xr, xi, ipc)
        out.append(dict(tag=tag, a=a, b=b, ar=ar, ai=ai, br=br, bi=bi, f=np.array(f), ip=ip, ok=ok, x=np.array(x), swaps=piv,
                        failed=L._stop(f, None, n, ok), fr=np.array(fr), fi=np.array(fi), ipc=ipc, okc=okc, xr=np.array(xr),
                        xi=np.array(xi), swapsc=pivc, cases=cases, failedc=L._stop(fr, fi, n, okc)))
    _REF[n] = out
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import torch
    so = str(tmp_path_factory.mktemp("radaugrouplu") / "libradau_group_lu_probe.so")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-Wno-unused-function", os.path.join(HERE, "helpers", "radau_group_lu_probe.hip"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.radau_group_lu_probe.restype = ctypes.c_int
    lib.radau_group_lu_probe.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_int]

    def run(n, ref):
        dev = torch.device("cuda:0")
        nm = len(ref)
        up = lambda key, shape: torch.as_tensor(np.ascontiguousarray(np.stack([r[key] for r in ref]).reshape(shape)), device=dev)
        a, ar, ai = (up(k, (nm, n * n)) for k in ("a", "ar", "ai"))
        b, br, bi = (up(k, (nm, n)) for k in ("b", "br", "bi"))
        piv, pivc = (torch.full((nm, n), -1, dtype=torch.int32, device=dev) for _ in range(2))
        ok, okc = (torch.full((nm,), -1, dtype=torch.int32, device=dev) for _ in range(2))
        rc = lib.radau_group_lu_probe(n, a.data_ptr(), b.data_ptr(), piv.data_ptr(), ok.data_ptr(), ar.data_ptr(), ai.data_ptr(),
                                      br.data_ptr(), bi.data_ptr(), pivc.data_ptr(), okc.data_ptr(), nm)
        assert rc == 0, rc
        host = lambda t: t.cpu().numpy()
        return dict(f=host(a).reshape(nm, n, n), x=host(b), piv=host(piv), ok=host(ok),
                    fr=host(ar).reshape(nm, n, n), fi=host(ai).reshape(nm, n, n), xr=host(br), xi=host(bi), pivc=host(pivc), okc=host(okc))
    return run


@pytest.mark.parametrize("n", WIDTHS)
def test_real_and_complex_lu_and_solves_equal_the_model(probe, n):
    ref = reference(n)
    # from the model alone: the set takes every branch the claim names
    by_tag = lambda t: [r for r in ref if r["tag"] == t]
    for tag in ("real", "imag", "general"):
        assert tag in by_tag(tag)[0]["cases"] and by_tag(tag)[0]["okc"], (n, tag)
    assert set().union(*(r["cases"] for r in ref)) == {"real", "imag", "general"}
    for r in by_tag("random"):   # exchanges in (almost) every column: every column of these is looked at
        assert r["ok"] and r["okc"] and 2 * len(r["swaps"]) > n - 1 and 2 * len(r["swapsc"]) > n - 1, n
    assert {k for r in ref for _, k, _ in r["swaps"]} >= set(range(n - 2)) and {k for r in ref for _, k, _ in r["swapsc"]} >= set(range(n - 2))
    zc, z, zp = by_tag("zero_column")[0], by_tag("zero_last_pivot")[0], by_tag("zero_complex_pivot")[0]
    assert not zc["ok"] and not zc["okc"] and zc["failed"] == zc["failedc"] == n // 2
    assert not z["ok"] and not z["okc"] and z["failed"] == z["failedc"] == n - 1
    assert not zp["okc"] and zp["failedc"] == 1

    got = probe(n, ref)
    eq = L._bits_equal
    for q, r in enumerate(ref):
        tag = f"n = {n}, matrix {q} ({r['tag']})"
        assert int(got["ok"][q]) == int(r["ok"]), tag
        assert eq(got["f"][q], r["f"]), (tag, "real factors")
        upto = n - 1 if r["ok"] else min(r["failed"] + 1, n - 1)
        assert [int(v) for v in got["piv"][q][:upto]] == [int(v) for v in r["ip"][:upto]], (tag, "real pivots")
        assert eq(got["x"][q], r["x"] if r["ok"] else r["b"]), (tag, "real solution" if r["ok"] else "right-hand side of a singular matrix touched")
        assert int(got["okc"][q]) == int(r["okc"]), tag
        assert eq(got["fr"][q], r["fr"]) and eq(got["fi"][q], r["fi"]), (tag, "complex factors")
        upto = n - 1 if r["okc"] else min(r["failedc"] + 1, n - 1)
        assert [int(v) for v in got["pivc"][q][:upto]] == [int(v) for v in r["ipc"][:upto]], (tag, "complex pivots")
        assert eq(got["xr"][q], r["xr"] if r["okc"] else r["br"]) and eq(got["xi"][q], r["xi"] if r["okc"] else r["bi"]), (tag, "complex solution")
