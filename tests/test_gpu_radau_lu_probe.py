"""The linear algebra of the Radau attempt on its own, on the MI355X: bdf_lu_decomp + radau_lin_solve and
radau_lu_decomp_complex + radau_lin_solve_complex (ivp_amd/csrc/bdf_core.h, radau_core.h) for N = 1..8, one lane per
matrix, against the CPU model's lu_decomp / lin_solve / lu_decomp_complex / lin_solve_complex (tests/radau_model.py:
src/matrix/lu.rs:37-302, src/matrix/linear.rs:55-217, one rounding per operation).

Claim: the verdict and every factor entry are bit-equal; the pivot word is bit-equal where the verdict is ok and equal
through the failing column otherwise (the reference returns at that column and leaves the later pivots undefined; the
attempt discards the word and factorises again); every solution component is bit-equal where the verdict is ok, and the
right-hand side of a singular matrix is untouched.

Through whole solves these functions are seen only after Newton contraction, which hides a wrong low-order bit or a wrong
exchange in a column that rarely pivots.  The matrices (tests/radau_lu_cases.py, 67 per N: one wavefront plus a tail) are
random and not diagonally dominant, the kernel's own E1 / E2, one per multiplier case of the complex elimination, a zero
column, a zero last pivot and an exact-zero complex pivot.  How accurate the model's solutions are is measured against
mpmath in tests/test_radau_cpu.py; the device inherits that through the bit equality asserted here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import radau_lu_cases as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import torch
    so = str(tmp_path_factory.mktemp("radaulu") / "libradau_lu_probe.so")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-Wno-unused-function", os.path.join(HERE, "helpers", "radau_lu_probe.hip"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.radau_lu_probe.restype = ctypes.c_int
    lib.radau_lu_probe.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_int]

    def run(n, ref):
        dev = torch.device("cuda:0")
        nm = len(ref)
        up = lambda key, shape: torch.as_tensor(np.ascontiguousarray(np.stack([r[key] for r in ref]).reshape(shape)), device=dev)
        a, ar, ai = (up(k, (nm, n * n)) for k in ("a", "ar", "ai"))
        b, br, bi = (up(k, (nm, n)) for k in ("b", "br", "bi"))
        piv, pivc = (torch.full((nm,), -1, dtype=torch.int32, device=dev) for _ in range(2))
        ok, okc = (torch.full((nm,), -1, dtype=torch.int32, device=dev) for _ in range(2))
        rc = lib.radau_lu_probe(n, a.data_ptr(), b.data_ptr(), piv.data_ptr(), ok.data_ptr(), ar.data_ptr(), ai.data_ptr(),
                                br.data_ptr(), bi.data_ptr(), pivc.data_ptr(), okc.data_ptr(), nm)
        assert rc == 0, rc
        host = lambda t: t.cpu().numpy()
        return dict(f=host(a).reshape(nm, n, n), x=host(b), piv=host(piv).view(np.uint32), ok=host(ok),
                    fr=host(ar).reshape(nm, n, n), fi=host(ai).reshape(nm, n, n), xr=host(br), xi=host(bi),
                    pivc=host(pivc).view(np.uint32), okc=host(okc))
    return run


def test_the_reference_set_exchanges_rows_and_takes_every_branch():
    """From the model alone: more than a quarter of all eliminated columns exchange rows, in the real and in the complex
    factorisation; for N >= 2 all three multiplier cases occur, each in the matrix built for it; every N has singular
    verdicts from a zero column, from the final check and (N >= 2) from the exact-zero complex pivot."""
    for n in range(1, 9):
        ref = L.reference(n)
        assert len(ref) == L.NMAT
        by_tag = lambda t: [r for r in ref if r["tag"] == t]
        assert not by_tag("zero_column")[0]["ok"] and not by_tag("zero_column")[0]["okc"]
        assert by_tag("zero_column")[0]["failed"] == by_tag("zero_column")[0]["failedc"] == n // 2
        z = by_tag("zero_last_pivot")[0]
        assert not z["ok"] and not z["okc"] and z["failed"] == z["failedc"] == n - 1
        assert sum(r["ok"] for r in ref) >= 60 and sum(r["okc"] for r in ref) >= 60
        if n == 1:
            continue
        cols = sum((n - 1) if r["failed"] is None else r["failed"] for r in ref)
        colsc = sum((n - 1) if r["failedc"] is None else r["failedc"] for r in ref)
        swaps, swapsc = sum(r["swaps"] for r in ref), sum(r["swapsc"] for r in ref)
        print(f"N = {n}: row exchanges {swaps} of {cols} real columns, {swapsc} of {colsc} complex columns")
        assert 4 * swaps > cols and 4 * swapsc > colsc, (n, swaps, cols, swapsc, colsc)
        for tag in ("real", "imag", "general"):
            assert tag in by_tag(tag)[0]["cases"] and by_tag(tag)[0]["okc"], (n, tag)
        assert set().union(*(r["cases"] for r in ref)) == {"real", "imag", "general"}
        zc = by_tag("zero_complex_pivot")[0]
        assert not zc["okc"] and zc["failedc"] == 1


@pytest.mark.parametrize("n", range(1, 9))
def test_real_and_complex_lu_and_solves_equal_the_model(probe, n):
    L.assert_equal_to_model(n, probe(n, L.reference(n)))
