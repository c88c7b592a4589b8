"""The fixed-seed matrices on which Radau's three linear-algebra functions are judged on their own, shared by
tests/test_radau_cpu.py (the model against mpmath) and tests/test_gpu_radau_lu_probe.py (the device against the model).

Per N = 1..8, 67 systems (one wavefront plus a tail on the device).  Each system is a real matrix with a real right-hand
side (lu_decomp / lin_solve) AND a complex matrix with a complex right-hand side (lu_decomp_complex / lin_solve_complex):
  * random, NOT diagonally dominant (uniform in [-1, 1]): partial pivoting exchanges rows in most columns;
  * the matrices the kernel builds, E1 = fac1 I - J and E2 = (alphn I - J) + i betan I for a random J and a random h
    (identity products multiplied out, as radau_core.h forms them);
  * for N >= 2 three matrices whose first elimination column has a real, a purely imaginary and a general complex
    multiplier in row 0, and random matrices with a random mix of real / imaginary / general / zero entries;
  * a zero column (singular at that pivot);
  * a zero LAST pivot that only the elimination produces (exact in binary: multipliers of 1/2);
  * for N >= 2 an exact-zero complex pivot as the rotation Jacobian gives it: [[i b, b], [-b, i b]] in the leading block.
"""
import numpy as np

from tests import radau_model as M

NMAT = 67


def _entry_mix(rng, n):
    """complex matrix whose entries are real, imaginary, general or zero at random"""
    kind = rng.integers(0, 4, (n, n))
    re = rng.uniform(-1.0, 1.0, (n, n))
    im = rng.uniform(-1.0, 1.0, (n, n))
    re[(kind == 1) | (kind == 3)] = 0.0
    im[(kind == 0) | (kind == 3)] = 0.0
    return re, im


def make_set(n):
    """[(tag, A real (n, n), b (n), Ar, Ai, br, bi)] -- float64 numpy arrays, 67 entries"""
    rng = np.random.default_rng(7000 + n)
    out = []

    def add(tag, a, ar, ai):
        out.append((tag, np.array(a, dtype=np.float64), rng.uniform(-1.0, 1.0, n), np.array(ar, dtype=np.float64),
                    np.array(ai, dtype=np.float64), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)))

    for _ in range(16):   # the kernel's own matrices
        J = rng.uniform(-1.0, 1.0, (n, n)) * 10.0 ** rng.uniform(-1.0, 3.0)
        h = 10.0 ** rng.uniform(-4.0, 0.0)
        fac1, alphn, betan = M.U1 / h, M.ALPH / h, M.BETA / h
        eye = np.eye(n)
        add("kernel", eye * fac1 - J, eye * alphn - J, eye * betan)
    if n >= 2:
        for tag, mult in (("real", (0.5, 0.0)), ("imag", (0.0, -0.75)), ("general", (0.25, 0.5))):
            ar, ai = rng.uniform(-1.0, 1.0, (n, n)), rng.uniform(-1.0, 1.0, (n, n))
            ar[0, 0], ai[0, 0] = 3.0, 2.0            # row 0 stays the pivot row of column 0
            ar[0, 1], ai[0, 1] = mult
            add(tag, rng.uniform(-1.0, 1.0, (n, n)), ar, ai)
        for _ in range(6):
            re, im = _entry_mix(rng, n)
            add("mix", rng.uniform(-1.0, 1.0, (n, n)), re, im)
        rot = np.eye(n)
        roti = np.eye(n) * 0.0
        rot[:2, :2] = [[0.0, 2.0], [-2.0, 0.0]]
        roti[0, 0] = roti[1, 1] = 2.0
        add("zero_complex_pivot", rng.uniform(-1.0, 1.0, (n, n)), rot, roti)
    zc = rng.uniform(-1.0, 1.0, (n, n))
    zr, zi = rng.uniform(-1.0, 1.0, (n, n)), rng.uniform(-1.0, 1.0, (n, n))
    zc[:, n // 2] = 0.0
    zr[:, n // 2] = 0.0
    zi[:, n // 2] = 0.0
    add("zero_column", zc, zr, zi)
    last = np.eye(n) * 2.0
    lastr, lasti = np.eye(n) * 2.0, np.zeros((n, n))
    if n == 1:
        last[0, 0] = lastr[0, 0] = 0.0
    else:
        last[0, 0], last[0, n - 1], last[n - 1, 0], last[n - 1, n - 1] = 4.0, 2.0, 2.0, 1.0
        lastr[0, 0], lasti[0, 0], lastr[0, n - 1] = 0.0, 4.0, 2.0
        lastr[n - 1, 0], lasti[n - 1, 0], lastr[n - 1, n - 1] = 0.0, 2.0, 1.0
    add("zero_last_pivot", last, lastr, lasti)
    while len(out) < NMAT:
        add("random", rng.uniform(-1.0, 1.0, (n, n)), rng.uniform(-1.0, 1.0, (n, n)), rng.uniform(-1.0, 1.0, (n, n)))
    assert len(out) == NMAT
    return out


def pack_piv(ip, n):
    """the kernels' pivot word: row of column k in bits 4k .. 4k + 3, k < n - 1"""
    return sum(int(ip[k]) << (4 * k) for k in range(n - 1))


_REF = {}


def reference(n):
    """Per N, once: a list of dicts with the model's factors, pivots, verdicts and solutions of make_set(n).
    `failed` is the column at which a singular factorisation stopped (n - 1: the final check)."""
    if n in _REF:
        return _REF[n]
    out = []
    for tag, a, b, ar, ai, br, bi in make_set(n):
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
        out.append(dict(tag=tag, a=a, b=b, ar=ar, ai=ai, br=br, bi=bi,
                        f=np.array(f), ip=ip, ok=ok, x=np.array(x), swaps=len(piv), failed=_stop(f, None, n, ok),
                        fr=np.array(fr), fi=np.array(fi), ipc=ipc, okc=okc, xr=np.array(xr), xi=np.array(xi), swapsc=len(pivc),
                        cases=cases, failedc=_stop(fr, fi, n, okc)))
    _REF[n] = out
    return out


def _stop(fr, fi, n, ok):
    """The column at which the model's factorisation gave up: the first k < n - 1 whose sub-diagonal multipliers were never
    formed is not recoverable from the factors alone, so re-derive it the way the model decides: column k fails when every
    candidate |re| + |im| in rows k.. is zero; otherwise the final check on the last diagonal entry failed."""
    if ok:
        return None
    for k in range(n - 1):
        if all(abs(fr[i][k]) + (abs(fi[i][k]) if fi is not None else 0.0) == 0.0 for i in range(k, n)):
            return k
    return n - 1


def _bits_equal(got, want):
    return np.array_equal(np.ascontiguousarray(got, dtype=np.float64).view(np.uint64), np.ascontiguousarray(want, dtype=np.float64).view(np.uint64))


def _piv_prefix(word, upto):
    return [(int(word) >> (4 * k)) & 0xF for k in range(upto)]


def assert_equal_to_model(n, got):
    """`got`: what the device probe (tests/helpers/radau_lu_probe.hip) or its host twin (emul_radau_lu) returns for
    reference(n) -- f, x, piv, ok for the real systems, fr, fi, xr, xi, pivc, okc for the complex ones.
    The verdict and every factor entry bit-equal; the pivot word bit-equal where ok, equal through the failing column
    otherwise (the reference returns there; the attempt discards the word); the solution bit-equal where ok, the right-hand
    side of a singular matrix untouched."""
    ref = reference(n)
    n_sing = n_singc = 0
    for q, r in enumerate(ref):
        tag = f"N = {n}, matrix {q} ({r['tag']})"
        # ---- real: bdf_lu_decomp + radau_lin_solve
        assert int(got["ok"][q]) == int(r["ok"]), tag
        assert _bits_equal(got["f"][q], r["f"]), (tag, "real factors", got["f"][q], r["f"])
        if r["ok"]:
            assert int(got["piv"][q]) == pack_piv(r["ip"], n), (tag, hex(int(got["piv"][q])), r["ip"])
            assert _bits_equal(got["x"][q], r["x"]), (tag, "real solution", got["x"][q], r["x"])
        else:
            n_sing += 1
            upto = min(r["failed"] + 1, n - 1)
            assert _piv_prefix(got["piv"][q], upto) == [int(v) for v in r["ip"][:upto]], tag
            assert _bits_equal(got["x"][q], r["b"]), tag + ": right-hand side of a singular matrix touched"
        # ---- complex: radau_lu_decomp_complex + radau_lin_solve_complex
        assert int(got["okc"][q]) == int(r["okc"]), tag
        assert _bits_equal(got["fr"][q], r["fr"]) and _bits_equal(got["fi"][q], r["fi"]), (tag, "complex factors")
        if r["okc"]:
            assert int(got["pivc"][q]) == pack_piv(r["ipc"], n), (tag, hex(int(got["pivc"][q])), r["ipc"])
            assert _bits_equal(got["xr"][q], r["xr"]) and _bits_equal(got["xi"][q], r["xi"]), (tag, "complex solution")
        else:
            n_singc += 1
            upto = min(r["failedc"] + 1, n - 1)
            assert _piv_prefix(got["pivc"][q], upto) == [int(v) for v in r["ipc"][:upto]], tag
            assert _bits_equal(got["xr"][q], r["br"]) and _bits_equal(got["xi"][q], r["bi"]), tag + ": right-hand side touched"
    assert n_sing >= 2 and n_singc >= 2
