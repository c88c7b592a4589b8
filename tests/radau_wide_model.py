"""tests/radau_model.py at the widths of the wide Radau kernels (64 < n <= 512), where its plain-Python linear algebra is too
slow: numpy restatements of lu_decomp, lin_solve, lu_decomp_complex, lin_solve_complex and fd_jac and of the dense linear
right-hand side, and `solve`, which runs radau_model.solve with the five swapped in.

They are vectorised over rows (and over rows and columns in the trailing update) and keep the model's operations per entry
in the model's order -- every entry is one chain of elementwise IEEE operations, so vectorising does not change a bit; the
three multiplier cases of the complex elimination are chosen per column by np.where (the columns of each case then take
that case's operation sequence).  tests/test_radau_wide_model_cpu.py
holds each of them to radau_model's bit for bit.

One addition: lu_decomp_complex records "skipped" in `cases` when a trailing column is left untouched by a pivot step --
its pivot-row entry is zero and the row exchange moves nothing -- the columns the device's elimination does not even read.
"""
import contextlib

import numpy as np

from tests import radau_model as M


def _rows_back(a, A):
    for r in range(len(a)):
        a[r][:] = A[r].tolist()


def _first_max_row(col):
    """offset of the first entry attaining the maximum of `col` (NaNs never win); 0 if col[0] is a NaN: the model's strict
    `>` scan from max_val = col[0]"""
    if col[0] != col[0]:
        return 0
    return int(np.argmax(np.where(np.isnan(col), -1.0, col)))


def lu_decomp(a, ip, pivots=None):
    n = len(a)
    if n == 1:
        return M_LU_DECOMP(a, ip, pivots)
    A = np.array(a, dtype=np.float64)
    ok = None
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            m = k + _first_max_row(np.abs(A[k:, k]))
            ip[k] = m
            if pivots is not None and m != k:
                pivots.append(("real", k, m))
            pivot = A[m, k]
            if pivot == 0.0:
                ok = False
                break
            if m != k:
                A[m, k], A[k, k] = A[k, k], A[m, k]
            t = np.float64(1.0) / pivot
            A[k + 1:, k] = -A[k + 1:, k] * t
            trow = A[m, k + 1:].copy()
            if m != k:
                A[m, k + 1:] = A[k, k + 1:]
                A[k, k + 1:] = trow
            nz = trow != 0.0
            if nz.all():   # (a slice instead of an index array: the same sums, without the gather and scatter)
                A[k + 1:, k + 1:] += np.outer(A[k + 1:, k], trow)
            elif nz.any():
                cols = np.nonzero(nz)[0] + (k + 1)
                A[k + 1:, cols] = A[k + 1:, cols] + np.outer(A[k + 1:, k], trow[nz])
    _rows_back(a, A)
    return bool(A[n - 1, n - 1] != 0.0) if ok is None else ok


def lin_solve(a, b, ip):
    n = len(a)
    if n == 1:
        return M_LIN_SOLVE(a, b, ip)
    A = np.array(a, dtype=np.float64)
    x = np.array(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            m = ip[k]
            t = x[m]
            x[m] = x[k]
            x[k] = t
            x[k + 1:] = x[k + 1:] + A[k + 1:, k] * t
        for k in range(n - 1, 0, -1):
            x[k] = x[k] / A[k, k]
            t = -x[k]
            x[:k] = x[:k] + A[:k, k] * t
        x[0] = x[0] / A[0, 0]
    b[:] = x.tolist()


def lu_decomp_complex(ar, ai, ip, pivots=None, cases=None):
    n = len(ar)
    if n == 1:
        return M_LU_DECOMP_COMPLEX(ar, ai, ip, pivots, cases)
    R = np.array(ar, dtype=np.float64)
    I = np.array(ai, dtype=np.float64)
    ok = None
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            m = k + _first_max_row(np.abs(R[k:, k]) + np.abs(I[k:, k]))
            ip[k] = m
            if pivots is not None and m != k:
                pivots.append(("complex", k, m))
            tr, ti = R[m, k], I[m, k]
            if abs(tr) + abs(ti) == 0.0:
                ok = False
                break
            if m != k:
                R[m, k], R[k, k] = R[k, k], R[m, k]
                I[m, k], I[k, k] = I[k, k], I[m, k]
            den = tr * tr + ti * ti
            tr, ti = tr / den, -ti / den
            cr, ci = R[k + 1:, k].copy(), I[k + 1:, k].copy()
            R[k + 1:, k] = -(cr * tr - ci * ti)
            I[k + 1:, k] = -(ci * tr + cr * ti)
            mr, mi = R[m, k + 1:].copy(), I[m, k + 1:].copy()
            moved = np.zeros(n - k - 1, dtype=bool)
            if m != k:
                moved = (mr.view(np.uint64) != R[k, k + 1:].view(np.uint64)) | (mi.view(np.uint64) != I[k, k + 1:].view(np.uint64))
                R[m, k + 1:] = R[k, k + 1:]
                I[m, k + 1:] = I[k, k + 1:]
                R[k, k + 1:] = mr
                I[k, k + 1:] = mi
            upd = np.abs(mr) + np.abs(mi) != 0.0
            if cases is not None and (~upd & ~moved).any():
                cases.add("skipped")
            if not upd.any():
                continue
            kind = np.where(mi == 0.0, 0, np.where(mr == 0.0, 1, 2))   # real, imaginary, general multiplier
            lr, li = R[k + 1:, k][:, None], I[k + 1:, k][:, None]
            for q, name in enumerate(("real", "imag", "general")):
                sel = upd & (kind == q)
                if not sel.any():
                    continue
                if cases is not None:
                    cases.add(name)
                cols = slice(k + 1, n) if sel.all() else np.nonzero(sel)[0] + (k + 1)   # (a slice where every column takes it)
                cmr, cmi = mr[sel], mi[sel]
                if q == 0:
                    prod_r, prod_i = lr * cmr, li * cmr
                elif q == 1:
                    prod_r, prod_i = -li * cmi, lr * cmi
                else:
                    prod_r, prod_i = lr * cmr, li * cmr
                    prod_r -= li * cmi
                    prod_i += lr * cmi
                R[k + 1:, cols] += prod_r
                I[k + 1:, cols] += prod_i
    _rows_back(ar, R)
    _rows_back(ai, I)
    return bool(abs(R[n - 1, n - 1]) + abs(I[n - 1, n - 1]) != 0.0) if ok is None else ok


def _cdiv(br, bi, ar, ai):
    den = ar * ar + ai * ai
    return (br * ar + bi * ai) / den, (bi * ar - br * ai) / den


def lin_solve_complex(ar, ai, br, bi, ip):
    n = len(ar)
    if n == 1:
        return M_LIN_SOLVE_COMPLEX(ar, ai, br, bi, ip)
    R = np.array(ar, dtype=np.float64)
    I = np.array(ai, dtype=np.float64)
    xr = np.array(br, dtype=np.float64)
    xi = np.array(bi, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            m = ip[k]
            tr, ti = xr[m], xi[m]
            xr[m], xi[m] = xr[k], xi[k]
            xr[k], xi[k] = tr, ti
            cr, ci = R[k + 1:, k], I[k + 1:, k]
            xr[k + 1:] = xr[k + 1:] + (cr * tr - ci * ti)
            xi[k + 1:] = xi[k + 1:] + (ci * tr + cr * ti)
        for k in range(n - 1, 0, -1):
            xr[k], xi[k] = _cdiv(xr[k], xi[k], R[k, k], I[k, k])
            tr, ti = -xr[k], -xi[k]
            cr, ci = R[:k, k], I[:k, k]
            xr[:k] = xr[:k] + (cr * tr - ci * ti)
            xi[:k] = xi[:k] + (ci * tr + cr * ti)
        xr[0], xi[0] = _cdiv(xr[0], xi[0], R[0, 0], I[0, 0])
    br[:] = xr.tolist()
    bi[:] = xi.tolist()


def fd_jac(f, x, y, jac):
    n = len(y)
    yp = list(y)
    fo = np.array(f(x, y), dtype=np.float64)
    eps = 1.4901161193847656e-08
    J = np.empty((n, n))
    with np.errstate(all="ignore"):
        for col in range(n):
            yo = y[col]
            pert = eps * M.rs_max(abs(yo), 1.0)
            yp[col] = yo + pert
            fp = np.array(f(x, yp), dtype=np.float64)
            yp[col] = yo
            J[:, col] = (fp - fo) / pert
    _rows_back(jac, J)


def rhs_dense_linear(a):
    """M.rhs_dense_linear: every row summed left to right (np.cumsum adds sequentially)."""
    A = np.array(a, dtype=np.float64)

    def f(x, y):
        with np.errstate(all="ignore"):
            return np.cumsum(A * np.array(y, dtype=np.float64)[None, :], axis=1)[:, -1].tolist()
    return f


def jac_dense_linear(a):
    rows = [list(map(float, r)) for r in a]

    def jac(x, y, J):
        for i, r in enumerate(rows):
            J[i][:] = r
    return jac


M_LU_DECOMP, M_LIN_SOLVE, M_LU_DECOMP_COMPLEX, M_LIN_SOLVE_COMPLEX, M_FD_JAC = \
    M.lu_decomp, M.lin_solve, M.lu_decomp_complex, M.lin_solve_complex, M.fd_jac


@contextlib.contextmanager
def swapped_in():
    M.lu_decomp, M.lin_solve, M.lu_decomp_complex, M.lin_solve_complex, M.fd_jac = \
        lu_decomp, lin_solve, lu_decomp_complex, lin_solve_complex, fd_jac
    try:
        yield
    finally:
        M.lu_decomp, M.lin_solve, M.lu_decomp_complex, M.lin_solve_complex, M.fd_jac = \
            M_LU_DECOMP, M_LIN_SOLVE, M_LU_DECOMP_COMPLEX, M_LIN_SOLVE_COMPLEX, M_FD_JAC


def solve(*args, **kw):
    """radau_model.solve with the numpy linear algebra and finite differences"""
    with swapped_in():
        return M.solve(*args, **kw)


# ---- matrix families of the linear-algebra tests (CPU: tests/test_radau_wide_model_cpu.py, device: the LU probe) -------------

def lu_families(n, seed=0):
    """[(tag, A (n, n), b (n), Ar, Ai, br, bi)], float64 arrays, row-major.  Every family names the branch it takes; the
    tests assert on the model's pivots / cases / verdicts that it does."""
    rng = np.random.default_rng(1000 * n + seed)
    noise = lambda s=1e-3: rng.uniform(-s, s, (n, n))
    out = []

    def add(tag, a, ar, ai):
        out.append((tag, np.array(a, dtype=np.float64), rng.uniform(-1.0, 1.0, n), np.array(ar, dtype=np.float64),
                    np.array(ai, dtype=np.float64), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)))

    def dominant(scale=1e-2):
        a = noise(scale)
        a[np.arange(n), np.arange(n)] = 2.0 + rng.uniform(0.0, 1.0, n)
        return a

    # a row exchange at exactly every second pivot: 2 x 2 blocks [[1, 4], [10, 1]] down the diagonal
    a = noise()
    for k in range(0, n - 1, 2):
        a[k, k], a[k, k + 1], a[k + 1, k], a[k + 1, k + 1] = 1.0, 4.0, 10.0, 1.0
    if n % 2:
        a[n - 1, n - 1] = 3.0
    add("exchange", a, a, noise())
    # each multiplier case of the complex elimination
    add("real", dominant(), dominant(), np.zeros((n, n)))
    add("imag", dominant(), np.zeros((n, n)), dominant())
    add("general", dominant(), dominant(), dominant(0.5))
    # a tie between two rows (the first wins); at n > 64 they lie in different slots of the device's row mapping
    a, ar, ai = dominant(), dominant(), noise()
    a[:, 0] = ar[:, 0] = rng.uniform(-1.0, 1.0, n)
    ai[:, 0] = 0.0
    a[2, 0] = a[n - 1, 0] = 7.0
    ar[2, 0], ar[n - 1, 0], ai[n - 1, 0] = 7.0, 3.0, -4.0
    add("tie", a, ar, ai)
    # a NaN at [k][k] (the pivot stays there), and a NaN elsewhere in column k (it never wins)
    a, ar, ai = dominant(), dominant(), dominant(0.5)
    a[1, 1] = ar[1, 1] = np.nan
    add("nan_diagonal", a, ar, ai)
    a, ar, ai = dominant(), dominant(), dominant(0.5)
    a[n - 2, 1] = ai[n - 2, 1] = np.nan
    add("nan_below", a, ar, ai)
    # a zero pivot in the middle: column n // 2 is zero
    a, ar, ai = dominant(), dominant(), dominant(0.5)
    a[:, n // 2] = ar[:, n // 2] = ai[:, n // 2] = 0.0
    add("zero_middle", a, ar, ai)
    # a zero last diagonal entry: the last row and column are zero
    a, ar, ai = dominant(), dominant(), dominant(0.5)
    for m_ in (a, ar, ai):
        m_[n - 1, :] = 0.0
        m_[:, n - 1] = 0.0
    add("zero_last", a, ar, ai)
    if n > 64:
        # the pivot row lies in a higher slot than row k at every step that has one: 5.0 at [k + 64][k]
        a, ar, ai = noise(), noise(), noise()
        for m_ in (a, ar):
            m_[np.arange(n), np.arange(n)] = 1.0
        for k in range(n - 64):
            a[k + 64, k] = 5.0
            ar[k + 64, k], ai[k + 64, k] = 3.0, -2.0
        add("higher_slot", a, ar, ai)
    return out


def same_bits(got, want):
    """bit equality of two float64 arrays, a NaN equal to any NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(got) & np.isnan(want)
    return bool(np.all(nan | (got.view(np.uint64) == want.view(np.uint64))))


def factorise_and_solve(fam, fns):
    """run one family through (lu_decomp, lin_solve, lu_decomp_complex, lin_solve_complex) = fns; a right-hand side is
    solved only where the factorisation reports ok, as the attempt does"""
    tag, a, b, ar, ai, br, bi = fam
    n = len(a)
    lu, ls, luc, lsc = fns
    f, ip, swaps = a.tolist(), [0] * n, []
    ok = lu(f, ip, swaps)
    x = b.tolist()
    if ok:
        ls(f, x, ip)
    fr, fi, ipc, swapsc, cases = ar.tolist(), ai.tolist(), [0] * n, [], set()
    okc = luc(fr, fi, ipc, swapsc, cases)
    xr, xi = br.tolist(), bi.tolist()
    if okc:
        lsc(fr, fi, xr, xi, ipc)
    return dict(tag=tag, ok=ok, f=np.array(f), ip=ip, swaps=swaps, x=np.array(x), okc=okc, fr=np.array(fr), fi=np.array(fi), ipc=ipc,
                swapsc=swapsc, cases=cases, xr=np.array(xr), xi=np.array(xi))


NUMPY_FNS = (lu_decomp, lin_solve, lu_decomp_complex, lin_solve_complex)
MODEL_FNS = (M_LU_DECOMP, M_LIN_SOLVE, M_LU_DECOMP_COMPLEX, M_LIN_SOLVE_COMPLEX)
