"""The linear algebra of the banded Radau attempt (ivp_amd/csrc/bdf_band.h, radau_band.h) restated in numpy ON THE BAND LAYOUT:
lu_decomp_band, lin_solve_band, lu_decomp_band_complex and lin_solve_band_complex.

Layout (bdf_band.h; KD = ml + mu): factor entry (i, j), j - KD <= i <= j + ml, at j * W + (KD + i - j), W = 2 ml + mu + 1; the
ml extra superdiagonals take the fill of row exchanges.  Slots of edge columns that correspond to no matrix entry hold +0.0
and are never touched.

Each function walks the pivots like the dense model (tests/radau_model.py, tests/radau_wide_model.py) and performs, on every
in-band entry, the dense model's operations on the same operands in the same order: the pivot search over rows
k..min(k + ml, n - 1) (first row attaining the maximum, NaNs never win, a NaN at [k][k] keeps m = k), the trailing columns
k + 1..min(k + KD, n - 1), the `t != 0` guard, the three multiplier cases of the complex elimination.  Every operation is one
float64 operation on numpy scalars, rounded once.  tests/test_radau_band_model_cpu.py holds the four to
radau_wide_model.NUMPY_FNS bit for bit on the band.
"""
import numpy as np


def width(ml, mu):
    return 2 * ml + mu + 1


def at(i, j, ml, mu):
    return j * width(ml, mu) + (ml + mu + i - j)


def band_slots(n, ml, mu):
    """(rows, cols, flat slots) of every factor-band slot that is a matrix entry"""
    kd, w = ml + mu, width(ml, mu)
    j, off = np.meshgrid(np.arange(n), np.arange(w), indexing="ij")
    i = j + off - kd
    ok = (i >= 0) & (i < n)
    return i[ok], j[ok], (j * w + off)[ok]


def pack(a, ml, mu):
    """a dense (n, n) matrix into a factor block (entries outside the factor band are dropped, unused slots +0.0)"""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    i, j, s = band_slots(n, ml, mu)
    out = np.zeros(n * width(ml, mu))
    out[s] = a[i, j]
    return out


def unpack(blk, n, ml, mu):
    """the in-band entries of a factor block as a dense matrix (zeros elsewhere)"""
    i, j, s = band_slots(n, ml, mu)
    out = np.zeros((n, n))
    out[i, j] = np.asarray(blk)[s]
    return out


def _first_max(vals):
    """offset of the first entry attaining the maximum (NaNs never win); 0 if vals[0] is a NaN"""
    if vals[0] != vals[0]:
        return 0
    best, m = vals[0], 0
    for r in range(1, len(vals)):
        if vals[r] > best:
            best, m = vals[r], r
    return m


def lu_decomp_band(a, n, ml, mu, ip, pivots=None):
    """in place on the float64 block a; pivot rows to ip[0..n-2]; False: singular"""
    kd = ml + mu
    A = lambda i, j: at(i, j, ml, mu)
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            last = min(k + ml, n - 1)
            m = k + _first_max([abs(a[A(i, k)]) for i in range(k, last + 1)])
            ip[k] = m
            if pivots is not None and m != k:
                pivots.append(("real", k, m))
            pivot = a[A(m, k)]
            if pivot == 0.0:
                return False
            if m != k:
                a[A(m, k)], a[A(k, k)] = a[A(k, k)], a[A(m, k)]
            t = np.float64(1.0) / pivot
            for i in range(k + 1, last + 1):
                a[A(i, k)] = -a[A(i, k)] * t
            for j in range(k + 1, min(k + kd, n - 1) + 1):
                tj = a[A(m, j)]
                if m != k:
                    a[A(m, j)] = a[A(k, j)]
                    a[A(k, j)] = tj
                if tj != 0.0:
                    for i in range(k + 1, last + 1):
                        a[A(i, j)] = a[A(i, j)] + a[A(i, k)] * tj
    return bool(a[A(n - 1, n - 1)] != 0.0)


def lin_solve_band(a, n, ml, mu, b, ip):
    kd = ml + mu
    A = lambda i, j: at(i, j, ml, mu)
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            m = ip[k]
            t = b[m]
            b[m] = b[k]
            b[k] = t
            for i in range(k + 1, min(k + ml, n - 1) + 1):
                b[i] = b[i] + a[A(i, k)] * t
        for k in range(n - 1, -1, -1):
            b[k] = b[k] / a[A(k, k)]
            t = -b[k]
            for i in range(max(k - kd, 0), k):
                b[i] = b[i] + a[A(i, k)] * t


def lu_decomp_band_complex(ar, ai, n, ml, mu, ip, pivots=None, cases=None):
    kd = ml + mu
    A = lambda i, j: at(i, j, ml, mu)
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            last = min(k + ml, n - 1)
            m = k + _first_max([abs(ar[A(i, k)]) + abs(ai[A(i, k)]) for i in range(k, last + 1)])
            ip[k] = m
            if pivots is not None and m != k:
                pivots.append(("complex", k, m))
            tr, ti = ar[A(m, k)], ai[A(m, k)]
            if abs(tr) + abs(ti) == 0.0:
                return False
            if m != k:
                ar[A(m, k)], ar[A(k, k)] = ar[A(k, k)], ar[A(m, k)]
                ai[A(m, k)], ai[A(k, k)] = ai[A(k, k)], ai[A(m, k)]
            den = tr * tr + ti * ti
            tr, ti = tr / den, -ti / den
            for i in range(k + 1, last + 1):
                cr, ci = ar[A(i, k)], ai[A(i, k)]
                ar[A(i, k)] = -(cr * tr - ci * ti)
                ai[A(i, k)] = -(ci * tr + cr * ti)
            for j in range(k + 1, min(k + kd, n - 1) + 1):
                mr, mi = ar[A(m, j)], ai[A(m, j)]
                if m != k:
                    ar[A(m, j)], ai[A(m, j)] = ar[A(k, j)], ai[A(k, j)]
                    ar[A(k, j)], ai[A(k, j)] = mr, mi
                if abs(mr) + abs(mi) == 0.0:
                    continue
                kind = "real" if mi == 0.0 else ("imag" if mr == 0.0 else "general")
                if cases is not None:
                    cases.add(kind)
                for i in range(k + 1, last + 1):
                    lr, li = ar[A(i, k)], ai[A(i, k)]
                    if kind == "real":
                        prod_r, prod_i = lr * mr, li * mr
                    elif kind == "imag":
                        prod_r, prod_i = -li * mi, lr * mi
                    else:
                        prod_r, prod_i = lr * mr - li * mi, li * mr + lr * mi
                    ar[A(i, j)] = ar[A(i, j)] + prod_r
                    ai[A(i, j)] = ai[A(i, j)] + prod_i
    return bool(abs(ar[A(n - 1, n - 1)]) + abs(ai[A(n - 1, n - 1)]) != 0.0)


def _cdiv(br, bi, ar, ai):
    den = ar * ar + ai * ai
    return (br * ar + bi * ai) / den, (bi * ar - br * ai) / den


def lin_solve_band_complex(ar, ai, n, ml, mu, br, bi, ip):
    kd = ml + mu
    A = lambda i, j: at(i, j, ml, mu)
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            m = ip[k]
            tr, ti = br[m], bi[m]
            br[m], bi[m] = br[k], bi[k]
            br[k], bi[k] = tr, ti
            for i in range(k + 1, min(k + ml, n - 1) + 1):
                cr, ci = ar[A(i, k)], ai[A(i, k)]
                br[i] = br[i] + (cr * tr - ci * ti)
                bi[i] = bi[i] + (ci * tr + cr * ti)
        for k in range(n - 1, -1, -1):
            br[k], bi[k] = _cdiv(br[k], bi[k], ar[A(k, k)], ai[A(k, k)])
            tr, ti = -br[k], -bi[k]
            for i in range(max(k - kd, 0), k):
                cr, ci = ar[A(i, k)], ai[A(i, k)]
                br[i] = br[i] + (cr * tr - ci * ti)
                bi[i] = bi[i] + (ci * tr + cr * ti)


# ---- matrix families of the linear-algebra tests (CPU: tests/test_radau_band_model_cpu.py, device: the band LU probe) --------

SHAPES_CPU = [(12, 1, 1), (24, 2, 1), (40, 1, 3), (65, 1, 1), (130, 4, 4)]


def band_families(n, ml, mu, seed=0):
    """[(tag, A (n, n), b (n), Ar, Ai, br, bi)] in the form of radau_wide_model.lu_families, every matrix zero outside the
    band (ml, mu).  Every family names the branch it takes; the tests assert from the model that it does."""
    rng = np.random.default_rng(100000 * n + 100 * ml + mu + seed)
    i, j = np.indices((n, n))
    band = (i - j <= ml) & (j - i <= mu)
    rnd = lambda lo=-1.0, hi=1.0: np.where(band, rng.uniform(lo, hi, (n, n)), 0.0)
    out = []

    def add(tag, a, ar, ai):
        out.append((tag, np.array(a, dtype=np.float64), rng.uniform(-1.0, 1.0, n), np.array(ar, dtype=np.float64),
                    np.array(ai, dtype=np.float64), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)))

    def dominant(scale=0.1):
        a = rnd(-scale, scale)
        a[np.arange(n), np.arange(n)] = 2.0 + rng.uniform(0.0, 1.0, n)
        return a

    # random inside the band, NOT diagonally dominant: partial pivoting really exchanges rows
    add("random0", rnd(), rnd(), rnd())
    add("random1", rnd(), rnd(), rnd())
    # each multiplier case of the complex elimination
    add("real", rnd(), rnd(), np.zeros((n, n)))
    add("imag", rnd(), np.zeros((n, n)), rnd())
    add("general", dominant(), dominant(), dominant(0.5))
    # a tie between rows 0 and 1 of column 0 (the first wins)
    a, ar, ai = dominant(), dominant(), dominant(0.5)
    a[0, 0] = a[1, 0] = 7.0
    ar[0, 0], ai[0, 0], ar[1, 0], ai[1, 0] = 7.0, 0.0, 3.0, -4.0
    add("tie", a, ar, ai)
    # a zero column: singular at that pivot
    a, ar, ai = rnd(), rnd(), rnd()
    a[:, n // 2] = ar[:, n // 2] = ai[:, n // 2] = 0.0
    add("zero_column", a, ar, ai)
    # a zero last diagonal entry: the last row and column are zero
    a, ar, ai = dominant(), dominant(), dominant(0.5)
    for m_ in (a, ar, ai):
        m_[n - 1, :] = 0.0
        m_[:, n - 1] = 0.0
    add("zero_last", a, ar, ai)
    return out


def factorise_and_solve_band(fam, ml, mu):
    """one family through the four band functions, in the form of radau_wide_model.factorise_and_solve; `f`, `fr`, `fi` are
    the factor blocks (flat), a right-hand side is solved only where the factorisation reports ok"""
    tag, a, b, ar, ai, br, bi = fam
    n = len(a)
    f, ip, swaps = pack(a, ml, mu), [0] * n, []
    ok = lu_decomp_band(f, n, ml, mu, ip, swaps)
    x = np.array(b, dtype=np.float64)
    if ok:
        lin_solve_band(f, n, ml, mu, x, ip)
    fr, fi, ipc, swapsc, cases = pack(ar, ml, mu), pack(ai, ml, mu), [0] * n, [], set()
    okc = lu_decomp_band_complex(fr, fi, n, ml, mu, ipc, swapsc, cases)
    xr, xi = np.array(br, dtype=np.float64), np.array(bi, dtype=np.float64)
    if okc:
        lin_solve_band_complex(fr, fi, n, ml, mu, xr, xi, ipc)
    return dict(tag=tag, ok=ok, f=f, ip=ip, swaps=swaps, x=x, okc=okc, fr=fr, fi=fi, ipc=ipc, swapsc=swapsc, cases=cases, xr=xr, xi=xi)

