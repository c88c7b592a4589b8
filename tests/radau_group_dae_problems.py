"""The problems of the group-form Radau DAE tests (8 < n <= 64, ``DeviceIVP(..., mass_col=True)``): for each, the device
snippet in component form (``ode_comp``, ``mass_col``, optionally ``jac_col``) and the right-hand side and mass matrix the
CPU model tests/radau_dae_model.py gets -- the same operations in the same order, no libm call anywhere, so that the two
can be compared bit for bit.  Shared by tests/test_radau_group_dae_cpu.py (the model side alone) and
tests/test_gpu_radau_group_dae.py."""
import math

ODE = "__device__ double ode_comp(int i, double x, const double* y, const double* p)"
MASS_COL = "__device__ void mass_col(int col, double* column, const double* p)"


def lit(v):
    return float(v).hex()


# ---- k uncoupled planar pendulums in one state vector, index-1 variables first ------------------------------------------------
# index-2 form, n = 5 k, partition (4 k, k, 0): [p1, p2, v1, v2] of pendulum 0, of pendulum 1, ..., then lam_0 .. lam_{k-1}
# index-3 form, n = 5 k, partition (2 k, 2 k, k): [p1, p2] of each, then [v1, v2] of each, then lam_0 .. lam_{k-1}
# p' = v, v' = -lam p - (0, 1), and 0 = p.v (index 2) or 0 = |p|^2 - 1 (index 3); M = diag(1, .., 1, 0, .., 0) with k zeros.

def pend2_rhs(k, select=None):
    """select (optional, one value per call): 0.0 replaces every constraint by its index-1 form lam = |v|^2 - p2"""
    def f(x, s):
        out = [0.0] * (5 * k)
        for q in range(k):
            p1, p2, v1, v2, lam = s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3], s[4 * k + q]
            out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3] = v1, v2, -lam * p1, -lam * p2 - 1.0
            out[4 * k + q] = p1 * v1 + p2 * v2 if (select is None or select != 0.0) else lam - (v1 * v1 + v2 * v2 - p2)
        return out
    return f


def pend2_source(k, selectable=False):
    con = "p1 * v1 + p2 * v2"
    if selectable:
        con = f"p[0] != 0.0 ? {con} : lam - (v1 * v1 + v2 * v2 - p2)"
    return (f"{ODE} {{\n"
            f"  const int q = i < {4 * k} ? i / 4 : i - {4 * k};\n"
            f"  const double p1 = y[4 * q], p2 = y[4 * q + 1], v1 = y[4 * q + 2], v2 = y[4 * q + 3], lam = y[{4 * k} + q];\n"
            f"  if (i >= {4 * k}) return {con};\n"
            "  const int r = i % 4;\n"
            "  if (r == 0) return v1;\n"
            "  if (r == 1) return v2;\n"
            "  if (r == 2) return -lam * p1;\n"
            "  return -lam * p2 - 1.0;\n}\n"
            f"{MASS_COL} {{ if (col < {4 * k}) column[col] = 1.0; }}\n")


def pend3_rhs(k):
    def f(x, s):
        out = [0.0] * (5 * k)
        for q in range(k):
            p1, p2, v1, v2, lam = s[2 * q], s[2 * q + 1], s[2 * k + 2 * q], s[2 * k + 2 * q + 1], s[4 * k + q]
            out[2 * q], out[2 * q + 1] = v1, v2
            out[2 * k + 2 * q], out[2 * k + 2 * q + 1] = -lam * p1, -lam * p2 - 1.0
            out[4 * k + q] = p1 * p1 + p2 * p2 - 1.0
        return out
    return f


def pend3_source(k):
    return (f"{ODE} {{\n"
            f"  const int q = i < {4 * k} ? (i % {2 * k}) / 2 : i - {4 * k};\n"
            f"  const double p1 = y[2 * q], p2 = y[2 * q + 1], v1 = y[{2 * k} + 2 * q], v2 = y[{2 * k} + 2 * q + 1], lam = y[{4 * k} + q];\n"
            f"  if (i >= {4 * k}) return p1 * p1 + p2 * p2 - 1.0;\n"
            f"  if (i < {2 * k}) return (i & 1) ? v2 : v1;\n"
            "  if (i & 1) return -lam * p2 - 1.0;\n"
            "  return -lam * p1;\n}\n"
            f"{MASS_COL} {{ if (col < {4 * k}) column[col] = 1.0; }}\n")


def pend_mass(k):
    n = 5 * k
    return [[1.0 if r == c and r < 4 * k else 0.0 for c in range(n)] for r in range(n)]


def pend2_state(singles):
    """[p1, p2, v1, v2, lam] per pendulum -> the stacked index-2 state"""
    return [v for s in singles for v in s[:4]] + [s[4] for s in singles]


def pend3_state(singles):
    return [v for s in singles for v in s[:2]] + [v for s in singles for v in s[2:4]] + [s[4] for s in singles]


def pend2_split(k, y):
    return [[y[4 * q], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3], y[4 * k + q]] for q in range(k)]


def pend3_split(k, y):
    return [[y[2 * q], y[2 * q + 1], y[2 * k + 2 * q], y[2 * k + 2 * q + 1], y[4 * k + q]] for q in range(k)]


def pend_at_rest(phi):
    """at rest at angle phi: lam = -sin phi balances gravity along the rod"""
    return [math.cos(phi), math.sin(phi), 0.0, 0.0, 0.0 - math.sin(phi)]


# ---- M y' = A y with a dense constant M whose diagonal carries a parameter ----------------------------------------------------

def dense_mass(n, p0):
    """diagonally dominant, every off-diagonal entry non-zero: m_rr = p0 + r / 8, |m_rc| <= 0.05 / n * 9"""
    s = 9.0 / n
    return [[(p0 + 0.125 * r) if r == c else (0.01 * s * (1 + (r + 2 * c) % 5)) * (-1.0 if (r + c) % 3 == 0 else 1.0) for c in range(n)]
            for r in range(n)]


def lin_ode_source(a):
    """y' = A y in component form, A fixed in the module, every row summed left to right (radau_model.rhs_dense_linear)"""
    n = len(a)
    return (f"__device__ const double lin_a[{n * n}] = {{" + ", ".join(lit(a[i][j]) for i in range(n) for j in range(n)) + "};\n"
            f"{ODE} {{\n"
            f"  double s = lin_a[i * {n}] * y[0];\n"
            f"  for (int j = 1; j < {n}; ++j) s = s + lin_a[i * {n} + j] * y[j];\n"
            "  return s;\n}\n")


def lin_jac_source(n):
    return ("__device__ void jac_col(int col, double x, const double* y, double* column, const double* p) {\n"
            f"  for (int r = 0; r < {n}; ++r) column[r] = lin_a[r * {n} + col];\n}}\n")


def dense_mass_source(n):
    """dense_mass(n, p[0]) by columns: the off-diagonal table is fixed in the module, the diagonal adds the parameter"""
    m = dense_mass(n, 0.0)
    return (f"__device__ const double lin_m[{n * n}] = {{" + ", ".join(lit(m[r][c]) for r in range(n) for c in range(n)) + "};\n"
            f"{MASS_COL} {{\n"
            f"  for (int r = 0; r < {n}; ++r) column[r] = r == col ? p[0] + lin_m[r * {n} + r] : lin_m[r * {n} + col];\n}}\n")


def identity_mass_source():
    return f"{MASS_COL} {{ column[col] = 1.0; }}\n"


def diag_mass_source(n, n_zero):
    """diag(1, .., 1, 0, .., 0) with n_zero zeros (n_zero = n: M = 0, the hook writes nothing)"""
    return f"{MASS_COL} {{ if (col < {n - n_zero}) column[col] = 1.0; }}\n"


def diag_mass(n, n_zero):
    return [[1.0 if r == c and r < n - n_zero else 0.0 for c in range(n)] for r in range(n)]


def identity(n):
    return diag_mass(n, 0)


# ---- the stacked pendulums' initial states ----------------------------------------------------------------------------------
# Pendulum q starts on the orbit of tests/test_radau_dae_model_cpu.py's pendulum_truth (released at rest at angle 0) at its own
# time tau_q, hence at its own angle, and is held against pendulum_truth(tau_q + t1) at the end.  The stacked system shares
# one step size, and the error of lam -- an index-2 variable, whose error scale is divided by the step ratio -- moves by an
# order of magnitude with the phases; these are phases at which every pendulum stays inside the single pendulum's bounds.
TAUS_INDEX2_K2 = (0.0, 1.0)
TAUS_INDEX2_K4 = (0.0, 1.25, 1.5, 2.5)
TAUS_INDEX3_K2 = (0.0, 0.1)
_ORBIT = {}


def orbit(tau):
    """[p1, p2, v1, v2, lam] of the reference pendulum at time tau"""
    if tau not in _ORBIT:
        from tests.test_radau_dae_model_cpu import pendulum_truth
        _ORBIT[tau] = [1.0, 0.0, 0.0, 0.0, 0.0] if tau == 0.0 else pendulum_truth(tau)
    return _ORBIT[tau]
