"""Three planar pendulums in ONE state vector as an index-2 differential-algebraic system (n = 15), a batch over initial
angles, with Radau IIA(5) on the group kernels (one matrix row per lane).

    p_q' = v_q,   v_q' = -lam_q p_q - (0, 1),   0 = p_q . v_q          (q = 0, 1, 2; p: position, v: velocity, lam: tension)

written as M y' = f(t, y) with the index-1 variables first -- y = (p_0, v_0, p_1, v_1, p_2, v_2, lam_0, lam_1, lam_2) -- and
the singular mass matrix M = diag(1, ..., 1, 0, 0, 0).  Beyond 8 states the problem is in component form (``ode_comp``
returns one derivative) and ``DeviceIVP(..., mass_col=True)`` carries M by columns, like ``jac_col`` carries a Jacobian;
``Radau(nind2=3)`` says that the three tensions are index-2 variables (``nind1`` is inferred as 12).  The pendulums are
uncoupled, so each is checked against the angle form phi'' = -cos phi -- but they share one step size."""
import numpy as np

from ivp_amd import DeviceIVP, Options, Radau

K = 3          # pendulums
N = 5 * K      # states: 4 K differential, K algebraic
SRC = f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p) {{
    const int q = i < {4 * K} ? i / 4 : i - {4 * K};                  // the pendulum this component belongs to
    const double p1 = y[4 * q], p2 = y[4 * q + 1], v1 = y[4 * q + 2], v2 = y[4 * q + 3], lam = y[{4 * K} + q];
    if (i >= {4 * K}) return p1 * v1 + p2 * v2;                      // the constraint, differentiated once: index 2
    switch (i % 4) {{
    case 0: return v1;
    case 1: return v2;
    case 2: return -lam * p1;
    default: return -lam * p2 - 1.0;
    }}
}}
__device__ void mass_col(int col, double* column, const double* p) {{   // column `col` of M, zeroed on entry
    if (col < {4 * K}) column[col] = 1.0;                              // the last K columns stay zero: algebraic equations
}}
"""


def angle_form(phi0, t1, steps=4000):
    """phi'' = -cos phi from rest at phi0, classical RK4 -> (p1, p2, v1, v2, lam) at t1"""
    f = lambda s: np.array([s[1], -np.cos(s[0])])
    s, h = np.array([phi0, 0.0]), t1 / steps
    for _ in range(steps):
        k1 = f(s); k2 = f(s + 0.5 * h * k1); k3 = f(s + 0.5 * h * k2); k4 = f(s + h * k3)
        s = s + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    phi, om = s
    return np.array([np.cos(phi), np.sin(phi), -om * np.sin(phi), om * np.cos(phi), om * om - np.sin(phi)])


B = 5
phi0 = np.array([[0.2 * b + 0.35 * q for q in range(K)] for b in range(B)])   # [B][K]: every pendulum at its own angle
# consistent initial values: at rest, each tension balances gravity along its rod
y0 = np.zeros((N, B))
for q in range(K):
    y0[4 * q], y0[4 * q + 1], y0[4 * K + q] = np.cos(phi0[:, q]), np.sin(phi0[:, q]), -np.sin(phi0[:, q])
chain = DeviceIVP(SRC, N, mass_col=True)
r = Radau(nind2=K).solve_batch(chain, 0.0, 2.0, y0, None, Options(rtol=1e-5, atol=1e-5))
assert (r.status == 0).all()
for b in range(B):
    worst = 0.0
    for q in range(K):
        got = np.array([r.y_end[4 * q + c, b] for c in range(4)] + [r.y_end[4 * K + q, b]])
        worst = max(worst, np.abs(got - angle_form(phi0[b, q], 2.0)).max())
    print(f"batch {b}: angles {phi0[b]}  {int(r.naccpt[b])} accepted / {int(r.nrejct[b])} rejected, max error {worst:.1e}")
    assert worst < 5e-2   # the tensions are the least accurate components, as for the single pendulum

# the same system with the pure-ODE partition does not get through: the index sets are not decoration
r = Radau().solve_batch(chain, 0.0, 2.0, y0[:, :1].copy(), None, Options(rtol=1e-5, atol=1e-5))
print("without nind2: status", int(r.status[0]), "(3 = StepSizeTooSmall)")
assert int(r.status[0]) == 3
