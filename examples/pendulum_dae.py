"""The unit pendulum as an index-2 differential-algebraic system, a batch over initial angles, with Radau IIA(5).

    p' = v,   v' = -lam p - (0, 1),   0 = p . v          (p: position on the unit circle, v: velocity, lam: rod tension)

written as M y' = f(t, y) with y = (p1, p2, v1, v2, lam) and the singular mass matrix M = diag(1, 1, 1, 1, 0):
``DeviceIVP(..., mass=True)`` carries M, ``Radau(nind1=4, nind2=1)`` says that lam is an index-2 variable, so its error
scale is divided by the step ratio (the reference's ``nind2``).  Checked against the angle form phi'' = -cos phi."""
import numpy as np

from ivp_amd import DeviceIVP, Options, Radau

SRC = """
__device__ void ode(double t, const double* y, double* d, const double* p) {
    const double p1 = y[0], p2 = y[1], v1 = y[2], v2 = y[3], lam = y[4];
    d[0] = v1;
    d[1] = v2;
    d[2] = -lam * p1;
    d[3] = -lam * p2 - 1.0;
    d[4] = p1 * v1 + p2 * v2;
}
__device__ void mass(double* m, const double* p) {     // row-major 5 x 5, zeroed on entry
    m[0] = 1.0; m[6] = 1.0; m[12] = 1.0; m[18] = 1.0;  // the last row stays zero: an algebraic equation
}
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


phi0 = np.linspace(0.0, 1.2, 7)
# consistent initial values: at rest, the tension balances gravity along the rod
y0 = np.stack([np.cos(phi0), np.sin(phi0), np.zeros(7), np.zeros(7), -np.sin(phi0)])
pendulum = DeviceIVP(SRC, 5, mass=True)
r = Radau(nind1=4, nind2=1, nind3=0).solve_batch(pendulum, 0.0, 2.0, y0, None, Options(rtol=1e-5, atol=1e-5))
assert (r.status == 0).all()
for b, a in enumerate(phi0):
    want = angle_form(a, 2.0)
    err = np.abs(r.y_end[:, b] - want)
    print(f"phi0 = {a:4.2f}: p = ({r.y_end[0, b]: .6f}, {r.y_end[1, b]: .6f})  lam = {r.y_end[4, b]: .6f}  |p| - 1 = {np.hypot(*r.y_end[:2, b]) - 1.0: .1e}"
          f"  {int(r.naccpt[b])} accepted / {int(r.nrejct[b])} rejected, max error {err.max():.1e}")
    assert err.max() < 5e-2   # the tension lam is the least accurate component (2e-2 at worst on this batch)

# the same system with the pure-ODE partition does not get through: the index sets are not decoration
r = Radau().solve_batch(pendulum, 0.0, 2.0, y0[:, :1].copy(), None, Options(rtol=1e-5, atol=1e-5))
print("without nind2: status", int(r.status[0]), "(3 = StepSizeTooSmall)")
assert int(r.status[0]) == 3
