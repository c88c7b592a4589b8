"""A stiff system with 256 states through Radau IIA(5): the method-of-lines heat equation on 256 interior points, compiled at
run time in component form with its analytic Jacobian column (jac_col).  One wavefront per trajectory, four matrix rows per
lane, the Jacobian and the three factors of a Radau attempt in global memory; the eliminations only touch the columns inside
the band.  The fastest mode decays 27 000 times faster than the first one; the steps follow the first.
(examples/heat_equation_radau.py is the same system on 64 points, with the factors in LDS.)"""
import numpy as np

from ivp_amd import DeviceIVP, Options, Radau

N, KAPPA = 256, 1.0
SCALE = KAPPA * (N + 1) ** 2   # kappa / dx^2, dx = 1 / (N + 1)
ODE = f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{{   // y_i' = kappa / dx^2 (y_(i-1) - 2 y_i + y_(i+1)), zero ends
    const double left = i > 0 ? y[i - 1] : 0.0, right = i < {N - 1} ? y[i + 1] : 0.0;
    return {SCALE!r} * (left - 2.0 * y[i] + right);
}}"""
JAC = f"""
__device__ void jac_col(int col, double t, const double* y, double* column, const double* p)
{{   // entries that are never written stay zero
    if (col > 0) column[col - 1] = {SCALE!r};
    column[col] = {-2.0 * SCALE!r};
    if (col < {N - 1}) column[col + 1] = {SCALE!r};
}}"""

x = np.arange(1, N + 1) / (N + 1.0)
y0 = np.sin(np.pi * x) + 0.25 * np.sin(5 * np.pi * x)
t_eval = [0.0, 0.01, 0.05, 0.2]
sol = Radau().solve(DeviceIVP(ODE + JAC, N, jac=True), 0.0, 0.2, y0, Options(rtol=1e-8, atol=1e-10, t_eval=t_eval))
lam = lambda m: SCALE * (2.0 - 2.0 * np.cos(np.pi * m / (N + 1)))   # eigenvalues of the discrete Laplacian
worst = 0.0
for t, y in zip(sol.t, np.asarray(sol.y)):
    exact = np.exp(-lam(1) * t) * np.sin(np.pi * x) + 0.25 * np.exp(-lam(5) * t) * np.sin(5 * np.pi * x)
    worst = max(worst, float(np.abs(y - exact).max()))
    print(f"t = {t:4.2f}: amplitude of the first mode {2.0 / (N + 1) * float(y @ np.sin(np.pi * x)):.8f} "
          f"(analytic {np.exp(-lam(1) * t):.8f}), error vs eigenmode solution {np.abs(y - exact).max():.1e}")
print(f"status {sol.status.name}, {sol.naccpt} accepted steps of {sol.nstep}, nfev {sol.nfev}, njev {sol.njev}, nlu {sol.nlu}; "
      f"stiffness ratio {lam(N) / lam(1):.0f}")
assert sol.status.name == "Success" and worst < 1e-6
