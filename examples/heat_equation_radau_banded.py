"""The 256-point heat equation of examples/heat_equation_radau_256.py through Radau IIA(5) in BAND STORAGE: the right-hand
side is compiled with its tridiagonal pattern and jac_storage="banded", and Radau.solve_banded keeps J and the three factors
of an attempt by bands -- 15 n = 3840 doubles per trajectory instead of 4 n^2 = 262 144 -- forms J from four right-hand sides
(three column groups and the base point) instead of 257, and factorises inside the band.  The results are, bit for bit, those
of the dense Radau call on the same source compiled without a pattern."""
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

i, j = np.indices((N, N))
pattern = (np.abs(i - j) <= 1).astype(np.int8)
problem = DeviceIVP(ODE, N, jac_sparsity=pattern, jac_storage="banded")
layout = problem.jac_layout
x = np.arange(1, N + 1) / (N + 1.0)
y0 = np.sin(np.pi * x) + 0.25 * np.sin(5 * np.pi * x)
t_eval = [0.0, 0.01, 0.05, 0.2]
opts = Options(rtol=1e-8, atol=1e-10, t_eval=t_eval)
sol = Radau().solve_banded(problem, 0.0, 0.2, y0, opts)
lam = lambda m: SCALE * (2.0 - 2.0 * np.cos(np.pi * m / (N + 1)))   # eigenvalues of the discrete Laplacian
worst = 0.0
for t, y in zip(sol.t, np.asarray(sol.y)):
    exact = np.exp(-lam(1) * t) * np.sin(np.pi * x) + 0.25 * np.exp(-lam(5) * t) * np.sin(5 * np.pi * x)
    worst = max(worst, float(np.abs(y - exact).max()))
    print(f"t = {t:4.2f}: amplitude of the first mode {2.0 / (N + 1) * float(y @ np.sin(np.pi * x)):.8f} "
          f"(analytic {np.exp(-lam(1) * t):.8f}), error vs eigenmode solution {np.abs(y - exact).max():.1e}")
doubles = layout["jac_doubles"] + 3 * layout["lu_doubles"]
print(f"status {sol.status.name}, {sol.naccpt} accepted steps of {sol.nstep}, nfev {sol.nfev}, njev {sol.njev}, nlu {sol.nlu}; "
      f"ml = {layout['ml']}, mu = {layout['mu']}: {doubles} doubles of matrices per trajectory instead of {4 * N * N}")
assert sol.status.name == "Success" and worst < 1e-6
# the dense call on the same source without a pattern: the same bits
dense = Radau().solve(DeviceIVP(ODE, N), 0.0, 0.2, y0, opts)
assert np.array_equal(np.asarray(sol.y), np.asarray(dense.y)) and (sol.nfev, sol.njev, sol.nlu, sol.nstep) == (dense.nfev, dense.njev, dense.nlu, dense.nstep)
print("equal to the dense Radau call bit for bit")
