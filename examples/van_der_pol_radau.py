"""Stiff Van der Pol oscillator with Radau IIA(5) (the reference's examples/van_der_pol.py, with its stiff method of
choice): the SciPy-style front end with ``method="Radau"``, parameters through ``args``, output on a ``t_eval`` grid --
and the direct per-method call ``ivp_amd.Radau`` with the settings ``solve_ivp`` cannot reach, on a small batch."""
import numpy as np

from ivp_amd import Options, Radau, StiffVanDerPol
from ivp_amd.pyfront import solve_ivp

eps = 1e-3
t_eval = np.linspace(0.0, 2.0, 21)
sol = solve_ivp("dydx[0] = y[1]; dydx[1] = ((1.0 - y[0] * y[0]) * y[1] - y[0]) / p[0];", (0.0, 2.0), [2.0, 0.0], method="Radau",
                t_eval=t_eval, args=(eps,), rtol=1e-9, atol=1e-9)
print("Status:", sol.message)
print("nfev:", sol.nfev)
print("njev:", sol.njev)
print("nlu:", sol.nlu)
print(f"y(2) = {sol.y[:, -1]}   (SciPy Radau at 1e-10: [1.7632345402, -0.8356886817])")
assert sol.success and sol.t.size == 21 and np.abs(sol.y[:, -1] - [1.7632345402033993, -0.8356886816853318]).max() < 1e-6

# the direct call: a tighter Newton loop and the classical controller, eight values of eps at once
radau = Radau(newton_maxiter=10, newton_tol=1e-4, predictive=False)
epss = np.geomspace(1e-4, 1e-1, 8)[None, :]
r = radau.solve_batch(StiffVanDerPol(), 0.0, 2.0, np.repeat([[2.0], [0.0]], 8, axis=1), epss, Options(rtol=1e-6, atol=1e-8))
for e, y, na, nr in zip(epss[0], r.y_end.T, r.naccpt, r.nrejct):
    print(f"eps = {e:8.2e}: y(2) = {y}, {int(na)} accepted / {int(nr)} rejected steps")
assert (r.status == 0).all()
