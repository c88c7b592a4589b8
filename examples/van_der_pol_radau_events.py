"""Relaxation oscillations of the Van der Pol oscillator with Radau IIA(5) and an event function: a sweep over the
stiffness mu, every zero crossing of y[0] from the CSR event log of ``ivp_amd.Radau.solve_batch_events`` -- no ``max_events``
to guess: the stiff trajectories cross far less often than the mild ones -- and a period estimate per trajectory, against
the asymptotic period of the relaxation oscillation, T ~ (3 - 2 ln 2) mu + 7.014 mu^(-1/3) (large mu)."""
import math

import numpy as np

from ivp_amd import DeviceIVP, EventConfig, Options, Radau

SRC = """
__device__ void ode(double t, const double* y, double* d, const double* p) {
  d[0] = y[1];
  d[1] = p[0] * (1.0 - y[0] * y[0]) * y[1] - y[0];
}
__device__ void events(double t, const double* y, double* g, const double* p) { g[0] = y[0]; }
"""

mus = np.array([1.0, 3.0, 10.0, 30.0, 100.0, 300.0])
B = mus.size
f = DeviceIVP(SRC, 2, params=(1.0,), events=[EventConfig().negative()])   # downward crossings: one per period
y0 = np.repeat([[2.0], [0.0]], B, axis=1)
r = Radau().solve_batch_events(f, 0.0, 2400.0, y0, mus[None, :], Options(rtol=1e-6, atol=1e-8))
assert (r.status.cpu().numpy() == 0).all()
hits = r.n_event_hits.cpu().numpy()[0]
print(f"{int(hits.sum())} crossings in all, {int(hits.min())} to {int(hits.max())} per trajectory; "
      f"passes = {r.event_info['passes']}, staging = {r.event_info['staging_bytes']} bytes")
for b, mu in enumerate(mus):
    t, y = r.events_of(b, 0)
    t = t.cpu().numpy()
    assert t.size == hits[b] >= 3 and np.abs(y.cpu().numpy()[:, 0]).max() < 1e-10   # on the interpolant the event state sits on y[0] = 0
    period = float(np.diff(t[1:]).mean())   # the first crossing still carries the transient
    asym = (3.0 - 2.0 * math.log(2.0)) * mu + 7.014 * mu ** (-1.0 / 3.0)
    print(f"mu = {mu:6.1f}: {t.size:4d} crossings, period {period:10.5f}   (asymptotic {asym:9.3f})")
    if mu >= 30.0:
        assert abs(period - asym) / asym < 0.05
    if mu == 1.0:
        assert abs(period - 6.6633) < 1e-3   # the classical value for mu = 1
