"""Poincare section of 10 000 perturbed Arenstorf orbits: every crossing of the x axis (event g = y) of every orbit,
with no cap to guess.  solve_ivp_batch_events returns the occurrences as a CSR log on the device -- record
event_offsets[i * B + b] + k is the k-th root of event i on trajectory b -- and events_all(0) is the section itself:
all roots of the event over the batch as one contiguous slice, with the trajectory each belongs to."""
import numpy as np
import torch

import ivp_amd
from ivp_amd import DeviceIVP, EventConfig, Options, solve_ivp_batch_events, workloads

SRC = r"""
__device__ void ode(double t, const double* s, double* d, const double* p)
{
    const double mu = p[0];
    const double x = s[0], y = s[1], z = s[2], vx = s[3], vy = s[4], vz = s[5];
    const double a = x + mu, b = x - 1.0 + mu;
    const double r1 = sqrt(a * a + y * y + z * z), r2 = sqrt(b * b + y * y + z * z);
    const double r13 = r1 * r1 * r1, r23 = r2 * r2 * r2;
    d[0] = vx; d[1] = vy; d[2] = vz;
    d[3] = x + 2.0 * vy - (1.0 - mu) * (x + mu) / r13 - mu * (x - 1.0 + mu) / r23;
    d[4] = y - 2.0 * vx - (1.0 - mu) * y / r13 - mu * y / r23;
    d[5] = -(1.0 - mu) * z / r13 - mu * z / r23;
}
__device__ void events(double t, const double* s, double* g, const double* p) { g[0] = s[1]; }   // crossings of the x axis
"""

B = 10_000
y0, mu, t0, t1 = workloads.cr3bp_batch(B)
dev = torch.device("cuda:0")
f = DeviceIVP(SRC, n=6, params=(workloads.ARENSTORF_MU,), events=[EventConfig()])
r = solve_ivp_batch_events(f, t0, t1, torch.as_tensor(y0, device=dev), torch.as_tensor(mu, device=dev),
                           Options(method="DOPRI5", rtol=1e-6, atol=1e-9, max_events=4))
hits = r.n_event_hits[0]
t, y, traj = r.events_all(0)
info = r.event_info
print(f"{B} orbits: {info['total']} crossings of the x axis, {int(hits.min())} .. {int(hits.max())} per orbit "
      f"({info['passes']} integration{'s' if info['passes'] > 1 else ''}, {info['total'] * 7 * 8 / 1e6:.1f} MB of records, "
      f"{info['staging_bytes'] / 1e6:.1f} MB of staging)")
assert bool((r.status == 0).all()) and info["total"] == int(hits.sum()) == t.shape[0] == traj.shape[0]
assert float(y[:, 1].abs().max()) < 1e-6                       # every record lies on the section y = 0
assert bool((traj[1:] >= traj[:-1]).all()) and torch.equal(torch.bincount(traj, minlength=B), hits.to(torch.int64))
# the section: (x, vx) of the upward crossings
up = y[:, 4] > 0
print(f"  upward crossings: {int(up.sum())}; x in [{float(y[up, 0].min()):.4f}, {float(y[up, 0].max()):.4f}], "
      f"vx in [{float(y[up, 3].min()):.4f}, {float(y[up, 3].max()):.4f}]")
# one orbit's own crossings, in detection order
tb, yb = r.events_of(B // 2, 0)
print(f"  orbit {B // 2}: crossings at t = {np.array2string(tb.cpu().numpy(), precision=4)}")
assert bool((tb[1:] > tb[:-1]).all())
