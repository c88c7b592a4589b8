"""A sweep over the stiffness of the Van der Pol oscillator with Radau IIA(5), without guessing ``max_log``: the step counts
of the sweep differ by a factor of several, so a bounded segment block sized for the longest trajectory would be mostly
empty.  ``Radau.solve_batch_dense`` returns every trajectory's complete continuous solution as one CSR log on the device
(``seg_offsets`` / ``seg_cont`` / ``seg_xold`` / ``seg_h``) and ``result.dense`` evaluates all of them there, here on one
grid shared by the sweep; ``Radau.solve_batch_logged`` does the same for the accepted steps themselves."""
import numpy as np
import torch

from ivp_amd import Options, Radau, StiffVanDerPol

dev = torch.device("cuda:0")
eps = np.geomspace(1e-4, 1e-1, 16)[None, :]
y0 = np.repeat([[2.0], [0.0]], eps.shape[1], axis=1)
opts = Options(rtol=1e-6, atol=1e-8)
radau = Radau()

r = radau.solve_batch_dense(StiffVanDerPol(), 0.0, 2.0, torch.as_tensor(y0, device=dev), torch.as_tensor(eps, device=dev), opts)
assert (r.status == 0).all()
n_seg = r.n_seg.cpu().numpy()
print(f"segments per trajectory: {n_seg.min()} .. {n_seg.max()}, {r.dense_info['segments']} in all "
      f"({r.dense_info['bytes'] / 1e3:.0f} kB; a block of max_log = {n_seg.max()} would hold {n_seg.max() * n_seg.size} segments), "
      f"{r.dense_info['passes']} integration(s)")

grid = np.linspace(0.0, 2.0, 9)
y, found = r.dense(grid)                     # y [9, 2, 16], found [9, 16]: evaluated on the device
assert (found == 1).all()
for e, col in zip(eps[0], y[:, 0, :].T.cpu().numpy()):
    print(f"eps = {e:8.2e}: y1(t) = " + " ".join(f"{v:8.4f}" for v in col))
# the interpolant meets the end state the solve returned
assert torch.equal(y[-1], r.y_end) or float((y[-1] - r.y_end).abs().max()) < 1e-12

lg = radau.solve_batch_logged(StiffVanDerPol(), 0.0, 2.0, torch.as_tensor(y0, device=dev), torch.as_tensor(eps, device=dev), opts)
t_last, _ = lg.log_of(eps.shape[1] - 1)
print(f"step log: {lg.log_info['records']} records from {lg.log_info['passes']} integration; the mildest trajectory took {len(t_last) - 1} steps")
assert int(lg.log_offsets[-1]) == int(n_seg.sum()) + n_seg.size   # every accepted step, and the initial point of each trajectory
