"""A method-of-lines reaction-diffusion system with a declared Jacobian sparsity pattern (the reference's
``jac_sparsity``, src/python/solve.rs:152-210 and src/python/sparsity.rs).

    u_t = D u_xx - a u^3  on 256 interior nodes, zero ends:  y_i' = k (y_{i-1} - 2 y_i + y_{i+1}) - a y_i^3

dF/dy is tridiagonal, so three column groups cover it: BDF's forward-difference Jacobian costs 3 + 1 right-hand sides
instead of 256 + 1, and -- the pattern contains every structural non-zero -- the solve is the dense one bit for bit.
"""
import numpy as np
import scipy.sparse as sp

import ivp_amd
from ivp_amd.pyfront import solve_ivp

N = 256
RHS = f"""
__device__ double ode_comp(int i, double t, const double* y, const double* p)
{{
    const double ym = i > 0 ? y[i - 1] : 0.0, yp = i < {N - 1} ? y[i + 1] : 0.0;
    return p[0] * ((ym - 2.0 * y[i]) + yp) - p[1] * ((y[i] * y[i]) * y[i]);
}}
"""
pattern = sp.diags([1, 1, 1], [-1, 0, 1], shape=(N, N))           # any scipy.sparse matrix, a dense array or (col_ptr, row_idx)
groups, n_groups = ivp_amd.api.jac_sparsity_groups(pattern, N)  # the reference's first-fit grouping, computed on the host
assert n_groups == 3 and groups.tolist() == [c % 3 for c in range(N)]

# 1. the SciPy-style entry point, as the reference's tests call it
x = np.linspace(0.0, 1.0, N + 2)[1:-1]
y0 = 1.0 + 0.5 * np.sin(np.pi * x)
kw = dict(method="BDF", args=(4000.0, 50.0), rtol=1e-5, atol=1e-8)
res = solve_ivp(RHS, [0, 0.05], y0, jac_sparsity=pattern, **kw)
dense = solve_ivp(RHS, [0, 0.05], y0, **kw)
assert res.success and np.array_equal(res.y, dense.y) and (res.nfev, res.njev, res.nlu) == (dense.nfev, dense.njev, dense.nlu)
print(f"one trajectory: {res.t.size - 1} steps, njev {res.njev}, nlu {res.nlu}; max y(0.05) = {res.y[:, -1].max():.6f}; "
      f"{n_groups} column groups, identical to the solve without the pattern")

# 2. a batch: one pattern per compiled problem, per-trajectory diffusion and reaction constants
B = 512
rng = np.random.default_rng(0)
y0b = y0[:, None] + 0.05 * rng.standard_normal((N, B))
params = np.stack([4000.0 * (1.0 + 0.1 * rng.uniform(-1, 1, B)), 50.0 * (1.0 + 0.1 * rng.uniform(-1, 1, B))])
f = ivp_amd.DeviceIVP(RHS, n=N, params=(1.0, 1.0), jac_sparsity=pattern)
r = ivp_amd.solve_ivp_batch(f, 0.0, 0.05, y0b, params, ivp_amd.Options(method="BDF", rtol=1e-5, atol=1e-8))
assert (np.asarray(r.status) == 0).all()
print(f"{B} trajectories: {int(np.asarray(r.naccpt).sum())} accepted steps, {int(np.asarray(r.njev).sum())} Jacobians of "
      f"{n_groups + 1} right-hand sides each instead of {N + 1}")
