// inband_deferred_probe.hip -- TEST-ONLY: the device forms of the guards of the strict CR3BP right-hand side in
// ivp_amd/csrc/rk_core.h, state by state, compiled the way the product is (-O3 -ffp-contract=off, gfx950): the per-call guard
// and the folded guard of the deferred form after one call of RhsCr3bp::ode_deferred<true> -- the device twin of
// inband_guards in tests/helpers/inband_guard_host.cpp.  Built by tests/test_gpu_inband_deferred.py into a temporary directory;
// the pointers are device (torch) tensors.
#include <hip/hip_runtime.h>
#define IVP_FAST 0
#include "../../ivp_amd/csrc/rk_core.h"

__global__ void guard_kernel(const double *x, const double *y, const double *z, const double *mu, int *per_call, int *folded, int len)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const double s[6] = {x[i], y[i], z[i], 0.25, -0.5, 0.125}, p[1] = {mu[i]};
    const double a = s[0] + p[0], b = s[0] - 1.0 + p[0];
    per_call[i] = ivp::RhsCr3bp::strict_inband(ivp::RhsCr3bp::strict_terms(s, p[0], a, b)) ? 1 : 0;
    ivp::IvpInbandAcc acc = ivp::ivp_inband_begin(ivp::RhsCr3bp::inband_seed(p));
    double d[6];
    ivp::RhsCr3bp::ode_deferred<true>(0.0, s, d, p, acc);
    folded[i] = ivp::ivp_inband_ok(acc) ? 1 : 0;
}

// thread i folds `calls` consecutive states (one mu per thread: the first state's) into ONE accumulator, as an attempt's stage
// block does, and reports the decision after the last of them
__global__ void fold_seq_kernel(const double *x, const double *y, const double *z, const double *mu, int calls, int *folded, int len)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const double p[1] = {mu[i * calls]};
    ivp::IvpInbandAcc acc = ivp::ivp_inband_begin(ivp::RhsCr3bp::inband_seed(p));
    for (int c = 0; c < calls; ++c) {
        const int q = i * calls + c;
        const double s[6] = {x[q], y[q], z[q], 0.25, -0.5, 0.125};
        double d[6];
        ivp::RhsCr3bp::ode_deferred<true>(0.0, s, d, p, acc);
    }
    folded[i] = ivp::ivp_inband_ok(acc) ? 1 : 0;
}

extern "C" int inband_fold_seq_device(const double *x, const double *y, const double *z, const double *mu, int calls, int *folded, int len)
{
    hipLaunchKernelGGL(fold_seq_kernel, dim3((len + 255) / 256), dim3(256), 0, 0, x, y, z, mu, calls, folded, len);
    if (hipGetLastError() != hipSuccess) return 1;
    return hipDeviceSynchronize() == hipSuccess ? 0 : 2;
}

extern "C" int inband_guards_device(const double *x, const double *y, const double *z, const double *mu, int *per_call, int *folded, int len)
{
    hipLaunchKernelGGL(guard_kernel, dim3((len + 255) / 256), dim3(256), 0, 0, x, y, z, mu, per_call, folded, len);
    if (hipGetLastError() != hipSuccess) return 1;
    return hipDeviceSynchronize() == hipSuccess ? 0 : 2;
}
