// inband_probe.hip -- TEST-ONLY: the in-range division / square root helpers of ivp_amd/csrc/rk_core.h next to the
// hardware `/` and sqrt() on the same operands, compiled the way the product is (-O3 -ffp-contract=off, gfx950).
// Built by tests/test_gpu_inband_div_sqrt.py into a temporary directory; the pointers are device (torch) tensors.
#include <hip/hip_runtime.h>
#define IVP_FAST 0
#include "../../ivp_amd/csrc/rk_core.h"

__global__ void probe_kernel(const double *n, const double *d, const double *x, double *q_hw, double *q_fast, double *s_hw,
                             double *s_fast, int *pred, int len)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const double ni = n[i], di = d[i], xi = x[i];
    q_hw[i] = ni / di;
    q_fast[i] = ivp::ivp_div_inband(ni, ivp::ivp_recip_inband(di));
    s_hw[i] = sqrt(xi);
    s_fast[i] = ivp::ivp_sqrt_inband(xi);
    pred[i] = (ivp::ivp_num_inband(ni) ? 1 : 0) | (ivp::ivp_sq_inband(xi) ? 2 : 0);
}

extern "C" int inband_probe(const double *n, const double *d, const double *x, double *q_hw, double *q_fast, double *s_hw,
                            double *s_fast, int *pred, int len)
{
    hipLaunchKernelGGL(probe_kernel, dim3((len + 255) / 256), dim3(256), 0, 0, n, d, x, q_hw, q_fast, s_hw, s_fast, pred, len);
    if (hipGetLastError() != hipSuccess) return 1;
    return hipDeviceSynchronize() == hipSuccess ? 0 : 2;
}
