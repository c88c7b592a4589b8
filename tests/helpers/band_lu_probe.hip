// band_lu_probe.hip -- TEST-ONLY: BdfBand::lu_decomp_band / lin_solve_band of ivp_amd/csrc/bdf_band.h on matrices the test
// chooses, in both residencies (factors in LDS, factors in global memory), compiled the way the product's strict build
// is (-O3 -ffp-contract=off, gfx950, IVP_FAST = 0).  Built by tests/test_gpu_band_lu_probe.py into a temporary directory;
// the pointers are device (torch) tensors.  One group of G lanes per matrix, 64 / G matrices per one-wavefront workgroup,
// exactly as the BDF kernels run them.
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#define IVP_HOIST 2
#define IVP_FAST 0
#define IVP_NS ivp_band_probe
#include "../../ivp_amd/csrc/rk_core.h"
#include "../../ivp_amd/csrc/bdf_core.h"
#include "../../ivp_amd/csrc/rk_global.h"
#include "../../ivp_amd/csrc/rk_group.h"
#include "../../ivp_amd/csrc/bdf_group.h"
#include "../../ivp_amd/csrc/bdf_band.h"

namespace {

// the functor stub: what BdfBand reads of a banded problem
template <int N_, int ML_, int MU_>
struct Stub {
    enum { N = N_, P = 1, SP_ML = ML_, SP_MU = MU_ };
    static __device__ __forceinline__ double ode_comp(int, double, const double *, const double *) { return 0.0; }
};

// lu [nmat][W * n] band blocks (in: the matrix, out: the factors), piv [nmat][n], b [nmat][n] (in: right-hand side, out: the
// solution, untouched for a singular matrix), ok [nmat]
template <class R, int G, bool LDS>
__global__ __launch_bounds__(IVP_WAVE) void probe_kernel(double *lu_all, uint32_t *piv_all, double *b_all, int *ok_all, int nmat)
{
    using BB = IVP_NS::BdfBand<R, G>;
    using BG = IVP_NS::BdfG<R, G>;
    constexpr int NT = R::N, LD = BB::LD, C = BG::C, NG = IVP_WAVE / G;
    const int j = (int)blockIdx.x * NG + (int)threadIdx.x / G;
    if (j >= nmat) return;
    double *lu_mem = lu_all + (size_t)j * LD, *lu = lu_mem;
    uint32_t *piv_mem = piv_all + (size_t)j * NT, *piv = piv_mem;
    if constexpr (LDS) {
        static_assert(NG * (LD * 8 + NT * 4) <= 65536, "probe: factors do not fit a static LDS allocation");
        __shared__ double lu_lds[NG * LD];
        __shared__ uint32_t piv_lds[NG * NT];
        lu = lu_lds + (size_t)((int)threadIdx.x / G) * LD;
        piv = piv_lds + (size_t)((int)threadIdx.x / G) * NT;
        for (int e = BG::gl(); e < LD; e += G) lu[e] = lu_mem[e];
        for (int e = BG::gl(); e < NT; e += G) piv[e] = 0u;
        __syncthreads();
    }
    const bool ok = BB::lu_decomp_band(lu, piv);
    __syncthreads();
    if (ok) {
        double bl[C];
#pragma unroll
        for (int c = 0; c < C; ++c) bl[c] = BG::own(c) ? b_all[(size_t)j * NT + BG::gi(c)] : 0.0;
        BB::lin_solve_band(lu, piv, bl);
#pragma unroll
        for (int c = 0; c < C; ++c) if (BG::own(c)) b_all[(size_t)j * NT + BG::gi(c)] = bl[c];
    }
    __syncthreads();
    if constexpr (LDS) {
        for (int e = BG::gl(); e < LD; e += G) lu_mem[e] = lu[e];
        for (int e = BG::gl(); e < NT; e += G) piv_mem[e] = piv[e];
    }
    if (BG::gl() == 0) ok_all[j] = ok ? 1 : 0;
}

template <int N, int ML, int MU>
int run(int lds, double *lu, uint32_t *piv, double *b, int *ok, int nmat)
{
    using R = Stub<N, ML, MU>;
    constexpr int G = N <= 16 ? 16 : (N <= 32 ? 32 : 64);   // ivp_group_width
    const dim3 grid((nmat + IVP_WAVE / G - 1) / (IVP_WAVE / G)), block(IVP_WAVE);
    if (lds) hipLaunchKernelGGL((probe_kernel<R, G, true>), grid, block, 0, 0, lu, piv, b, ok, nmat);
    else hipLaunchKernelGGL((probe_kernel<R, G, false>), grid, block, 0, 0, lu, piv, b, ok, nmat);
    if (hipGetLastError() != hipSuccess) return 1;
    return hipDeviceSynchronize() == hipSuccess ? 0 : 2;
}

}  // namespace

extern "C" int band_lu_probe(int n, int ml, int mu, int lds, double *lu, uint32_t *piv, double *b, int *ok, int nmat)
{
    if (n == 12 && ml == 1 && mu == 1) return run<12, 1, 1>(lds, lu, piv, b, ok, nmat);
    if (n == 24 && ml == 2 && mu == 1) return run<24, 2, 1>(lds, lu, piv, b, ok, nmat);
    if (n == 40 && ml == 1 && mu == 3) return run<40, 1, 3>(lds, lu, piv, b, ok, nmat);
    if (n == 65 && ml == 1 && mu == 1) return run<65, 1, 1>(lds, lu, piv, b, ok, nmat);
    if (n == 100 && ml == 8 && mu == 8) return run<100, 8, 8>(lds, lu, piv, b, ok, nmat);
    if (n == 130 && ml == 4 && mu == 4) return run<130, 4, 4>(lds, lu, piv, b, ok, nmat);
    if (n == 512 && ml == 1 && mu == 1) return run<512, 1, 1>(lds, lu, piv, b, ok, nmat);
    return 3;
}
