// radau_band_lu_probe.hip -- TEST-ONLY: RadauBand::lu_decomp_band_complex / lin_solve_band_complex of
// ivp_amd/csrc/radau_band.h on band blocks the test chooses, in global memory, one group of G lanes per matrix, 64 / G
// matrices per one-wavefront workgroup, exactly as the banded Radau kernels run them; compiled the way their hiprtc modules
// are (-O3 -ffp-contract=off, gfx950, IVP_HOIST = 0, strict arithmetic).  Built by tests/test_gpu_radau_band_lu_probe.py into
// a temporary directory; the pointers are device (torch) tensors.
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#define IVP_HOIST 0
#define IVP_FAST 0
#define IVP_NS ivp_radau_band_probe
#include "../../ivp_amd/csrc/rk_core.h"
#include "../../ivp_amd/csrc/bdf_core.h"
#include "../../ivp_amd/csrc/rk_global.h"
#include "../../ivp_amd/csrc/rk_group.h"
#include "../../ivp_amd/csrc/bdf_group.h"
#include "../../ivp_amd/csrc/radau_core.h"
#include "../../ivp_amd/csrc/radau_group.h"
#include "../../ivp_amd/csrc/bdf_band.h"
#include "../../ivp_amd/csrc/radau_band.h"

namespace {

// the functor stub: what RadauBand reads of a banded problem
template <int N_, int ML_, int MU_>
struct Stub {
    enum { N = N_, P = 1, SP_ML = ML_, SP_MU = MU_ };
    static __device__ __forceinline__ double ode_comp(int, double, const double *, const double *) { return 0.0; }
};

// ar / ai [nmat][W * n] band blocks (in: the matrix, out: the factors), piv [nmat][n], br / bi [nmat][n] (in: the right-hand
// sides, out: the solution, untouched for a singular matrix), ok [nmat]
template <class R, int G>
__global__ __launch_bounds__(IVP_WAVE) void probe_kernel(double *ar_all, double *ai_all, uint32_t *piv_all, double *br_all, double *bi_all,
                                                         int *ok_all, int nmat)
{
    using RB = IVP_NS::RadauBand<R, G>;
    constexpr int NT = R::N, LD = RB::LD, C = RB::C, NG = IVP_WAVE / G;
    const int j = (int)blockIdx.x * NG + (int)threadIdx.x / G;
    if (j >= nmat) return;
    double *ar = ar_all + (size_t)j * LD, *ai = ai_all + (size_t)j * LD;
    uint32_t *piv = piv_all + (size_t)j * NT;
    const bool ok = RB::lu_decomp_band_complex(ar, ai, piv);
    __syncthreads();
    if (ok) {
        double br[C], bi[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            br[c] = RB::own(c) ? br_all[(size_t)j * NT + RB::gi(c)] : 0.0;
            bi[c] = RB::own(c) ? bi_all[(size_t)j * NT + RB::gi(c)] : 0.0;
        }
        RB::lin_solve_band_complex(ar, ai, piv, br, bi);
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (RB::own(c)) { br_all[(size_t)j * NT + RB::gi(c)] = br[c]; bi_all[(size_t)j * NT + RB::gi(c)] = bi[c]; }
    }
    if (RB::gl() == 0) ok_all[j] = ok ? 1 : 0;
}

template <int N, int ML, int MU>
int run(double *ar, double *ai, uint32_t *piv, double *br, double *bi, int *ok, int nmat)
{
    using R = Stub<N, ML, MU>;
    constexpr int G = N <= 16 ? 16 : (N <= 32 ? 32 : 64);   // ivp_group_width
    const dim3 grid((nmat + IVP_WAVE / G - 1) / (IVP_WAVE / G)), block(IVP_WAVE);
    hipLaunchKernelGGL((probe_kernel<R, G>), grid, block, 0, 0, ar, ai, piv, br, bi, ok, nmat);
    if (hipGetLastError() != hipSuccess) return 1;
    return hipDeviceSynchronize() == hipSuccess ? 0 : 2;
}

}  // namespace

extern "C" int radau_band_lu_probe(int n, int ml, int mu, double *ar, double *ai, uint32_t *piv, double *br, double *bi, int *ok, int nmat)
{
    if (nmat <= 0) return 3;
    if (n == 12 && ml == 1 && mu == 1) return run<12, 1, 1>(ar, ai, piv, br, bi, ok, nmat);
    if (n == 24 && ml == 2 && mu == 1) return run<24, 2, 1>(ar, ai, piv, br, bi, ok, nmat);
    if (n == 40 && ml == 1 && mu == 3) return run<40, 1, 3>(ar, ai, piv, br, bi, ok, nmat);
    if (n == 65 && ml == 1 && mu == 1) return run<65, 1, 1>(ar, ai, piv, br, bi, ok, nmat);
    if (n == 100 && ml == 8 && mu == 8) return run<100, 8, 8>(ar, ai, piv, br, bi, ok, nmat);
    if (n == 130 && ml == 4 && mu == 4) return run<130, 4, 4>(ar, ai, piv, br, bi, ok, nmat);
    if (n == 512 && ml == 1 && mu == 1) return run<512, 1, 1>(ar, ai, piv, br, bi, ok, nmat);
    return 3;
}
