// radau_wide_lu_probe.hip -- TEST-ONLY: the linear algebra of the wide Radau attempt (radau_group.h, 64 < n <= 512) on matrices
// the test chooses, one wavefront per matrix, C = ceil(n / 64) rows per lane, the matrices in GLOBAL memory, exactly as the
// Radau kernels run them; compiled the way their hiprtc modules are (-O3 -ffp-contract=off, gfx950, IVP_HOIST = 0, strict
// arithmetic):
//   BdfG::lu_decomp then BdfG::lin_solve (bdf_group.h), and RadauW::lu_decomp_complex then RadauW::lin_solve_complex,
//   for n = 65, 129, 512.
// Built by tests/test_gpu_radau_wide_lu_probe.py into a temporary directory; the pointers are device (torch) tensors.
// Layout: matrix q of a set is the COLUMN-major block [q][n * n] (the kernels' own layout: the factors come back in place),
// its right-hand side [q][n], its pivot rows [q][n].  A right-hand side is solved only where the factorisation reports ok,
// as the attempt does.
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#define IVP_HOIST 0
#define IVP_FAST 0
#define IVP_NS ivp_radau_wide_probe
#include "../../ivp_amd/csrc/rk_core.h"
#include "../../ivp_amd/csrc/bdf_core.h"
#include "../../ivp_amd/csrc/radau_core.h"
#include "../../ivp_amd/csrc/rk_global.h"
#include "../../ivp_amd/csrc/rk_group.h"
#include "../../ivp_amd/csrc/bdf_group.h"
#include "../../ivp_amd/csrc/radau_group.h"

namespace {

template <int N_>
struct Stub {
    enum { N = N_, P = 1 };
    static __device__ __forceinline__ double ode_comp(int, double, const double *, const double *) { return 0.0; }
};

template <int N>
__global__ __launch_bounds__(IVP_WAVE) void probe_kernel(double *a_all, double *b_all, uint32_t *piv_all, int *ok_all, double *ar_all,
                                                         double *ai_all, double *br_all, double *bi_all, uint32_t *pivc_all, int *okc_all,
                                                         int nmat)
{
    constexpr int G = IVP_WAVE;
    using RW = IVP_NS::RadauW<Stub<N>, G>;
    using BG = IVP_NS::BdfG<Stub<N>, G>;
    constexpr int C = RW::C;
    const int q = (int)blockIdx.x;
    if (q >= nmat) return;
    const size_t m0 = (size_t)q * N * N, v0 = (size_t)q * N;
    double *e1 = a_all + m0, *er = ar_all + m0, *ei = ai_all + m0;
    uint32_t *piv = piv_all + v0, *pivc = pivc_all + v0;
    double b[C], br[C], bi[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int i = RW::gi(c);
        b[c] = i < N ? b_all[v0 + i] : 0.0;
        br[c] = i < N ? br_all[v0 + i] : 0.0;
        bi[c] = i < N ? bi_all[v0 + i] : 0.0;
    }
    const bool ok = BG::lu_decomp(e1, piv);
    __syncthreads();
    if (ok) BG::lin_solve(e1, piv, b);
    const bool okc = RW::lu_decomp_complex(er, ei, pivc);
    __syncthreads();
    if (okc) RW::lin_solve_complex(er, ei, pivc, br, bi);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int i = RW::gi(c);
        if (i < N) {
            if (ok) b_all[v0 + i] = b[c];
            if (okc) { br_all[v0 + i] = br[c]; bi_all[v0 + i] = bi[c]; }
        }
    }
    if (RW::gl() == 0) { ok_all[q] = ok ? 1 : 0; okc_all[q] = okc ? 1 : 0; }
}

template <int N>
int run(double *a, double *b, uint32_t *piv, int *ok, double *ar, double *ai, double *br, double *bi, uint32_t *pivc, int *okc, int nmat)
{
    const dim3 grid(nmat), block(IVP_WAVE);
    hipLaunchKernelGGL((probe_kernel<N>), grid, block, 0, 0, a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    if (hipGetLastError() != hipSuccess) return 1;
    return hipDeviceSynchronize() == hipSuccess ? 0 : 2;
}

}  // namespace

// every array holds nmat blocks: a / ar / ai [nmat][n * n] column-major, b / br / bi [nmat][n], piv / pivc [nmat][n], ok / okc [nmat]
extern "C" int radau_wide_lu_probe(int n, double *a, double *b, uint32_t *piv, int *ok, double *ar, double *ai, double *br, double *bi,
                                   uint32_t *pivc, int *okc, int nmat)
{
    if (nmat <= 0) return 3;
    switch (n) {
    case 65: return run<65>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 129: return run<129>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 512: return run<512>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    }
    return 3;
}
