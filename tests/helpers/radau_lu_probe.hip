// radau_lu_probe.hip -- TEST-ONLY: the linear algebra of the Radau attempt on matrices the test chooses, one lane per matrix,
// compiled the way rk_radau.hip is (-O3 -ffp-contract=off, gfx950, IVP_HOIST = 2, strict arithmetic):
//   bdf_lu_decomp<N> (bdf_core.h) then radau_lin_solve<N>, and radau_lu_decomp_complex<N> then radau_lin_solve_complex<N>
//   (radau_core.h), for N = 1..8.
// Built by tests/test_gpu_radau_lu_probe.py into a temporary directory; the pointers are device (torch) tensors.
// Layout: matrix q of a set is the row-major block [q][N * N], its right-hand side [q][N]; the factors and the solution
// come back in place.  A right-hand side is solved only where the factorisation reports ok, as the attempt does.
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#define IVP_HOIST 2
#define IVP_FAST 0
#define IVP_NS ivp_radau_probe
#include "../../ivp_amd/csrc/rk_core.h"
#include "../../ivp_amd/csrc/bdf_core.h"
#include "../../ivp_amd/csrc/radau_core.h"

namespace {

template <int N>
__global__ __launch_bounds__(IVP_WAVE) void probe_kernel(double *a_all, double *b_all, uint32_t *piv_all, int *ok_all, double *ar_all,
                                                         double *ai_all, double *br_all, double *bi_all, uint32_t *pivc_all, int *okc_all,
                                                         int nmat)
{
    const int q = (int)blockIdx.x * IVP_WAVE + (int)threadIdx.x;
    if (q >= nmat) return;
    const size_t m0 = (size_t)q * (N * N), v0 = (size_t)q * N;
    {
        double a[N][N], b[N];
#pragma unroll
        for (int r = 0; r < N; ++r) {
            b[r] = b_all[v0 + r];
#pragma unroll
            for (int c = 0; c < N; ++c) a[r][c] = a_all[m0 + r * N + c];
        }
        uint32_t piv;
        const bool ok = IVP_NS::bdf_lu_decomp<N>(a, piv);
        if (ok) IVP_NS::radau_lin_solve<N>(a, b, piv);
#pragma unroll
        for (int r = 0; r < N; ++r) {
            b_all[v0 + r] = b[r];
#pragma unroll
            for (int c = 0; c < N; ++c) a_all[m0 + r * N + c] = a[r][c];
        }
        piv_all[q] = piv;
        ok_all[q] = ok ? 1 : 0;
    }
    {
        double ar[N][N], ai[N][N], br[N], bi[N];
#pragma unroll
        for (int r = 0; r < N; ++r) {
            br[r] = br_all[v0 + r];
            bi[r] = bi_all[v0 + r];
#pragma unroll
            for (int c = 0; c < N; ++c) { ar[r][c] = ar_all[m0 + r * N + c]; ai[r][c] = ai_all[m0 + r * N + c]; }
        }
        uint32_t piv;
        const bool ok = IVP_NS::radau_lu_decomp_complex<N>(ar, ai, piv);
        if (ok) IVP_NS::radau_lin_solve_complex<N>(ar, ai, br, bi, piv);
#pragma unroll
        for (int r = 0; r < N; ++r) {
            br_all[v0 + r] = br[r];
            bi_all[v0 + r] = bi[r];
#pragma unroll
            for (int c = 0; c < N; ++c) { ar_all[m0 + r * N + c] = ar[r][c]; ai_all[m0 + r * N + c] = ai[r][c]; }
        }
        pivc_all[q] = piv;
        okc_all[q] = ok ? 1 : 0;
    }
}

template <int N>
int run(double *a, double *b, uint32_t *piv, int *ok, double *ar, double *ai, double *br, double *bi, uint32_t *pivc, int *okc, int nmat)
{
    const dim3 grid((nmat + IVP_WAVE - 1) / IVP_WAVE), block(IVP_WAVE);
    hipLaunchKernelGGL((probe_kernel<N>), grid, block, 0, 0, a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    if (hipGetLastError() != hipSuccess) return 1;
    return hipDeviceSynchronize() == hipSuccess ? 0 : 2;
}

}  // namespace

// every array holds nmat blocks: a / ar / ai [nmat][n * n], b / br / bi [nmat][n], piv / ok / pivc / okc [nmat]
extern "C" int radau_lu_probe(int n, double *a, double *b, uint32_t *piv, int *ok, double *ar, double *ai, double *br, double *bi,
                              uint32_t *pivc, int *okc, int nmat)
{
    if (nmat <= 0) return 3;
    switch (n) {
    case 1: return run<1>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 2: return run<2>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 3: return run<3>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 4: return run<4>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 5: return run<5>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 6: return run<6>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 7: return run<7>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 8: return run<8>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    }
    return 3;
}
