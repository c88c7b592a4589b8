// radau_group_lu_probe.hip -- TEST-ONLY: the linear algebra of the group-per-trajectory Radau attempt (radau_group.h) on
// matrices the test chooses, one group of G lanes per matrix, 64 / G matrices per one-wavefront workgroup, factors in LDS,
// exactly as the Radau kernels run them; compiled the way rk_radau_group.hip is (-O3 -ffp-contract=off, gfx950,
// IVP_HOIST = 0, strict arithmetic):
//   BdfG::lu_decomp then BdfG::lin_solve (bdf_group.h), and RadauG::lu_decomp_complex then RadauG::lin_solve_complex,
//   for n = 9, 16, 17, 33, 64.
// Built by tests/test_gpu_radau_group_lu_probe.py into a temporary directory; the pointers are device (torch) tensors.
// Layout: matrix q of a set is the row-major block [q][n * n], its right-hand side [q][n], its pivot rows [q][n]; the
// factors and the solution come back in place.  A right-hand side is solved only where the factorisation reports ok, as
// the attempt does.
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#define IVP_HOIST 0
#define IVP_FAST 0
#define IVP_NS ivp_radau_group_probe
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

template <int N, int G>
__global__ __launch_bounds__(IVP_WAVE) void probe_kernel(double *a_all, double *b_all, uint32_t *piv_all, int *ok_all, double *ar_all,
                                                         double *ai_all, double *br_all, double *bi_all, uint32_t *pivc_all, int *okc_all,
                                                         int nmat)
{
    using RG = IVP_NS::RadauG<Stub<N>, G>;
    using BG = IVP_NS::BdfG<Stub<N>, G>;
    constexpr int NN = N * N;
    const int q = (int)blockIdx.x * (IVP_WAVE / G) + (int)threadIdx.x / G;
    if (q >= nmat) return;
    const int i = RG::gl();
    double *e1 = RG::factors(), *er = e1 + NN, *ei = e1 + 2 * NN;
    uint32_t *piv = RG::pivots(), *pivc = piv + N;
    const size_t m0 = (size_t)q * NN, v0 = (size_t)q * N;
    for (int e = i; e < NN; e += G) {   // row-major in memory, column-major in LDS
        const int r = e / N, c = e - r * N;
        e1[c * N + r] = a_all[m0 + e];
        er[c * N + r] = ar_all[m0 + e];
        ei[c * N + r] = ai_all[m0 + e];
    }
    for (int e = i; e < 2 * N; e += G) piv[e] = 0xFFFFFFFFu;
    __syncthreads();
    const bool ok = BG::lu_decomp(e1, piv);
    double b[1] = {i < N ? b_all[v0 + i] : 0.0};
    if (ok) BG::lin_solve(e1, piv, b);
    const bool okc = RG::lu_decomp_complex(er, ei, pivc);
    double br = i < N ? br_all[v0 + i] : 0.0, bi = i < N ? bi_all[v0 + i] : 0.0;
    if (okc) RG::lin_solve_complex(er, ei, pivc, br, bi);
    __syncthreads();
    for (int e = i; e < NN; e += G) {
        const int r = e / N, c = e - r * N;
        a_all[m0 + e] = e1[c * N + r];
        ar_all[m0 + e] = er[c * N + r];
        ai_all[m0 + e] = ei[c * N + r];
    }
    if (i < N) {
        b_all[v0 + i] = b[0];
        br_all[v0 + i] = br;
        bi_all[v0 + i] = bi;
        piv_all[v0 + i] = piv[i];
        pivc_all[v0 + i] = pivc[i];
    }
    if (i == 0) { ok_all[q] = ok ? 1 : 0; okc_all[q] = okc ? 1 : 0; }
}

template <int N, int G>
int run(double *a, double *b, uint32_t *piv, int *ok, double *ar, double *ai, double *br, double *bi, uint32_t *pivc, int *okc, int nmat)
{
    constexpr int NG = IVP_WAVE / G;
    const dim3 grid((nmat + NG - 1) / NG), block(IVP_WAVE);
    hipLaunchKernelGGL((probe_kernel<N, G>), grid, block, 0, 0, a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    if (hipGetLastError() != hipSuccess) return 1;
    return hipDeviceSynchronize() == hipSuccess ? 0 : 2;
}

}  // namespace

// every array holds nmat blocks: a / ar / ai [nmat][n * n], b / br / bi [nmat][n], piv / pivc [nmat][n], ok / okc [nmat]
extern "C" int radau_group_lu_probe(int n, double *a, double *b, uint32_t *piv, int *ok, double *ar, double *ai, double *br, double *bi,
                                    uint32_t *pivc, int *okc, int nmat)
{
    if (nmat <= 0) return 3;
    switch (n) {
    case 9: return run<9, 16>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 16: return run<16, 16>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 17: return run<17, 32>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 33: return run<33, 64>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    case 64: return run<64, 64>(a, b, piv, ok, ar, ai, br, bi, pivc, okc, nmat);
    }
    return 3;
}
