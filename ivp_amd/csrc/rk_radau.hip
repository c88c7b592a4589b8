// rk_radau.hip -- thread-per-trajectory Radau IIA(5) kernels (radau_core.h, n <= 8) and their launch table.
//
// Stiff batches are small and long, like BDF's: the waves own their SIMDs, so these kernels are built the way rk_bdf.hip
// is -- __launch_bounds__(64, 1) and every coefficient pinned in a vector register (IVP_HOIST = 2, see KC() in
// rk_core.h).  Strict arithmetic is the only build: the Radau attempt has no fused site.
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#ifndef IVP_HOIST
#define IVP_HOIST 2
#endif
#define IVP_MIN_WAVES 1   // chunk_kernel_t (rk_global.h): one wave per SIMD, 512 registers per lane
#define IVP_NS ivp_radau_strict
#define IVP_RHS_INBAND 0
#include "rk_core.h"
#include "bdf_core.h"
#include "radau_core.h"
#include "rk_global.h"
#include "rk_launch.h"

namespace {

using namespace IVP_NS;

template <class R, int FULL>
hipError_t launch_one(int what, const IvpKArgs &a, uint32_t lanes, hipStream_t s)
{
    const uint32_t per_wave = (what == IVP_LAUNCH_CHUNK && a.lpw) ? a.lpw : (uint32_t)IVP_WAVE;   // thin waves (ivp_kargs.h)
    const dim3 grid((lanes + per_wave - 1) / per_wave), block(IVP_WAVE);
    if (grid.x == 0) return hipSuccess;
    (void)hipGetLastError();   // drop a stale error of some earlier runtime call: the value returned below is this launch's
    if (what == IVP_LAUNCH_INIT) hipLaunchKernelGGL((init_kernel_t<M_RADAU, R, FULL>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((chunk_kernel_t<M_RADAU, R, FULL>), grid, block, 0, s, a);
    return hipGetLastError();
}

template <class R>
hipError_t launch_rhs(int what, int full, const IvpKArgs &a, uint32_t lanes, hipStream_t s)
{
    return full ? launch_one<R, true>(what, a, lanes, s) : launch_one<R, false>(what, a, lanes, s);
}

}  // namespace

hipError_t ivp_launch_radau_strict(int what, int rhs_id, int full, const IvpKArgs &a, uint32_t lanes, hipStream_t s)
{
    switch (rhs_id) {
    case 0: return launch_rhs<IVP_NS::RhsDecay>(what, full, a, lanes, s);
    case 1: return launch_rhs<IVP_NS::RhsSho>(what, full, a, lanes, s);
    case 2: return launch_rhs<IVP_NS::RhsVdp>(what, full, a, lanes, s);
    case 3: return launch_rhs<IVP_NS::RhsCr3bp>(what, full, a, lanes, s);
    case 4: return launch_rhs<IVP_NS::RhsLorenz>(what, full, a, lanes, s);
    case 5: return launch_rhs<IVP_NS::RhsZero>(what, full, a, lanes, s);
    case 6: return launch_rhs<IVP_NS::RhsRational>(what, full, a, lanes, s);
    case 7: return launch_rhs<IVP_NS::RhsExp2>(what, full, a, lanes, s);
    case 8: return launch_rhs<IVP_NS::RhsLinear>(what, full, a, lanes, s);
    case 9: return launch_rhs<IVP_NS::RhsRobertson>(what, full, a, lanes, s);
    case 10: return launch_rhs<IVP_NS::RhsVdpEps>(what, full, a, lanes, s);
    // problems with event functions (ivp_radau_solve_events*, the only call the host lets them through) always run FULL:
    // DefaultSolOut with so_events, every root refined inline
    case 11: return launch_one<IVP_NS::RhsShoEv, true>(what, a, lanes, s);
    case 12: return launch_one<IVP_NS::RhsBall, true>(what, a, lanes, s);
    case 13: return launch_one<IVP_NS::RhsCannon, true>(what, a, lanes, s);
    case 14: return launch_one<IVP_NS::RhsRationalEv, true>(what, a, lanes, s);
    case 15: return launch_rhs<IVP_NS::RhsRobertsonJac>(what, full, a, lanes, s);   // analytic jac
    }
    return hipErrorInvalidValue;
}
