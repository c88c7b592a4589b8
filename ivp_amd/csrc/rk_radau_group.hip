// rk_radau_group.hip -- group-per-trajectory Radau IIA(5) kernels (group_init_kernel / group_chunk_kernel of rk_group.h with
// M_RADAU: radau_core.h's bodies over radau_group.h's policy, 8 < n <= 64) and their launch table.
//
// Built like the BDF group kernels of rk_group.hip -- one wavefront per workgroup, strict arithmetic (the only build: the
// Radau attempt has no fused site) -- except for the coefficients: IVP_HOIST = 0, the lean form of KC() in rk_core.h.  With
// the literals of ivp_pow and of the tableau resident in vector registers (IVP_HOIST = 1 / 2) the chunk kernels at n = 32
// and n = 64 spilled 104-172 vector registers, 92-316 bytes of scratch per lane; re-materialised where they are used
// they spill 16, into accumulation registers, and no kernel uses scratch (profiles/r10_kernel_resources_radau_group.txt).
// The only built-in problem with 8 < n <= 64 is id 102 (IVP_RHS_DENSE_64).
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#ifndef IVP_HOIST
#define IVP_HOIST 0
#endif
#define IVP_NS ivp_radau_group_strict
#include "rk_core.h"
#include "bdf_core.h"
#include "radau_core.h"
#include "rk_global.h"
#include "rk_group.h"
#include "bdf_group.h"
#include "radau_group.h"
#include "rk_launch.h"

namespace {

template <class R, int FULL>
hipError_t launch_one(int what, const IvpKArgs &a, uint32_t trajectories, hipStream_t s)
{
    const dim3 grid(trajectories), block(IVP_WAVE);   // built-in problems: one wavefront per trajectory
    if (grid.x == 0) return hipSuccess;
    (void)hipGetLastError();   // drop a stale error of some earlier runtime call: the value returned below is this launch's
    if (what == IVP_LAUNCH_INIT) hipLaunchKernelGGL((IVP_NS::group_init_kernel<IVP_NS::M_RADAU, R, FULL>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((IVP_NS::group_chunk_kernel<IVP_NS::M_RADAU, R, FULL>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t ivp_launch_radau_group_strict(int what, int rhs_id, int full, const IvpKArgs &a, uint32_t trajectories, hipStream_t s)
{
    switch (rhs_id) {
    case 102: return full ? launch_one<IVP_NS::RhsDense64, true>(what, a, trajectories, s) : launch_one<IVP_NS::RhsDense64, false>(what, a, trajectories, s);
    }
    return hipErrorInvalidValue;   // built-in problems with n > 64 (100, 101): rejected by the host before any launch
}
