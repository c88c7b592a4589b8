// radau_wide_resources.hip -- the wide form of the group Radau IIA(5) kernels (radau_group.h: 64 < n <= 512, C = ceil(n / 64)
// rows per lane, every matrix in global memory) instantiated at n = 65, 128, 129, 257 and 512 (C = 2, 2, 3, 5, 8) for
// tools/kernel_resources.sh.  Such instantiations exist only in hiprtc modules; this file builds them the way those
// modules are built -- one wavefront per workgroup, G = 64, IVP_HOIST = 0, strict arithmetic -- so that their register,
// scratch and LDS use can be read without a GPU.  It is compiled to nothing: not part of libivp_hip.so.
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#ifndef IVP_HOIST
#define IVP_HOIST 0
#endif
#define IVP_NS ivp_radau_wide_res
#include "rk_core.h"
#include "bdf_core.h"
#include "radau_core.h"
#include "rk_global.h"
#include "rk_group.h"
#include "bdf_group.h"
#include "radau_group.h"

namespace IVP_NS {

// y' = A y, a_ij = p0 / (1 + i + j): a dense right-hand side; JAC adds the analytic jac_col
template <int NN_, bool JAC>
struct ResDense {
    enum { N = NN_, P = 1 };
    static __device__ __forceinline__ double ode_comp(int i, double, const double *y, const double *p)
    {
        double s = 0.0;
        for (int j = 0; j < N; ++j) s += p[0] / (double)(1 + i + j) * y[j];
        return s;
    }
};
template <int NN_>
struct ResDense<NN_, true> : ResDense<NN_, false> {
    enum { N = NN_ };
    static __device__ __forceinline__ void jac_col(int col, double, const double *, double *column, const double *p)
    {
        for (int i = 0; i < N; ++i) column[i] = p[0] / (double)(1 + i + col);
    }
};

template <int NN_, bool JAC, int FULL, int G>
__global__ __launch_bounds__(IVP_WAVE) void res_init(const IvpKArgs a) { group_init_body<M_RADAU, ResDense<NN_, JAC>, FULL, G>(a); }
template <int NN_, bool JAC, int FULL, int G>
__global__ __launch_bounds__(IVP_WAVE) void res_chunk(const IvpKArgs a) { group_chunk_body<M_RADAU, ResDense<NN_, JAC>, FULL, G>(a); }

#define RES(n, g)                                                     \
    template __global__ void res_init<n, false, 1, g>(const IvpKArgs);  \
    template __global__ void res_chunk<n, false, 0, g>(const IvpKArgs); \
    template __global__ void res_chunk<n, false, 1, g>(const IvpKArgs); \
    template __global__ void res_chunk<n, true, 0, g>(const IvpKArgs);  \
    template __global__ void res_chunk<n, true, 1, g>(const IvpKArgs);
RES(65, 64)
RES(128, 64)
RES(129, 64)
RES(257, 64)
RES(512, 64)

}  // namespace IVP_NS
