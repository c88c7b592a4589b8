// radau_group_dae_resources.hip -- the mass-matrix instantiations of the group-per-trajectory Radau IIA(5) kernels
// (radau_group.h with a mass_col functor) at n = 9, 16, 32, 33 and 64 for tools/kernel_resources.sh.  Such instantiations
// exist only in hiprtc modules (problems compiled with IVP_RHS_HAS_MASS_COL); this file builds them the way those modules
// are built -- one wavefront per workgroup, IVP_HOIST = 0, strict arithmetic, G = ivp_group_width(n) -- so that their
// register, scratch and LDS use can be read without a GPU.  It is tools/radau_group_resources.hip with a dense constant M.
// It is compiled to nothing: not part of libivp_hip.so.
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#ifndef IVP_HOIST
#define IVP_HOIST 0
#endif
#define IVP_NS ivp_radau_group_dae_res
#include "rk_core.h"
#include "bdf_core.h"
#include "radau_core.h"
#include "rk_global.h"
#include "rk_group.h"
#include "bdf_group.h"
#include "radau_group.h"

namespace IVP_NS {

// M y' = A y, a_ij = p0 / (1 + i + j), m_ij = (i == j ? 2 : 0) + 1 / (2 + i + j): dense right-hand side, dense constant M;
// JAC adds the analytic jac_col
template <int NN_, bool JAC>
struct ResDenseDae {
    enum { N = NN_, P = 1 };
    static __device__ __forceinline__ double ode_comp(int i, double, const double *y, const double *p)
    {
        double s = 0.0;
        for (int j = 0; j < N; ++j) s += p[0] / (double)(1 + i + j) * y[j];
        return s;
    }
    static __device__ __forceinline__ void mass_col(int col, double *column, const double *)
    {
        for (int i = 0; i < N; ++i) column[i] = (i == col ? 2.0 : 0.0) + 1.0 / (double)(2 + i + col);
    }
};
template <int NN_>
struct ResDenseDae<NN_, true> : ResDenseDae<NN_, false> {
    enum { N = NN_ };
    static __device__ __forceinline__ void jac_col(int col, double, const double *, double *column, const double *p)
    {
        for (int i = 0; i < N; ++i) column[i] = p[0] / (double)(1 + i + col);
    }
};

template <int NN_, bool JAC, int FULL, int G>
__global__ __launch_bounds__(IVP_WAVE) void res_dae_init(const IvpKArgs a) { group_init_body<M_RADAU, ResDenseDae<NN_, JAC>, FULL, G>(a); }
template <int NN_, bool JAC, int FULL, int G>
__global__ __launch_bounds__(IVP_WAVE) void res_dae_chunk(const IvpKArgs a) { group_chunk_body<M_RADAU, ResDenseDae<NN_, JAC>, FULL, G>(a); }

#define RES(n, g)                                                         \
    template __global__ void res_dae_init<n, false, 1, g>(const IvpKArgs);  \
    template __global__ void res_dae_chunk<n, false, 0, g>(const IvpKArgs); \
    template __global__ void res_dae_chunk<n, false, 1, g>(const IvpKArgs); \
    template __global__ void res_dae_chunk<n, true, 0, g>(const IvpKArgs);  \
    template __global__ void res_dae_chunk<n, true, 1, g>(const IvpKArgs);
RES(9, 16)
RES(16, 16)
RES(32, 32)
RES(33, 64)
RES(64, 64)

}  // namespace IVP_NS
