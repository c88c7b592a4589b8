// radau_events_resources.hip -- the Radau IIA(5) kernels of problems WITH event functions (ivp_radau_solve_events*), FULL
// flavour, for tools/kernel_resources.sh: the thread form at n = 8 (two events) and at n = 5 with a mass matrix (the index-2
// pendulum, one event), the group form at n = 16 (G = 16) and n = 64 (G = 64), forward differences and jac_col.  Apart from
// the built-ins of rk_radau.hip (n = 2) such instantiations exist only in hiprtc modules; this file builds them the way
// those modules are built -- thread form: __launch_bounds__(64, 1), IVP_HOIST = 2; group form: one wavefront per workgroup,
// IVP_HOIST = 0 (-DIVP_RES_GROUP); strict arithmetic -- so that their register, scratch and LDS use can be read without a
// GPU.  It is compiled to nothing: not part of libivp_hip.so.
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#ifdef IVP_RES_GROUP
#define IVP_HOIST 0
#else
#define IVP_HOIST 2
#define IVP_MIN_WAVES 1
#endif
#define IVP_NS ivp_radau_events_res
#define IVP_RHS_INBAND 0
#include "rk_core.h"
#include "bdf_core.h"
#include "radau_core.h"
#include "rk_global.h"
#ifdef IVP_RES_GROUP
#include "rk_group.h"
#include "bdf_group.h"
#include "radau_group.h"
#endif

namespace IVP_NS {

#ifndef IVP_RES_GROUP

struct EvLin8 {   // y' = A y with a full constant matrix; events on components 0 and 7
    enum { N = 8, P = 0, NE = 2 };
    static IVP_HD double a_at(int i, int j) { return i == j ? -1.0 - 0.25 * i : (i % 2 && j == i - 1) ? 200.0 : 1e-3 * (1 + ((3 * i + 5 * j) % 7)); }
    static IVP_HD void ode(double, const double *y, double *d, const double *)
    {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double s = a_at(i, 0) * y[0];
#pragma unroll
            for (int j = 1; j < N; ++j) s = s + a_at(i, j) * y[j];
            d[i] = s;
        }
    }
    static IVP_HD void events(double, const double *y, double *g, const double *) { g[0] = y[0] - 0.5; g[1] = y[7] - 0.25; }
};
struct EvPendulum {   // index 2: M = diag(1, 1, 1, 1, 0); the event is the passage through the vertical
    enum { N = 5, P = 0, NE = 1 };
    static IVP_HD void ode(double, const double *s, double *d, const double *)
    {
        const double p1 = s[0], p2 = s[1], v1 = s[2], v2 = s[3], lam = s[4];
        d[0] = v1;
        d[1] = v2;
        d[2] = -lam * p1;
        d[3] = -lam * p2 - 1.0;
        d[4] = p1 * v1 + p2 * v2;
    }
    static IVP_HD void mass(double (&m)[5][5], const double *)
    {
        for (int i = 0; i < 4; ++i) m[i][i] = 1.0;
    }
    static IVP_HD void events(double, const double *y, double *g, const double *) { g[0] = y[0]; }
};

template <class R>
void instantiate(const IvpKArgs &a)
{
    hipLaunchKernelGGL((init_kernel_t<M_RADAU, R, true>), dim3(1), dim3(IVP_WAVE), 0, nullptr, a);
    hipLaunchKernelGGL((chunk_kernel_t<M_RADAU, R, true>), dim3(1), dim3(IVP_WAVE), 0, nullptr, a);
}

#else

// y' = A y, a_ij = p0 / (1 + i + j); events on component 0 and on the last one; JAC adds the analytic jac_col
template <int NN_, bool JAC>
struct ResDenseEv {
    enum { N = NN_, P = 1, NE = 2 };
    static __device__ __forceinline__ double ode_comp(int i, double, const double *y, const double *p)
    {
        double s = 0.0;
        for (int j = 0; j < N; ++j) s += p[0] / (double)(1 + i + j) * y[j];
        return s;
    }
    static __device__ __forceinline__ void events(double, const double *y, double *g, const double *) { g[0] = y[0] - 0.5; g[1] = y[N - 1] - 0.25; }
};
template <int NN_>
struct ResDenseEv<NN_, true> : ResDenseEv<NN_, false> {
    enum { N = NN_ };
    static __device__ __forceinline__ void jac_col(int col, double, const double *, double *column, const double *p)
    {
        for (int i = 0; i < N; ++i) column[i] = p[0] / (double)(1 + i + col);
    }
};

// (one wavefront per workgroup: the barriers of GroupRhs::events sit inside a root search that the groups of a wavefront
// enter and leave independently)
template <int NN_, bool JAC, int G>
__global__ __launch_bounds__(IVP_WAVE) void ev_init(const IvpKArgs a) { group_init_body<M_RADAU, ResDenseEv<NN_, JAC>, 1, G>(a); }
template <int NN_, bool JAC, int G>
__global__ __launch_bounds__(IVP_WAVE) void ev_chunk(const IvpKArgs a) { group_chunk_body<M_RADAU, ResDenseEv<NN_, JAC>, 1, G>(a); }

#define RES(n, g)                                                  \
    template __global__ void ev_init<n, false, g>(const IvpKArgs);  \
    template __global__ void ev_chunk<n, false, g>(const IvpKArgs); \
    template __global__ void ev_chunk<n, true, g>(const IvpKArgs);
RES(16, 16)
RES(64, 64)

#endif

}  // namespace IVP_NS

#ifndef IVP_RES_GROUP
void ivp_radau_events_resources(const IvpKArgs &a)
{
    using namespace IVP_NS;
    instantiate<EvLin8>(a);
    instantiate<EvPendulum>(a);
}
#endif
