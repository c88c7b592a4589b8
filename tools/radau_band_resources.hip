// radau_band_resources.hip -- the band form of the group Radau IIA(5) kernels (radau_band.h: 8 < n <= 512, J and the three
// factors by bands in global memory) instantiated for tools/kernel_resources.sh: a tridiagonal system at n = 12, 40, 65, 130
// and 512 (G = 16, 64, 64, 64, 64; C = 1, 1, 2, 3, 8) and one with ml = mu = 8 at n = 100.  Such instantiations exist only
// in hiprtc modules; this file builds them the way those modules are built -- one wavefront per workgroup, IVP_HOIST = 0,
// strict arithmetic, the pattern's tables in the functor -- so that their register, scratch and LDS use can be read without
// a GPU.  It is compiled to nothing: not part of libivp_hip.so.
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#ifndef IVP_HOIST
#define IVP_HOIST 0
#endif
#define IVP_NS ivp_radau_band_res
#include "rk_core.h"
#include "bdf_core.h"
#include "rk_global.h"
#include "rk_group.h"
#include "bdf_group.h"
#include "radau_core.h"
#include "radau_group.h"
#include "bdf_band.h"
#include "radau_band.h"

namespace IVP_NS {

// the tables of a full band (ml, mu) as ivp_jit.cpp would write them: first-fit grouping puts column c into group
// c % (ml + mu + 1); hit[g * n + row] is the one column of group g among row - ml .. row + mu, or -1
template <int NN_, int ML_, int MU_>
struct BandTables {
    short group_of[NN_];
    short hit[(ML_ + MU_ + 1) * NN_];
    constexpr BandTables() : group_of(), hit()
    {
        constexpr int NG = ML_ + MU_ + 1;
        for (int c = 0; c < NN_; ++c) group_of[c] = (short)(c % NG);
        for (int g = 0; g < NG; ++g)
            for (int row = 0; row < NN_; ++row) {
                short h = -1;
                for (int c = row - MU_; c <= row + ML_; ++c)
                    if (c >= 0 && c < NN_ && c % NG == g) h = (short)c;
                hit[g * NN_ + row] = h;
            }
    }
};
template <int NN_, int ML_, int MU_>
__device__ const BandTables<NN_, ML_, MU_> res_tables{};

// y'_i = sum over the band of p0 / (1 + i + j) * y_j
template <int NN_, int ML_, int MU_>
struct ResBand {
    enum { N = NN_, P = 1, SP_NGROUPS = ML_ + MU_ + 1, SP_ML = ML_, SP_MU = MU_ };
    static __device__ __forceinline__ double ode_comp(int i, double, const double *y, const double *p)
    {
        double s = 0.0;
        for (int j = i - ML_; j <= i + MU_; ++j)
            if (j >= 0 && j < N) s += p[0] / (double)(1 + i + j) * y[j];
        return s;
    }
    static __device__ __forceinline__ int sp_group_of(int c) { return res_tables<NN_, ML_, MU_>.group_of[c]; }
    static __device__ __forceinline__ int sp_hit(int e) { return res_tables<NN_, ML_, MU_>.hit[e]; }
};

template <int NN_, int ML_, int MU_, int FULL, int G>
__global__ __launch_bounds__(IVP_WAVE) void res_init(const IvpKArgs a) { group_init_body<M_RADAU, ResBand<NN_, ML_, MU_>, FULL, G>(a); }
template <int NN_, int ML_, int MU_, int FULL, int G>
__global__ __launch_bounds__(IVP_WAVE) void res_chunk(const IvpKArgs a) { group_chunk_body<M_RADAU, ResBand<NN_, ML_, MU_>, FULL, G>(a); }

#define RES(n, ml, mu, g)                                                  \
    template __global__ void res_init<n, ml, mu, 1, g>(const IvpKArgs);   \
    template __global__ void res_chunk<n, ml, mu, 0, g>(const IvpKArgs);  \
    template __global__ void res_chunk<n, ml, mu, 1, g>(const IvpKArgs);
RES(12, 1, 1, 16)
RES(40, 1, 1, 64)
RES(65, 1, 1, 64)
RES(100, 8, 8, 64)
RES(130, 1, 1, 64)
RES(512, 1, 1, 64)

}  // namespace IVP_NS
