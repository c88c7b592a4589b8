// radau_dae_resources.hip -- the Radau IIA(5) kernels for problems with a mass matrix (radau_core.h HasMass), instantiated
// at n = 1, 2, 3, 5, 8 for tools/kernel_resources.sh.  Such instantiations exist only in hiprtc modules (IVP_RHS_HAS_MASS);
// this file builds them the way those modules and rk_radau.hip are built -- __launch_bounds__(64, 1), IVP_HOIST = 2, strict
// arithmetic -- so that their register and scratch use can be read without a GPU.  It is compiled to nothing: not part of
// libivp_hip.so.
#include <hip/hip_runtime.h>

#define IVP_HD __host__ __device__ __forceinline__
#define IVP_HOIST 2
#define IVP_MIN_WAVES 1
#define IVP_NS ivp_radau_dae
#define IVP_RHS_INBAND 0
#include "rk_core.h"
#include "bdf_core.h"
#include "radau_core.h"
#include "rk_global.h"

namespace IVP_NS {

struct DaeScalar {   // p0 y' = p1 / (1 + t^2) - y
    enum { N = 1, P = 2, NE = 0 };
    static IVP_HD void ode(double x, const double *y, double *d, const double *p) { d[0] = p[1] / (1.0 + x * x) - y[0]; }
    static IVP_HD void mass(double (&m)[1][1], const double *p) { m[0][0] = p[0]; }
};
struct DaeSemi {   // the 2 x 2 mass matrix in the parameters
    enum { N = 2, P = 4, NE = 0 };
    static IVP_HD void ode(double x, const double *y, double *d, const double *)
    {
        d[0] = -y[0] + y[1];
        d[1] = y[1] - x / (1.0 + x * x);
    }
    static IVP_HD void mass(double (&m)[2][2], const double *p) { m[0][0] = p[0]; m[0][1] = p[1]; m[1][0] = p[2]; m[1][1] = p[3]; }
};
struct DaeRobertson {   // M = diag(1, 1, 0)
    enum { N = 3, P = 0, NE = 0 };
    static IVP_HD void ode(double, const double *s, double *d, const double *)
    {
        const double xx = s[0], y = s[1], z = s[2];
        d[0] = -0.04 * xx + 1e4 * y * z;
        d[1] = 0.04 * xx - 1e4 * y * z - 3e7 * y * y;
        d[2] = xx + y + z - 1.0;
    }
    static IVP_HD void mass(double (&m)[3][3], const double *) { m[0][0] = 1.0; m[1][1] = 1.0; }
};
struct DaePendulum {   // index 2: M = diag(1, 1, 1, 1, 0)
    enum { N = 5, P = 0, NE = 0 };
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
};
struct DaeLin8 {   // M y' = A y with full constant matrices
    enum { N = 8, P = 0, NE = 0 };
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
    static IVP_HD void mass(double (&m)[8][8], const double *)
    {
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) m[r][c] = r == c ? 1.0 + 0.125 * r : 0.01 * (1 + (r + 2 * c) % 5) * ((r + c) % 3 == 0 ? -1.0 : 1.0);
    }
};

template <class R>
void instantiate(const IvpKArgs &a)
{
    static_assert(HasMass<R>::v, "a functor with the mass hook");
    hipLaunchKernelGGL((init_kernel_t<M_RADAU, R, false>), dim3(1), dim3(IVP_WAVE), 0, nullptr, a);
    hipLaunchKernelGGL((chunk_kernel_t<M_RADAU, R, false>), dim3(1), dim3(IVP_WAVE), 0, nullptr, a);
    hipLaunchKernelGGL((init_kernel_t<M_RADAU, R, true>), dim3(1), dim3(IVP_WAVE), 0, nullptr, a);
    hipLaunchKernelGGL((chunk_kernel_t<M_RADAU, R, true>), dim3(1), dim3(IVP_WAVE), 0, nullptr, a);
}

}  // namespace IVP_NS

void ivp_radau_dae_resources(const IvpKArgs &a)
{
    using namespace IVP_NS;
    instantiate<DaeScalar>(a);
    instantiate<DaeSemi>(a);
    instantiate<DaeRobertson>(a);
    instantiate<DaePendulum>(a);
    instantiate<DaeLin8>(a);
}
