// emul_dae.cpp -- TEST-ONLY harness: the Radau IIA(5) kernel bodies of ivp_amd/csrc/radau_core.h for problems WITH A MASS
// MATRIX (HasMass: M y' = f, DAE index sets), run on the CPU lane by lane with the GPU launch loop's
// init -> chunk -> chunk ... schedule.  The twin of tests/host_emul/emul.cpp, which runs the bodies without the hook; the
// functors here are test-only and carry a `mass` member.  Not part of the product: nothing in ivp_amd/ links or loads it.
// Compiled with g++ -ffp-contract=off (strict arithmetic, the only Radau build).
#include <cstdint>
#include <cstring>
#include <vector>

#define IVP_HD inline
#define IVP_NS ivp_emul_dae
#include "../../ivp_amd/csrc/rk_core.h"
#include "../../ivp_amd/csrc/bdf_core.h"
#include "../../ivp_amd/csrc/radau_core.h"

using namespace ivp_emul_dae;

// M y' = A y: A (row-major) in p[0 .. N N), M in p[N N .. 2 N N).  Each row is summed left to right.
template <int N_>
struct DaeLin {
    enum { N = N_, P = 2 * N_ * N_, NE = 0 };
    static IVP_HD void ode(double, const double *y, double *d, const double *p)
    {
        for (int i = 0; i < N; ++i) {
            double s = p[i * N] * y[0];
            for (int j = 1; j < N; ++j) s = s + p[i * N + j] * y[j];
            d[i] = s;
        }
    }
    static IVP_HD void mass(double (&m)[N_][N_], const double *p)
    {
        for (int r = 0; r < N_; ++r)
            for (int c = 0; c < N_; ++c) m[r][c] = p[N_ * N_ + r * N_ + c];
    }
};

// p0 y' = p1 / (1 + t^2) - y: p0 = 0 is the algebraic equation, and p0 may differ per trajectory
struct DaeScalar {
    enum { N = 1, P = 2, NE = 0 };
    static IVP_HD void ode(double x, const double *y, double *d, const double *p) { d[0] = p[1] / (1.0 + x * x) - y[0]; }
    static IVP_HD void mass(double (&m)[1][1], const double *p) { m[0][0] = p[0]; }
};

// f = (-y1 + y2, y2 - t / (1 + t^2)) with the whole 2 x 2 mass matrix in the parameters: diag(1, 0) is the semi-explicit
// index-1 system, a dense non-singular M an implicit ODE
struct DaeSemi {
    enum { N = 2, P = 4, NE = 0 };
    static IVP_HD void ode(double x, const double *y, double *d, const double *)
    {
        d[0] = -y[0] + y[1];
        d[1] = y[1] - x / (1.0 + x * x);
    }
    static IVP_HD void mass(double (&m)[2][2], const double *p)
    {
        m[0][0] = p[0]; m[0][1] = p[1]; m[1][0] = p[2]; m[1][1] = p[3];
    }
};

// Robertson with the conservation law as third equation, M = diag(1, 1, 0): the hook writes the two non-zeros only
struct DaeRobertson {
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

// the unit pendulum p' = v, v' = -lam p - (0, 1), M = diag(1, 1, 1, 1, 0); INDEX = 2: 0 = p.v, INDEX = 3: 0 = |p|^2 - 1
template <int INDEX>
struct DaePendulum {
    enum { N = 5, P = 0, NE = 0 };
    static IVP_HD void ode(double, const double *s, double *d, const double *)
    {
        const double p1 = s[0], p2 = s[1], v1 = s[2], v2 = s[3], lam = s[4];
        d[0] = v1;
        d[1] = v2;
        d[2] = -lam * p1;
        d[3] = -lam * p2 - 1.0;
        d[4] = INDEX == 2 ? p1 * v1 + p2 * v2 : p1 * p1 + p2 * p2 - 1.0;
    }
    static IVP_HD void mass(double (&m)[5][5], const double *)
    {
        for (int i = 0; i < 4; ++i) m[i][i] = 1.0;
    }
};

template <class R, int FULL>
static void run_all(IvpKArgs a, uint64_t *chunks_out)
{
    static_assert(HasMass<R>::v, "every functor of this harness has the mass hook");
    uint64_t chunks = 0;
    for (uint32_t j = 0; j < a.B; ++j) {
        int32_t st = any_init_body<M_RADAU, R, FULL>(a, j);
        while (st == IVP_RUNNING) {
            any_chunk_body<M_RADAU, R, FULL>(a, j, st);
            ++chunks;
        }
    }
    if (chunks_out) *chunks_out = chunks;
}

template <class R>
static int run_rhs(int full, const IvpKArgs &a, uint64_t *chunks)
{
    full ? run_all<R, 1>(a, chunks) : run_all<R, 0>(a, chunks);
    return 0;
}

// mass_out (optional): [n n][B], what the init body left in the fifth persistent matrix
extern "C" int emul_dae_solve(int rhs_id, int n, int full, IvpKArgs *args, uint64_t *chunks, double *mass_out)
{
    IvpKArgs a = *args;
    const size_t B = a.B;
    // scratch sized as ivp_capi.cpp sizes it for a problem with a mass matrix: 5 n n B doubles behind bdf_jac,
    // (5 n + 3) B behind bdf_d, two pivot words per trajectory; filled with NaN so that a read of anything unwritten shows
    const double nan = __builtin_nan("");
    std::vector<double> k1((size_t)n * B, nan), facold(B, nan), hlamb(B, nan), t_last(B);
    std::vector<uint32_t> flags(B);
    std::vector<int32_t> next_idx(B);
    uint32_t err_flag = 0;
    a.err_flag = &err_flag;
    std::vector<double> rad_cont((size_t)(5 * n + 3) * B, nan), rad_mat((size_t)5 * n * n * B, nan);
    std::vector<uint32_t> rad_piv(2 * B);
    a.bdf_d = rad_cont.data(); a.bdf_jac = rad_mat.data(); a.bdf_lu = nullptr; a.bdf_piv = rad_piv.data();
    a.k1 = k1.data(); a.facold = facold.data(); a.hlamb = hlamb.data(); a.flags = flags.data();
    a.t_last = t_last.data(); a.next_idx = next_idx.data();
    int rc = -1;
    switch (rhs_id) {
    case 0: rc = n == 1 ? run_rhs<DaeScalar>(full, a, chunks) : -1; break;
    case 1: rc = n == 2 ? run_rhs<DaeSemi>(full, a, chunks) : -1; break;
    case 2: rc = n == 3 ? run_rhs<DaeRobertson>(full, a, chunks) : -1; break;
    case 3: rc = n == 5 ? run_rhs<DaePendulum<2>>(full, a, chunks) : -1; break;
    case 4: rc = n == 5 ? run_rhs<DaePendulum<3>>(full, a, chunks) : -1; break;
    case 5:
        switch (n) {
        case 1: rc = run_rhs<DaeLin<1>>(full, a, chunks); break;
        case 2: rc = run_rhs<DaeLin<2>>(full, a, chunks); break;
        case 3: rc = run_rhs<DaeLin<3>>(full, a, chunks); break;
        case 5: rc = run_rhs<DaeLin<5>>(full, a, chunks); break;
        case 8: rc = run_rhs<DaeLin<8>>(full, a, chunks); break;
        }
        break;
    }
    if (rc == 0 && mass_out) std::memcpy(mass_out, rad_mat.data() + (size_t)4 * n * n * B, sizeof(double) * (size_t)n * n * B);
    if (rc == 0 && (err_flag & 0x1u)) return -5;  // IVP_ERR_INVALID_STEP_SIZE
    return rc;
}

extern "C" size_t emul_dae_kargs_size(void) { return sizeof(IvpKArgs); }
