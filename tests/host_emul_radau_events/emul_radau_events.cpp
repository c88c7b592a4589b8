// emul_radau_events.cpp -- TEST-ONLY harness: the Radau IIA(5) kernel bodies of ivp_amd/csrc/radau_core.h for problems WITH
// EVENT FUNCTIONS (FULL flavour: DefaultSolOut with so_events / so_event_root of rk_core.h), pure ODEs and M y' = f, run on the
// CPU lane by lane with the GPU launch loop's init -> chunk -> chunk ... schedule.  A sibling of tests/host_emul (whose Radau
// entry rejects event problems) and tests/host_emul_dae; the functors here are test-only.  Not part of the product: nothing
// in ivp_amd/ links or loads it.  Compiled with g++ -ffp-contract=off (strict arithmetic, the only Radau build).
// Built as a shared library for the tests and, with -DEMUL_MAIN, as a stand-alone program (its own main) for gdb or a host
// sanitizer.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define IVP_HD inline
#define IVP_NS ivp_emul_rev
#include "../../ivp_amd/csrc/rk_core.h"
#include "../../ivp_amd/csrc/bdf_core.h"
#include "../../ivp_amd/csrc/radau_core.h"

using namespace ivp_emul_rev;

// y' = -p0 (y - p1), event: y = p2
struct EvRelax {
    enum { N = 1, P = 3, NE = 1 };
    static IVP_HD void ode(double, const double *y, double *d, const double *p) { d[0] = -p[0] * (y[0] - p[1]); }
    static IVP_HD void events(double, const double *y, double *g, const double *p) { g[0] = y[0] - p[2]; }
};

// y' = A y, A row-major in p[0 .. N N), each row summed left to right; two events: y[0] = p[N N], y[N - 1] = p[N N + 1]
template <int N_>
struct EvLin {
    enum { N = N_, P = N_ * N_ + 2, NE = 2 };
    static IVP_HD void ode(double, const double *y, double *d, const double *p)
    {
        for (int i = 0; i < N; ++i) {
            double s = p[i * N] * y[0];
            for (int j = 1; j < N; ++j) s = s + p[i * N + j] * y[j];
            d[i] = s;
        }
    }
    static IVP_HD void events(double, const double *y, double *g, const double *p)
    {
        g[0] = y[0] - p[N * N];
        g[1] = y[N - 1] - p[N * N + 1];
    }
};

// Robertson, forward-difference Jacobian; event: the threshold p0 on y[1]
struct EvRobertson {
    enum { N = 3, P = 1, NE = 1 };
    static IVP_HD void ode(double, const double *s, double *d, const double *)
    {
        const double xx = s[0], y = s[1], z = s[2];
        d[0] = -0.04 * xx + 1e4 * y * z;
        d[1] = 0.04 * xx - 1e4 * y * z - 3e7 * y * y;
        d[2] = 3e7 * y * y;
    }
    static IVP_HD void events(double, const double *y, double *g, const double *p) { g[0] = y[1] - p[0]; }
};

// the unit pendulum, index 2 (0 = p.v), M = diag(1, 1, 1, 1, 0); event: the passage through the vertical, p1 = 0
struct EvPendulum {
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
static int run_all(IvpKArgs a, uint64_t *chunks_out)
{
    static_assert(R::NE > 0, "every functor of this harness has event functions");
    uint64_t chunks = 0;
    for (uint32_t j = 0; j < a.B; ++j) {
        int32_t st = any_init_body<M_RADAU, R, 1>(a, j);
        while (st == IVP_RUNNING) {
            any_chunk_body<M_RADAU, R, 1>(a, j, st);
            ++chunks;
        }
    }
    if (chunks_out) *chunks_out = chunks;
    return 0;
}

// rhs_id: 0 relax (n = 1), 1 lin<n> (n = 2, 8), 2 robertson (n = 3), 3 pendulum (n = 5, mass, index 2)
extern "C" int emul_rev_solve(int rhs_id, int n, int ne, IvpKArgs *args, uint64_t *chunks)
{
    IvpKArgs a = *args;
    const size_t B = a.B;
    // scratch sized as ivp_capi.cpp sizes it for a problem with a mass matrix (a superset of the plain layout), filled with
    // NaN so that a read of anything unwritten shows; prev_event as submit_impl reserves it: [n_events][B]
    const double nan = __builtin_nan("");
    std::vector<double> k1((size_t)n * B, nan), facold(B, nan), hlamb(B, nan), t_last(B), prev((size_t)ne * B, nan);
    std::vector<uint32_t> flags(B);
    std::vector<int32_t> next_idx(B);
    uint32_t err_flag = 0;
    a.err_flag = &err_flag;
    std::vector<double> rad_cont((size_t)(5 * n + 3) * B, nan), rad_mat((size_t)5 * n * n * B, nan);
    std::vector<uint32_t> rad_piv(2 * B);
    a.bdf_d = rad_cont.data(); a.bdf_jac = rad_mat.data(); a.bdf_lu = nullptr; a.bdf_piv = rad_piv.data();
    a.k1 = k1.data(); a.facold = facold.data(); a.hlamb = hlamb.data(); a.flags = flags.data();
    a.t_last = t_last.data(); a.next_idx = next_idx.data();
    a.prev_event = prev.data();
    a.evd_rec = nullptr;   // Radau refines inline
    int rc = -1;
    switch (rhs_id) {
    case 0: rc = (n == 1 && ne == 1) ? run_all<EvRelax>(a, chunks) : -1; break;
    case 1:
        if (ne == 2 && n == 2) rc = run_all<EvLin<2>>(a, chunks);
        if (ne == 2 && n == 8) rc = run_all<EvLin<8>>(a, chunks);
        break;
    case 2: rc = (n == 3 && ne == 1) ? run_all<EvRobertson>(a, chunks) : -1; break;
    case 3: rc = (n == 5 && ne == 1) ? run_all<EvPendulum>(a, chunks) : -1; break;
    }
    if (rc == 0 && (err_flag & 0x1u)) return -5;  // IVP_ERR_INVALID_STEP_SIZE
    return rc;
}

extern "C" size_t emul_rev_kargs_size(void) { return sizeof(IvpKArgs); }

#ifdef EMUL_MAIN
// stand-alone: the relaxation problem with a terminal crossing and the two-event linear system, chunk lengths 1, 7, unbounded
int main()
{
    int bad = 0;
    const uint32_t chunks[3] = {1u, 7u, 0xFFFFFFFFu};
    for (int prob = 0; prob < 2; ++prob)
        for (uint32_t chunk : chunks) {
            const int n = prob == 0 ? 1 : 2, ne = prob == 0 ? 1 : 2, np = prob == 0 ? 3 : 6;
            const uint32_t B = 3, mev = 4;
            std::vector<double> y0((size_t)n * B), par((size_t)np * B), t0(1, 0.0), t1(1, 4.0);
            for (uint32_t b = 0; b < B; ++b) {
                if (prob == 0) { y0[b] = 2.0 + b; par[b] = 50.0; par[B + b] = 0.5; par[2 * B + b] = 1.0; }
                else {
                    y0[b] = 1.0; y0[B + b] = 0.0;
                    const double A[4] = {-0.1, 1.0 + 0.25 * b, -1.0 - 0.25 * b, -0.1};
                    for (int q = 0; q < 4; ++q) par[(size_t)q * B + b] = A[q];
                    par[4 * B + b] = 0.0; par[5 * B + b] = 0.0;
                }
            }
            std::vector<double> y((size_t)n * B), x(B), h(B), tev((size_t)ne * mev * B), yev((size_t)ne * mev * n * B), tterm(B);
            std::vector<int32_t> status(B), n_filled(B);
            std::vector<uint64_t> cnt(6 * (size_t)B);
            std::vector<uint32_t> n_ev((size_t)ne * B), n_log(B), n_seg(B);
            IvpKArgs a;
            std::memset(&a, 0, sizeof a);
            a.B = B; a.y0 = y0.data(); a.params = par.data(); a.t0 = t0.data(); a.t1 = t1.data();
            for (int i = 0; i < IVP_MAX_N; ++i) { a.rtol[i] = 1e-6; a.atol[i] = 1e-9; }
            a.nmax = UINT64_MAX;
            a.ctl_uround = 2.3e-16; a.ctl_safety = 0.9; a.ctl_facc1 = 1.0 / 0.2; a.ctl_facc2 = 1.0 / 8.0; a.ctl_nstiff = 7ull | 0x200ull;
            a.y = y.data(); a.x = x.data(); a.h = h.data(); a.status = status.data();
            a.nfev = cnt.data(); a.nstep = cnt.data() + B; a.naccpt = cnt.data() + 2 * B; a.nrejct = cnt.data() + 3 * B;
            a.njev = cnt.data() + 4 * B; a.nlu = cnt.data() + 5 * B;
            a.chunk = chunk; a.n_eval = -1;
            a.n_filled = n_filled.data(); a.n_log = n_log.data(); a.n_seg = n_seg.data();
            a.max_events = mev; a.t_events = tev.data(); a.y_events = yev.data(); a.n_ev = n_ev.data(); a.t_term = tterm.data();
            a.ev_terminal[0] = prob == 0 ? 1u : 0u;
            uint64_t launches = 0;
            const int rc = emul_rev_solve(prob, n, ne, &a, &launches);
            for (uint32_t b = 0; b < B; ++b) {
                const int want = prob == 0 ? 1 : 0;
                if (rc != 0 || status[b] != want || n_ev[b] == 0) bad = 1;
                std::printf("prob %d chunk %u traj %u: rc %d status %d hits %u first t %.17g launches %llu\n", prob, chunk, b, rc, status[b], n_ev[b],
                            tev[b], (unsigned long long)launches);
            }
        }
    return bad;
}
#endif
