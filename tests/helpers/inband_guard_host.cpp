// inband_guard_host.cpp -- TEST-ONLY: the host restatements of the guards of the strict CR3BP right-hand side in
// ivp_amd/csrc/rk_core.h, for tests/test_inband_deferred_cpu.py and tests/test_gpu_inband_deferred.py (built with g++ into a
// temporary directory and loaded with ctypes).
//   inband_guards   per state (x, y, z, mu): the per-call guard (ivp_sq_inband / ivp_num_inband on s1, s2 and the six
//                   products) and the folded guard of the deferred form after this one call (ivp_inband_seed, the fold
//                   inside RhsCr3bp::ode_deferred<true>, ivp_inband_ok)
//   inband_trace    one trajectory, attempt by attempt: which stages of each attempt's stage block are in band
#include <cstdint>
#include <cstring>
#include <vector>

#define IVP_HD inline
#define IVP_NS ivp_guard
#include "../../ivp_amd/csrc/rk_core.h"

namespace ivp_guard {
// an accumulator that keeps every call's own answer (found by argument-dependent lookup from ode_deferred)
struct TraceAcc { int n; int ok[16]; };
inline void ivp_inband_fold(TraceAcc &t, double s1, double s2, double a, double b, double y, double z)
{
    IvpInbandAcc acc = ivp_inband_begin(0);
    ivp_inband_fold(acc, s1, s2, a, b, y, z);
    t.ok[t.n++] = ivp_inband_ok(acc) ? 1 : 0;
}
}  // namespace ivp_guard

using namespace ivp_guard;

extern "C" void inband_guards(const double *x, const double *y, const double *z, const double *mu, int *per_call, int *folded, long n)
{
    for (long i = 0; i < n; ++i) {
        const double s[6] = {x[i], y[i], z[i], 0.25, -0.5, 0.125}, p[1] = {mu[i]};
        const double a = s[0] + p[0], b = s[0] - 1.0 + p[0];
        per_call[i] = RhsCr3bp::strict_inband(RhsCr3bp::strict_terms(s, p[0], a, b)) ? 1 : 0;
        IvpInbandAcc acc = ivp_inband_begin(RhsCr3bp::inband_seed(p));
        double d[6];
        RhsCr3bp::ode_deferred<true>(0.0, s, d, p, acc);
        folded[i] = ivp_inband_ok(acc) ? 1 : 0;
    }
}

// DOPRI5 (method 1) or DOP853 (method 2) on one trajectory with the default controller, rtol / atol as given; before each
// attempt the stage block is evaluated on the lane's state and stage_ok[attempt][0 .. n_stages) says which of its calls were
// in band (the step the attempt takes may be shorter: the last one is cut to the interval's end).  Returns the attempts made.
extern "C" int inband_trace(const double *y0, double mu, double t1, int method, double rtol, double atol, int max_attempts, int *stage_ok,
                            int *n_stages)
{
    constexpr int N = 6;
    IvpKArgs a;
    std::memset(&a, 0, sizeof a);
    a.B = 1;
    const double t0 = 0.0;
    a.y0 = y0; a.params = &mu; a.t0 = &t0; a.t1 = &t1;
    for (int i = 0; i < IVP_MAX_N; ++i) { a.rtol[i] = rtol; a.atol[i] = atol; }
    a.nmax = UINT64_MAX;
    a.ctl_nstiff = 1000;
    a.chunk = 1;
    a.n_eval = -1;
    double y[N], k1[N], x, h, facold, hlamb;
    uint32_t flags = 0, err_flag = 0;
    int32_t status = 0;
    uint64_t cnt[4] = {0, 0, 0, 0};
    a.y = y; a.k1 = k1; a.x = &x; a.h = &h; a.facold = &facold; a.hlamb = &hlamb; a.flags = &flags; a.status = &status;
    a.nfev = cnt; a.nstep = cnt + 1; a.naccpt = cnt + 2; a.nrejct = cnt + 3; a.err_flag = &err_flag;
    int32_t st = method == 2 ? init_body<M_DOP853, RhsCr3bp, 0>(a, 0) : init_body<M_DOPRI5, RhsCr3bp, 0>(a, 0);
    *n_stages = method == 2 ? 11 : 6;
    int it = 0;
    while (st == IVP_RUNNING && it < max_attempts) {
        TraceAcc t;
        t.n = 0;
        double k2[N], k3[N], k4[N], k5[N], k6[N], k7[N], k8[N], k9[N], k10[N], y1[N], xph;
        if (method == 2) dop853_stages<RhsCr3bp, true>(x, h, xph, y, k1, &mu, 0, k2, k3, k4, k5, k6, k7, k8, k9, k10, y1, t);
        else dopri5_stages<RhsCr3bp, true>(x, h, xph, y, k1, &mu, 0, k2, k3, k4, k5, k6, y1, t);
        for (int s = 0; s < *n_stages; ++s) stage_ok[it * 12 + s] = t.ok[s];
        if (method == 2) chunk_body<M_DOP853, RhsCr3bp, 0>(a, 0, st);
        else chunk_body<M_DOPRI5, RhsCr3bp, 0>(a, 0, st);
        ++it;
    }
    return it;
}
