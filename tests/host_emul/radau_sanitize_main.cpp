// radau_sanitize_main.cpp -- TEST-ONLY stand-alone program: a handful of Radau cases through emul.cpp's emul_solve, to be built
// with a host sanitizer (`make -C tests/host_emul sanitize`, see the Makefile) and run on its own.  It checks no results --
// tests/test_radau_emul_cpu.py does that -- only that the kernel body reads and writes inside its arrays and stays within
// defined behaviour on the branches those tests name: restarts of every kind, step bounds, every output, N = 1, 2, 8,
// zero-length and NaN intervals.  Every array is sized exactly, so an index past its end is a heap overflow.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../ivp_amd/csrc/ivp_kargs.h"

extern "C" int emul_solve(int method, int rhs_id, int full, IvpKArgs *args, uint64_t *chunks);

namespace {

const double U1 = 3.637834252744496, ALPH = 2.6810828736277523, BETA = 3.0504301992474105;

struct Case {
    const char *name;
    int rhs_id, n, np;
    std::vector<double> y0, params;   // [n][B], [np][B]
    double t0, t1;
    int newton_maxiter = 7;
    double first_step = 0.0, max_step = 0.0, min_step = 0.0;   // 0: not given
    int out = 0;                                               // 0 end state, 1 t_eval, 2 log + dense segments
};

int run(const Case &c, uint32_t B, uint32_t chunk)
{
    const int n = c.n;
    IvpKArgs a;
    std::memset(&a, 0, sizeof a);
    a.B = B;
    std::vector<double> t0(1, c.t0), t1(1, c.t1), params(c.params.empty() ? std::vector<double>(B, 0.0) : c.params);
    a.y0 = c.y0.data(); a.params = params.data(); a.t0 = t0.data(); a.t1 = t1.data();
    for (int i = 0; i < IVP_MAX_N; ++i) { a.rtol[i] = 1e-6; a.atol[i] = 1e-8; }
    a.first_step = c.first_step; a.has_first_step = c.first_step != 0.0;
    a.max_step = c.max_step; a.has_max_step = c.max_step != 0.0;
    a.min_step = c.min_step; a.has_min_step = c.min_step != 0.0;
    a.nmax = UINT64_MAX;
    a.ctl_uround = 2.3e-16; a.ctl_safety = 0.9; a.ctl_facc1 = 1.0 / 0.2; a.ctl_facc2 = 1.0 / 8.0;
    a.ctl_nstiff = (uint64_t)c.newton_maxiter | 0x200ull;   // predictive
    std::vector<double> y((size_t)n * B), x(B), h(B);
    std::vector<int32_t> status(B);
    std::vector<uint64_t> cnt(6 * (size_t)B);
    a.y = y.data(); a.x = x.data(); a.h = h.data(); a.status = status.data();
    a.nfev = cnt.data(); a.nstep = cnt.data() + B; a.naccpt = cnt.data() + 2 * B; a.nrejct = cnt.data() + 3 * B;
    a.njev = cnt.data() + 4 * B; a.nlu = cnt.data() + 5 * B;
    a.chunk = chunk;
    a.n_eval = -1;
    const uint32_t max_log = 5;   // small: the records past it must be dropped, not written
    std::vector<double> te = {c.t0, c.t0 + 5e-13, 0.5 * (c.t0 + c.t1), c.t1, c.t1 + 1.0};
    std::vector<int32_t> n_filled(B), eval_idx(te.size() * B);
    std::vector<uint32_t> n_log(B), n_seg(B);
    std::vector<double> y_eval(te.size() * n * B), t_log((size_t)max_log * B), y_log((size_t)max_log * n * B);
    std::vector<double> seg_cont((size_t)max_log * 4 * n * B), seg_xold((size_t)max_log * B), seg_h((size_t)max_log * B);
    if (c.out) {
        a.n_filled = n_filled.data(); a.n_log = n_log.data(); a.n_seg = n_seg.data();
        if (c.out == 1) {
            a.n_eval = (int32_t)te.size(); a.t_eval = te.data(); a.y_eval = y_eval.data(); a.eval_idx = eval_idx.data();
        } else {
            a.max_log = max_log; a.t_log = t_log.data(); a.y_log = y_log.data();
            a.seg_cont = seg_cont.data(); a.seg_xold = seg_xold.data(); a.seg_h = seg_h.data(); a.collect_dense = 1;
        }
    }
    uint64_t chunks = 0;
    const int rc = emul_solve(4, c.rhs_id, c.out ? 1 : 0, &a, &chunks);
    std::printf("%-28s chunk %-10u rc %d status", c.name, chunk, rc);
    for (uint32_t b = 0; b < B; ++b) std::printf(" %d", status[b]);
    std::printf("  nstep %llu  launches %llu\n", (unsigned long long)cnt[B], (unsigned long long)chunks);
    return rc;
}

}  // namespace

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double h6 = std::ldexp(1.0, -6), h10 = std::ldexp(1.0, -10);
    std::vector<double> a8(64 * 2), y8 = {1.0, 0.5, 0.5, 0.5, -0.5, 0.5, 0.25, 0.5, 0.0, 0.5, 1e-3, 0.5, -1.0, 0.5, 2.0, 0.5};
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) {
            double v = 1e-3 * (1 + ((3 * i + 5 * j) % 7));
            if (i == j) v = -1.0 - 0.25 * i;
            if ((i % 2) && j == i - 1) v = 200.0;
            a8[(size_t)(i * 8 + j) * 2] = a8[(size_t)(i * 8 + j) * 2 + 1] = v;
        }
    const double ra = ALPH / h6, rb = BETA / h6;
    std::vector<Case> cases = {
        {"stiff VdP", 10, 2, 1, {2.0, 2.1, 0.0, 0.1}, {1e-3, 2e-3}, 0.0, 2.0},
        {"stiff VdP maxiter 1", 10, 2, 1, {2.0, 2.1, 0.0, 0.1}, {1e-3, 2e-3}, 0.0, 2.0, 1},
        {"stiff VdP maxiter 2", 10, 2, 1, {2.0, 2.1, 0.0, 0.1}, {1e-3, 2e-3}, 0.0, 2.0, 2},
        {"stiff VdP step bounds log", 10, 2, 1, {2.0, 2.1, 0.0, 0.1}, {1e-3, 2e-3}, 0.0, 2.0, 7, 0.5, 0.02, 1e-3, 2},
        {"decay real zero pivot", 0, 1, 1, {0.0, std::ldexp(1.0, -26)}, {-(U1 / 0.01), -(U1 / 0.01)}, 0.0, 0.05, 7, 0.01},
        {"rotation complex zero pivot", 17, 2, 4, {1.0, 0.3, 0.0, -0.7}, {ra, ra, -rb, -rb, rb, rb, ra, ra}, 0.0, 4.0 * h6, 7, h6},
        {"imaginary multiplier", 17, 2, 4, {1.0, 0.5, 0.0, 0.25}, {0.0, 0.0, 1.0, 1.0, -1e5, -1e5, ALPH / h10, ALPH / h10}, 0.0, 8.0 * h10, 7, h10},
        {"Robertson jac t_eval", 15, 3, 0, {1.0, 1.0, 0.0, 0.0, 0.0, 0.0}, {}, 0.0, 1e3, 7, 0.0, 0.0, 0.0, 1},
        {"8 x 8 linear fd t_eval", 24, 8, 64, y8, a8, 0.0, 3.0, 7, 0.0, 0.0, 0.0, 1},
        {"8 x 8 linear jac dense", 25, 8, 64, y8, a8, 0.0, 3.0, 7, 0.0, 0.0, 0.0, 2},
        {"8 x 8 backwards dense", 25, 8, 64, y8, a8, 0.0, -1.0, 7, 0.0, 0.0, 0.0, 2},
        {"zero-length t_eval", 25, 8, 64, y8, a8, 0.25, 0.25, 7, 0.0, 0.0, 0.0, 1},
        {"zero-length dense", 25, 8, 64, y8, a8, 0.25, 0.25, 7, 0.0, 0.0, 0.0, 2},
        {"NaN interval dense", 25, 8, 64, y8, a8, 0.25, nan, 7, 0.0, 0.0, 0.0, 2},
    };
    int bad = 0;
    for (const Case &c : cases)
        for (uint32_t chunk : {1u, 7u, 0xFFFFFFFFu}) bad += run(c, 2, chunk) != 0;
    std::printf("%s\n", bad ? "FAILED" : "all cases ran");
    return bad ? 1 : 0;
}
