// balance_emul_main.cpp -- TEST-ONLY stand-alone program (its own main, no GPU, no Python): a batch of 443 CR3BP trajectories
// (7 blocks of 64 list entries, the last one ragged) through the kernel bodies of ivp_amd/csrc/rk_core.h on the host, once
// with the plain schedule (init, then chunks of 64 attempts until every trajectory has retired) and once with the schedule
// of the launch loop's balanced rounds: per round the plan of ivp_amd/csrc/ivp_balance.h, its L launches walked workgroup by
// workgroup and piece by piece exactly as balanced_chunk_kernel_t (rk_global.h) does, survivors appended by a block's last
// piece, and three plain launches where the plan does not apply.  Every result array must be bit-identical, every
// trajectory that is still running at the end of a balanced round must have taken exactly R attempts in it, and no list
// entry may be lost or doubled.  Built with -fsanitize=address,undefined by tests/test_balance_emul_cpu.py; every array is
// sized exactly.  Exit status 0 = all held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#define IVP_HD inline
#define IVP_NS ivp_bal_emul
#include "../../ivp_amd/csrc/rk_core.h"
#include "../../ivp_amd/csrc/ivp_balance.h"

using namespace ivp_bal_emul;

namespace {

constexpr uint32_t B = 443;
constexpr int N = 6;
constexpr uint32_t kChunk = 64, kLaunchesPerPoll = 3, kMaxLog = 40;
int failures = 0;

struct Batch { std::vector<double> y0, mu, t1; };

// orbits around the Earth-Moon system; every seventh interval has zero length (the trajectory retires in the init body) and
// the others differ in length by a factor of eight, so that trajectories retire in the middle of rounds and whole blocks die
Batch make_batch()
{
    Batch b;
    b.y0.assign((size_t)N * B, 0.0);
    b.mu.assign(B, 0.0121505856);
    b.t1.assign(B, 0.0);
    for (uint32_t j = 0; j < B; ++j) {
        const double s = (double)(j % 61) / 61.0;
        b.y0[0 * B + j] = 0.82 + 0.2 * s;
        b.y0[1 * B + j] = 0.02 * (j % 3);
        b.y0[2 * B + j] = (j % 2) ? 0.05 * s : 0.0;
        b.y0[3 * B + j] = 0.01 * (j % 4);
        b.y0[4 * B + j] = 0.12 - 0.3 * s;
        b.y0[5 * B + j] = (j % 2) ? 0.01 : 0.0;
        b.t1[j] = (j % 7 == 3) ? 0.0 : 0.5 * (1 + j % 8);
        if (j >= 64 && j < 128) b.t1[j] = (j % 2) ? 0.0 : 0.25;   // a block that is gone after its first piece or two
    }
    return b;
}

struct Out {
    std::vector<double> y, x, h, t_log, y_log;
    std::vector<int32_t> status;
    std::vector<uint32_t> n_log;
    std::vector<uint64_t> cnt;
    bool same(const Out &o) const
    {
        auto eq = [](const auto &u, const auto &v) { return u.size() == v.size() && (u.empty() || std::memcmp(u.data(), v.data(), u.size() * sizeof(u[0])) == 0); };
        return eq(y, o.y) && eq(x, o.x) && eq(h, o.h) && eq(t_log, o.t_log) && eq(y_log, o.y_log) && eq(status, o.status) && eq(n_log, o.n_log) && eq(cnt, o.cnt);
    }
};

// S = 0: the plain schedule
template <int M, int FULL>
Out run(const Batch &b, uint32_t S, unsigned long long *balanced_rounds)
{
    using R = RhsCr3bp;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    IvpKArgs a;
    std::memset(&a, 0, sizeof a);
    a.B = B;
    const double t0 = 0.0;
    a.y0 = b.y0.data(); a.params = b.mu.data(); a.t0 = &t0; a.t1 = b.t1.data(); a.t1_stride = 1;
    for (int i = 0; i < IVP_MAX_N; ++i) { a.rtol[i] = 1e-6; a.atol[i] = 1e-9; }
    a.nmax = 800;   // the few orbits that pass close to a primary stop here (status 2)
    a.ctl_nstiff = 1000;
    a.chunk = kChunk;
    a.n_eval = -1;
    Out o;
    o.y.assign((size_t)N * B, nan); o.x.assign(B, nan); o.h.assign(B, nan); o.status.assign(B, 0); o.cnt.assign(4 * (size_t)B, 0);
    std::vector<double> k1((size_t)N * B), facold(B), hlamb(B), t_last(B);
    std::vector<uint32_t> flags(B), n_seg(B);
    std::vector<int32_t> next_idx(B), n_filled(B);
    uint32_t err_flag = 0;
    a.err_flag = &err_flag;
    a.y = o.y.data(); a.x = o.x.data(); a.h = o.h.data(); a.status = o.status.data();
    a.nfev = o.cnt.data(); a.nstep = o.cnt.data() + B; a.naccpt = o.cnt.data() + 2 * B; a.nrejct = o.cnt.data() + 3 * B;
    a.k1 = k1.data(); a.facold = facold.data(); a.hlamb = hlamb.data(); a.flags = flags.data();
    a.t_last = t_last.data(); a.next_idx = next_idx.data();
    if (FULL) {
        o.n_log.assign(B, 0);
        a.n_filled = n_filled.data(); a.n_log = o.n_log.data(); a.n_seg = n_seg.data();
        a.max_log = kMaxLog;   // fewer than the steps of the long trajectories: the records past it are dropped, not written
        o.t_log.assign((size_t)kMaxLog * B, nan); o.y_log.assign((size_t)kMaxLog * N * B, nan);
        a.t_log = o.t_log.data(); a.y_log = o.y_log.data();
    }
    std::vector<uint32_t> list, next;
    for (uint32_t j = 0; j < B; ++j)
        if (init_body<M, R, FULL>(a, j) == IVP_RUNNING) list.push_back(j);
    if (S == 0) {
        for (uint32_t j : list) {
            int32_t st = IVP_RUNNING;
            while (st == IVP_RUNNING) chunk_body<M, R, FULL>(a, j, st);
        }
        return o;
    }
    std::vector<uint32_t> took(B), touched(B);
    while (!list.empty()) {
        const uint32_t count = (uint32_t)list.size(), Rr = kLaunchesPerPoll * kChunk;
        const IvpBalancePlan p = ivp_balance_plan(count, Rr, S, kChunk);
        next.clear();
        if (p.L == 0) {   // plain launches
            for (uint32_t r = 0; r < kLaunchesPerPoll; ++r) {
                next.clear();
                for (uint32_t j : list) {
                    int32_t st = IVP_RUNNING;
                    chunk_body<M, R, FULL>(a, j, st);
                    if (st == IVP_RUNNING) next.push_back(j);
                }
                list.swap(next);
            }
            continue;
        }
        *balanced_rounds += 1;
        std::fill(took.begin(), took.end(), 0u);
        const uint32_t nb = (count + 63u) / 64u;
        for (uint32_t l = 0; l < p.L; ++l) {
            std::fill(touched.begin(), touched.end(), 0u);
            for (uint32_t w = 0; w < p.W; ++w) {
                // the kernel's own arithmetic (rk_global.h)
                const uint64_t total = (uint64_t)nb * Rr;
                uint64_t u = ((uint64_t)w * p.L + l) * p.q;
                const uint64_t uend = u + p.q < total ? u + p.q : total;
                while (u < uend) {
                    const uint32_t blk = (uint32_t)(u / Rr);
                    const uint64_t bend = (uint64_t)(blk + 1u) * Rr;
                    const uint32_t n = (uint32_t)((uend < bend ? uend : bend) - u);
                    const bool last = ivp_balance_last_launch(blk, Rr, p.q, p.L) == l;
                    u += n;
                    for (uint32_t t = 0; t < 64u; ++t) {
                        const uint32_t i = blk * 64u + t;
                        if (i >= count) continue;
                        const uint32_t j = list[i];
                        if (touched[j]++) { std::printf("FAILED: trajectory %u twice in launch %u (S = %u)\n", j, l, S); ++failures; }
                        int32_t st = 0;
                        const bool active = a.status[j] == IVP_RUNNING;
                        if (active) took[j] += chunk_body<M, R, FULL, false, true>(a, j, st, n);
                        if (last && active && st == IVP_RUNNING) next.push_back(j);
                    }
                }
            }
        }
        for (uint32_t j : list)
            if (a.status[j] == IVP_RUNNING && took[j] != Rr) { std::printf("FAILED: trajectory %u took %u of %u attempts (S = %u)\n", j, took[j], Rr, S); ++failures; }
        uint32_t running = 0;
        for (uint32_t j : list) running += a.status[j] == IVP_RUNNING ? 1u : 0u;
        if (running != next.size()) { std::printf("FAILED: %u running, %zu on the output list (S = %u)\n", running, next.size(), S); ++failures; }
        list.swap(next);
    }
    return o;
}

template <int M, int FULL>
void compare(const Batch &b, const char *what)
{
    unsigned long long none = 0;
    const Out plain = run<M, FULL>(b, 0, &none);
    unsigned long long steps = 0;
    for (uint32_t j = 0; j < B; ++j) steps += plain.cnt[B + j];
    for (uint32_t S : {5u, 4u, 2u, 1u}) {
        unsigned long long rounds = 0;
        const Out bal = run<M, FULL>(b, S, &rounds);
        const bool same = bal.same(plain);
        std::printf("%s: %llu attempts, %u wave slots, %llu balanced rounds: %s\n", what, steps, S, rounds, same ? "bit-identical" : "DIFFERENT   <-- FAILED");
        if (!same || rounds == 0) ++failures;
    }
}

}  // namespace

int main()
{
    const Batch b = make_batch();
    compare<M_DOPRI5, 0>(b, "DOPRI5 end state");
    compare<M_DOPRI5, 2>(b, "DOPRI5 step log ");
    compare<M_DOP853, 0>(b, "DOP853 end state");
    std::printf("%d failures\n", failures);
    return failures == 0 ? 0 : 1;
}
