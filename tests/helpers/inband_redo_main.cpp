// inband_redo_main.cpp -- TEST-ONLY stand-alone program (its own main, no GPU, no Python): whole DOPRI5 and DOP853 solves of 16
// CR3BP trajectories through the kernel bodies of ivp_amd/csrc/rk_core.h, lane by lane, in every output flavour, with the
// launch loop's init -> chunk -> chunk schedule.  Every result array is written to the file named on the command line.
//
// tests/test_inband_deferred_cpu.py builds it twice -- as is, and with -DIVP_INBAND_FORCE_REDO, which makes the deferred
// guard answer "out of band" after every stage block, so that every attempt runs the block a second time on the plain
// operators -- and compares the two files byte for byte: the redo must be a pure recomputation (nothing written before the
// decision, nothing left over from the first pass).  The same source is built with -fsanitize=address,undefined and run on
// its own; every array is sized exactly, so an index past its end is a heap overflow.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#define IVP_HD inline
#define IVP_NS ivp_redo
#include "../../ivp_amd/csrc/rk_core.h"

using namespace ivp_redo;

namespace {

constexpr uint32_t B = 16;
constexpr int N = 6;

struct Batch { std::vector<double> y0, mu; };

// 16 initial states: planar and spatial orbits around the Earth-Moon system, plus the trajectories that leave the band of
// the in-range division and square root (tests/test_gpu_inband_div_sqrt.py: a tiny out-of-plane offset, a denormal
// coordinate, at rest 1e-31 from the first primary) and coefficients the per-chunk test rejects (mu = 2^-60, mu = 0)
Batch make_batch()
{
    Batch b;
    b.y0.assign((size_t)N * B, 0.0);
    b.mu.assign(B, 0.0121505856);
    for (uint32_t j = 0; j < B; ++j) {
        const double s = (double)j / B;
        b.y0[0 * B + j] = 0.82 + 0.2 * s;
        b.y0[1 * B + j] = 0.02 * (j % 3);
        b.y0[2 * B + j] = (j % 2) ? 0.05 * s : 0.0;
        b.y0[3 * B + j] = 0.01 * (j % 4);
        b.y0[4 * B + j] = 0.12 - 0.3 * s;
        b.y0[5 * B + j] = (j % 2) ? 0.01 : 0.0;
    }
    b.y0[2 * B + 3] = 1e-200; b.y0[5 * B + 3] = 0.0;
    b.y0[1 * B + 6] = 5e-324;
    const double mu = b.mu[9];
    const double rest[N] = {-mu, 1e-31, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < N; ++c) b.y0[c * B + 9] = rest[c];
    b.mu[12] = std::ldexp(1.0, -60);
    b.mu[13] = 0.0;
    return b;
}

struct Out {
    std::vector<double> y, x, h, y_eval, t_log, y_log, seg_cont, seg_xold, seg_h, def_rec;
    std::vector<int32_t> status, n_filled, eval_idx;
    std::vector<uint32_t> n_log, n_seg;
    std::vector<uint64_t> cnt;
    void dump(std::FILE *f) const
    {
        auto w = [&](const void *p, size_t bytes) { if (bytes) std::fwrite(p, 1, bytes, f); };
        w(y.data(), y.size() * 8); w(x.data(), x.size() * 8); w(h.data(), h.size() * 8); w(y_eval.data(), y_eval.size() * 8);
        w(t_log.data(), t_log.size() * 8); w(y_log.data(), y_log.size() * 8); w(seg_cont.data(), seg_cont.size() * 8);
        w(seg_xold.data(), seg_xold.size() * 8); w(seg_h.data(), seg_h.size() * 8); w(def_rec.data(), def_rec.size() * 8);
        w(status.data(), status.size() * 4); w(n_filled.data(), n_filled.size() * 4); w(eval_idx.data(), eval_idx.size() * 4);
        w(n_log.data(), n_log.size() * 4); w(n_seg.data(), n_seg.size() * 4); w(cnt.data(), cnt.size() * 8);
    }
};

// flavour: 0 end state, 1 t_eval (whole DefaultSolOut), 2 step log + dense segments (whole DefaultSolOut), 3 log-only,
// 4 deferred t_eval sampling (DOP853 only)
template <int M, int FULL>
void run(const Batch &b, int flavour, uint32_t chunk, std::FILE *f)
{
    using R = RhsCr3bp;
    constexpr int NC = (M == M_DOP853 ? 8 : 5) * N;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    IvpKArgs a;
    std::memset(&a, 0, sizeof a);
    a.B = B;
    const double t0 = 0.0, t1 = 2.5;
    a.y0 = b.y0.data(); a.params = b.mu.data(); a.t0 = &t0; a.t1 = &t1;
    for (int i = 0; i < IVP_MAX_N; ++i) { a.rtol[i] = 1e-6; a.atol[i] = 1e-9; }
    a.nmax = 600;
    a.ctl_nstiff = 1000;
    a.chunk = chunk;
    a.n_eval = -1;
    Out o;
    o.y.assign((size_t)N * B, nan); o.x.assign(B, nan); o.h.assign(B, nan); o.status.assign(B, 0); o.cnt.assign(4 * (size_t)B, 0);
    std::vector<double> k1((size_t)N * B), facold(B), hlamb(B), t_last(B);
    std::vector<uint32_t> flags(B);
    std::vector<int32_t> next_idx(B);
    uint32_t err_flag = 0;
    a.err_flag = &err_flag;
    a.y = o.y.data(); a.x = o.x.data(); a.h = o.h.data(); a.status = o.status.data();
    a.nfev = o.cnt.data(); a.nstep = o.cnt.data() + B; a.naccpt = o.cnt.data() + 2 * B; a.nrejct = o.cnt.data() + 3 * B;
    a.k1 = k1.data(); a.facold = facold.data(); a.hlamb = hlamb.data(); a.flags = flags.data();
    a.t_last = t_last.data(); a.next_idx = next_idx.data();
    std::vector<double> te;
    for (int i = 0; i <= 20; ++i) te.push_back(t0 + (t1 - t0) * i / 20.0);
    const uint32_t max_log = 48;   // fewer than the steps of most trajectories: the records past it must be dropped
    if (flavour) {
        o.n_filled.assign(B, 0); o.n_log.assign(B, 0); o.n_seg.assign(B, 0);
        a.n_filled = o.n_filled.data(); a.n_log = o.n_log.data(); a.n_seg = o.n_seg.data();
    }
    if (flavour == 1 || flavour == 4) {
        a.n_eval = (int32_t)te.size(); a.t_eval = te.data();
        o.y_eval.assign(te.size() * N * B, nan); o.eval_idx.assign(te.size() * B, -1);
        a.y_eval = o.y_eval.data(); a.eval_idx = o.eval_idx.data();
    }
    if (flavour == 2 || flavour == 3) {
        a.max_log = max_log;
        o.t_log.assign((size_t)max_log * B, nan); o.y_log.assign((size_t)max_log * N * B, nan);
        a.t_log = o.t_log.data(); a.y_log = o.y_log.data();
    }
    if (flavour == 2) {
        o.seg_cont.assign((size_t)max_log * NC * B, nan); o.seg_xold.assign((size_t)max_log * B, nan); o.seg_h.assign((size_t)max_log * B, nan);
        a.seg_cont = o.seg_cont.data(); a.seg_xold = o.seg_xold.data(); a.seg_h = o.seg_h.data(); a.collect_dense = 1;
    }
    if (flavour == 4) {
        a.def_cap = (uint32_t)te.size();
        o.def_rec.assign((size_t)a.def_cap * (N + 4) * B, nan);
        a.def_rec = o.def_rec.data();
    }
    uint64_t chunks = 0;
    for (uint32_t j = 0; j < B; ++j) {
        int32_t st = init_body<M, R, FULL>(a, j);
        while (st == IVP_RUNNING) { chunk_body<M, R, FULL>(a, j, st); ++chunks; }
    }
    if constexpr (M == M_DOP853 && FULL == 3) {
        for (uint32_t j = 0; j < B; ++j)
            for (uint32_t k = 0; k < a.n_seg[j] && k < a.def_cap; ++k) dop853_sample_body<R>(a, j, k);
    }
    o.dump(f);
    unsigned long long steps = 0;
    for (uint32_t j = 0; j < B; ++j) steps += o.cnt[B + j];
    std::printf("method %d flavour %d chunk %-3u launches %-6llu attempts %-6llu status", M, flavour, chunk, (unsigned long long)chunks, steps);
    for (uint32_t j = 0; j < B; ++j) std::printf(" %d", o.status[j]);
    std::printf("\n");
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s OUTPUT\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    const Batch b = make_batch();
    for (uint32_t chunk : {1u, 64u}) {
        run<M_DOPRI5, 0>(b, 0, chunk, f);
        run<M_DOPRI5, 1>(b, 1, chunk, f);
        run<M_DOPRI5, 1>(b, 2, chunk, f);
        run<M_DOPRI5, 2>(b, 3, chunk, f);
        run<M_DOP853, 0>(b, 0, chunk, f);
        run<M_DOP853, 1>(b, 1, chunk, f);
        run<M_DOP853, 1>(b, 2, chunk, f);
        run<M_DOP853, 2>(b, 3, chunk, f);
        run<M_DOP853, 3>(b, 4, chunk, f);
    }
    std::fclose(f);
#if defined(IVP_INBAND_FORCE_REDO)
    std::printf("every stage block redone\n");
#endif
    return 0;
}
