// ivp_events.cpp -- ivp_batch_solve_events*(): every trajectory's complete Solution.t_events / Solution.y_events
// (src/solve/solution.rs:10-11, Vecs that grow with every occurrence, src/solve/solout.rs:158-331) as a CSR log.
//
// Flow of an events solve (layout and ownership: include/ivp_hip.h), the flow of ivp_dense.cpp:
//   1. the counting solve: ivp_batch_solve_device with a bounded block of opt->max_events slots per event and trajectory
//      (none when max_events == 0) -- it delivers every other output of `out` and counts every occurrence (n_event_hits
//      keeps counting past the block);
//   2. exclusive scan of the counts, viewed as one array of n_events * B runs -> offsets, total (ivp_log_scan);
//   3. destination = the caller's buffers if they hold `total` records, else library-owned;
//   4. the records: packed straight from the counting solve's block when every run fitted it, else a filling solve over
//      trajectory ranges whose bounded blocks fit the free device memory, each block packed into its CSR runs
//      (event_pack_kernel, event_pack.hip).  The pack kernel checks that the filling solve reproduced every count.
// The stepping kernels are the existing ones, unchanged (their event sink writes the bounded block); no arithmetic of the
// integration happens here.  Peak device memory is the result (sum(hits) records of n + 1 doubles) PLUS the staging block
// of the filling solve, [n_events][max hits of the range][n + 1] doubles per trajectory of a range, capped at half of the
// free memory or at IVP_EVENT_STAGING_BYTES, at the price of one filling solve per range -- and the filling solve's own
// scratch: its deferred event refinement (ivp_capi.cpp) notes up to n_events * max_events steps of 4 + 3 n_events + n +
// ncoef n doubles per trajectory when a quarter of the free memory holds them (inline refinement otherwise).  Writing the
// runs directly from the deferred event kernel is the follow-up that removes the block.
#include "ivp_ctx.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

#ifndef IVP_HD
#define IVP_HD inline
#endif
#include "event_kernels.h"
#include "event_pack.h"
#include "log_gather.h"

using namespace ivp_host;

namespace {

// device memory for the duration of one call
struct Tmp {
    void *p = nullptr;
    Tmp() = default;
    Tmp(const Tmp &) = delete;
    Tmp &operator=(const Tmp &) = delete;
    ~Tmp() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    hipError_t get(size_t bytes) { release(); return hipMalloc(&p, std::max<size_t>(bytes, 8)); }
};

int need_free(ivp_ctx *ctx, size_t bytes, const char *what)
{
    size_t fr = 0, tot = 0;
    HIP_TRY(ctx, hipMemGetInfo(&fr, &tot));
    if (bytes > fr)
        return fail(ctx, IVP_ERR_HIP, "event output: %s needs %zu bytes, device %d has %zu free", what, bytes, ctx->device, fr);
    return IVP_OK;
}

// ivp_event_log_t carries no record width: the library remembers it for the device logs it owns (y pointer -> n), from
// the allocation to ivp_event_log_free(), so that ivp_event_log_fetch_device() knows how much to copy
std::mutex g_owned_mu;
std::unordered_map<const void *, size_t> g_owned_n;

// the caller's buffers, or exactly `total` records of device memory owned by the log (released by ivp_event_log_free)
int device_destination(ivp_ctx *ctx, ivp_event_log_t *ev, uint64_t total, size_t n)
{
    if (ev->t || ev->y) {
        if (ev->capacity < total)
            return fail(ctx, IVP_ERR_LOG_CAPACITY, "the event log has %llu records, t / y hold %llu", (unsigned long long)total, (unsigned long long)ev->capacity);
        return IVP_OK;
    }
    const size_t recs = (size_t)std::max<uint64_t>(total, 1);
    int rc = need_free(ctx, recs * (n + 1) * sizeof(double), "the CSR event log");
    if (rc != IVP_OK) return rc;
    void *t = nullptr, *y = nullptr;
    hipError_t e = hipMalloc(&t, recs * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&y, recs * n * sizeof(double));
    if (e != hipSuccess) {
        if (t) (void)hipFree(t);
        return fail(ctx, IVP_ERR_HIP, "hipMalloc of %zu event records: %s", recs, hipGetErrorString(e));
    }
    try {
        std::lock_guard<std::mutex> lock(g_owned_mu);
        g_owned_n[y] = n;
    } catch (const std::bad_alloc &) {
        (void)hipFree(t); (void)hipFree(y);
        return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out of host memory");
    }
    ev->t = (double *)t; ev->y = (double *)y;
    ev->capacity = recs;
    ev->owned = 1;
    ev->device = ctx->device;
    return IVP_OK;
}

// Step 4 with a filling solve: trajectory ranges [first, first + cnt) whose bounded blocks ([n_events][max hits][n + 1]
// doubles per trajectory) fit half of the free memory, each integrated again and packed into its runs.  y0 / params /
// t0 / t1: device arrays of the whole batch (SoA stride B); off: device offsets [n_events * B + 1]; most: the largest
// count of any event per trajectory, on the host.
int fill_pass(ivp_ctx *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params, const double *t0, size_t t0_len,
              const double *t1, size_t t1_len, const ivp_options_t *opt, int n, int np, size_t nev, const std::vector<uint32_t> &most,
              const unsigned long long *off, ivp_event_log_t *ev, uint32_t *err, hipStream_t s)
{
    const size_t rec = nev * (size_t)(n + 1) * sizeof(double);   // one slot of every event of one trajectory
    size_t fr = 0, tot = 0;
    HIP_TRY(ctx, hipMemGetInfo(&fr, &tot));
    size_t budget = fr / 2;   // the rest: the solve's own scratch
    // IVP_EVENT_STAGING_BYTES caps the block: less peak memory for more (and narrower) filling solves
    if (const char *cap = std::getenv("IVP_EVENT_STAGING_BYTES")) {
        const unsigned long long v = std::strtoull(cap, nullptr, 10);
        if (v > 0) budget = std::min<size_t>(budget, (size_t)v);
    }
    ivp_options_t o = *opt;
    o.t_eval = nullptr; o.n_eval = 0; o.t_eval_offsets = nullptr;   // samples do not steer the integration; they came with step 1
    o.max_log = 0;                                                   // neither do the step log and the dense segments
    o.dense_output = 0;
    o.count_log = 0;
    o.profile = 0;   // ctx->stats stay those of the counting solve (the caller restores them)
    Tmp st, in, cnt_buf;
    for (size_t first = 0; first < B;) {
        size_t cnt = 0;
        uint32_t me = 0;
        while (first + cnt < B) {
            const uint32_t m2 = std::max<uint32_t>(me, std::max<uint32_t>(most[first + cnt], 1u));
            if (cnt > 0 && (size_t)m2 * rec * (cnt + 1) > budget) break;
            me = m2;
            ++cnt;
        }
        const size_t bytes = (size_t)me * rec * cnt;
        if (bytes > fr)
            return fail(ctx, IVP_ERR_HIP, "event output: trajectory %zu has %u occurrences of one event (%zu bytes of staging), device %d has %zu bytes free",
                        first, me, bytes, ctx->device, fr);
        ev->staging_bytes = std::max<uint64_t>(ev->staging_bytes, bytes);
        HIP_TRY(ctx, st.get(bytes));
        HIP_TRY(ctx, cnt_buf.get(sizeof(uint32_t) * nev * cnt));
        const double *ys = y0, *ps = params, *t0s = t0, *t1s = t1;
        if (cnt != B) {   // the range's inputs with SoA stride cnt
            HIP_TRY(ctx, in.get(sizeof(double) * cnt * (size_t)(n + std::max(np, 0))));
            double *yb = (double *)in.p, *pb = yb + (size_t)n * cnt;
            HIP_TRY(ctx, hipMemcpy2DAsync(yb, cnt * 8, y0 + first, B * 8, cnt * 8, n, hipMemcpyDeviceToDevice, s));
            if (np > 0) HIP_TRY(ctx, hipMemcpy2DAsync(pb, cnt * 8, params + first, B * 8, cnt * 8, np, hipMemcpyDeviceToDevice, s));
            ys = yb;
            ps = np > 0 ? pb : nullptr;
            if (t0_len != 1) t0s = t0 + first;
            if (t1_len != 1) t1s = t1 + first;
        }
        ivp_batch_result_t r;
        std::memset(&r, 0, sizeof r);
        r.t_events = (double *)st.p;
        r.y_events = r.t_events + nev * (size_t)me * cnt;
        r.n_event_hits = (uint32_t *)cnt_buf.p;
        o.max_events = me;
        int rc = ivp_batch_solve_device(ctx, prob, cnt, ys, ps, t0s, t0_len == 1 ? 1 : cnt, t1s, t1_len == 1 ? 1 : cnt, &o, &r, s);
        if (rc != IVP_OK) return rc;
        EventPackArgs p{r.t_events, r.y_events, r.n_event_hits, off, ev->t, ev->y, err, (unsigned long long)B, (unsigned long long)first,
                        (uint32_t)cnt, me, (uint32_t)n, (uint32_t)nev};
        HIP_TRY(ctx, ivp_event_pack(p, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));   // st / in are reused by the next range
        first += cnt;
    }
    return IVP_OK;
}

int check_err(ivp_ctx *ctx, const uint32_t *err, hipStream_t s)
{
    uint32_t e = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&e, err, sizeof e, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (e) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "event output: the filling solve produced other event counts than the counting solve (were the inputs changed in between?)");
    return IVP_OK;
}

// arguments of both entry points; *nev_out = the problem's number of event functions
int check_args(ivp_ctx *ctx, const ivp_problem_t *prob, size_t B, const ivp_options_t *opt, const ivp_batch_result_t *out, const ivp_event_log_t *ev,
               int *n_out, int *np_out, size_t *nev_out)
{
    if (!opt || !out || !ev || !ev->offsets) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "null options / out / ev / ev->offsets");
    if (out->t_events || out->y_events)
        return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out.t_events / y_events are the bounded layout: leave them NULL, the occurrences go to `ev`");
    if ((ev->t != nullptr) != (ev->y != nullptr)) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "ivp_event_log_t: t and y must both be given or both be NULL");
    int rc = validate(ctx, prob, B, opt, n_out, np_out);
    if (rc != IVP_OK) return rc;
    const size_t nev = result_shape(prob, opt, *n_out).nev;
    if (nev == 0) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "the problem defines no event functions: there is no event log to deliver");
    if (B > 0xFFFFFFFFull / nev) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "n_events * B = %zu * %zu runs (at most 4294967295)", nev, B);
    *nev_out = nev;
    return IVP_OK;
}

void reset_out(ivp_event_log_t *ev, size_t nev)
{
    ev->owned = 0; ev->device = -1; ev->passes = 0; ev->n_events = (uint32_t)nev; ev->total = 0; ev->staging_bytes = 0;
}

// largest count of any event, per trajectory (sizes the filling solve's blocks) and over the batch
uint32_t most_per_trajectory(const std::vector<uint32_t> &hits, size_t nev, size_t B, std::vector<uint32_t> &most)
{
    uint32_t all = 0;
    for (size_t b = 0; b < B; ++b) {
        uint32_t m = 0;
        for (size_t i = 0; i < nev; ++i) m = std::max(m, hits[i * B + b]);
        most[b] = m;
        all = std::max(all, m);
    }
    return all;
}

}  // namespace

extern "C" {

int ivp_batch_solve_events_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                                  const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                                  ivp_batch_result_t *out, ivp_event_log_t *ev, void *hip_stream)
{
    if (!ctx) return IVP_ERR_BAD_ARGUMENT;
    ctx->err.clear();
    int n = 0, np = 0;
    size_t nev = 0;
    int rc = check_args(ctx, prob, B, opt, out, ev, &n, &np, &nev);
    if (rc != IVP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)hip_stream;
    reset_out(ev, nev);
    const size_t runs = nev * B, me1 = opt->max_events;
    // ---- 1. the counting solve ----
    const size_t stage1 = nev * me1 * (size_t)(n + 1) * sizeof(double) * B;
    rc = need_free(ctx, stage1 + sizeof(uint32_t) * runs + sizeof(double) * n * B, "the counting solve's event block");
    if (rc != IVP_OK) return rc;
    Tmp st, cnt_buf, yend, scan, err;
    ivp_batch_result_t r = *out;
    if (me1 > 0) {
        HIP_TRY(ctx, st.get(stage1));
        r.t_events = (double *)st.p;
        r.y_events = r.t_events + nev * me1 * B;
    }
    if (!r.n_event_hits) { HIP_TRY(ctx, cnt_buf.get(sizeof(uint32_t) * runs)); r.n_event_hits = (uint32_t *)cnt_buf.p; }
    const bool alias = out->y_end != nullptr && (const double *)out->y_end == y0;   // the filling solve needs y0 intact
    if (alias) { HIP_TRY(ctx, yend.get(sizeof(double) * n * B)); r.y_end = (double *)yend.p; }
    ev->staging_bytes = stage1;
    rc = ivp_batch_solve_device(ctx, prob, B, y0, params, t0, t0_len, t1, t1_len, opt, &r, hip_stream);
    if (rc != IVP_OK) return rc;
    const ivp_run_stats_t stats = ctx->stats;   // what the caller's options asked for describes the counting solve
    ev->passes = 1;
    // ---- 2. offsets and the counts ----
    HIP_TRY(ctx, scan.get(ivp_log_scan_scratch_bytes(runs)));
    HIP_TRY(ctx, ivp_log_scan(r.n_event_hits, runs, (unsigned long long *)ev->offsets, scan.p, s));
    std::vector<uint32_t> hits, most;
    try { hits.resize(runs); most.resize(B); } catch (const std::bad_alloc &) { return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out of host memory for %zu event counts", runs); }
    unsigned long long total = 0;
    if (runs) HIP_TRY(ctx, hipMemcpyAsync(hits.data(), r.n_event_hits, sizeof(uint32_t) * runs, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&total, ev->offsets + runs, sizeof total, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ev->total = total;
    // ---- 3. destination ----
    rc = device_destination(ctx, ev, total, (size_t)n);
    if (rc != IVP_OK) return rc;
    // ---- 4. the records ----
    HIP_TRY(ctx, err.get(sizeof(uint32_t)));
    HIP_TRY(ctx, hipMemsetAsync(err.p, 0, sizeof(uint32_t), s));
    const uint32_t all = most_per_trajectory(hits, nev, B, most);
    if (total == 0) {
        // nothing to write
    } else if (all <= me1) {   // every run fitted the counting solve's block
        EventPackArgs p{r.t_events, r.y_events, r.n_event_hits, (const unsigned long long *)ev->offsets, ev->t, ev->y, (uint32_t *)err.p,
                        (unsigned long long)B, 0ull, (uint32_t)B, (uint32_t)me1, (uint32_t)n, (uint32_t)nev};
        HIP_TRY(ctx, ivp_event_pack(p, s));
    } else {
        st.release();
        rc = fill_pass(ctx, prob, B, y0, params, t0, t0_len, t1, t1_len, opt, n, np, nev, most, (const unsigned long long *)ev->offsets, ev,
                       (uint32_t *)err.p, s);
        ctx->stats = stats;
        if (rc != IVP_OK) return rc;
        ev->passes = 2;
    }
    if (alias) HIP_TRY(ctx, hipMemcpyAsync(out->y_end, yend.p, sizeof(double) * n * B, hipMemcpyDeviceToDevice, s));
    return check_err(ctx, (const uint32_t *)err.p, s);
}

int ivp_batch_solve_events(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                           const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                           ivp_batch_result_t *out, ivp_event_log_t *ev)
{
    if (!ctx) return IVP_ERR_BAD_ARGUMENT;
    ctx->err.clear();
    int n = 0, np = 0;
    size_t nev = 0;
    int rc = check_args(ctx, prob, B, opt, out, ev, &n, &np, &nev);
    if (rc != IVP_OK) return rc;
    if (!y0 || !t0 || !t1) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "null y0/t0/t1");
    if (np > 0 && !params) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "params required (n_params=%d)", np);
    if ((t0_len != 1 && t0_len != B) || (t1_len != 1 && t1_len != B)) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "t0/t1 length must be 1 or B");
    DeviceGuard restore_device;
    reset_out(ev, nev);
    const size_t runs = nev * B, me1 = opt->max_events, un = (size_t)n;
    // ---- 1. the counting solve through the host entry point (it stages `out` itself) ----
    std::vector<double> hst, y0_keep;
    std::vector<uint32_t> hits, most;
    const bool alias = out->y_end != nullptr && (const double *)out->y_end == y0;   // the filling solve needs y0 intact
    try {
        if (alias) y0_keep.assign(y0, y0 + un * B);
        hst.resize(nev * me1 * (un + 1) * B);
        hits.resize(runs);
        most.resize(B);
    } catch (const std::bad_alloc &) {
        return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out of host memory for the counting solve's event block (%zu slots x %zu runs)", me1, runs);
    }
    ivp_batch_result_t r = *out;
    if (me1 > 0) {
        r.t_events = hst.data();
        r.y_events = r.t_events + nev * me1 * B;
    }
    r.n_event_hits = hits.data();
    ev->staging_bytes = hst.size() * sizeof(double);
    rc = ivp_batch_solve(ctx, prob, B, y0, params, t0, t0_len, t1, t1_len, opt, &r);
    if (rc != IVP_OK) return rc;
    const ivp_run_stats_t stats = ctx->stats;
    if (out->n_event_hits) std::memcpy(out->n_event_hits, hits.data(), sizeof(uint32_t) * runs);
    ev->passes = 1;
    // ---- 2. offsets (host) ----
    uint64_t total = 0;
    ev->offsets[0] = 0;
    for (size_t q = 0; q < runs; ++q) { total += hits[q]; ev->offsets[q + 1] = total; }
    ev->total = total;
    // ---- 3. destination (host) ----
    if (ev->t && ev->capacity < total)
        return fail(ctx, IVP_ERR_LOG_CAPACITY, "the event log has %llu records, t / y hold %llu", (unsigned long long)total, (unsigned long long)ev->capacity);
    if (total == 0) {
        if (!ev->t) ev->capacity = 0;
        return IVP_OK;
    }
    // ---- 4. the records: from the host block when every run fitted it, else a filling solve on the device ----
    const uint32_t all = most_per_trajectory(hits, nev, B, most);
    double *t_out = ev->t, *y_out = ev->y;
    bool mine = false;
    if (!t_out) {
        t_out = (double *)std::malloc(total * sizeof(double));
        y_out = (double *)std::malloc(total * un * sizeof(double));
        mine = true;
        if (!t_out || !y_out) { std::free(t_out); std::free(y_out); return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out of host memory for %llu event records", (unsigned long long)total); }
    }
    auto bail = [&](int code) { if (mine) { std::free(t_out); std::free(y_out); } return code; };
    if (all <= me1) {   // the pack kernel's own arithmetic (event_pack.h), run by run on the host block
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "offsets are 64-bit");
        bool bad = false;
        for (size_t i = 0; i < nev; ++i)
            for (size_t b = 0; b < B; ++b)
                bad |= event_pack_run(r.t_events, r.y_events, hits.data(), (const unsigned long long *)ev->offsets, t_out, y_out, (uint32_t)i, b, 0, B, B,
                                      (uint32_t)me1, (uint32_t)n, 0u, 1u);
        if (bad) return bail(fail(ctx, IVP_ERR_BAD_ARGUMENT, "event output: the counts do not match the offsets"));
    } else {
        hst.clear(); hst.shrink_to_fit();
        if (hipSetDevice(ctx->device) != hipSuccess) return bail(fail(ctx, IVP_ERR_HIP, "hipSetDevice(%d)", ctx->device));
        const size_t l0 = t0_len == 1 ? 1 : B, l1 = t1_len == 1 ? 1 : B;
        Tmp in, off, td, yd2, err;
        if (in.get(sizeof(double) * (un * B + (size_t)std::max(np, 0) * B + l0 + l1)) != hipSuccess || off.get(sizeof(uint64_t) * (runs + 1)) != hipSuccess ||
            td.get(total * sizeof(double)) != hipSuccess || yd2.get(total * un * sizeof(double)) != hipSuccess || err.get(sizeof(uint32_t)) != hipSuccess)
            return bail(fail(ctx, IVP_ERR_HIP, "event output: device memory for %llu records and the inputs", (unsigned long long)total));
        double *yd = (double *)in.p, *pd = yd + un * B, *t0d = pd + (size_t)std::max(np, 0) * B, *t1d = t0d + l0;
        hipStream_t s = nullptr;
        if (hipMemcpyAsync(yd, alias ? y0_keep.data() : y0, sizeof(double) * un * B, hipMemcpyHostToDevice, s) != hipSuccess ||
            (np > 0 && hipMemcpyAsync(pd, params, sizeof(double) * np * B, hipMemcpyHostToDevice, s) != hipSuccess) ||
            hipMemcpyAsync(t0d, t0, sizeof(double) * l0, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(t1d, t1, sizeof(double) * l1, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(off.p, ev->offsets, sizeof(uint64_t) * (runs + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemsetAsync(err.p, 0, sizeof(uint32_t), s) != hipSuccess)
            return bail(fail(ctx, IVP_ERR_HIP, "event output: staging the inputs"));
        ivp_event_log_t dd = *ev;
        dd.t = (double *)td.p; dd.y = (double *)yd2.p;
        rc = fill_pass(ctx, prob, B, yd, np > 0 ? pd : nullptr, t0d, l0, t1d, l1, opt, n, np, nev, most, (const unsigned long long *)off.p, &dd, (uint32_t *)err.p, s);
        ctx->stats = stats;
        if (rc == IVP_OK) rc = check_err(ctx, (const uint32_t *)err.p, s);
        if (rc != IVP_OK) return bail(rc);
        ev->staging_bytes = std::max<uint64_t>(ev->staging_bytes, dd.staging_bytes);
        if (hipMemcpy(t_out, td.p, total * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(y_out, yd2.p, total * un * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            return bail(fail(ctx, IVP_ERR_HIP, "event output: copying the records to the host"));
        ev->passes = 2;
    }
    if (mine) {
        ev->t = t_out; ev->y = y_out;
        ev->capacity = total;
        ev->owned = 1;
        ev->device = -1;
    }
    return IVP_OK;
}

int ivp_event_log_fetch_device(ivp_event_log_t *ev, double *t, double *y, void *hip_stream)
{
    if (!ev || !ev->owned || ev->device < 0 || !t || !y) return IVP_ERR_BAD_ARGUMENT;
    DeviceGuard restore;
    if (hipSetDevice(ev->device) != hipSuccess) return IVP_ERR_HIP;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t total = (size_t)ev->total;
    size_t n = 0;
    {
        std::lock_guard<std::mutex> lock(g_owned_mu);
        const auto it = g_owned_n.find(ev->y);
        if (it == g_owned_n.end()) return IVP_ERR_BAD_ARGUMENT;   // not a log this library allocated (or already freed)
        n = it->second;
    }
    if (total) {
        if (hipMemcpyAsync(t, ev->t, total * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync(y, ev->y, total * n * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return IVP_ERR_HIP;
    }
    ivp_event_log_free(ev);
    ev->t = t; ev->y = y;
    ev->capacity = total;
    return IVP_OK;
}

void ivp_event_log_free(ivp_event_log_t *ev)
{
    if (!ev || !ev->owned) return;
    if (ev->device >= 0) {
        DeviceGuard restore;
        (void)hipSetDevice(ev->device);
        {
            std::lock_guard<std::mutex> lock(g_owned_mu);
            g_owned_n.erase(ev->y);
        }
        if (ev->t) (void)hipFree(ev->t);
        if (ev->y) (void)hipFree(ev->y);
    } else {
        std::free(ev->t);
        std::free(ev->y);
    }
    ev->t = nullptr; ev->y = nullptr; ev->capacity = 0; ev->owned = 0; ev->device = -1;
}

}  // extern "C"
