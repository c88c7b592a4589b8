// ivp_csr.cpp -- the staging driver of the counted CSR logs (flow and the description of a kind: ivp_csr.h).
// The stepping kernels are the existing ones, unchanged (their sinks write the bounded block); no arithmetic of the
// integration happens here.  Peak device memory is the result PLUS the staging block of the filling solve, capped at half
// of the free memory or at the kind's environment variable, at the price of one filling solve per range.  A sink in the
// stepping kernels that writes the CSR runs directly is the follow-up that removes the block -- for both kinds at once.
#include "ivp_csr.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "ivp_csr_plan.h"
#include "log_gather.h"

namespace ivp_host {

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

int need_free(ivp_ctx *ctx, const CsrKind &k, size_t bytes, const char *what)
{
    size_t fr = 0, tot = 0;
    HIP_TRY(ctx, hipMemGetInfo(&fr, &tot));
    if (bytes > fr) return fail(ctx, IVP_ERR_HIP, "%s: %s needs %zu bytes, device %d has %zu free", k.name, what, bytes, ctx->device, fr);
    return IVP_OK;
}

// what a staging block may take: half of the free memory (the rest: the solve's own scratch), less if the kind's
// environment variable says so -- less peak memory for more (and narrower) filling solves
int staging_budget(ivp_ctx *ctx, const CsrKind &k, size_t *free_bytes, size_t *budget)
{
    size_t tot = 0;
    HIP_TRY(ctx, hipMemGetInfo(free_bytes, &tot));
    *budget = *free_bytes / 2;
    if (const char *cap = std::getenv(k.staging_env)) {
        const unsigned long long v = std::strtoull(cap, nullptr, 10);
        if (v > 0) *budget = std::min<size_t>(*budget, (size_t)v);
    }
    return IVP_OK;
}

// trajectories [first, first + cnt) of a batch on device pointers: y0 / params with SoA stride cnt (in `buf`), t0 / t1
// offset when they are per trajectory
int slice_inputs(ivp_ctx *ctx, const CsrInputs &all, size_t first, size_t cnt, Tmp &buf, CsrInputs *part, hipStream_t s)
{
    *part = all;
    part->B = cnt;
    part->t0_len = all.t0_len == 1 ? 1 : cnt;
    part->t1_len = all.t1_len == 1 ? 1 : cnt;
    if (cnt == all.B) return IVP_OK;
    const size_t n = (size_t)all.n, np = (size_t)std::max(all.np, 0);
    HIP_TRY(ctx, buf.get(sizeof(double) * cnt * (n + np)));
    double *yb = (double *)buf.p, *pb = yb + n * cnt;
    HIP_TRY(ctx, hipMemcpy2DAsync(yb, cnt * 8, all.y0 + first, all.B * 8, cnt * 8, n, hipMemcpyDeviceToDevice, s));
    if (np > 0) HIP_TRY(ctx, hipMemcpy2DAsync(pb, cnt * 8, all.params + first, all.B * 8, cnt * 8, np, hipMemcpyDeviceToDevice, s));
    part->y0 = yb;
    part->params = np > 0 ? pb : nullptr;
    if (all.t0_len != 1) part->t0 = all.t0 + first;
    if (all.t1_len != 1) part->t1 = all.t1 + first;
    return IVP_OK;
}

// Step 4 with a filling solve: trajectory ranges whose bounded blocks fit the budget, each integrated again and packed into
// its runs.  in: device arrays of the whole batch (SoA stride B); off: device offsets; need: the slots every trajectory
// fills, on the host; *staging_bytes grows to the largest block.
int fill_pass(ivp_ctx *ctx, const CsrKind &k, const CsrInputs &in, const std::vector<uint32_t> &need, const unsigned long long *off,
              const CsrArrays &dst, uint32_t *err, uint64_t *staging_bytes, hipStream_t s)
{
    size_t fr = 0, budget = 0;
    int rc = staging_budget(ctx, k, &fr, &budget);
    if (rc != IVP_OK) return rc;
    ivp_options_t o = k.fill_opt;
    Tmp st, sliced, cnt_buf;
    for (size_t first = 0; first < in.B;) {
        const IvpCsrRange g = ivp_csr_plan_range(need.data(), first, in.B, k.rec, budget);
        const size_t bytes = (size_t)g.cap * k.rec * g.cnt;
        if (bytes > fr)
            return fail(ctx, IVP_ERR_HIP, "%s: trajectory %zu fills %u slots (%zu bytes of staging), device %d has %zu bytes free", k.name, first,
                        g.cap, bytes, ctx->device, fr);
        *staging_bytes = std::max<uint64_t>(*staging_bytes, bytes);
        HIP_TRY(ctx, st.get(bytes));
        HIP_TRY(ctx, cnt_buf.get(sizeof(uint32_t) * k.runs_per_traj * g.cnt));
        CsrInputs part;
        rc = slice_inputs(ctx, in, first, g.cnt, sliced, &part, s);
        if (rc != IVP_OK) return rc;
        ivp_batch_result_t r;
        std::memset(&r, 0, sizeof r);
        k.bind(r, (double *)st.p, g.cap, g.cnt);
        r.*k.counts = (uint32_t *)cnt_buf.p;
        o.*k.depth = g.cap;
        rc = solve_device(ctx, part.prob, part.B, part.y0, part.params, part.t0, part.t0_len, part.t1, part.t1_len, &o, &r, s, k.rad);
        if (rc != IVP_OK) return rc;
        HIP_TRY(ctx, k.pack(r, off, dst, err, first, g.cnt, g.cap, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));   // st / sliced are reused by the next range
        first += g.cnt;
    }
    return IVP_OK;
}

// the word the pack kernels set when a run's count is not what the offsets were scanned from
int check_counts(ivp_ctx *ctx, const CsrKind &k, const uint32_t *err, hipStream_t s)
{
    uint32_t e = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&e, err, sizeof e, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (e) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "%s: the filling solve produced other counts than the counting solve (were the inputs changed in between?)", k.name);
    return IVP_OK;
}

int check_capacity(ivp_ctx *ctx, const CsrKind &k, uint64_t total)
{
    if (k.given.p[0] && *k.capacity < total)
        return fail(ctx, IVP_ERR_LOG_CAPACITY, "%s: the log has %llu records, the caller's buffers hold %llu", k.name, (unsigned long long)total,
                    (unsigned long long)*k.capacity);
    return IVP_OK;
}

// need[b] = the largest run of trajectory b; returns the largest of the batch
uint32_t needs_of(const CsrKind &k, const std::vector<uint32_t> &counts, size_t B, std::vector<uint32_t> &need)
{
    uint32_t most = 0;
    for (size_t b = 0; b < B; ++b) {
        uint32_t m = 0;
        for (size_t i = 0; i < k.runs_per_traj; ++i) m = std::max(m, counts[i * B + b]);
        need[b] = m;
        most = std::max(most, m);
    }
    return most;
}

// exactly `total` records (one at least) of device memory, owned by the log from here on
int owned_destination(ivp_ctx *ctx, const CsrKind &k, uint64_t total, CsrArrays *dst)
{
    const size_t recs = (size_t)std::max<uint64_t>(total, 1);
    size_t per = 0;
    for (int i = 0; i < k.narrays; ++i) per += k.width[i];
    int rc = need_free(ctx, k, recs * per * sizeof(double), "the CSR log");
    if (rc != IVP_OK) return rc;
    CsrArrays a;
    auto drop = [&] { for (int i = 0; i < k.narrays; ++i) if (a.p[i]) (void)hipFree(a.p[i]); };
    for (int i = 0; i < k.narrays; ++i) {
        const hipError_t e = hipMalloc((void **)&a.p[i], recs * k.width[i] * sizeof(double));
        if (e != hipSuccess) { drop(); return fail(ctx, IVP_ERR_HIP, "%s: hipMalloc of %zu records: %s", k.name, recs, hipGetErrorString(e)); }
    }
    rc = k.adopt(a, recs, ctx->device);
    if (rc != IVP_OK) { drop(); return rc; }
    *dst = a;
    return IVP_OK;
}

// the host form's destination: the caller's arrays, or malloc'ed ones that are released unless the log adopts them
struct HostArrays {
    CsrArrays a;
    bool mine = false;
    ~HostArrays() { if (mine) for (double *q : a.p) std::free(q); }
};

}  // namespace

int check_host_inputs(ivp_ctx *ctx, const CsrInputs &in)
{
    if (!in.y0 || !in.t0 || !in.t1) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "null y0/t0/t1");
    if (in.np > 0 && !in.params) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "params required (n_params=%d)", in.np);
    if ((in.t0_len != 1 && in.t0_len != in.B) || (in.t1_len != 1 && in.t1_len != in.B)) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "t0/t1 length must be 1 or B");
    return IVP_OK;
}

int csr_solve_device(ivp_ctx *ctx, const CsrKind &k, const CsrInputs &in, ivp_batch_result_t *out, hipStream_t s)
{
    const size_t B = in.B, runs = k.runs_per_traj * B, ybytes = sizeof(double) * (size_t)in.n * B;
    const uint32_t depth = k.count_opt.*k.depth;
    // ---- 1. the counting solve ----
    const size_t stage1 = (size_t)depth * k.rec * B;
    int rc = need_free(ctx, k, stage1 + sizeof(uint32_t) * runs + ybytes, "the counting solve's block");
    if (rc != IVP_OK) return rc;
    Tmp st, cnt_buf, yend, scan, err;
    ivp_batch_result_t r = *out;
    if (depth > 0) {
        HIP_TRY(ctx, st.get(stage1));
        k.bind(r, (double *)st.p, depth, B);
    }
    if (!(r.*k.counts)) { HIP_TRY(ctx, cnt_buf.get(sizeof(uint32_t) * runs)); r.*k.counts = (uint32_t *)cnt_buf.p; }
    const bool alias = out->y_end != nullptr && (const double *)out->y_end == in.y0;   // the filling solve needs y0 intact
    if (alias) { HIP_TRY(ctx, yend.get(ybytes)); r.y_end = (double *)yend.p; }
    *k.staging_bytes = stage1;
    rc = solve_device(ctx, in.prob, B, in.y0, in.params, in.t0, in.t0_len, in.t1, in.t1_len, &k.count_opt, &r, s, k.rad);
    if (rc != IVP_OK) return rc;
    const ivp_run_stats_t stats = ctx->stats;   // what the caller's options asked for describes the counting solve
    *k.passes = 1;
    // ---- 2. offsets and the counts ----
    unsigned long long *off = (unsigned long long *)k.offsets;
    HIP_TRY(ctx, scan.get(ivp_log_scan_scratch_bytes(runs)));
    HIP_TRY(ctx, ivp_log_scan(r.*k.counts, runs, off, scan.p, s));
    std::vector<uint32_t> counts, need;
    try { counts.resize(runs); need.resize(B); } catch (const std::bad_alloc &) { return fail(ctx, IVP_ERR_BAD_ARGUMENT, "%s: out of host memory for %zu counts", k.name, runs); }
    unsigned long long total = 0;
    if (runs) HIP_TRY(ctx, hipMemcpyAsync(counts.data(), r.*k.counts, sizeof(uint32_t) * runs, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&total, off + runs, sizeof total, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    *k.total = total;
    // ---- 3. destination ----
    CsrArrays dst = k.given;
    rc = dst.p[0] ? check_capacity(ctx, k, total) : owned_destination(ctx, k, total, &dst);
    if (rc != IVP_OK) return rc;
    // ---- 4. the records ----
    HIP_TRY(ctx, err.get(sizeof(uint32_t)));
    HIP_TRY(ctx, hipMemsetAsync(err.p, 0, sizeof(uint32_t), s));
    const uint32_t most = needs_of(k, counts, B, need);
    if (total == 0) {
        // nothing to write
    } else if (most <= depth) {   // every run fitted the counting solve's block
        HIP_TRY(ctx, k.pack(r, off, dst, (uint32_t *)err.p, 0, B, depth, s));
    } else {
        st.release();
        rc = fill_pass(ctx, k, in, need, off, dst, (uint32_t *)err.p, k.staging_bytes, s);
        ctx->stats = stats;
        if (rc != IVP_OK) return rc;
        *k.passes = 2;
    }
    if (alias) HIP_TRY(ctx, hipMemcpyAsync(out->y_end, yend.p, ybytes, hipMemcpyDeviceToDevice, s));
    return check_counts(ctx, k, (const uint32_t *)err.p, s);
}

int csr_solve_host(ivp_ctx *ctx, const CsrKind &k, const CsrInputs &in, ivp_batch_result_t *out)
{
    const size_t B = in.B, runs = k.runs_per_traj * B, n = (size_t)in.n, np = (size_t)std::max(in.np, 0);
    const uint32_t depth = k.count_opt.*k.depth;
    // ---- 1. the counting solve through the host entry point (it stages `out` itself) ----
    std::vector<double> block, y0_keep;
    std::vector<uint32_t> counts, need;
    const bool alias = out->y_end != nullptr && (const double *)out->y_end == in.y0;   // it writes y_end over y0: the filling solve needs y0 intact
    try {
        if (alias) y0_keep.assign(in.y0, in.y0 + n * B);
        block.resize((size_t)depth * (k.rec / sizeof(double)) * B);
        counts.resize(runs);
        need.resize(B);
    } catch (const std::bad_alloc &) {
        return fail(ctx, IVP_ERR_BAD_ARGUMENT, "%s: out of host memory for the counting solve's block (%u slots x %zu runs)", k.name, depth, runs);
    }
    ivp_batch_result_t r = *out;
    if (depth > 0) k.bind(r, block.data(), depth, B);
    r.*k.counts = counts.data();
    *k.staging_bytes = block.size() * sizeof(double);
    int rc = solve_host(ctx, in.prob, B, in.y0, in.params, in.t0, in.t0_len, in.t1, in.t1_len, &k.count_opt, &r, k.rad);
    if (rc != IVP_OK) return rc;
    const ivp_run_stats_t stats = ctx->stats;
    if (out->*k.counts) std::memcpy(out->*k.counts, counts.data(), sizeof(uint32_t) * runs);
    *k.passes = 1;
    // ---- 2. offsets (host) ----
    uint64_t total = 0;
    k.offsets[0] = 0;
    for (size_t q = 0; q < runs; ++q) { total += counts[q]; k.offsets[q + 1] = total; }
    *k.total = total;
    // ---- 3. destination (host) ----
    rc = check_capacity(ctx, k, total);
    if (rc != IVP_OK) return rc;
    if (total == 0) {
        if (!k.given.p[0]) *k.capacity = 0;
        return IVP_OK;
    }
    HostArrays dst;
    dst.a = k.given;
    if (!dst.a.p[0]) {
        dst.mine = true;
        for (int i = 0; i < k.narrays; ++i)
            if (!(dst.a.p[i] = (double *)std::malloc(total * k.width[i] * sizeof(double))))
                return fail(ctx, IVP_ERR_BAD_ARGUMENT, "%s: out of host memory for %llu records", k.name, (unsigned long long)total);
    }
    // ---- 4. the records: from the host block when every run fitted it, else a filling solve on the device ----
    if (needs_of(k, counts, B, need) <= depth) {
        if (!k.pack_host(r, counts.data(), dst.a)) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "%s: the counts do not match the offsets", k.name);
    } else {
        block.clear(); block.shrink_to_fit();
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t l0 = in.t0_len == 1 ? 1 : B, l1 = in.t1_len == 1 ? 1 : B;
        Tmp staged, off, err, dev[kCsrArrays];
        hipError_t e = staged.get(sizeof(double) * ((n + np) * B + l0 + l1));
        if (e == hipSuccess) e = off.get(sizeof(uint64_t) * (runs + 1));
        if (e == hipSuccess) e = err.get(sizeof(uint32_t));
        CsrArrays ddst;
        for (int i = 0; i < k.narrays && e == hipSuccess; ++i) {
            e = dev[i].get(total * k.width[i] * sizeof(double));
            ddst.p[i] = (double *)dev[i].p;
        }
        if (e != hipSuccess) return fail(ctx, IVP_ERR_HIP, "%s: device memory for %llu records and the inputs", k.name, (unsigned long long)total);
        CsrInputs din = in;
        double *yd = (double *)staged.p, *pd = yd + n * B, *t0d = pd + np * B, *t1d = t0d + l0;
        din.y0 = yd; din.params = np > 0 ? pd : nullptr; din.t0 = t0d; din.t0_len = l0; din.t1 = t1d; din.t1_len = l1;
        hipStream_t s = nullptr;
        e = hipMemcpyAsync(yd, alias ? y0_keep.data() : in.y0, sizeof(double) * n * B, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && np > 0) e = hipMemcpyAsync(pd, in.params, sizeof(double) * np * B, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(t0d, in.t0, sizeof(double) * l0, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(t1d, in.t1, sizeof(double) * l1, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(off.p, k.offsets, sizeof(uint64_t) * (runs + 1), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemsetAsync(err.p, 0, sizeof(uint32_t), s);
        if (e != hipSuccess) return fail(ctx, IVP_ERR_HIP, "%s: staging the inputs", k.name);
        uint64_t filled = 0;
        rc = fill_pass(ctx, k, din, need, (const unsigned long long *)off.p, ddst, (uint32_t *)err.p, &filled, s);
        ctx->stats = stats;
        if (rc == IVP_OK) rc = check_counts(ctx, k, (const uint32_t *)err.p, s);
        if (rc != IVP_OK) return rc;
        *k.staging_bytes = std::max<uint64_t>(*k.staging_bytes, filled);
        for (int i = 0; i < k.narrays; ++i)
            if (hipMemcpy(dst.a.p[i], dev[i].p, total * k.width[i] * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(ctx, IVP_ERR_HIP, "%s: copying the records to the host", k.name);
        *k.passes = 2;
    }
    if (dst.mine) {
        rc = k.adopt(dst.a, total, -1);
        if (rc != IVP_OK) return rc;
        dst.mine = false;
    }
    return IVP_OK;
}

}  // namespace ivp_host
