// ivp_dense.cpp -- ivp_batch_solve_dense*(): every trajectory's complete ContinuousOutput (src/solve/cont.rs:9-153) as a
// CSR log, and ivp_dense_eval_device(): that continuous solution at query times on the device.
//
// Flow of a dense solve (layout and ownership: include/ivp_hip.h):
//   1. the counting solve: ivp_batch_solve_device with dense_output on and a bounded segment block of max(max_log, 1)
//      records -- it delivers every other output of `out` and counts every trajectory's segments (n_seg keeps counting
//      past the block, the constant segment of a zero-length interval included);
//   2. exclusive scan of the counts -> offsets, total (ivp_log_scan, log_gather.hip);
//   3. destination = the caller's buffers if they hold `total` records, else library-owned;
//   4. the segments: packed straight from the counting solve's block when every run fitted it, else a filling solve over
//      trajectory ranges whose bounded blocks fit the free device memory, each block packed into its CSR runs
//      (dense_pack_kernel, dense_eval.hip).  The pack kernel checks that the filling solve reproduced every count.
// The stepping kernels are the existing ones, unchanged (their dense sink writes the bounded block); no arithmetic of the
// integration happens here.  Peak device memory is therefore the result (sum(n_seg) records) PLUS the staging block of
// the filling solve, [max n_seg][ncoef n + 2] doubles per trajectory of a range (BASELINE C2: profiles/r05_dense_c2_*.json),
// capped at half of the free memory or at IVP_DENSE_STAGING_BYTES, at the price of one filling solve per range.  A sink
// in the stepping kernels that writes the CSR runs directly is the follow-up that removes the block.
#include "ivp_ctx.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "dense_kernels.h"
#include "log_gather.h"

using namespace ivp_host;

namespace {

int ncoef_of(int method) { return method == IVP_DOPRI5 ? 5 : method == IVP_DOP853 ? 8 : method == IVP_BDF ? 7 : 4; }

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
        return fail(ctx, IVP_ERR_HIP, "dense output: %s needs %zu bytes, device %d has %zu free", what, bytes, ctx->device, fr);
    return IVP_OK;
}

// the caller's buffers, or exactly `total` records of device memory owned by the log (released by ivp_dense_log_free)
int device_destination(ivp_ctx *ctx, ivp_dense_log_t *d, uint64_t total, size_t nc)
{
    const bool any = d->cont || d->xold || d->h;
    if (any) {
        if (!(d->cont && d->xold && d->h)) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "ivp_dense_log_t: cont, xold and h must all be given or all be NULL");
        if (d->capacity < total)
            return fail(ctx, IVP_ERR_LOG_CAPACITY, "the dense log has %llu segments, cont / xold / h hold %llu", (unsigned long long)total, (unsigned long long)d->capacity);
        return IVP_OK;
    }
    const size_t recs = (size_t)std::max<uint64_t>(total, 1);
    int rc = need_free(ctx, recs * (nc + 2) * sizeof(double), "the CSR segment log");
    if (rc != IVP_OK) return rc;
    void *c = nullptr, *x = nullptr, *h = nullptr;
    hipError_t e = hipMalloc(&c, recs * nc * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&x, recs * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&h, recs * sizeof(double));
    if (e != hipSuccess) {
        if (c) (void)hipFree(c);
        if (x) (void)hipFree(x);
        return fail(ctx, IVP_ERR_HIP, "hipMalloc of %zu dense segments: %s", recs, hipGetErrorString(e));
    }
    d->cont = (double *)c; d->xold = (double *)x; d->h = (double *)h;
    d->capacity = recs;
    d->owned = 1;
    d->device = ctx->device;
    return IVP_OK;
}

// Step 4 with a filling solve: trajectory ranges [first, first + cnt) whose bounded blocks ([max n_seg][nc + 2] doubles
// per trajectory) fit half of the free memory, each integrated again and packed into its runs.  y0 / params / t0 / t1:
// device arrays of the whole batch (SoA stride B); off: device offsets [B + 1]; ns: the counts on the host.
int fill_pass(ivp_ctx *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params, const double *t0, size_t t0_len,
              const double *t1, size_t t1_len, const ivp_options_t *opt, int n, int np, size_t nc, const std::vector<uint32_t> &ns,
              const unsigned long long *off, ivp_dense_log_t *d, uint32_t *err, hipStream_t s, RadauCall *rad = nullptr)
{
    const size_t rec = (nc + 2) * sizeof(double);
    size_t fr = 0, tot = 0;
    HIP_TRY(ctx, hipMemGetInfo(&fr, &tot));
    size_t budget = fr / 2;   // the rest: the solve's own scratch
    // IVP_DENSE_STAGING_BYTES caps the block: less peak memory for more (and narrower) filling solves
    if (const char *cap = std::getenv("IVP_DENSE_STAGING_BYTES")) {
        const unsigned long long v = std::strtoull(cap, nullptr, 10);
        if (v > 0) budget = std::min<size_t>(budget, (size_t)v);
    }
    ivp_options_t o = *opt;
    o.dense_output = 1;
    o.t_eval = nullptr; o.n_eval = 0; o.t_eval_offsets = nullptr;   // samples do not steer the integration; they came with step 1
    o.count_log = 0;
    o.max_events = 0;                                                // event occurrences are detected (terminal ones stop), not stored
    o.profile = 0;   // ctx->stats stay those of the counting solve (the caller restores them)
    Tmp st, in, cnt_buf;
    for (size_t first = 0; first < B;) {
        size_t cnt = 0;
        uint32_t ml = 0;
        while (first + cnt < B) {
            const uint32_t m2 = std::max<uint32_t>(ml, std::max<uint32_t>(ns[first + cnt], 1u));
            if (cnt > 0 && (size_t)m2 * rec * (cnt + 1) > budget) break;
            ml = m2;
            ++cnt;
        }
        const size_t bytes = (size_t)ml * rec * cnt;
        if (bytes > fr)
            return fail(ctx, IVP_ERR_HIP, "dense output: trajectory %zu has %u segments (%zu bytes of staging), device %d has %zu bytes free",
                        first, ml, bytes, ctx->device, fr);
        d->staging_bytes = std::max<uint64_t>(d->staging_bytes, bytes);
        HIP_TRY(ctx, st.get(bytes));
        HIP_TRY(ctx, cnt_buf.get(sizeof(uint32_t) * cnt));
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
        r.seg_cont = (double *)st.p;
        r.seg_xold = r.seg_cont + (size_t)ml * nc * cnt;
        r.seg_h = r.seg_xold + (size_t)ml * cnt;
        r.n_seg = (uint32_t *)cnt_buf.p;
        o.max_log = ml;
        int rc = solve_device(ctx, prob, cnt, ys, ps, t0s, t0_len == 1 ? 1 : cnt, t1s, t1_len == 1 ? 1 : cnt, &o, &r, s, rad);
        if (rc != IVP_OK) return rc;
        DensePackArgs p{r.seg_cont, r.seg_xold, r.seg_h, r.n_seg, off + first, d->cont, d->xold, d->h, err, (uint32_t)cnt, ml, (uint32_t)nc};
        HIP_TRY(ctx, ivp_dense_pack(p, s));
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
    if (e) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "dense output: the filling solve produced other segment counts than the counting solve (were the inputs changed in between?)");
    return IVP_OK;
}

int check_args(ivp_ctx *ctx, const ivp_options_t *opt, const ivp_batch_result_t *out, const ivp_dense_log_t *d)
{
    if (!opt || !out || !d || !d->offsets) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "null options / out / dense / dense->offsets");
    if (out->seg_cont || out->seg_xold || out->seg_h)
        return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out.seg_cont / seg_xold / seg_h are the bounded layout: leave them NULL, the segments go to `dense`");
    if ((d->cont || d->xold || d->h) && !(d->cont && d->xold && d->h))
        return fail(ctx, IVP_ERR_BAD_ARGUMENT, "ivp_dense_log_t: cont, xold and h must all be given or all be NULL");
    return IVP_OK;
}

// the dense solve on device pointers; rad: the direct Radau call (ivp_radau_solve_dense_device: opt->method is ignored, the
// segments are Radau's), NULL otherwise -- it is handed to the counting solve and to every filling solve
int dense_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                 const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                 ivp_batch_result_t *out, ivp_dense_log_t *dense, void *hip_stream, RadauCall *rad)
{
    if (!ctx) return IVP_ERR_BAD_ARGUMENT;
    ctx->err.clear();
    int rc = check_args(ctx, opt, out, dense);
    if (rc != IVP_OK) return rc;
    int n = 0, np = 0;
    ivp_options_t radau_opt;
    if (rad) {   // as submit_impl reads them
        radau_opt = *opt;
        radau_opt.method = IVP_RADAU;
        radau_opt.has_settings = 0;
        opt = &radau_opt;
    }
    rc = rad ? radau_validate(ctx, prob, B, opt, rad, &n, &np) : validate(ctx, prob, B, opt, &n, &np);
    if (rc != IVP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)hip_stream;
    dense->owned = 0; dense->device = -1; dense->passes = 0; dense->total = 0; dense->staging_bytes = 0;
    const size_t nc = (size_t)ncoef_of(opt->method) * (size_t)n, rec = (nc + 2) * sizeof(double);
    dense->ncoef_n = (uint32_t)nc;
    // ---- 1. the counting solve ----
    ivp_options_t o = *opt;
    o.dense_output = 1;
    o.max_log = std::max<uint32_t>(opt->max_log, 1u);
    const size_t stage1 = (size_t)o.max_log * rec * B;
    rc = need_free(ctx, stage1 + sizeof(uint32_t) * B + sizeof(double) * n * B, "the counting solve's segment block");
    if (rc != IVP_OK) return rc;
    Tmp st, cnt_buf, yend, scan, err;
    HIP_TRY(ctx, st.get(stage1));
    ivp_batch_result_t r = *out;
    if (opt->max_log == 0 && !out->log_offsets) { r.t_log = nullptr; r.y_log = nullptr; }   // the one record of the block is for segments only
    r.seg_cont = (double *)st.p;
    r.seg_xold = r.seg_cont + (size_t)o.max_log * nc * B;
    r.seg_h = r.seg_xold + (size_t)o.max_log * B;
    if (!r.n_seg) { HIP_TRY(ctx, cnt_buf.get(sizeof(uint32_t) * B)); r.n_seg = (uint32_t *)cnt_buf.p; }
    const bool alias = out->y_end != nullptr && (const double *)out->y_end == y0;   // the filling solve needs y0 intact
    if (alias) { HIP_TRY(ctx, yend.get(sizeof(double) * n * B)); r.y_end = (double *)yend.p; }
    dense->staging_bytes = stage1;
    rc = solve_device(ctx, prob, B, y0, params, t0, t0_len, t1, t1_len, &o, &r, hip_stream, rad);
    if (rc != IVP_OK) return rc;
    const ivp_run_stats_t stats = ctx->stats;   // what the caller's options asked for describes the counting solve
    dense->passes = 1;
    // ---- 2. offsets and the counts ----
    HIP_TRY(ctx, scan.get(ivp_log_scan_scratch_bytes(B)));
    HIP_TRY(ctx, ivp_log_scan(r.n_seg, B, (unsigned long long *)dense->offsets, scan.p, s));
    std::vector<uint32_t> ns;
    try { ns.resize(B); } catch (const std::bad_alloc &) { return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out of host memory for %zu segment counts", B); }
    unsigned long long total = 0;
    if (B) HIP_TRY(ctx, hipMemcpyAsync(ns.data(), r.n_seg, sizeof(uint32_t) * B, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&total, dense->offsets + B, sizeof total, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    dense->total = total;
    // ---- 3. destination ----
    rc = device_destination(ctx, dense, total, nc);
    if (rc != IVP_OK) return rc;
    // ---- 4. the segments ----
    HIP_TRY(ctx, err.get(sizeof(uint32_t)));
    HIP_TRY(ctx, hipMemsetAsync(err.p, 0, sizeof(uint32_t), s));
    const uint32_t most = B ? *std::max_element(ns.begin(), ns.end()) : 0u;
    if (total == 0) {
        // nothing to write
    } else if (most <= o.max_log) {   // every run fitted the counting solve's block
        DensePackArgs p{r.seg_cont, r.seg_xold, r.seg_h, r.n_seg, (const unsigned long long *)dense->offsets, dense->cont, dense->xold, dense->h,
                        (uint32_t *)err.p, (uint32_t)B, o.max_log, (uint32_t)nc};
        HIP_TRY(ctx, ivp_dense_pack(p, s));
    } else {
        st.release();
        rc = fill_pass(ctx, prob, B, y0, params, t0, t0_len, t1, t1_len, opt, n, np, nc, ns, (const unsigned long long *)dense->offsets, dense,
                       (uint32_t *)err.p, s, rad);
        ctx->stats = stats;
        if (rc != IVP_OK) return rc;
        dense->passes = 2;
    }
    if (alias) HIP_TRY(ctx, hipMemcpyAsync(out->y_end, yend.p, sizeof(double) * n * B, hipMemcpyDeviceToDevice, s));
    return check_err(ctx, (const uint32_t *)err.p, s);
}

}  // namespace

extern "C" {

int ivp_batch_solve_dense_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                                 const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                                 ivp_batch_result_t *out, ivp_dense_log_t *dense, void *hip_stream)
{
    return dense_device(ctx, prob, B, y0, params, t0, t0_len, t1, t1_len, opt, out, dense, hip_stream, nullptr);
}

int ivp_radau_solve_dense_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                                 const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                                 const ivp_radau_settings_t *settings, const ivp_radau_dae_t *dae, ivp_batch_result_t *out,
                                 ivp_dense_log_t *dense, void *hip_stream)
{
    RadauCall call = radau_call(settings, dae);
    return dense_device(ctx, prob, B, y0, params, t0, t0_len, t1, t1_len, opt, out, dense, hip_stream, &call);
}

int ivp_batch_solve_dense(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                          const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                          ivp_batch_result_t *out, ivp_dense_log_t *dense)
{
    if (!ctx) return IVP_ERR_BAD_ARGUMENT;
    ctx->err.clear();
    int rc = check_args(ctx, opt, out, dense);
    if (rc != IVP_OK) return rc;
    int n = 0, np = 0;
    rc = validate(ctx, prob, B, opt, &n, &np);
    if (rc != IVP_OK) return rc;
    if (!y0 || !t0 || !t1) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "null y0/t0/t1");
    if (np > 0 && !params) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "params required (n_params=%d)", np);
    if ((t0_len != 1 && t0_len != B) || (t1_len != 1 && t1_len != B)) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "t0/t1 length must be 1 or B");
    DeviceGuard restore_device;
    dense->owned = 0; dense->device = -1; dense->passes = 0; dense->total = 0; dense->staging_bytes = 0;
    const size_t nc = (size_t)ncoef_of(opt->method) * (size_t)n;
    dense->ncoef_n = (uint32_t)nc;
    // ---- 1. the counting solve through the host entry point (it stages `out` itself) ----
    ivp_options_t o = *opt;
    o.dense_output = 1;
    o.max_log = std::max<uint32_t>(opt->max_log, 1u);
    const size_t ml = o.max_log;
    std::vector<double> hst;
    std::vector<uint32_t> ns;
    try {
        hst.resize(ml * (nc + 2) * B);
        ns.resize(B);
    } catch (const std::bad_alloc &) {
        return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out of host memory for the counting solve's segment block (%zu records x %zu trajectories)", ml, B);
    }
    ivp_batch_result_t r = *out;
    if (opt->max_log == 0 && !out->log_offsets) { r.t_log = nullptr; r.y_log = nullptr; }   // the one record of the block is for segments only
    r.seg_cont = hst.data();
    r.seg_xold = r.seg_cont + ml * nc * B;
    r.seg_h = r.seg_xold + ml * B;
    r.n_seg = ns.data();
    dense->staging_bytes = hst.size() * sizeof(double);
    rc = ivp_batch_solve(ctx, prob, B, y0, params, t0, t0_len, t1, t1_len, &o, &r);
    if (rc != IVP_OK) return rc;
    const ivp_run_stats_t stats = ctx->stats;
    if (out->n_seg) std::memcpy(out->n_seg, ns.data(), sizeof(uint32_t) * B);
    dense->passes = 1;
    // ---- 2. offsets (host) ----
    uint64_t total = 0;
    dense->offsets[0] = 0;
    for (size_t b = 0; b < B; ++b) { total += ns[b]; dense->offsets[b + 1] = total; }
    dense->total = total;
    // ---- 3. destination (host) ----
    if (dense->cont) {
        if (dense->capacity < total)
            return fail(ctx, IVP_ERR_LOG_CAPACITY, "the dense log has %llu segments, cont / xold / h hold %llu", (unsigned long long)total, (unsigned long long)dense->capacity);
    }
    if (total == 0) {
        if (!dense->cont) { dense->capacity = 0; }
        return IVP_OK;
    }
    // ---- 4. the segments: from the host block when every run fitted it, else a filling solve on the device ----
    const uint32_t most = *std::max_element(ns.begin(), ns.end());
    double *c_out = dense->cont, *x_out = dense->xold, *h_out = dense->h;
    bool mine = false;
    if (!c_out) {
        c_out = (double *)std::malloc(total * nc * sizeof(double));
        x_out = (double *)std::malloc(total * sizeof(double));
        h_out = (double *)std::malloc(total * sizeof(double));
        mine = true;
        if (!c_out || !x_out || !h_out) { std::free(c_out); std::free(x_out); std::free(h_out); return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out of host memory for %llu dense segments", (unsigned long long)total); }
    }
    if (most <= ml) {
        for (size_t b = 0; b < B; ++b)
            for (uint32_t k = 0; k < ns[b]; ++k) {
                const size_t q = (size_t)dense->offsets[b] + k;
                x_out[q] = r.seg_xold[k * B + b];
                h_out[q] = r.seg_h[k * B + b];
                for (size_t c = 0; c < nc; ++c) c_out[q * nc + c] = r.seg_cont[(k * nc + c) * B + b];
            }
    } else {
        hst.clear(); hst.shrink_to_fit();
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t l0 = t0_len == 1 ? 1 : B, l1 = t1_len == 1 ? 1 : B;
        Tmp in, off, cd, xd, hd, err;
        auto bail = [&](int code) { if (mine) { std::free(c_out); std::free(x_out); std::free(h_out); } return code; };
        if (in.get(sizeof(double) * ((size_t)n * B + (size_t)std::max(np, 0) * B + l0 + l1)) != hipSuccess || off.get(sizeof(uint64_t) * (B + 1)) != hipSuccess ||
            cd.get(total * nc * sizeof(double)) != hipSuccess || xd.get(total * sizeof(double)) != hipSuccess || hd.get(total * sizeof(double)) != hipSuccess ||
            err.get(sizeof(uint32_t)) != hipSuccess)
            return bail(fail(ctx, IVP_ERR_HIP, "dense output: device memory for %llu segments and the inputs", (unsigned long long)total));
        double *yd = (double *)in.p, *pd = yd + (size_t)n * B, *t0d = pd + (size_t)std::max(np, 0) * B, *t1d = t0d + l0;
        hipStream_t s = nullptr;
        if (hipMemcpyAsync(yd, y0, sizeof(double) * n * B, hipMemcpyHostToDevice, s) != hipSuccess ||
            (np > 0 && hipMemcpyAsync(pd, params, sizeof(double) * np * B, hipMemcpyHostToDevice, s) != hipSuccess) ||
            hipMemcpyAsync(t0d, t0, sizeof(double) * l0, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(t1d, t1, sizeof(double) * l1, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(off.p, dense->offsets, sizeof(uint64_t) * (B + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemsetAsync(err.p, 0, sizeof(uint32_t), s) != hipSuccess)
            return bail(fail(ctx, IVP_ERR_HIP, "dense output: staging the inputs"));
        ivp_dense_log_t dd = *dense;
        dd.cont = (double *)cd.p; dd.xold = (double *)xd.p; dd.h = (double *)hd.p;
        rc = fill_pass(ctx, prob, B, yd, np > 0 ? pd : nullptr, t0d, l0, t1d, l1, opt, n, np, nc, ns, (const unsigned long long *)off.p, &dd, (uint32_t *)err.p, s);
        ctx->stats = stats;
        if (rc == IVP_OK) rc = check_err(ctx, (const uint32_t *)err.p, s);
        if (rc != IVP_OK) return bail(rc);
        dense->staging_bytes = std::max<uint64_t>(dense->staging_bytes, dd.staging_bytes);
        if (hipMemcpy(c_out, cd.p, total * nc * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(x_out, xd.p, total * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(h_out, hd.p, total * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            return bail(fail(ctx, IVP_ERR_HIP, "dense output: copying the segments to the host"));
        dense->passes = 2;
    }
    if (mine) {
        dense->cont = c_out; dense->xold = x_out; dense->h = h_out;
        dense->capacity = total;
        dense->owned = 1;
        dense->device = -1;
    }
    return IVP_OK;
}

int ivp_dense_log_fetch_device(ivp_dense_log_t *dense, double *cont, double *xold, double *h, void *hip_stream)
{
    if (!dense || !dense->owned || dense->device < 0 || !cont || !xold || !h) return IVP_ERR_BAD_ARGUMENT;
    DeviceGuard restore;
    if (hipSetDevice(dense->device) != hipSuccess) return IVP_ERR_HIP;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t total = (size_t)dense->total;
    if (total) {
        if (hipMemcpyAsync(cont, dense->cont, total * dense->ncoef_n * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync(xold, dense->xold, total * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync(h, dense->h, total * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return IVP_ERR_HIP;
    }
    ivp_dense_log_free(dense);
    dense->cont = cont; dense->xold = xold; dense->h = h;
    dense->capacity = total;
    return IVP_OK;
}

void ivp_dense_log_free(ivp_dense_log_t *dense)
{
    if (!dense || !dense->owned) return;
    if (dense->device >= 0) {
        DeviceGuard restore;
        (void)hipSetDevice(dense->device);
        if (dense->cont) (void)hipFree(dense->cont);
        if (dense->xold) (void)hipFree(dense->xold);
        if (dense->h) (void)hipFree(dense->h);
    } else {
        std::free(dense->cont);
        std::free(dense->xold);
        std::free(dense->h);
    }
    dense->cont = nullptr; dense->xold = nullptr; dense->h = nullptr; dense->capacity = 0; dense->owned = 0; dense->device = -1;
}

int ivp_dense_eval_device(ivp_ctx_t *ctx, int32_t method, int32_t n, int32_t fp_mode, size_t B, const uint64_t *offsets,
                          const double *cont, const double *xold, const double *h, const double *t, const uint64_t *t_offsets,
                          uint64_t m, int32_t extrapolate, double *y, int32_t *found, void *hip_stream)
{
    if (!ctx) return IVP_ERR_BAD_ARGUMENT;
    ctx->err.clear();
    if (method < IVP_RK23 || method > IVP_BDF) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "method %d", method);
    if (n < 1 || n > 512) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "n = %d (1 .. 512)", n);
    if (fp_mode != IVP_FP_STRICT && fp_mode != IVP_FP_FMA) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "fp_mode %d", fp_mode);
    if (B == 0 || m == 0) return IVP_OK;
    if (!offsets || !cont || !xold || !h || !t || !y || !found) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "null offsets / cont / xold / h / t / y / found");
    if (B > 0xFFFFFFFFull) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "B = %zu", B);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DenseEvalArgs e;
    e.off = (const unsigned long long *)offsets;
    e.cont = cont; e.xold = xold; e.h = h; e.t = t;
    e.t_off = (const unsigned long long *)t_offsets;
    e.nq = t_offsets ? m : m * (unsigned long long)B;
    e.B = B;
    e.y = y; e.found = found;
    e.n = n;
    e.extrapolate = extrapolate ? 1 : 0;
    e.wide = ((uintptr_t)cont & 15u) == 0 ? 1 : 0;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, fp_mode == IVP_FP_FMA ? ivp_dense_eval_fast(method, e, s) : ivp_dense_eval_strict(method, e, s));
    return IVP_OK;
}

}  // extern "C"
