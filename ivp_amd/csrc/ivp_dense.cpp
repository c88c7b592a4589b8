// ivp_dense.cpp -- ivp_batch_solve_dense*(): every trajectory's complete ContinuousOutput (src/solve/cont.rs:9-153) as a
// CSR log, and ivp_dense_eval_device(): that continuous solution at query times on the device.
//
// A dense solve is the counted CSR log of ivp_csr.h (counting solve, scan, destination, pack or filling solve; layout and
// ownership: include/ivp_hip.h) with one run per trajectory: the counting solve has dense_output on and a bounded segment
// block of max(max_log, 1) records (n_seg keeps counting past the block, the constant segment of a zero-length interval
// included), and dense_pack_kernel (dense_eval.hip) moves a block into its runs.  The staging block of the filling solve is
// [max n_seg][ncoef n + 2] doubles per trajectory of a range (BASELINE C2: profiles/r05_dense_c2_*.json), capped at half of
// the free memory or at IVP_DENSE_STAGING_BYTES.  This file holds what is the dense log's own: the argument checks, the
// description of the kind, the host packing loop, the entry points, the log's ownership calls and the evaluation.
#include "ivp_csr.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "dense_kernels.h"

using namespace ivp_host;

namespace {

int check_args(ivp_ctx *ctx, const ivp_options_t *opt, const ivp_batch_result_t *out, const ivp_dense_log_t *d)
{
    if (!opt || !out || !d || !d->offsets) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "null options / out / dense / dense->offsets");
    if (out->seg_cont || out->seg_xold || out->seg_h)
        return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out.seg_cont / seg_xold / seg_h are the bounded layout: leave them NULL, the segments go to `dense`");
    if ((d->cont || d->xold || d->h) && !(d->cont && d->xold && d->h))
        return fail(ctx, IVP_ERR_BAD_ARGUMENT, "ivp_dense_log_t: cont, xold and h must all be given or all be NULL");
    return IVP_OK;
}

// the dense log as the staging driver sees it; nc = ncoef n, the doubles of cont per segment.  Resets the log's out members.
CsrKind dense_kind(const ivp_options_t *opt, const ivp_batch_result_t *out, ivp_dense_log_t *d, size_t nc, size_t B, RadauCall *rad)
{
    d->owned = 0; d->device = -1; d->passes = 0; d->total = 0; d->staging_bytes = 0;
    d->ncoef_n = (uint32_t)nc;
    CsrKind k;
    k.name = "dense output";
    k.staging_env = "IVP_DENSE_STAGING_BYTES";
    k.runs_per_traj = 1;
    k.counts = &ivp_batch_result_t::n_seg;
    k.depth = &ivp_options_t::max_log;
    k.rec = (nc + 2) * sizeof(double);
    k.narrays = 3;
    k.width[0] = nc; k.width[1] = 1; k.width[2] = 1;
    k.count_opt = *opt;
    k.count_opt.dense_output = 1;
    k.count_opt.max_log = std::max<uint32_t>(opt->max_log, 1u);
    k.fill_opt = *opt;
    k.fill_opt.dense_output = 1;
    k.fill_opt.t_eval = nullptr; k.fill_opt.n_eval = 0; k.fill_opt.t_eval_offsets = nullptr;   // samples do not steer the integration; they came with the counting solve
    k.fill_opt.count_log = 0;
    k.fill_opt.max_events = 0;   // event occurrences are detected (terminal ones stop), not stored
    k.fill_opt.profile = 0;      // ctx->stats stay those of the counting solve (the driver restores them)
    k.rad = rad;
    k.offsets = d->offsets; k.capacity = &d->capacity; k.total = &d->total; k.staging_bytes = &d->staging_bytes; k.passes = &d->passes;
    k.given.p[0] = d->cont; k.given.p[1] = d->xold; k.given.p[2] = d->h;
    const bool segments_only = opt->max_log == 0 && !out->log_offsets;   // the one record of the counting block is for segments only
    k.bind = [nc, segments_only](ivp_batch_result_t &r, double *block, size_t depth, size_t cnt) {
        if (segments_only) { r.t_log = nullptr; r.y_log = nullptr; }
        r.seg_cont = block;
        r.seg_xold = r.seg_cont + depth * nc * cnt;
        r.seg_h = r.seg_xold + depth * cnt;
    };
    k.pack = [nc](const ivp_batch_result_t &r, const unsigned long long *off, const CsrArrays &dst, uint32_t *err, size_t first, size_t cnt,
                  uint32_t depth, hipStream_t s) {
        DensePackArgs p{r.seg_cont, r.seg_xold, r.seg_h, r.n_seg, off + first, dst.p[0], dst.p[1], dst.p[2], err, (uint32_t)cnt, depth, (uint32_t)nc};
        return ivp_dense_pack(p, s);
    };
    k.pack_host = [d, nc, B](const ivp_batch_result_t &r, const uint32_t *ns, const CsrArrays &dst) {
        for (size_t b = 0; b < B; ++b)
            for (uint32_t i = 0; i < ns[b]; ++i) {
                const size_t q = (size_t)d->offsets[b] + i;
                dst.p[1][q] = r.seg_xold[i * B + b];
                dst.p[2][q] = r.seg_h[i * B + b];
                for (size_t c = 0; c < nc; ++c) dst.p[0][q * nc + c] = r.seg_cont[(i * nc + c) * B + b];
            }
        return true;
    };
    k.adopt = [d](const CsrArrays &a, uint64_t capacity, int device) {   // released by ivp_dense_log_free
        d->cont = a.p[0]; d->xold = a.p[1]; d->h = a.p[2];
        d->capacity = capacity;
        d->owned = 1;
        d->device = device;
        return (int)IVP_OK;
    };
    return k;
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
    const CsrKind k = dense_kind(opt, out, dense, result_shape(prob, opt, n).nc, B, rad);
    return csr_solve_device(ctx, k, CsrInputs{prob, B, y0, params, t0, t0_len, t1, t1_len, n, np}, out, (hipStream_t)hip_stream);
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
    const CsrInputs in{prob, B, y0, params, t0, t0_len, t1, t1_len, n, np};
    rc = check_host_inputs(ctx, in);
    if (rc != IVP_OK) return rc;
    DeviceGuard restore_device;
    return csr_solve_host(ctx, dense_kind(opt, out, dense, result_shape(prob, opt, n).nc, B, nullptr), in, out);
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
