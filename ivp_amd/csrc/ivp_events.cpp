// ivp_events.cpp -- ivp_batch_solve_events*(): every trajectory's complete Solution.t_events / Solution.y_events
// (src/solve/solution.rs:10-11, Vecs that grow with every occurrence, src/solve/solout.rs:158-331) as a CSR log.
//
// An events solve is the counted CSR log of ivp_csr.h (counting solve, scan, destination, pack or filling solve; layout and
// ownership: include/ivp_hip.h) with n_events runs per trajectory, event-major: the counting solve is the caller's own with
// a bounded block of opt->max_events slots per event and trajectory (none when max_events == 0; n_event_hits keeps counting
// past the block), and event_pack_kernel (event_pack.hip) moves a block into its runs.  The staging block of the filling
// solve is [n_events][max hits of the range][n + 1] doubles per trajectory of a range, capped at half of the free memory or
// at IVP_EVENT_STAGING_BYTES -- beside the filling solve's own scratch: its deferred event refinement (ivp_capi.cpp) notes
// up to n_events * max_events steps of 4 + 3 n_events + n + ncoef n doubles per trajectory when a quarter of the free memory
// holds them (inline refinement otherwise).  This file holds what is the event log's own: the argument checks, the
// description of the kind, the host packing loop, the entry points and the log's ownership calls with their width table.
// ivp_radau_solve_events*() are the same log over the direct Radau call (CsrKind::rad): the one Radau entry point that accepts a
// problem with event functions (radau_validate's events mode, ivp_capi.cpp); Radau refines every root inline.
#include "ivp_csr.h"

#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <new>
#include <unordered_map>

#ifndef IVP_HD
#define IVP_HD inline
#endif
#include "event_kernels.h"
#include "event_pack.h"

using namespace ivp_host;

namespace {

// ivp_event_log_t carries no record width: the library remembers it for the device logs it owns (y pointer -> n), from
// the allocation to ivp_event_log_free(), so that ivp_event_log_fetch_device() knows how much to copy
std::mutex g_owned_mu;
std::unordered_map<const void *, size_t> g_owned_n;

// arguments of all entry points; *nev_out = the problem's number of event functions.  rad != NULL: the direct Radau call
// (ivp_radau_solve_events*), whose *opt has been made Radau's (method, has_settings) by the caller
int check_args(ivp_ctx *ctx, const ivp_problem_t *prob, size_t B, const ivp_options_t *opt, const ivp_batch_result_t *out, const ivp_event_log_t *ev,
               int *n_out, int *np_out, size_t *nev_out, RadauCall *rad = nullptr)
{
    if (!opt || !out || !ev || !ev->offsets) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "null options / out / ev / ev->offsets");
    if (out->t_events || out->y_events)
        return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out.t_events / y_events are the bounded layout: leave them NULL, the occurrences go to `ev`");
    if ((ev->t != nullptr) != (ev->y != nullptr)) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "ivp_event_log_t: t and y must both be given or both be NULL");
    int rc = rad ? radau_validate(ctx, prob, B, opt, rad, n_out, np_out) : validate(ctx, prob, B, opt, n_out, np_out);
    if (rc != IVP_OK) return rc;
    const size_t nev = result_shape(prob, opt, *n_out).nev;
    if (nev == 0) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "the problem defines no event functions: there is no event log to deliver");
    if (B > 0xFFFFFFFFull / nev) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "n_events * B = %zu * %zu runs (at most 4294967295)", nev, B);
    *nev_out = nev;
    return IVP_OK;
}

// the event log as the staging driver sees it.  Resets the log's out members.
CsrKind event_kind(ivp_ctx *ctx, const ivp_options_t *opt, ivp_event_log_t *ev, size_t n, size_t nev, size_t B)
{
    ev->owned = 0; ev->device = -1; ev->passes = 0; ev->n_events = (uint32_t)nev; ev->total = 0; ev->staging_bytes = 0;
    CsrKind k;
    k.name = "event output";
    k.staging_env = "IVP_EVENT_STAGING_BYTES";
    k.runs_per_traj = nev;
    k.counts = &ivp_batch_result_t::n_event_hits;
    k.depth = &ivp_options_t::max_events;
    k.rec = nev * (n + 1) * sizeof(double);
    k.narrays = 2;
    k.width[0] = 1; k.width[1] = n; k.width[2] = 0;
    k.count_opt = *opt;
    k.fill_opt = *opt;
    k.fill_opt.t_eval = nullptr; k.fill_opt.n_eval = 0; k.fill_opt.t_eval_offsets = nullptr;   // samples do not steer the integration; they came with the counting solve
    k.fill_opt.max_log = 0;        // neither do the step log and the dense segments
    k.fill_opt.dense_output = 0;
    k.fill_opt.count_log = 0;
    k.fill_opt.profile = 0;        // ctx->stats stay those of the counting solve (the driver restores them)
    k.offsets = ev->offsets; k.capacity = &ev->capacity; k.total = &ev->total; k.staging_bytes = &ev->staging_bytes; k.passes = &ev->passes;
    k.given.p[0] = ev->t; k.given.p[1] = ev->y;
    k.bind = [nev](ivp_batch_result_t &r, double *block, size_t depth, size_t cnt) {
        r.t_events = block;
        r.y_events = r.t_events + nev * depth * cnt;
    };
    k.pack = [n, nev, B](const ivp_batch_result_t &r, const unsigned long long *off, const CsrArrays &dst, uint32_t *err, size_t first, size_t cnt,
                         uint32_t depth, hipStream_t s) {
        EventPackArgs p{r.t_events, r.y_events, r.n_event_hits, off, dst.p[0], dst.p[1], err, (unsigned long long)B, (unsigned long long)first,
                        (uint32_t)cnt, depth, (uint32_t)n, (uint32_t)nev};
        return ivp_event_pack(p, s);
    };
    // the pack kernel's own arithmetic (event_pack.h), run by run on the host block
    k.pack_host = [ev, n, nev, B, depth = opt->max_events](const ivp_batch_result_t &r, const uint32_t *hits, const CsrArrays &dst) {
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "offsets are 64-bit");
        bool bad = false;
        for (size_t i = 0; i < nev; ++i)
            for (size_t b = 0; b < B; ++b)
                bad |= event_pack_run(r.t_events, r.y_events, hits, (const unsigned long long *)ev->offsets, dst.p[0], dst.p[1], (uint32_t)i, b, 0, B, B,
                                      depth, (uint32_t)n, 0u, 1u);
        return !bad;
    };
    k.adopt = [ctx, ev, n](const CsrArrays &a, uint64_t capacity, int device) {   // released by ivp_event_log_free
        if (device >= 0) {
            try {
                std::lock_guard<std::mutex> lock(g_owned_mu);
                g_owned_n[a.p[1]] = n;
            } catch (const std::bad_alloc &) {
                return fail(ctx, IVP_ERR_BAD_ARGUMENT, "out of host memory");
            }
        }
        ev->t = a.p[0]; ev->y = a.p[1];
        ev->capacity = capacity;
        ev->owned = 1;
        ev->device = device;
        return (int)IVP_OK;
    };
    return k;
}

// opt as the Radau path reads it (submit_impl does the same): method and the explicit methods' controller fields are ignored
ivp_options_t radau_options(const ivp_options_t *opt)
{
    ivp_options_t o = *opt;
    o.method = IVP_RADAU;
    o.has_settings = 0;
    return o;
}

RadauCall radau_events_call(const ivp_radau_settings_t *settings, const ivp_radau_dae_t *dae)
{
    RadauCall call = radau_call(settings, dae);
    call.events_call = 1;
    return call;
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
    return csr_solve_device(ctx, event_kind(ctx, opt, ev, (size_t)n, nev, B), CsrInputs{prob, B, y0, params, t0, t0_len, t1, t1_len, n, np}, out,
                            (hipStream_t)hip_stream);
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
    const CsrInputs in{prob, B, y0, params, t0, t0_len, t1, t1_len, n, np};
    rc = check_host_inputs(ctx, in);
    if (rc != IVP_OK) return rc;
    DeviceGuard restore_device;
    return csr_solve_host(ctx, event_kind(ctx, opt, ev, (size_t)n, nev, B), in, out);
}

// ---- the direct Radau call with event functions: the same log over the Radau solve (every round of the driver runs it with
// the settings / partition copied here; the caller's structs are not read once the first submit has returned) ----

int ivp_radau_events_check(const ivp_problem_t *prob, size_t B, const ivp_options_t *opt, const ivp_radau_settings_t *settings,
                           const ivp_radau_dae_t *dae, char *message, size_t message_len)
{
    ivp_ctx scratch;   // carries the message, owns no device memory, touches no HIP call
    int n = 0, np = 0, rc;
    if (!prob || !opt) rc = fail(&scratch, IVP_ERR_BAD_ARGUMENT, "null problem/options");
    else {
        const ivp_options_t o = radau_options(opt);
        RadauCall call = radau_events_call(settings, dae);
        rc = radau_validate(&scratch, prob, B, &o, &call, &n, &np);
        if (rc == IVP_OK) {
            const int nev = (int)result_shape(prob, &o, n).nev;
            if (nev > 4 && !(o.ev_direction_vec && o.ev_terminal_vec && o.n_event_cfg == nev))
                rc = fail(&scratch, IVP_ERR_BAD_ARGUMENT, "%d event functions need ev_direction_vec / ev_terminal_vec with n_event_cfg = %d entries", nev, nev);
        }
    }
    if (message && message_len) std::snprintf(message, message_len, "%s", scratch.err.c_str());
    return rc;
}

int ivp_radau_solve_events_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                                  const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                                  const ivp_radau_settings_t *settings, const ivp_radau_dae_t *dae, ivp_batch_result_t *out,
                                  ivp_event_log_t *ev, void *hip_stream)
{
    if (!ctx) return IVP_ERR_BAD_ARGUMENT;
    ctx->err.clear();
    if (!opt) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "null options / out / ev / ev->offsets");
    const ivp_options_t o = radau_options(opt);
    RadauCall call = radau_events_call(settings, dae);
    int n = 0, np = 0;
    size_t nev = 0;
    int rc = check_args(ctx, prob, B, &o, out, ev, &n, &np, &nev, &call);
    if (rc != IVP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    CsrKind k = event_kind(ctx, &o, ev, (size_t)n, nev, B);
    k.rad = &call;
    return csr_solve_device(ctx, k, CsrInputs{prob, B, y0, params, t0, t0_len, t1, t1_len, n, np}, out, (hipStream_t)hip_stream);
}

int ivp_radau_solve_events(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                           const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                           const ivp_radau_settings_t *settings, const ivp_radau_dae_t *dae, ivp_batch_result_t *out, ivp_event_log_t *ev)
{
    if (!ctx) return IVP_ERR_BAD_ARGUMENT;
    ctx->err.clear();
    if (!opt) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "null options / out / ev / ev->offsets");
    const ivp_options_t o = radau_options(opt);
    RadauCall call = radau_events_call(settings, dae);
    int n = 0, np = 0;
    size_t nev = 0;
    int rc = check_args(ctx, prob, B, &o, out, ev, &n, &np, &nev, &call);
    if (rc != IVP_OK) return rc;
    const CsrInputs in{prob, B, y0, params, t0, t0_len, t1, t1_len, n, np};
    rc = check_host_inputs(ctx, in);
    if (rc != IVP_OK) return rc;
    DeviceGuard restore_device;
    CsrKind k = event_kind(ctx, &o, ev, (size_t)n, nev, B);
    k.rad = &call;
    return csr_solve_host(ctx, k, in, out);
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
