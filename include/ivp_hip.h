/*
 * ivp_hip.h -- C ABI of libivp_hip.so: the MI355X (gfx950) batched explicit Runge-Kutta integrator.
 *
 * This is the drop-in boundary for ONE path of the Rust crate Ryan-D-Gast/ivp 0.5.1: the explicit
 * RK stepping core (DOPRI5 / DOP853 / RK23 stage evaluation, weighted error norm, step-size
 * controller, initial-step heuristic) behind solve_ivp().  The reference has no C ABI of its own
 * (its only exported symbol is the PyO3 module init, src/python/mod.rs:26); the entry points below
 * are what a `#[link(name = "ivp_hip")] extern "C"` block in the crate would bind -- see
 * INTEGRATION.md for that binding.  Each declaration cites the reference interface it replaces
 * (file:line relative to the reference tree).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types;
 *   - all state is struct-of-arrays: component c of trajectory b lives at a[c*B + b];
 *   - a "trajectory" is one reference solve_ivp() call; a batch is B independent calls;
 *   - whole-call validation failures are returned as negative codes (the reference's
 *     Err(Error::Config(..)) values, src/error.rs:18-60); per-trajectory integration failures are
 *     reported only in status[b] (the reference's Ok(..) with a non-success Status,
 *     src/methods/dopri5.rs:268-277); nothing throws or aborts across this boundary;
 *   - the library never falls back to a CPU path: without a usable HIP device every compute entry
 *     point returns IVP_ERR_NO_DEVICE.
 */
#ifndef IVP_HIP_H
#define IVP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVP_HIP_ABI_VERSION 5

/* Method: same order as `enum Method`, src/solve/options.rs:14-27. The explicit RK methods (RK23, DOPRI5,
 * DOP853, the fixed-step RK4) and the variable-order implicit BDF are on the accelerated path of solve_ivp().  RADAU
 * runs on the device through its direct per-method call, ivp_radau_solve*() below (n <= 64, hiprtc problems n <= 512); as ivp_options_t.method
 * it still returns IVP_ERR_UNSUPPORTED_METHOD from the solve_ivp() entry points. */
typedef enum {
    IVP_RK23 = 0,
    IVP_DOPRI5 = 1, /* "RK45" */
    IVP_DOP853 = 2,
    IVP_RK4 = 3,
    IVP_RADAU = 4,
    IVP_BDF = 5
} ivp_method_t;

/* Status: same order as `enum Status`, src/status.rs:4-19. */
typedef enum {
    IVP_STATUS_SUCCESS = 0,
    IVP_STATUS_USER_INTERRUPT = 1,
    IVP_STATUS_NEED_LARGER_NMAX = 2,
    IVP_STATUS_STEP_SIZE_TOO_SMALL = 3,
    IVP_STATUS_PROBABLY_STIFF = 4,
    IVP_STATUS_SINGULAR_MATRIX = 5,
    IVP_STATUS_POOR_CONVERGENCE = 6
} ivp_status_t;

/* Return codes. The negative config codes map 1:1 onto `enum ConfigError`, src/error.rs:18-60. */
typedef enum {
    IVP_OK = 0,
    IVP_ERR_MUST_BE_POSITIVE = -1,        /* ConfigError::MustBePositive       */
    IVP_ERR_OUT_OF_RANGE = -2,            /* ConfigError::OutOfRange           */
    IVP_ERR_NEGATIVE_TOLERANCE = -3,      /* ConfigError::NegativeTolerance    */
    IVP_ERR_TOLERANCE_SIZE_MISMATCH = -4, /* ConfigError::ToleranceSizeMismatch (a panic in the reference, src/methods/mod.rs:156-161) */
    IVP_ERR_INVALID_STEP_SIZE = -5,       /* ConfigError::InvalidStepSize (RK4: first_step zero / wrong sign, rk4.rs:81-87) */
    IVP_ERR_INVALID_SCALE_FACTORS = -6,   /* ConfigError::InvalidScaleFactors  */
    IVP_ERR_INVALID_DAE_PARTITION = -7,   /* ConfigError::InvalidDAEPartition (ivp_radau_solve_dae*: nind1 + nind2 + nind3 != n) */
    IVP_ERR_BAD_ARGUMENT = -100,          /* NULL pointer, unknown rhs id, n mismatch ...            */
    IVP_ERR_UNSUPPORTED_METHOD = -101,    /* RADAU as ivp_options_t.method: solve_ivp() does not route to it yet (ivp_radau_solve*() is the way in) */
    IVP_ERR_NO_DEVICE = -102,             /* no HIP device: there is deliberately no CPU fallback    */
    IVP_ERR_HIP = -103,                   /* a HIP runtime call failed; see ivp_last_error_string()  */
    IVP_ERR_JIT = -104,                   /* hiprtc compilation of a user RHS failed                 */
    IVP_ERR_LOG_CAPACITY = -105           /* ivp_step_log_t: the caller's t / y hold fewer than `total` records (total is set) */
} ivp_error_t;

/* Right-hand sides that ship as device functors: the `impl IVP for ..` blocks of the reference's
 * examples, tests and benchmark (trait IVP::ode, src/ivp.rs:27-29). User-defined systems are
 * compiled at run time from a HIP source snippet with ivp_rhs_compile(). */
typedef enum {
    IVP_RHS_DECAY = 0,    /* y' = -k y                 p={k}           n=1  examples/exponential_decay.rs:9-13 */
    IVP_RHS_SHO = 1,      /* y0'=y1, y1'=-y0                           n=2  tests/common.rs:3-9                */
    IVP_RHS_VDP = 2,      /* Van der Pol               p={mu}          n=2  benches/benchmark.py:22-27         */
    IVP_RHS_CR3BP = 3,    /* restricted 3-body         p={mu}          n=6  examples/cr3bp.rs:23-36            */
    IVP_RHS_LORENZ = 4,   /* Lorenz                    p={sigma,rho,beta} n=3  benches/benchmark.py:30-37      */
    IVP_RHS_ZERO = 5,     /* y' = 0                                    n=3  tests/ivp.rs:11-19                 */
    IVP_RHS_RATIONAL = 6, /* SciPy "rational" problem                  n=2  tests/test_helpers.py:23-25        */
    IVP_RHS_EXP2 = 7,     /* y' = y                                    n=2  tests/ivp.rs:291-298               */
    IVP_RHS_LINEAR = 8,   /* y' = A y, A = [[-1,-5],[1,1]]            n=2  tests/test_helpers.py:11-12        */
    IVP_RHS_ROBERTSON = 9,/* Robertson kinetics                        n=3  tests/test_ivp.py:327-333          */
    IVP_RHS_VDP_EPS = 10, /* stiff Van der Pol        p={eps}          n=2  examples/van_der_pol.rs:9-14       */
    /* problems that carry event functions (trait IVP::events / n_events, src/ivp.rs:31-46) */
    IVP_RHS_SHO_EV = 11,  /* SHO, event g = y0                          n=2  tests/ivp.rs:151-221               */
    IVP_RHS_BALL = 12,    /* bouncing ball  p={gravity,drag}, g = height n=2  examples/bouncing_ball.rs:5-31     */
    IVP_RHS_CANNON = 13,  /* y'' = -9.80665, g = y0                     n=2  tests/test_ivp.py:152-160          */
    IVP_RHS_RATIONAL_EV = 14, /* rational problem + 3 events            n=2  tests/test_ivp.py:345-353          */
    IVP_RHS_ROBERTSON_JAC = 15, /* Robertson + analytic `jac` override (trait IVP::jac, src/ivp.rs:67-107)  n=3 */
    IVP_RHS_BUILTIN_COUNT = 16,
    /* Large state dimensions (8 < n <= 512): one 64-lane wavefront integrates one trajectory, the state is
     * distributed over its lanes and the error norm is a wavefront reduction.  RK23 / DOPRI5 / DOP853 / RK4 with
     * every output mode (t_eval, step log, dense output), events (hiprtc problems) and scalar or vector tolerances;
     * BDF with the n x n matrices J and LU = (I - cJ) per trajectory (in LDS for n <= 128, see ivp_options_t.variant). */
    IVP_RHS_LINEAR_DECAY_100 = 100, /* y' = -y                            n=100 benches/benchmark.py:40-42,139-148 */
    IVP_RHS_HEAT1D_256 = 101,       /* y_i' = k (y_{i-1} - 2 y_i + y_{i+1}), p={k}  n=256 (method of lines)  */
    IVP_RHS_DENSE_64 = 102,         /* y' = A y, A dense 64 x 64: a_ii = -k (4 + i mod 5), a_ij = (((5 i + 3 j) & 15) - 8) / 256,
                                       p={k}: a FULL Jacobian for the per-trajectory LU of BDF (n=64) */
    IVP_RHS_JIT = 1000    /* problem.jit holds a handle from ivp_rhs_compile() */
} ivp_rhs_id_t;

/* The device-side analogue of `impl IVP for T` (src/ivp.rs:27-121). */
typedef struct {
    int32_t rhs_id;   /* ivp_rhs_id_t */
    int32_t n;        /* state dimension (must match the functor's) */
    int32_t n_params; /* per-trajectory parameters (the fields of the user's struct, e.g. CR3BP{mu}) */
    void *jit;        /* ivp_rhs_compile() handle when rhs_id == IVP_RHS_JIT, else NULL */
} ivp_problem_t;

/* Floating-point mode of the kernels. */
typedef enum {
    IVP_FP_STRICT = 0, /* no FMA contraction, reference expression order: bit-comparable with a CPU
                          restatement of the reference (Rust never contracts a*b+c) */
    IVP_FP_FMA = 1,    /* the FMA arithmetic mode: the same operation sequence with the multiply-add sites of the stage
                          combinations, error estimates, dense coefficients, interpolants and tolerance scales as single
                          fused operations, and the built-in right-hand sides in their FMA form (one reciprocal per
                          denominator).  A DEFINED arithmetic (written out in the kernel source, compiled without
                          compiler contraction): results are identical in every kernel variant and for every batch
                          size, and bit-comparable with the oracle's FMA build (oracle/liboracle_fma.so).  Differs from
                          STRICT at the 1e-16-per-operation level; a hiprtc right-hand side is evaluated as written
                          (call fma() yourself where you want it) */
    IVP_FP_FAST = IVP_FP_FMA   /* ABI v3 name */
} ivp_fp_mode_t;

/* Mirrors `struct Options` (src/solve/options.rs:75-123) field by field for the fields the explicit
 * RK path reads; the remaining fields (jac_storage, mass_storage, nind1-3, min_step) belong to
 * RADAU/BDF only. Fill with ivp_options_default() first. */
typedef struct {
    int32_t method;         /* ivp_method_t; Options.method, default DOPRI5 */
    double rtol;            /* Options.rtol scalar form, default 1e-3 */
    double atol;            /* Options.atol scalar form, default 1e-6 */
    const double *rtol_vec; /* optional per-component rtol[n] (Tolerance::Vector), host pointer */
    const double *atol_vec; /* optional per-component atol[n], host pointer */
    int32_t rtol_vec_len;   /* must equal n when rtol_vec != NULL */
    int32_t atol_vec_len;
    uint64_t max_steps;     /* Options.max_steps; 0 = None = unlimited (src/solve/solve_ivp.rs:218) */
    const double *t_eval;   /* Options.t_eval: output grid shared by the batch (or B concatenated grids, see
                               t_eval_offsets below), host pointer, or NULL = None */
    int64_t n_eval;         /* number of t_eval points (ignored when t_eval == NULL) */
    int32_t has_first_step; /* Options.first_step is Some(..) */
    double first_step;
    int32_t has_max_step;   /* Options.max_step is Some(..) */
    double max_step;
    int32_t dense_output;   /* Options.dense_output: record per-step interpolants (needs max_log > 0) */
    /* event_config(i) of the problem (src/solve/event.rs:5-77), for problems whose functor defines events */
    int32_t ev_direction[4];  /* Direction: 0 All, > 0 Positive, < 0 Negative  (up to 4 events; more: *_vec below) */
    uint32_t ev_terminal[4];  /* terminal_count: 0 = None, k = interrupt at the k-th occurrence   */
    uint32_t max_events;      /* capacity of t_events / y_events per event and trajectory          */
    int32_t has_min_step;   /* Options.min_step is Some(..) (read by BDF only, src/solve/solve_ivp.rs:271) */
    double min_step;
    /* ---- knobs that exist only on the GPU path ---- */
    int32_t fp_mode;        /* ivp_fp_mode_t, default IVP_FP_STRICT */
    int32_t chunk_attempts; /* step attempts per kernel launch between compactions; 0 = auto */
    uint32_t max_log;       /* capacity (per trajectory) of the accepted-step log t_log/y_log and of the
                               dense-segment log; 0 = do not record (end state only) */
    int32_t variant;        /* stepping-kernel variant: 0 = auto, 1 = lean registers, 2 = coefficients resident,
                               3 = lane-cooperative (eight lanes per trajectory: DOPRI5 / DOP853, every output mode,
                               problems with events, built-in and hiprtc systems with n <= 8; otherwise as 0).
                               Large-n BDF (8 < n <= 128, built-in problems): 0 / 2 = factors of (I - cJ) resident in
                               LDS, 1 = in global memory.  Results do not depend on the variant in either arithmetic mode. */
    int32_t profile;        /* 1: time every kernel launch with HIP events (see ivp_run_stats_t);
                               2: additionally sum naccpt / attempts over the batch on the host */
    /* ---- direct per-method call: `DOPRI5 {..}.solve()`, `DOP853 {..}.solve()`, `RK23 {..}.solve()` ----
     * (src/methods/dopri5.rs:34-72,122-198, dop853.rs:34-63,114-193, rk23.rs:17-37,81-129).
     * has_settings == 0 (default): the struct defaults, i.e. exactly what solve_ivp() runs.
     * has_settings != 0: the fields below replace the struct's controller fields and are validated like
     * XXX::solve() validates them (OutOfRange / MustBePositive / InvalidScaleFactors); max_steps is then the struct's
     * `usize` field taken literally (0 => IVP_ERR_MUST_BE_POSITIVE).  Fill with ivp_options_method_defaults() first.
     * RK23 reads safety_factor / scale_min / scale_max only; RK4 / BDF reject has_settings. */
    int32_t has_settings;
    double uround;          /* default 2.3e-16                                   */
    double safety_factor;   /* default 0.9                                       */
    double scale_min;       /* default 0.2 (DOPRI5, RK23), 0.333 (DOP853)        */
    double scale_max;       /* default 10  (DOPRI5, RK23), 6 (DOP853)            */
    double beta;            /* default 0.04 (DOPRI5), 0 (DOP853)                 */
    uint64_t stiff_test;    /* default 1000                                      */
    int32_t count_log;      /* 1: run DefaultSolOut's accepted-step recording without storing anything: out->n_log
                               receives the number of records per trajectory (first pass of the CSR log) */
    /* ---- ABI v4 ---- */
    /* Per-trajectory output grids.  Every reference solve_ivp() call has its own Options.t_eval
     * (src/solve/options.rs:75-123); t_eval_offsets != NULL (host pointer, [B + 1], offsets[0] = 0, non-decreasing,
     * offsets[B] = n_eval) makes t_eval the concatenation of B grids: trajectory b samples
     * t_eval[offsets[b] .. offsets[b+1]).  The outputs are then time-major CSR records like Solution.y
     * (Vec<Vec<f64>>): with e = 1 for problems with event functions (a terminal event appends its own sample,
     * src/solve/solout.rs:316-319) and 0 otherwise, the k-th sample of trajectory b is record
     * q = offsets[b] + b * e + k:  y_eval[q * n + c], eval_idx[q] (index into b's OWN grid, -1 for the terminal sample);
     * y_eval holds (n_eval + B * e) * n doubles, eval_idx n_eval + B * e entries, n_filled[b] counts b's samples.
     * Every entry point takes them: ivp_batch_solve / ivp_batch_solve_multi_host copy the records back to the host arrays,
     * ivp_batch_solve_multi hands each shard its slice of the grids (offsets re-based to 0: a shard's y_eval / eval_idx
     * hold its own records) and places the shards' runs in the gathered arrays at the batch-wide offsets. */
    const uint64_t *t_eval_offsets;
    /* event_config(i) for problems with MORE than 4 event functions (trait IVP::n_events is unbounded,
     * src/ivp.rs:31-52): host arrays of n_event_cfg entries that replace ev_direction / ev_terminal above */
    const int32_t *ev_direction_vec;
    const uint32_t *ev_terminal_vec;
    int32_t n_event_cfg;
} ivp_options_t;

/* Per-trajectory results: `struct Solution` (src/solve/solution.rs:7-20) + IntegrationResult.h
 * (src/methods/mod.rs:30-39), struct-of-arrays over the batch. Any pointer may be NULL = not wanted.
 * For ivp_batch_solve() these are host pointers, for ivp_batch_solve_device() device pointers.
 * A capacity-bounded array (samples, log records, segments, event hits) is written up to its count; the
 * slots past it keep what the caller put there, with host pointers as with device pointers. */
typedef struct {
    double *y_end;      /* [n][B]  state at t_end (Solution.y.last())                           */
    double *t_end;      /* [B]     final x (xend on Success)                                    */
    int32_t *status;    /* [B]     ivp_status_t                                                 */
    uint64_t *nfev;     /* [B]     Solution.nfev  (njev = nlu = 0 on this path)                 */
    uint64_t *nstep;    /* [B]     Solution.nstep                                               */
    uint64_t *naccpt;   /* [B]     Solution.naccpt                                              */
    uint64_t *nrejct;   /* [B]     Solution.nrejct                                              */
    double *h_next;     /* [B]     IntegrationResult.h: the step the controller would try next  */
    /* t_eval mode (Options.t_eval = Some): Solution.t/y hold the sampled points, in order */
    double *y_eval;     /* [n_eval (+1 if the problem has events)][n][B]  k-th emitted sample   */
    int32_t *eval_idx;  /* [same rows][B]  index into t_eval of the k-th emitted sample; -1 = the terminal-event point */
    int32_t *n_filled;  /* [B]             number of emitted samples                            */
    /* accepted-step mode (Options.t_eval = None, max_log > 0): Solution.t/y, capped at max_log */
    double *t_log;      /* [max_log][B]                                                         */
    double *y_log;      /* [max_log][n][B]                                                      */
    uint32_t *n_log;    /* [B]  number of records the reference would hold (may exceed max_log) */
    /* dense_output: ContinuousOutput segments (src/solve/cont.rs:9-28), capped at max_log      */
    double *seg_cont;   /* [max_log][ncoef*n][B]  ncoef = Method::coeffs_per_state (options.rs:34-43) */
    double *seg_xold;   /* [max_log][B]                                                         */
    double *seg_h;      /* [max_log][B]                                                         */
    uint32_t *n_seg;    /* [B]  segments the reference would hold (may exceed max_log); 0 for a solve without dense_output, t_eval solves included */
    /* events: Solution.t_events / Solution.y_events (src/solve/solution.rs:10-11), capped at max_events */
    double *t_events;   /* [n_events][max_events][B]                                            */
    double *y_events;   /* [n_events][max_events][n][B]                                         */
    uint32_t *n_event_hits; /* [n_events][B] occurrences detected (may exceed max_events)       */
    double *t_term;     /* [B] t_eval mode: time of the appended terminal-event sample (eval_idx = -1) */
    /* implicit methods (BDF): Solution.njev / Solution.nlu; zero for the explicit RK methods  */
    uint64_t *njev;     /* [B]                                                                  */
    uint64_t *nlu;      /* [B]                                                                  */
    /* Unbounded accepted-step log in CSR form (the reference's Solution.t / Solution.y are Vecs that grow with every
     * accepted step, src/solve/solout.rs:387-428): an INPUT, like the other members a host array for ivp_batch_solve() /
     * ivp_batch_solve_multi_host() and a device array for the device-pointer entry points.  When non-NULL it holds B+1 record
     * offsets; trajectory b's k-th record then lives at t_log[log_offsets[b] + k] and
     * y_log[(log_offsets[b] + k) * n + c] (time-major like Vec<Vec<f64>>), so the log takes sum(n_log) records
     * instead of max_log x B.  Callers that want the whole log should use ivp_batch_solve_logged*() below: ONE integration
     * that records as it goes and delivers offsets, t_log and y_log in this very layout (ABI v5).  The two-pass form stays
     * for callers that manage the offsets themselves: a counting solve (options.count_log = 1, only n_log is written), an
     * exclusive scan of n_log, then the filling solve with these offsets. */
    const uint64_t *log_offsets;
} ivp_batch_result_t;

/* What the last solve on a context did (filled when options.profile == 1). */
typedef struct {
    uint32_t launches;          /* stepping-kernel launches (chunks)                     */
    uint32_t init_launches;
    double step_kernel_ms;      /* sum of HIP-event durations of the stepping kernels    */
    double init_kernel_ms;
    double total_ms;            /* first launch -> last kernel done, on the stream       */
    uint64_t total_accepted;    /* sum over the batch of naccpt                          */
    uint64_t total_attempts;    /* sum over the batch of step attempts                   */
    uint64_t lane_attempt_slots;/* sum over launches of (lanes launched x attempts the wave ran): divergence accounting */
    uint64_t lane_launches;     /* sum over launches of trajectories that loaded + stored their state */
    uint32_t coop_launches;     /* of `launches`: lane-cooperative tail launches (variant 3 / auto policy) */
    double coop_kernel_ms;      /* of `step_kernel_ms`: time in those launches                            */
    /* ABI v4: (bulk, cooperative) launch pairs -- exactly one launch of a pair works, the other returns at once */
    uint32_t declined_launches;      /* pair halves that declined (not counted in `launches`)            */
    uint32_t declined_coop_launches; /* of those: cooperative-kernel halves                              */
    double declined_ms;              /* their HIP-event durations (included in step_kernel_ms)           */
    double declined_coop_ms;         /* of that: cooperative-kernel halves (included in coop_kernel_ms)  */
} ivp_run_stats_t;

typedef struct ivp_ctx ivp_ctx_t;

/* Library / device queries. */
int ivp_abi_version(void);
int ivp_device_count(void);

/* A context owns the device scratch of one (device, stream) pair; it is not thread-safe, distinct
 * contexts may be used concurrently (the reference is re-entrant and single-threaded per call,
 * src/ivp.rs:27). */
int ivp_ctx_create(ivp_ctx_t **ctx, int device);
void ivp_ctx_destroy(ivp_ctx_t *ctx);
const char *ivp_last_error_string(const ivp_ctx_t *ctx);
int ivp_ctx_get_stats(const ivp_ctx_t *ctx, ivp_run_stats_t *stats);

/* Options::builder().build() defaults (src/solve/options.rs:75-123). */
void ivp_options_default(ivp_options_t *opt);

/* `DOPRI5::default()` / `DOP853::default()` / `RK23::default()` (src/methods/dopri5.rs:34-72, dop853.rs:34-81,
 * rk23.rs:17-50): sets method and fills uround .. stiff_test with that struct's defaults (has_settings stays as it is). */
int ivp_options_method_defaults(ivp_options_t *opt, int32_t method);

/* Dimension lookup for built-in right-hand sides; ivp_rhs_n_events = IVP::n_events() (src/ivp.rs:42-46). */
int ivp_rhs_dims(int32_t rhs_id, int32_t *n, int32_t *n_params);
int ivp_rhs_n_events(int32_t rhs_id);

/*
 * B independent solve_ivp() calls (src/solve/solve_ivp.rs:99-108:
 *   solve_ivp(f, x0, xend, y0, options) -> Result<Solution, Error>), host buffers.
 *   y0[n][B], params[n_params][B] (may be NULL when n_params == 0),
 *   t0/t1: [B] when *_len == B, or a single shared value when *_len == 1.
 * Returns IVP_OK or a negative ivp_error_t.
 */
int ivp_batch_solve(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0,
                    const double *params, const double *t0, size_t t0_len, const double *t1,
                    size_t t1_len, const ivp_options_t *opt, ivp_batch_result_t *out);

/*
 * Same, with every array argument (y0, params, t0, t1 and all `out` members) already resident in
 * device memory; work is enqueued on `hip_stream` (a hipStream_t, NULL = default stream) and the
 * call returns after the stream has drained the integration (it has to poll the active count).
 * opt->t_eval / rtol_vec / atol_vec stay host pointers.  y_end may alias y0.
 */
int ivp_batch_solve_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0,
                           const double *params, const double *t0, size_t t0_len, const double *t1,
                           size_t t1_len, const ivp_options_t *opt, ivp_batch_result_t *out,
                           void *hip_stream);

/*
 * The same solve (src/solve/solve_ivp.rs:99-108, B calls) as a resumable operation, so that one host thread can keep several contexts (= several batches,
 * each on its own stream) in flight: a solve is a sequence of rounds (a few kernel launches, then the count of
 * still-running trajectories travels to the host), and only the hand-over between rounds needs the host.
 *   ivp_batch_submit_device  validates, enqueues the init kernel and the first round, returns without waiting;
 *                            arguments as for ivp_batch_solve_device; one solve in flight per context
 *   ivp_batch_poll           non-blocking: if the current round has finished, starts the next one or completes the
 *                            solve; *done = 1 once the results are final (also when nothing is in flight)
 *   ivp_batch_wait           blocks until the solve is complete
 * ivp_batch_solve_device() is submit + wait.  A failed poll / wait abandons the solve.
 */
int ivp_batch_submit_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0,
                            const double *params, const double *t0, size_t t0_len, const double *t1,
                            size_t t1_len, const ivp_options_t *opt, ivp_batch_result_t *out,
                            void *hip_stream);
int ivp_batch_poll(ivp_ctx_t *ctx, int *done);
int ivp_batch_wait(ivp_ctx_t *ctx);

/*
 * Radau IIA(5), the direct per-method call: B independent RADAU::builder()...build().solve(f, x0, y0, xend, rtol, atol,
 * Some(&mut DefaultSolOut)) calls (src/methods/radau.rs:19-127) for pure ODEs with the identity mass matrix, n <= 512,
 * strict arithmetic: one lane per trajectory for n <= 8; for 8 < n <= 64 (the built-in IVP_RHS_DENSE_64, and hiprtc problems
 * in component form, ode_comp with an optional jac_col) one group of 16 / 32 / 64 lanes per trajectory, one matrix row per
 * lane, the three factors of the attempt resident in LDS -- 3 n^2 doubles, which is what sets that bound; for 64 < n <= 512
 * (hiprtc problems in component form without a mass hook only: no built-in beyond IVP_RHS_DENSE_64 is instantiated) one
 * wavefront per trajectory, ceil(n / 64) matrix rows per lane, J and the three factors in global memory -- 4 n^2 doubles per
 * trajectory, 8 MB at n = 512, 32 GB for B = 4096: an allocation that fails is IVP_ERR_HIP with HIP's out-of-memory text.
 * ivp_radau_settings_t carries the struct fields solve_ivp() cannot reach; the fields it can come
 * from ivp_options_t: rtol / atol (scalar or vector), max_steps (0 = unlimited, the solve_ivp convention), t_eval with
 * or without t_eval_offsets, first_step, max_step, min_step, dense_output, max_log, chunk_attempts, profile.
 * opt->method is ignored.  Arguments otherwise as for ivp_batch_solve_device / ivp_batch_solve; settings == NULL means
 * ivp_radau_settings_default().  out->njev / out->nlu are filled.  dense_output segments are 4 n coefficients
 * [coef][component]; ivp_dense_eval_device(method = IVP_RADAU) evaluates them.
 * Errors, reported before the device is touched: the ConfigErrors of radau.rs:132-262 (MUST_BE_POSITIVE: newton_maxiter;
 * OUT_OF_RANGE: uround, safety_factor, newton_maxiter > 15; INVALID_SCALE_FACTORS; INVALID_STEP_SIZE: first_step == 0;
 * NEGATIVE_TOLERANCE / TOLERANCE_SIZE_MISMATCH) and IVP_ERR_BAD_ARGUMENT with a "not yet" message for n > 64 (a built-in problem, or one with a mass hook), problems
 * with event functions (their one way in is ivp_radau_solve_events*, declared behind ivp_event_log_t below), fp_mode = FMA,
 * variant = 3 and, for n > 8, a problem compiled with IVP_RHS_BANDED or with a jac_sparsity pattern
 * (ivp_rhs_compile_sparse).  The multi-device forms are not on this path yet.
 *
 * M y' = f(t, y) with a constant, possibly singular mass matrix and index-1/2/3 algebraic variables: ivp_radau_solve_dae*()
 * and ivp_radau_dae_check(), the three calls above plus `dae`.  The mass matrix comes from the problem -- a hiprtc snippet
 * compiled with IVP_RHS_HAS_MASS (n <= 8) or IVP_RHS_HAS_MASS_COL (8 < n <= 64; both below) -- and is evaluated once per
 * trajectory, as the reference calls f.mass() once
 * (radau.rs:358-359); a problem without the hook is solved with the identity, and gives what ivp_radau_solve*() gives.
 * ivp_radau_dae_t is the reference's nind1 / nind2 / nind3 (Option<usize> each: has_x = 0 means None), validated by its rules
 * in its order (radau.rs:210-246): none given -- nind1 = n (a pure ODE partition; dae == NULL means the same); nind1 omitted
 * -- inferred as n - nind2 - nind3, IVP_ERR_INVALID_DAE_PARTITION if nind2 + nind3 > n; else the three must sum to n.  A
 * negative count (not expressible in the reference) gets the same error.  Variables are ordered index-1 first, then
 * index-2, then index-3; the error scale of an index-2 (index-3) variable is divided by the step ratio hhfac (hhfac^2)
 * on every attempt (radau.rs:435-444).  nind2 + nind3 > 0 for a problem WITHOUT a mass hook is IVP_ERR_BAD_ARGUMENT
 * ("not yet").  The refusals above (n > 64, events, FMA, variant = 3, banded storage and patterns beyond n = 8) apply
 * unchanged.  For 8 < n <= 64 a problem compiled with IVP_RHS_HAS_MASS_COL runs on the group kernels (one matrix row per
 * lane; M is a fifth n^2 block of the trajectory's matrices and is copied into LDS by every launch) with every output form
 * of the three calls; a pure index-1 partition of a larger problem without the hook takes the path of ivp_radau_solve*().
 * Deliberate deviation: a problem compiled with IVP_RHS_HAS_MASS or IVP_RHS_HAS_MASS_COL is refused (IVP_ERR_BAD_ARGUMENT) by every other entry
 * point, ivp_radau_solve*() included -- the reference's explicit methods and BDF ignore IVP::mass silently, which solves a
 * different equation without saying so.
 */
typedef struct {
    double uround;          /* 2.3e-16 */
    double safety_factor;   /* 0.9 */
    double scale_min;       /* 0.2 */
    double scale_max;       /* 8.0 */
    double newton_tol;      /* read when has_newton_tol != 0; else derived from the tolerances (radau.rs:198-205) */
    int32_t newton_maxiter; /* 7; at most 15 */
    int32_t has_newton_tol; /* 0 */
    int32_t predictive;     /* 1: Gustafsson controller */
    int32_t reserved;       /* 0 */
} ivp_radau_settings_t;

typedef struct {
    int32_t has_nind1, nind1;   /* index-1 variables (default: all) */
    int32_t has_nind2, nind2;   /* index-2 variables (default: 0)   */
    int32_t has_nind3, nind3;   /* index-3 variables (default: 0)   */
    int32_t reserved[2];        /* 0 */
} ivp_radau_dae_t;

void ivp_radau_settings_default(ivp_radau_settings_t *settings);
/* The validation of ivp_batch_solve*() (ivp_options_check) and of ivp_radau_solve*() (ivp_radau_check) on its own: no
 * context, no device.  Returns what the solve would return for these arguments before it touches the device; the text
 * ivp_last_error_string() would carry goes to message[message_len] (may be NULL). */
int ivp_options_check(const ivp_problem_t *prob, size_t B, const ivp_options_t *opt, char *message, size_t message_len);
int ivp_radau_check(const ivp_problem_t *prob, size_t B, const ivp_options_t *opt, const ivp_radau_settings_t *settings,
                    char *message, size_t message_len);
int ivp_radau_solve(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                    const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                    const ivp_radau_settings_t *settings, ivp_batch_result_t *out);
int ivp_radau_solve_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                           const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                           const ivp_radau_settings_t *settings, ivp_batch_result_t *out, void *hip_stream);
int ivp_radau_dae_check(const ivp_problem_t *prob, size_t B, const ivp_options_t *opt, const ivp_radau_settings_t *settings,
                        const ivp_radau_dae_t *dae, char *message, size_t message_len);
int ivp_radau_solve_dae(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                        const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                        const ivp_radau_settings_t *settings, const ivp_radau_dae_t *dae, ivp_batch_result_t *out);
int ivp_radau_solve_dae_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                               const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                               const ivp_radau_settings_t *settings, const ivp_radau_dae_t *dae, ivp_batch_result_t *out,
                               void *hip_stream);
/*
 * The direct Radau call in the resumable, the one-pass step log and the CSR dense forms (device pointers).  dae == NULL:
 * the rules of ivp_radau_solve_device (settings == NULL = the defaults, a problem with a mass matrix is refused); else
 * those of ivp_radau_solve_dae_device.  Every refusal of those two answers here with the same code and text.
 *   ivp_radau_submit_device        what ivp_batch_submit_device is to ivp_batch_solve_device; completed by ivp_batch_poll /
 *                                  ivp_batch_wait.  `settings` and `dae` are read before it returns: they may go out of
 *                                  scope while the solve is in flight (`out` and the input arrays may not).
 *   ivp_radau_solve_logged_device  the contract of ivp_batch_solve_logged_device below, member for member (reserve, defer,
 *                                  caller- or library-owned buffers, passes, pool_bytes, pool_used_bytes, the counted second
 *                                  integration when the pool runs dry); ivp_step_log_fetch_device / ivp_step_log_free apply.
 *   ivp_radau_solve_dense_device   the contract of ivp_batch_solve_dense_device below; ncoef_n = 4 n, and
 *                                  ivp_dense_eval_device(method = IVP_RADAU) evaluates the result.
 * (The latter two are declared below, behind ivp_step_log_t and ivp_dense_log_t.)
 */
int ivp_radau_submit_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                            const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                            const ivp_radau_settings_t *settings, const ivp_radau_dae_t *dae, ivp_batch_result_t *out,
                            void *hip_stream);
/*
 * Radau IIA(5) in BAND STORAGE: the direct call for a hiprtc problem compiled with IVP_RHS_BANDED (ivp_rhs_compile_sparse,
 * 8 < n <= 512, pure ODE, no event functions) -- and for nothing else: any other problem is IVP_ERR_BAD_ARGUMENT with a
 * message saying that this call has nothing to do for it.  Every entry point above keeps refusing such a problem ("not
 * yet"); this is its one way in.  Arguments, settings == NULL, results and every other refusal (event functions, fp_mode =
 * FMA, variant = 3, the ConfigErrors) are those of ivp_radau_check / ivp_radau_solve / ivp_radau_solve_device; there is no
 * DAE partition.  variant 0, 1 and 2 behave alike.  `out` carries what a plain Radau solve returns: end state, h_next,
 * status, the six counters, t_eval samples, the bounded step log, dense segments.
 * Layout (ml = max(row - col), mu = max(col - row) of the declared pattern, ivp_rhs_jac_layout; KD = ml + mu): one
 * contiguous block per trajectory in global memory holds J in LAPACK general-band form, WJ = ml + mu + 1 doubles per column
 * (entry (i, j) at j WJ + mu + i - j), then E1 = fac1 I - J, E2r = alphn I - J and E2i = betan I in the factor form, W =
 * 2 ml + mu + 1 doubles per column (entry (i, j) at j W + KD + i - j; the ml extra superdiagonals take the fill of row
 * exchanges): (WJ + 3 W) n doubles per trajectory instead of 4 n^2 -- 15 n for a tridiagonal system, 60 KB instead of
 * 8 MB at n = 512.  The Jacobian is formed by grouped forward differences (n_groups + 1 right-hand sides), E1 is factorised
 * by the band LU of the BDF path, E2 by its complex counterpart.  Nothing is kept in LDS across attempts, so the results do
 * not depend on chunk_attempts.
 * Contract: for a finite right-hand side and a pattern that contains every structurally non-zero entry, every result --
 * status, t_end, y_end, h_next, all six counters (Radau does not count Jacobian differences in nfev), t_eval samples, step
 * log and dense segments -- equals bit for bit what ivp_radau_solve*() gives for the same source compiled WITHOUT a pattern
 * (forward differences, full matrices).  Outside the claim, as for banded BDF: the sign of a zero and non-finite values.  A
 * pattern that omits non-zero entries is an error of the caller that is not detected.
 * Not here yet: the resumable, logged and CSR dense forms, event functions, mass matrices and DAE index sets, the
 * multi-device forms, n <= 8, an analytic jac_col.
 */
int ivp_radau_banded_check(const ivp_problem_t *prob, size_t B, const ivp_options_t *opt, const ivp_radau_settings_t *settings,
                           char *message, size_t message_len);
int ivp_radau_solve_banded(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                           const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                           const ivp_radau_settings_t *settings, ivp_batch_result_t *out);
int ivp_radau_solve_banded_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                                  const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                                  const ivp_radau_settings_t *settings, ivp_batch_result_t *out, void *hip_stream);

/*
 * Solution.t / Solution.y of B solve_ivp() calls in ONE call and ONE integration (ABI v5).
 *
 * Without Options.t_eval the reference records every accepted step while it integrates (DefaultSolOut mode 2,
 * src/solve/solout.rs:387-428) and hands the two growing Vecs back as Solution.t / Solution.y
 * (src/solve/solve_ivp.rs:288-312).  The entry points below do the same for a batch: the stepping kernels append each
 * accepted step to pages drawn from a device pool (one page per wavefront and 32 record slots, the records of one attempt
 * side by side, chained per trajectory), and once every trajectory has finished a gather kernel lays the records out as a
 * CSR log in trajectory order:
 *     trajectory b's k-th record:  t[offsets[b] + k],  y[(offsets[b] + k) * n + c]      (time-major like Vec<Vec<f64>>)
 * with offsets[B] = total.  `out` takes the end-state members / statistics as in ivp_batch_solve (its t_log / y_log /
 * log_offsets are ignored; n_log, if given, receives the counts); opt->t_eval must be NULL.  Everything else about the
 * solve (events, first_step enforcement, dense_output segments, every method and state dimension) is unchanged, and the
 * records are bit-identical to those of the dense [max_log] log and of the counted two-pass CSR log above.
 *
 * ivp_step_log_t -- who owns what:
 *   offsets   [B + 1], ALWAYS the caller's (device memory for the *_device / *_multi forms, host memory for the host form)
 *   t, y      the caller's buffers of `capacity` records, or both NULL: the library allocates exactly `total` records
 *             (hipMalloc on the context's / gather device, malloc for the host form), sets owned = 1, and the caller
 *             releases them with ivp_step_log_free() -- the C rendering of a Vec the callee returns
 *   reserve   in, optional: expected total number of records; sizes the page pool.  0 = automatic (the previous logged
 *             solve of this batch size on the context, else 1024 records per trajectory and at least 256 MB, never more
 *             than half of the free device memory).  A pool that runs dry is not an error: the solve is repeated as the counted fill pass
 *             (passes = 2), so a log is never truncated
 *   defer     in: 1 = integrate and count only (total, offsets and `out` are final on return); the records stay in the
 *             context's pool until its next solve and are fetched with ivp_step_log_fetch_device() into buffers the
 *             caller sizes from `total`.  "Its next solve" is ANY ivp_batch_submit_device / ivp_batch_solve* on the context,
 *             logged or not: every submit ends the life of the deferred log, and a fetch after it returns
 *             IVP_ERR_BAD_ARGUMENT ("no complete step log in this context's pool") without touching log->t / log->y
 * Returns IVP_ERR_LOG_CAPACITY (with total and offsets set) when the caller's t / y are too small; the records are then
 * still in the pool: enlarge the buffers and call ivp_step_log_fetch_device().
 */
typedef struct {
    uint64_t *offsets;
    double *t;
    double *y;
    uint64_t capacity;
    uint64_t reserve;
    int32_t defer;
    /* ---- out ---- */
    int32_t owned;        /* 1: t / y were allocated by the library                                           */
    int32_t device;       /* HIP device of owned device memory, -1 for host memory                             */
    uint32_t passes;      /* integrations it took: 1 (page pool) or 2 (the pool ran dry: counted fill pass)    */
    uint64_t total;       /* number of records = offsets[B]                                                    */
    uint64_t pool_bytes;       /* size of the page pool during the solve / bytes of it the pages took (records + the slots  */
    uint64_t pool_used_bytes;  /* of rejected attempts and retired lanes + column headers)                                  */
    uint32_t page_slots;       /* record slots per trajectory and page                                                      */
} ivp_step_log_t;

int ivp_batch_solve_logged_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0,
                                  const double *params, const double *t0, size_t t0_len, const double *t1,
                                  size_t t1_len, const ivp_options_t *opt, ivp_batch_result_t *out,
                                  ivp_step_log_t *log, void *hip_stream);
/* ... through the direct Radau call (see ivp_radau_submit_device): opt->method is ignored */
int ivp_radau_solve_logged_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                                  const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                                  const ivp_radau_settings_t *settings, const ivp_radau_dae_t *dae, ivp_batch_result_t *out,
                                  ivp_step_log_t *log, void *hip_stream);
/* the records of the context's last logged solve (defer = 1, or after IVP_ERR_LOG_CAPACITY) into log->t / log->y
 * (device memory, `capacity` records; both NULL: allocated here); log->offsets is not touched.  That solve must be the
 * context's LAST solve of any kind, else IVP_ERR_BAD_ARGUMENT; the same code with "the page pool ran dry ..." in
 * ivp_last_error_string() when its pool overflowed (the records are not all there: solve again) */
int ivp_step_log_fetch_device(ivp_ctx_t *ctx, ivp_step_log_t *log, void *hip_stream);
/* host pointers throughout (arguments as ivp_batch_solve; log->offsets / t / y are host memory) */
int ivp_batch_solve_logged(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0,
                           const double *params, const double *t0, size_t t0_len, const double *t1,
                           size_t t1_len, const ivp_options_t *opt, ivp_batch_result_t *out, ivp_step_log_t *log);
void ivp_step_log_free(ivp_step_log_t *log);

/*
 * Every trajectory's complete ContinuousOutput (Solution.sol / sol_many, src/solve/cont.rs:9-153, solution.rs:25-69) in
 * CSR form: the dense-output segments of B solve_ivp(.., Options.dense_output = true) calls without a cap.
 *
 *     trajectory b's k-th segment is record q = offsets[b] + k:  xold[q], h[q],
 *     cont[q * (ncoef * n) + ..]   ncoef = Method::coeffs_per_state; RK: [coef][component], BDF: per-state blocks
 *                                  [D0, D1..D5, order] (cont.rs:44-51)
 * exactly the segments the reference pushes (src/solve/solout.rs:141-146), in integration order, and the single constant
 * segment (h = 1e-15) of a zero-length interval.  The result takes sum(n_seg) x (2 + ncoef n) doubles.
 *
 * How: a counting solve (the solve itself: `out` receives every member as in ivp_batch_solve_device -- t_eval samples,
 * events, a bounded step log of opt->max_log records -- and n_seg, if given, the counts), an exclusive scan of the counts
 * into `offsets`, then the segments: from the counting solve's own block when every run fits opt->max_log (passes = 1),
 * else from a filling solve over trajectory ranges whose bounded blocks fit half of the free device memory, packed into
 * the CSR arrays (passes = 2).  out->seg_cont / seg_xold / seg_h must be NULL; opt->dense_output is implied.
 * PEAK device memory: the result plus that staging block, [max n_seg of the range][2 + ncoef n] doubles per trajectory
 * of a range (reported in staging_bytes; BASELINE C2: about 3x the result, as much as the bounded dense solve takes);
 * the environment variable IVP_DENSE_STAGING_BYTES caps the block, at the price of one filling solve per range.
 *
 * ivp_dense_log_t -- who owns what (as ivp_step_log_t):
 *   offsets   [B + 1], ALWAYS the caller's (device memory for the device form, host memory for the host form)
 *   cont, xold, h   the caller's buffers of `capacity` records, or all NULL: the library allocates exactly `total`
 *             records (hipMalloc on the context's device, malloc for the host form), sets owned = 1, and the caller
 *             releases them with ivp_dense_log_free()
 * Returns IVP_ERR_LOG_CAPACITY (with total and offsets set) when the caller's buffers are too small, IVP_ERR_HIP with a
 * message when the device has not the memory for the result or the staging: never a truncated log.
 */
typedef struct {
    uint64_t *offsets;
    double *cont;
    double *xold;
    double *h;
    uint64_t capacity;
    /* ---- out ---- */
    int32_t owned;            /* 1: cont / xold / h were allocated by the library                                   */
    int32_t device;           /* HIP device of owned device memory, -1 for host memory                             */
    uint32_t passes;          /* integrations it took: 1 (every run fitted the counting solve's block) or 2         */
    uint32_t ncoef_n;         /* doubles per record of cont                                                        */
    uint64_t total;           /* number of segments = offsets[B]                                                   */
    uint64_t staging_bytes;   /* largest bounded segment block a solve of this call wrote into                     */
} ivp_dense_log_t;

int ivp_batch_solve_dense_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0,
                                 const double *params, const double *t0, size_t t0_len, const double *t1,
                                 size_t t1_len, const ivp_options_t *opt, ivp_batch_result_t *out,
                                 ivp_dense_log_t *dense, void *hip_stream);
/* ... through the direct Radau call (see ivp_radau_submit_device): opt->method is ignored, cont is [c0, c1, c2, c3][component] */
int ivp_radau_solve_dense_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                                 const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                                 const ivp_radau_settings_t *settings, const ivp_radau_dae_t *dae, ivp_batch_result_t *out,
                                 ivp_dense_log_t *dense, void *hip_stream);
/* host pointers throughout (arguments as ivp_batch_solve; dense->offsets / cont / xold / h are host memory) */
int ivp_batch_solve_dense(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                          const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                          ivp_batch_result_t *out, ivp_dense_log_t *dense);
/* an owned device log (owned = 1, device >= 0) into the caller's device buffers of dense->total records, on hip_stream;
 * the owned memory is released and dense then points at the caller's buffers (owned = 0) */
int ivp_dense_log_fetch_device(ivp_dense_log_t *dense, double *cont, double *xold, double *h, void *hip_stream);
void ivp_dense_log_free(ivp_dense_log_t *dense);

/*
 * ContinuousOutput::evaluate (extrapolate == 0) / evaluate_extrapolate (extrapolate != 0), src/solve/cont.rs:104-153, of
 * every trajectory of a CSR dense log at query times, on the device (all arrays device memory, enqueued on hip_stream).
 *   t_offsets == NULL: one grid t[m] shared by the batch; y [m][n][B] (the SoA layout of a shared t_eval), found [m][B]
 *   t_offsets != NULL: [B + 1] offsets of per-trajectory grids concatenated in t[m], m = t_offsets[B]; y [m][n]
 *                      (time-major, the layout of per-trajectory t_eval), found [m]
 * found: 0 = no segment (y = NaN), 1 = inside a segment, 2 = extrapolated.  The segment is the reference's choice
 * (the first one with left - 1e-12 <= t <= right + 1e-12), found by binary search: a trajectory's run must be monotone
 * in its integration direction, as every run ivp_batch_solve_dense* writes is.  fp_mode: the interpolant of the
 * stepping kernels of that arithmetic (IVP_FP_STRICT: the crate's association).
 */
int ivp_dense_eval_device(ivp_ctx_t *ctx, int32_t method, int32_t n, int32_t fp_mode, size_t B, const uint64_t *offsets,
                          const double *cont, const double *xold, const double *h, const double *t,
                          const uint64_t *t_offsets, uint64_t m, int32_t extrapolate, double *y, int32_t *found,
                          void *hip_stream);

/*
 * Every trajectory's complete Solution.t_events / Solution.y_events (src/solve/solution.rs:10-11: Vecs that grow with
 * every occurrence, src/solve/solout.rs:158-331) in CSR form: the events of B solve_ivp() calls without the max_events cap.
 *
 *     the k-th occurrence of event i on trajectory b is record q = offsets[i * B + b] + k:  t[q],  y[q * n + c]
 * Runs are event-major (run r = i * B + b: all roots of event i over the batch are ONE contiguous slice,
 * offsets[i * B] .. offsets[(i + 1) * B)), records within a run in detection order; offsets[n_events * B] = total.
 * n_events * B may not exceed 4294967295; a problem without event functions is IVP_ERR_BAD_ARGUMENT.
 *
 * How: a counting solve (the solve itself: `out` receives every member as in ivp_batch_solve_device -- end state, t_eval
 * samples, bounded step log and dense segments -- and n_event_hits, if given, the counts) with a temporary block of
 * opt->max_events slots per event and trajectory (max_events = 0: count only), an exclusive scan of the counts into
 * `offsets`, then the records: from the counting solve's own block when every run fits opt->max_events (passes = 1, ONE
 * integration), else from a filling solve over trajectory ranges (t_eval, step log, dense output and profiling off) whose
 * bounded blocks, [n_events][max hits of the range][n + 1] doubles per trajectory, fit half of the free device memory,
 * packed into the CSR arrays (passes = 2).  out->t_events / y_events must be NULL: they are the bounded layout.
 * PEAK device memory: the result plus that staging block (reported in staging_bytes) plus the scratch of the solve that
 * fills it -- for explicit methods without a terminal event the deferred event refinement notes up to n_events * max_events
 * steps of 4 + 3 n_events + n + ncoef n doubles per trajectory (about six staging blocks for n = 6, DOPRI5) when a quarter
 * of the free memory holds them, and refines inline otherwise.  The environment variable IVP_EVENT_STAGING_BYTES caps
 * the staging block (and with it that scratch), at the price of one filling solve per range.
 *
 * ivp_event_log_t -- who owns what (as ivp_dense_log_t):
 *   offsets   [n_events * B + 1], ALWAYS the caller's (device memory for the device form, host memory for the host form)
 *   t, y      the caller's buffers of `capacity` records ([capacity], [capacity][n]), or both NULL: the library allocates
 *             exactly `total` records (hipMalloc on the context's device, malloc for the host form), sets owned = 1, and
 *             the caller releases them with ivp_event_log_free()
 * Returns IVP_ERR_LOG_CAPACITY (with total and offsets set) when the caller's buffers are too small, IVP_ERR_HIP with a
 * message when the device has not the memory for the result or the staging: never a truncated log.
 */
typedef struct {
    uint64_t *offsets;
    double *t;
    double *y;
    uint64_t capacity;
    /* ---- out ---- */
    int32_t owned;            /* 1: t / y were allocated by the library                                            */
    int32_t device;           /* HIP device of owned device memory, -1 for host memory                             */
    uint32_t passes;          /* integrations it took: 1 (every run fitted the counting solve's block) or 2         */
    uint32_t n_events;        /* event functions of the problem: offsets holds n_events * B + 1 entries            */
    uint64_t total;           /* number of records = offsets[n_events * B]                                         */
    uint64_t staging_bytes;   /* largest bounded event block a solve of this call wrote into                       */
} ivp_event_log_t;

int ivp_batch_solve_events_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0,
                                  const double *params, const double *t0, size_t t0_len, const double *t1,
                                  size_t t1_len, const ivp_options_t *opt, ivp_batch_result_t *out,
                                  ivp_event_log_t *ev, void *hip_stream);
/* host pointers throughout (arguments as ivp_batch_solve; ev->offsets / t / y are host memory) */
int ivp_batch_solve_events(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                           const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                           ivp_batch_result_t *out, ivp_event_log_t *ev);
/*
 * ... through the direct Radau call: the way in for Radau IIA(5) with event functions.  The contract above, member for
 * member (event-major runs, who owns t / y, IVP_ERR_LOG_CAPACITY, passes, staging_bytes, IVP_EVENT_STAGING_BYTES,
 * out->t_events / y_events NULL); `out` receives what the counting solve computes -- end state, counters, njev / nlu, t_eval
 * samples with the terminal event's appended sample (eval_idx = -1, t_term), the bounded step log with the terminal point
 * appended, dense segments, n_event_hits.  opt->method is ignored.  settings / dae follow ivp_radau_submit_device
 * (dae == NULL: the ODE rules, a problem with a mass matrix is refused); both are read before the first solve is
 * submitted and kept for the filling solves.  Radau refines every root inline, in the stepping kernels.
 * This is the ONLY Radau entry point that accepts a problem with event functions: ivp_radau_check, ivp_radau_dae_check and
 * every other ivp_radau_* call keep refusing one.  Refused here (IVP_ERR_BAD_ARGUMENT, before the device is touched), on
 * top of everything ivp_radau_solve_dae_device refuses: a problem without event functions, and n > 64 ("Radau with event
 * functions for n = %d: not yet (n <= 64)").  For 8 < n <= 64 the problem is a compiled component-form one without a mass
 * hook (IVP_RHS_HAS_MASS_COL cannot be compiled with event functions).  ivp_radau_events_check runs those checks alone.
 */
int ivp_radau_events_check(const ivp_problem_t *prob, size_t B, const ivp_options_t *opt, const ivp_radau_settings_t *settings,
                           const ivp_radau_dae_t *dae, char *message, size_t message_len);
int ivp_radau_solve_events_device(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                                  const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                                  const ivp_radau_settings_t *settings, const ivp_radau_dae_t *dae, ivp_batch_result_t *out,
                                  ivp_event_log_t *ev, void *hip_stream);
int ivp_radau_solve_events(ivp_ctx_t *ctx, const ivp_problem_t *prob, size_t B, const double *y0, const double *params,
                           const double *t0, size_t t0_len, const double *t1, size_t t1_len, const ivp_options_t *opt,
                           const ivp_radau_settings_t *settings, const ivp_radau_dae_t *dae, ivp_batch_result_t *out,
                           ivp_event_log_t *ev);
/* an owned device log (owned = 1, device >= 0) into the caller's device buffers of ev->total records, on hip_stream;
 * the owned memory is released and ev then points at the caller's buffers (owned = 0) */
int ivp_event_log_fetch_device(ivp_event_log_t *ev, double *t, double *y, void *hip_stream);
void ivp_event_log_free(ivp_event_log_t *ev);

/*
 * One batch over several devices.  The reference has no parallelism (a batch is B back-to-back solve_ivp() calls,
 * src/solve/solve_ivp.rs:99-313, with no coupling between them), so the batch shards by trajectory range: shard k is
 * integrated by its own context on its own device with no communication, and the only data movement is the final
 * gather of the result arrays.  ONE host thread drives all contexts through ivp_batch_submit_device / ivp_batch_poll.
 *
 * ivp_shard_t: trajectories [first, first + count) of a batch of B; every pointer is device memory on
 * ctx's device with SoA stride `count` (component c of the shard's i-th trajectory at a[c*count + i]); `out` members
 * may be NULL like in ivp_batch_solve_device.  count == 0 is allowed (the shard is skipped).
 *
 * ivp_batch_solve_multi: integrates all shards concurrently; when `gathered` is not NULL every member that is
 * non-NULL both in `gathered` and in a shard's `out` is copied into `gathered` (device memory on `gather_device`,
 * stride B) at column offset `first` -- same-device copies for shards that live on gather_device,
 * hipMemcpyPeerAsync / peer-enabled 2-D copies (xGMI) otherwise -- and the call returns when everything has landed.
 * Two contexts on ONE device are legal (the degenerate case the single-GPU tests run).
 * What travels is the reference's whole `Solution` (src/solve/solution.rs:7-20), not only the end states: the t_eval
 * samples (y_eval / eval_idx / n_filled), event records and dense [max_log] logs are SoA members like y_end; a CSR
 * step log (out.log_offsets / t_log / y_log per shard, offsets starting at 0 in the shard's own buffers: run the
 * counting pass first, options.count_log = 1, with out.n_log gathered) is gathered into gathered->t_log /
 * gathered->y_log in trajectory order, and gathered->log_offsets[B + 1] (device memory, written here) holds the shard
 * offsets re-based by the records of the shards before them.
 *
 * ivp_batch_solve_multi_host: host-pointer convenience form (arguments as ivp_batch_solve): splits the batch into
 * n_ctx contiguous balanced shards (the first B % n_ctx shards get one more), stages each to its context's device,
 * integrates concurrently and writes the results back into the caller's host arrays.
 */
typedef struct {
    ivp_ctx_t *ctx;
    size_t first, count;
    const double *y0;         /* [n][count]        */
    const double *params;     /* [n_params][count] */
    const double *t0;         /* [count] or [1]    */
    size_t t0_len;
    const double *t1;
    size_t t1_len;
    ivp_batch_result_t out;   /* stride count      */
    void *hip_stream;         /* stream on ctx's device, NULL = its default stream */
} ivp_shard_t;

int ivp_batch_solve_multi(ivp_shard_t *shards, int32_t n_shards, const ivp_problem_t *prob, size_t B,
                          const ivp_options_t *opt, int32_t gather_device, ivp_batch_result_t *gathered);
int ivp_batch_solve_multi_host(ivp_ctx_t *const *ctxs, int32_t n_ctx, const ivp_problem_t *prob, size_t B,
                               const double *y0, const double *params, const double *t0, size_t t0_len,
                               const double *t1, size_t t1_len, const ivp_options_t *opt, ivp_batch_result_t *out);
/*
 * ivp_batch_solve_multi + the one-pass step log (BASELINE config C4's "gather of sol.y": Solution.y is every accepted
 * step, src/solve/solution.rs:7-20): every shard integrates ONCE into its own context's page pool; afterwards each
 * shard's chains are laid out as one contiguous run of the batch-wide CSR log on gather_device -- directly by the
 * gather kernel for shards that live there, through a staging buffer and a peer copy (xGMI) otherwise -- in trajectory
 * order, and log->offsets [B + 1] (device memory on gather_device) holds the batch-wide offsets.  `gathered` takes the
 * SoA members as in ivp_batch_solve_multi (may be NULL); log->t / log->y as in ivp_batch_solve_logged_device
 * (gather_device memory; NULL = allocated there).  A shard whose pool ran dry repeats its solve as the counted fill pass.
 */
int ivp_batch_solve_logged_multi(ivp_shard_t *shards, int32_t n_shards, const ivp_problem_t *prob, size_t B,
                                 const ivp_options_t *opt, int32_t gather_device, ivp_batch_result_t *gathered,
                                 ivp_step_log_t *log);
/* log->defer = 1 in the call above: the records of every shard into log->t / log->y now (same shards, problem, options) */
int ivp_step_log_fetch_multi(ivp_shard_t *shards, int32_t n_shards, const ivp_problem_t *prob, size_t B,
                             const ivp_options_t *opt, int32_t gather_device, ivp_step_log_t *log);

/*
 * User-defined right-hand side: the device-side `impl IVP for T { fn ode(..) }` (src/ivp.rs:29).
 * `ode_source` is HIP device code defining
 *     __device__ void ode(double x, const double* y, double* dydx, const double* p);
 * for state dimension n <= 8 and n_params <= 16 parameters (the fields of the user's struct, one value of each per
 * trajectory); it is compiled with hiprtc for the context's
 * device and instantiates the same stepping kernels as the built-ins.  Free with ivp_rhs_free().
 * For 8 < n <= 512 (wave-per-trajectory kernels, see IVP_RHS_LINEAR_DECAY_100) the snippet defines the
 * component form instead -- y points at the whole state, the function returns dy_i/dx:
 *     __device__ double ode_comp(int i, double x, const double* y, const double* p);
 * (its events(), if any, keep the whole-state signature below).
 * Compiled code objects are cached on disk when the environment variable IVP_JIT_CACHE_DIR names an existing
 * directory (key: hash of the generated source, options and hiprtc version).
 * ivp_rhs_compile_events: the snippet additionally defines the trait's event functions
 *     __device__ void events(double x, const double* y, double* g, const double* p);   // g[0..n_events)
 * ivp_rhs_compile_ex: flags & IVP_RHS_HAS_JAC -- the snippet also overrides the trait's Jacobian (src/ivp.rs:67-107;
 * used by BDF instead of the default forward differences).  n <= 8: the whole matrix, row-major j[row*n + col],
 *     __device__ void jac(double x, const double* y, double* j, const double* p);
 * 8 < n <= 512 (one wavefront per trajectory): column form -- write column `col` of dF/dy into column[0..n),
 *     __device__ void jac_col(int col, double x, const double* y, double* column, const double* p);
 * Either way the storage starts zeroed and persists between calls like the reference's Matrix (bdf.rs:152): entries an
 * override never writes are 0.
 * flags & IVP_RHS_HAS_MASS (ivp_rhs_compile_ex only, n <= 8, not with IVP_RHS_BANDED) -- the snippet also defines the
 * trait's constant mass matrix (src/ivp.rs:111-120), row-major m[row*n + col]:
 *     __device__ void mass(double* m, const double* p);
 * m starts zeroed (entries the hook never writes are 0, like the reference's full Matrix); p holds the trajectory's
 * parameters, so M may differ per trajectory.  Read by ivp_radau_solve_dae*() only; every other entry point refuses such a
 * problem (see there).
 * flags & IVP_RHS_HAS_MASS_COL (ivp_rhs_compile_ex only, 8 < n <= 64, n_events == 0, alone or with IVP_RHS_HAS_JAC, not with
 * IVP_RHS_HAS_MASS) -- the column form of the same hook for a component-form snippet (ode_comp, optional jac_col), the exact
 * analogue of jac_col: write column `col` of M into column[0..n),
 *     __device__ void mass_col(int col, double* column, const double* p);
 * column[] is zeroed on entry (entries the hook never writes are 0); it is called once per column and trajectory.  Outside
 * those bounds the call is IVP_ERR_BAD_ARGUMENT with a message that names the flag and the bound (n <= 8: use
 * IVP_RHS_HAS_MASS).  A snippet whose mass_col does not compile is IVP_ERR_JIT.  The value is 16, not 8: 8 stays an
 * unknown flag of ivp_rhs_compile_ex, and ivp_rhs_compile_sparse knows neither mass flag.
 */
#define IVP_RHS_HAS_JAC 1u
#define IVP_RHS_HAS_MASS 4u
#define IVP_RHS_HAS_MASS_COL 16u
int ivp_rhs_compile(ivp_ctx_t *ctx, const char *ode_source, int32_t n, int32_t n_params, void **handle);
int ivp_rhs_compile_events(ivp_ctx_t *ctx, const char *source, int32_t n, int32_t n_params, int32_t n_events, void **handle);
int ivp_rhs_compile_ex(ivp_ctx_t *ctx, const char *source, int32_t n, int32_t n_params, int32_t n_events, uint32_t flags, void **handle);
void ivp_rhs_free(void *handle);

/*
 * Jacobian sparsity for BDF on 8 < n <= 512 (the reference's `jac_sparsity`, src/python/solve.rs:152-210 and
 * src/python/sparsity.rs): ivp_rhs_compile_ex plus a pattern of dF/dy in compressed sparse column form -- col_ptr[n + 1],
 * row_idx[col_ptr[n]]: rows col_ptr[c] .. col_ptr[c + 1] of row_idx are the rows of column c that may be non-zero.  ONE
 * pattern per compiled problem, shared by every trajectory of a batch.  The forward-difference Jacobian then perturbs
 * whole GROUPS of columns that share no declared row: n_groups + 1 evaluations of the right-hand side instead of n + 1.
 *   - Grouping is the reference's first-fit: columns in index order, each into the first group none of whose used rows
 *     it touches, else a new group (a column without rows joins group 0).  ivp_jac_sparsity_groups() returns it; it is a
 *     pure host function (no context, no device).
 *   - A pattern that contains every structurally non-zero entry gives the dense forward differences' matrix -- and so
 *     every result of the solve -- bit for bit, in both arithmetic modes, as long as the right-hand side stays finite.
 *     Entries outside the pattern are never written (they stay 0).  An under-declared pattern gives an approximate
 *     Jacobian, as in the reference: still deterministic, no longer equal to the dense solve.
 *   - IVP_ERR_BAD_ARGUMENT unless col_ptr[0] == 0, col_ptr is non-decreasing, every row index is in [0, n) and
 *     8 < n <= 512.  Duplicate rows within a column are accepted.
 *   - With IVP_RHS_HAS_JAC the snippet's jac_col wins and the pattern is ignored (ivp_wrapper.rs:245-258).
 *   - The pattern is compiled into the BDF code objects as constant tables: 2 n (n_groups + 1) bytes (3 KB for a
 *     tridiagonal system at n = 512; 512 KB in the worst case, n = 512 with n groups).  Explicit methods ignore it.
 *
 * Banded storage: flags & IVP_RHS_BANDED (ivp_rhs_compile_sparse only) is the reference's
 * `jac_storage = MatrixStorage::Banded{ml, mu}` (src/solve/options.rs:104-108) with ml = max(row - col) and
 * mu = max(col - row) over the declared entries (ivp_jac_sparsity_bandwidth(): pure host, same validation and error codes
 * as ivp_jac_sparsity_groups(); an empty or diagonal pattern gives (0, 0)).  BDF then stores J and the factors of
 * (I - cJ) by bands and factorises / solves with banded kernels whose factors stay in LDS whenever they fit.
 *   - Layout (LAPACK general band, column-major, one contiguous block per trajectory): J entry (i, j) at
 *     j (ml + mu + 1) + (mu + i - j); factor entry (i, j), j - ml - mu <= i <= j + ml, at j W + (ml + mu + i - j) with
 *     W = 2 ml + mu + 1 (the ml extra superdiagonals take the fill of row exchanges).  ivp_rhs_jac_layout() reports the
 *     per-trajectory sizes of any compiled problem: n n twice (dense), or (ml + mu + 1) n and (2 ml + mu + 1) n.
 *   - Contract: for a finite right-hand side and a pattern that contains every structurally non-zero entry, every result
 *     of the solve equals the dense solve with the same pattern bit for bit, in both arithmetic modes and for any chunk
 *     length.  Outside the claim: the sign of a zero (the dense solves add (+-0) b[k] to out-of-band rows, which turns a
 *     -0.0 there into +0.0; banded leaves it) and non-finite values (0 * inf outside the band).
 *   - IVP_ERR_BAD_ARGUMENT (message in ivp_last_error_string) when n <= 8, when combined with IVP_RHS_HAS_JAC (an
 *     analytic jac_col in band storage is not supported), and when 2 ml + mu + 1 >= n (the band is as wide as the matrix).
 *   - ivp_options_t.variant == 1 keeps the banded factors in global memory; 0 and 2 keep them in LDS when they fit.
 */
#define IVP_RHS_BANDED 2u
int ivp_jac_sparsity_bandwidth(int32_t n, const int32_t *col_ptr, const int32_t *row_idx, int32_t *ml_out, int32_t *mu_out);
int ivp_rhs_jac_layout(const void *handle, int32_t *banded, int32_t *ml, int32_t *mu, uint64_t *jac_doubles, uint64_t *lu_doubles);
int ivp_jac_sparsity_groups(int32_t n, const int32_t *col_ptr, const int32_t *row_idx, int32_t *groups_out /* [n] */, int32_t *n_groups_out);
int ivp_rhs_compile_sparse(ivp_ctx_t *ctx, const char *source, int32_t n, int32_t n_params, int32_t n_events, uint32_t flags,
                           const int32_t *col_ptr, const int32_t *row_idx, void **handle);

#ifdef __cplusplus
}
#endif
#endif /* IVP_HIP_H */
