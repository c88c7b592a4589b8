// ivp_csr.h -- PRIVATE: the one staging driver behind the CSR logs that are counted first and filled afterwards, the dense
// log (ivp_dense.cpp) and the event log (ivp_events.cpp).  Both are the same program (ivp_csr.cpp):
//   1. the counting solve: the caller's solve with a bounded block of `depth` slots per run -- it delivers every other
//      output of `out` and counts every run's records (the counts keep counting past the block);
//   2. exclusive scan of the counts -> offsets, total (ivp_log_scan, log_gather.hip);
//   3. destination = the caller's buffers if they hold `total` records, else library-owned;
//   4. the records: packed straight from the counting solve's block when every run fitted it (passes = 1), else a filling
//      solve over trajectory ranges whose bounded blocks fit the staging budget, each block packed into its CSR runs by the
//      kind's pack kernel, which also checks that the filling solve reproduced every count (passes = 2).
// What differs between the kinds is the CsrKind below; ivp_dense.cpp and ivp_events.cpp fill one in per call.
#pragma once
#include "ivp_ctx.h"

#include <functional>

namespace ivp_host {

// the arrays of a CSR log, each `width[i]` doubles per record (dense: cont, xold, h; events: t, y)
constexpr int kCsrArrays = 3;
struct CsrArrays { double *p[kCsrArrays] = {nullptr, nullptr, nullptr}; };

// the batch as every entry point receives it, plus what validate() made of the problem
struct CsrInputs {
    const ivp_problem_t *prob;
    size_t B;
    const double *y0, *params, *t0;
    size_t t0_len;
    const double *t1;
    size_t t1_len;
    int n, np;
};

struct CsrKind {
    const char *name;                              // message prefix: "dense output" / "event output"
    const char *staging_env;                       // environment variable that caps a staging block, read on every call
    size_t runs_per_traj;                          // runs are [runs_per_traj][B]; a trajectory needs its LARGEST run's slots
    uint32_t *ivp_batch_result_t::*counts;         // n_seg / n_event_hits
    uint32_t ivp_options_t::*depth;                // max_log / max_events: the slots per run of a bounded block
    size_t rec;                                    // bytes of one slot of every run of one trajectory
    int narrays;
    size_t width[kCsrArrays];
    ivp_options_t count_opt, fill_opt;             // count_opt.*depth slots in the counting block (0: none); fill_opt.*depth is set per range
    RadauCall *rad = nullptr;                      // the direct Radau call behind every solve, or NULL
    // the log's own members
    uint64_t *offsets, *capacity, *total, *staging_bytes;
    uint32_t *passes;
    CsrArrays given;                               // the caller's buffers (all NULL: the library allocates)
    // r's bounded members of this kind -> a block of `depth` slots for `cnt` trajectories
    std::function<void(ivp_batch_result_t &r, double *block, size_t depth, size_t cnt)> bind;
    // the pack kernel: r's block of trajectories [first, first + cnt) of the batch -> their runs in `dst` (device memory)
    std::function<hipError_t(const ivp_batch_result_t &r, const unsigned long long *off, const CsrArrays &dst, uint32_t *err, size_t first,
                             size_t cnt, uint32_t depth, hipStream_t s)> pack;
    // ... and on the host, from the counting block of the whole batch; false: the counts do not match the offsets
    std::function<bool(const ivp_batch_result_t &r, const uint32_t *counts, const CsrArrays &dst)> pack_host;
    // the log takes ownership of arrays the library allocated (device >= 0: hipMalloc there, -1: malloc)
    std::function<int(const CsrArrays &a, uint64_t capacity, int device)> adopt;
};

// what a host-pointer entry point asks of its arrays (the device forms leave that to the solve)
int check_host_inputs(ivp_ctx *ctx, const CsrInputs &in);
// steps 1 - 4 on device pointers (ctx's device is current) and on host pointers (the counting solve is ivp_batch_solve, or --
// k.rad -- the host form of the direct Radau call: ivp_host::solve_host)
int csr_solve_device(ivp_ctx *ctx, const CsrKind &k, const CsrInputs &in, ivp_batch_result_t *out, hipStream_t s);
int csr_solve_host(ivp_ctx *ctx, const CsrKind &k, const CsrInputs &in, ivp_batch_result_t *out);

}  // namespace ivp_host
