// dense_kernels.h -- host entry points of dense_eval.hip (batch dense output: CSR packing and device evaluation).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// Query times against the CSR dense-output log (include/ivp_hip.h, ivp_dense_log_t).
struct DenseEvalArgs {
    const unsigned long long *off;   // [B + 1] segment offsets
    const double *cont;              // [total][ncoef * n]
    const double *xold;              // [total]
    const double *h;                 // [total]
    const double *t;                 // shared grid [m] (t_off == NULL) or concatenated per-trajectory grids [nq]
    const unsigned long long *t_off; // [B + 1] query offsets, or NULL = one grid shared by the batch
    unsigned long long nq;           // queries: m * B (shared grid) or t_off[B]
    unsigned long long B;
    double *y;                       // [m][n][B] (shared grid) or [nq][n]
    int32_t *found;                  // [m][B] or [nq]: 0 no segment, 1 inside one, 2 extrapolated
    int32_t n;
    int32_t extrapolate;
    int32_t wide;                    // cont is 16-byte aligned: the n <= 8 kernels read coefficient pairs
};

// the segments of trajectories [0, count) of a filling solve's bounded block ([max_log][nc][count], [max_log][count]) into
// their CSR runs off[i] .. off[i + 1) (off points at the batch-wide offsets of the block's first trajectory)
struct DensePackArgs {
    const double *st_cont;
    const double *st_xold;
    const double *st_h;
    const uint32_t *n_seg;           // [count] segments the filling solve produced
    const unsigned long long *off;   // [count + 1]
    double *cont;
    double *xold;
    double *h;
    uint32_t *err;                   // device word: bit 0 = some count differs from its run
    uint32_t count;
    uint32_t max_log;
    uint32_t nc;
};

hipError_t ivp_dense_eval_strict(int method, const DenseEvalArgs &e, hipStream_t s);
hipError_t ivp_dense_eval_fast(int method, const DenseEvalArgs &e, hipStream_t s);
hipError_t ivp_dense_pack(const DensePackArgs &p, hipStream_t s);
