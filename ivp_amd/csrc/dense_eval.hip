// dense_eval.hip -- gfx950 kernels of the batch dense output (ivp_batch_solve_dense*, ivp_dense_eval_device; host side in
// ivp_dense.cpp, layout in include/ivp_hip.h):
//   dense_pack_kernel   the segments a filling solve left in its bounded [max_log][ncoef n][count] block -> the CSR log
//                       (record offsets[b] + k, coefficients contiguous per record)
//   dense_eval_*        ContinuousOutput::evaluate / evaluate_extrapolate (src/solve/cont.rs:104-153) of every trajectory
//                       at query times: binary search over the trajectory's run (dense_eval.h), then the stepping kernels'
//                       own interpolate<M, 1> per component
//
// Compiled twice like rk_kernels.hip: -DIVP_FAST=0 (strict: the crate's association) and -DIVP_FAST=1 (the fused
// interpolant the FMA kernels use for t_eval); both -ffp-contract=off.  The pack kernel does no arithmetic and lives in
// the strict build only.
#include <hip/hip_runtime.h>

#include <algorithm>

#define IVP_HD __host__ __device__ __forceinline__
#if IVP_FAST
#define IVP_NS ivp_fast
#define IVP_DENSE_EVAL_NAME ivp_dense_eval_fast
#else
#define IVP_NS ivp_strict
#define IVP_DENSE_EVAL_NAME ivp_dense_eval_strict
#endif
#include "rk_core.h"
#include "dense_eval.h"
#include "dense_kernels.h"

namespace {

using namespace IVP_NS;

constexpr int kEvalThreads = 256;

// query g -> (trajectory, time, first output element, stride between components)
struct Query { uint32_t b; double t; size_t y0, ys; };
__device__ __forceinline__ Query dense_query(const DenseEvalArgs &e, unsigned long long g, int n)
{
    Query r;
    if (e.t_off == nullptr) {   // shared grid t[m]: query g = k * B + b, y [m][n][B], found [m][B]
        const unsigned long long k = g / e.B;
        r.b = (uint32_t)(g - k * e.B);
        r.t = e.t[k];
        r.y0 = (size_t)k * (size_t)n * e.B + r.b;
        r.ys = e.B;
    } else {                    // per-trajectory grids (CSR): trajectory = last b with t_off[b] <= g, y [total][n]
        uint32_t lo = 0, hi = (uint32_t)e.B;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (e.t_off[mid] <= g) lo = mid; else hi = mid - 1;
        }
        r.b = lo;
        r.t = e.t[g];
        r.y0 = (size_t)g * (size_t)n;
        r.ys = 1;
    }
    return r;
}

// n <= 8: one lane per query; the segment's coefficient block (ncoef n doubles, contiguous) comes in with 16-byte loads
template <int M, int N>
__global__ __launch_bounds__(kEvalThreads) void dense_eval_lane(DenseEvalArgs e)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * kEvalThreads + threadIdx.x;
    if (g >= e.nq) return;
    const Query qy = dense_query(e, g, N);
    const unsigned long long lo = e.off[qy.b], cnt = e.off[qy.b + 1] - lo;
    unsigned long long q = 0;
    const int f = dense_find(e.xold, e.h, lo, cnt, qy.t, e.extrapolate, &q);
    e.found[g] = f;
    if (f == IVP_DENSE_NONE) {
#pragma unroll
        for (int c = 0; c < N; ++c) e.y[qy.y0 + (size_t)c * qy.ys] = __builtin_nan("");
        return;
    }
    constexpr int NC = NCoef<M>::v * N;
    double r[NC];
    const double *seg = e.cont + q * NC;
    if (NC % 2 == 0 && e.wide) {
        const double2 *s2 = reinterpret_cast<const double2 *>(seg);
#pragma unroll
        for (int i = 0; i < NC / 2; ++i) { const double2 v = s2[i]; r[2 * i] = v.x; r[2 * i + 1] = v.y; }
    } else {
#pragma unroll
        for (int i = 0; i < NC; ++i) r[i] = seg[i];
    }
    const double xo = e.xold[q], hh = e.h[q];
#pragma unroll
    for (int c = 0; c < N; ++c) e.y[qy.y0 + (size_t)c * qy.ys] = dense_component<M>(dense_comp_view<M>(r, N, c), qy.t, xo, hh);
}

// 8 < n <= 512: one wavefront per query; its first lane searches, every lane interpolates components lane, lane + 64, ..
template <int M>
__global__ __launch_bounds__(kEvalThreads) void dense_eval_wave(DenseEvalArgs e)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * (kEvalThreads / IVP_WAVE) + threadIdx.x / IVP_WAVE;
    if (g >= e.nq) return;   // wave-uniform
    const int lane = (int)(threadIdx.x % IVP_WAVE), n = e.n;
    const Query qy = dense_query(e, g, n);
    int f = IVP_DENSE_NONE;
    unsigned long long q = 0;
    if (lane == 0) {
        const unsigned long long lo = e.off[qy.b], cnt = e.off[qy.b + 1] - lo;
        f = dense_find(e.xold, e.h, lo, cnt, qy.t, e.extrapolate, &q);
        e.found[g] = f;
    }
    f = __shfl(f, 0);
    q = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(q >> 32), 0) << 32) | (uint32_t)__shfl((int)(uint32_t)q, 0);
    if (f == IVP_DENSE_NONE) {
        for (int c = lane; c < n; c += IVP_WAVE) e.y[qy.y0 + (size_t)c * qy.ys] = __builtin_nan("");
        return;
    }
    const double *seg = e.cont + q * (size_t)(NCoef<M>::v * n);
    const double xo = e.xold[q], hh = e.h[q];
    for (int c = lane; c < n; c += IVP_WAVE) e.y[qy.y0 + (size_t)c * qy.ys] = dense_component<M>(dense_comp_view<M>(seg, n, c), qy.t, xo, hh);
}

template <int M>
hipError_t launch_eval(const DenseEvalArgs &e, hipStream_t s)
{
    (void)hipGetLastError();
    if (e.n > IVP_MAX_N) {
        const unsigned long long per = kEvalThreads / IVP_WAVE;
        hipLaunchKernelGGL((dense_eval_wave<M>), dim3((unsigned)((e.nq + per - 1) / per)), dim3(kEvalThreads), 0, s, e);
        return hipGetLastError();
    }
    const dim3 grid((unsigned)((e.nq + kEvalThreads - 1) / kEvalThreads)), block(kEvalThreads);
    switch (e.n) {
    case 1: hipLaunchKernelGGL((dense_eval_lane<M, 1>), grid, block, 0, s, e); break;
    case 2: hipLaunchKernelGGL((dense_eval_lane<M, 2>), grid, block, 0, s, e); break;
    case 3: hipLaunchKernelGGL((dense_eval_lane<M, 3>), grid, block, 0, s, e); break;
    case 4: hipLaunchKernelGGL((dense_eval_lane<M, 4>), grid, block, 0, s, e); break;
    case 5: hipLaunchKernelGGL((dense_eval_lane<M, 5>), grid, block, 0, s, e); break;
    case 6: hipLaunchKernelGGL((dense_eval_lane<M, 6>), grid, block, 0, s, e); break;
    case 7: hipLaunchKernelGGL((dense_eval_lane<M, 7>), grid, block, 0, s, e); break;
    case 8: hipLaunchKernelGGL((dense_eval_lane<M, 8>), grid, block, 0, s, e); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

#if !IVP_FAST
// The bounded block is SoA ([k][c][i]: one trajectory's record is strided by `count`), the CSR run of a trajectory is
// contiguous.  A workgroup takes 64 trajectories and kk records at a time through LDS: it reads the tile with
// coalesced 512-byte rows (64 trajectories of one coefficient) and writes every trajectory's kk records as one
// contiguous run.  (One lane per trajectory writing its own records scattered every store over 64 records: 9.2 ms for
// BASELINE C2's 4.3 GB, half of the CSR solve.)  A trajectory writes min(its count, its CSR room off[i + 1] - off[i])
// records, so nothing lands outside its run; a count that differs from the run's length (the filling solve did not
// reproduce the counting solve) raises *err.  LDS row stride 65 doubles: the run-order reads hit distinct banks.
constexpr int kPackThreads = 256, kPackCols = 64, kPackLd = kPackCols + 1;
__global__ __launch_bounds__(kPackThreads) void dense_pack_kernel(DensePackArgs p, uint32_t kk)
{
    extern __shared__ double tile[];   // [kk][nc + 2][kPackLd]: coefficients, then xold, then h
    __shared__ unsigned long long lo_s[kPackCols];
    __shared__ uint32_t km_s[kPackCols];
    __shared__ uint32_t kmax_blk;
    const uint32_t tid = threadIdx.x, i0 = blockIdx.x * kPackCols, nc = p.nc, rows = nc + 2;
    if (tid == 0) kmax_blk = 0;
    __syncthreads();
    if (tid < kPackCols) {
        const uint32_t i = i0 + tid;
        unsigned long long lo = 0, km = 0;
        if (i < p.count) {
            lo = p.off[i];
            const unsigned long long room = p.off[i + 1] - lo;
            const uint32_t ns = p.n_seg[i];
            if (blockIdx.y == 0 && (ns != room || ns > p.max_log)) atomicOr(p.err, 1u);
            km = ns < p.max_log ? ns : p.max_log;
            km = km < room ? km : room;
        }
        lo_s[tid] = lo;
        km_s[tid] = (uint32_t)km;
        atomicMax(&kmax_blk, (uint32_t)km);
    }
    __syncthreads();
    const uint32_t kmax = kmax_blk;
    const size_t cnt = p.count;
    for (uint32_t k0 = blockIdx.y * kk; k0 < kmax; k0 += gridDim.y * kk) {
        // ---- read: element e = (r, c, l) of the tile, l fastest: coalesced over trajectories ----
        const uint32_t elems = kk * rows * kPackCols;
        for (uint32_t e = tid; e < elems; e += kPackThreads) {
            const uint32_t l = e % kPackCols, rc = e / kPackCols, c = rc % rows, r = rc / rows, k = k0 + r, i = i0 + l;
            double v = 0.0;
            if (i < cnt && k < km_s[l]) {
                if (c < nc) v = p.st_cont[((size_t)k * nc + c) * cnt + i];
                else if (c == nc) v = p.st_xold[(size_t)k * cnt + i];
                else v = p.st_h[(size_t)k * cnt + i];
            }
            tile[((size_t)r * rows + c) * kPackLd + l] = v;
        }
        __syncthreads();
        // ---- write: each wave takes 16 trajectories; a trajectory's records k0 .. k0 + m as one contiguous run ----
        const uint32_t wave = tid / IVP_WAVE, lane = tid % IVP_WAVE;
        for (uint32_t l = wave; l < kPackCols; l += kPackThreads / IVP_WAVE) {
            const uint32_t km = km_s[l];
            if (k0 >= km) continue;
            const uint32_t m = km - k0 < kk ? km - k0 : kk;
            const size_t q0 = (size_t)lo_s[l] + k0;
            for (uint32_t e = lane; e < m * nc; e += IVP_WAVE) {
                const uint32_t r = e / nc, c = e % nc;
                p.cont[q0 * nc + e] = tile[((size_t)r * rows + c) * kPackLd + l];
            }
            for (uint32_t r = lane; r < m; r += IVP_WAVE) {
                p.xold[q0 + r] = tile[((size_t)r * rows + nc) * kPackLd + l];
                p.h[q0 + r] = tile[((size_t)r * rows + nc + 1) * kPackLd + l];
            }
        }
        __syncthreads();
    }
}
// Records wider than the LDS tile allows (the wave-per-trajectory systems, ncoef n > 90): one lane per trajectory copies
// its records, segments strided over grid.y; the same bounds and count check.
__global__ __launch_bounds__(IVP_WAVE) void dense_pack_lanes(DensePackArgs p)
{
    const uint32_t i = blockIdx.x * IVP_WAVE + threadIdx.x;
    if (i >= p.count) return;
    const unsigned long long lo = p.off[i], room = p.off[i + 1] - lo;
    const uint32_t ns = p.n_seg[i];
    if (blockIdx.y == 0 && (ns != room || ns > p.max_log)) atomicOr(p.err, 1u);
    unsigned long long kmax = ns < p.max_log ? ns : p.max_log;
    kmax = kmax < room ? kmax : room;
    const size_t cnt = p.count, nc = p.nc;
    for (unsigned long long k = blockIdx.y; k < kmax; k += gridDim.y) {
        const size_t q = (size_t)(lo + k);
        p.xold[q] = p.st_xold[(size_t)k * cnt + i];
        p.h[q] = p.st_h[(size_t)k * cnt + i];
        for (size_t c = 0; c < nc; ++c) p.cont[q * nc + c] = p.st_cont[((size_t)k * nc + c) * cnt + i];
    }
}
#endif

}  // namespace

hipError_t IVP_DENSE_EVAL_NAME(int method, const DenseEvalArgs &e, hipStream_t s)
{
    if (e.nq == 0) return hipSuccess;
    switch (method) {
    case M_RK23: return launch_eval<M_RK23>(e, s);
    case M_DOPRI5: return launch_eval<M_DOPRI5>(e, s);
    case M_DOP853: return launch_eval<M_DOP853>(e, s);
    case M_RK4: return launch_eval<M_RK4>(e, s);
    case M_BDF: return launch_eval<M_BDF>(e, s);
    case M_RADAU: return launch_eval<M_RADAU>(e, s);
    }
    return hipErrorInvalidValue;
}

#if !IVP_FAST
hipError_t ivp_dense_pack(const DensePackArgs &p, hipStream_t s)
{
    if (p.count == 0 || p.max_log == 0) return hipSuccess;
    // records per tile: as many as 48 KB of LDS hold, at most 8 (C2, ncoef n = 30: 2 records = 33 KB)
    const size_t row_bytes = (size_t)(p.nc + 2) * kPackLd * sizeof(double);
    const uint32_t kk = (uint32_t)std::min<size_t>(8, (48u << 10) / row_bytes);
    (void)hipGetLastError();
    if (kk == 0) {
        const dim3 grid((p.count + IVP_WAVE - 1) / IVP_WAVE, p.max_log < 256u ? p.max_log : 256u), block(IVP_WAVE);
        hipLaunchKernelGGL(dense_pack_lanes, grid, block, 0, s, p);
        return hipGetLastError();
    }
    const uint32_t ky = std::min<uint32_t>((p.max_log + kk - 1) / kk, 64u);
    const dim3 grid((p.count + kPackCols - 1) / kPackCols, ky), block(kPackThreads);
    hipLaunchKernelGGL(dense_pack_kernel, grid, block, (size_t)kk * row_bytes, s, p, kk);
    return hipGetLastError();
}
#endif
