// event_pack.hip -- gfx950 kernels of the unbounded batch event output (ivp_batch_solve_events*; host side in
// ivp_events.cpp, layout in include/ivp_hip.h, index arithmetic in event_pack.h):
//   event_pack_kernel   the occurrences a solve left in its bounded [n_events][cap][1 + n][cnt] block -> the CSR log
//                       (record off[i * B + b] + k, the state contiguous per record)
//   event_pack_lanes    the same for records wider than the LDS tile (the wave-per-trajectory systems)
// Pure data movement, no arithmetic: one build serves both arithmetic modes.
#include <hip/hip_runtime.h>

#include <algorithm>

#define IVP_HD __host__ __device__ __forceinline__
#include "ivp_kargs.h"
#include "event_pack.h"
#include "event_kernels.h"

namespace {

// The bounded block is SoA (one trajectory's record is strided by `cnt`), the CSR run of (event, trajectory) is
// contiguous.  The shape dense_pack_kernel settled on (dense_eval.hip): a workgroup takes 64 trajectories of one event and
// kk records at a time through LDS, reads the tile with coalesced 512-byte rows (64 trajectories of one component) and
// writes every trajectory's kk records as one contiguous run, one wave per 16 trajectories.  LDS row stride 65 doubles:
// the run-order reads hit distinct banks.  A run receives event_pack_count() records, so nothing lands outside it; a
// count that differs from the run's length raises *err.  grid: x = trajectory tiles, y = record blocks, z = events.
constexpr int kPackThreads = 256, kPackCols = 64, kPackLd = kPackCols + 1;
__global__ __launch_bounds__(kPackThreads) void event_pack_kernel(EventPackArgs p, uint32_t kk)
{
    extern __shared__ double tile[];   // [kk][n + 1][kPackLd]: the state, then the time
    __shared__ unsigned long long lo_s[kPackCols];
    __shared__ uint32_t km_s[kPackCols];
    __shared__ uint32_t kmax_blk;
    const uint32_t tid = threadIdx.x, j0 = blockIdx.x * kPackCols, ev = blockIdx.z, n = p.n, rows = n + 1, cap = p.cap;
    const size_t cnt = p.cnt;
    if (tid == 0) kmax_blk = 0;
    __syncthreads();
    if (tid < kPackCols) {
        const size_t j = (size_t)j0 + tid;
        unsigned long long lo = 0;
        uint32_t km = 0;
        if (j < cnt) {
            const size_t r = event_run(ev, (size_t)p.first, j, (size_t)p.B);
            lo = p.off[r];
            const unsigned long long room = p.off[r + 1] - lo;
            const uint32_t h = p.hits[event_hits_at(ev, j, cnt)];
            if (blockIdx.y == 0 && event_pack_mismatch(h, cap, room)) atomicOr(p.err, 1u);
            km = event_pack_count(h, cap, room);
        }
        lo_s[tid] = lo;
        km_s[tid] = km;
        atomicMax(&kmax_blk, km);
    }
    __syncthreads();
    const uint32_t kmax = kmax_blk;
    for (uint32_t k0 = blockIdx.y * kk; k0 < kmax; k0 += gridDim.y * kk) {
        // ---- read: element e = (r, c, l) of the tile, l fastest: coalesced over trajectories ----
        const uint32_t elems = kk * rows * kPackCols;
        for (uint32_t e = tid; e < elems; e += kPackThreads) {
            const uint32_t l = e % kPackCols, rc = e / kPackCols, c = rc % rows, r = rc / rows, k = k0 + r;
            const size_t j = (size_t)j0 + l;
            double v = 0.0;
            if (j < cnt && k < km_s[l]) v = c < n ? p.st_y[event_src_y(ev, k, c, j, cap, n, cnt)] : p.st_t[event_src_t(ev, k, j, cap, cnt)];
            tile[((size_t)r * rows + c) * kPackLd + l] = v;
        }
        __syncthreads();
        // ---- write: each wave takes 16 trajectories; a trajectory's records k0 .. k0 + m as one contiguous run ----
        const uint32_t wave = tid / IVP_WAVE, lane = tid % IVP_WAVE;
        for (uint32_t l = wave; l < kPackCols; l += kPackThreads / IVP_WAVE) {
            const uint32_t km = km_s[l];
            if (k0 >= km) continue;
            const uint32_t m = km - k0 < kk ? km - k0 : kk;
            const unsigned long long lo = lo_s[l];
            const size_t y0 = event_dst_y(lo, k0, 0, n);
            for (uint32_t e = lane; e < m * n; e += IVP_WAVE) {
                const uint32_t r = e / n, c = e % n;
                p.y[y0 + e] = tile[((size_t)r * rows + c) * kPackLd + l];
            }
            for (uint32_t r = lane; r < m; r += IVP_WAVE) p.t[event_dst_t(lo, k0 + r)] = tile[((size_t)r * rows + n) * kPackLd + l];
        }
        __syncthreads();
    }
}

// Records wider than the LDS tile allows (n + 1 > 94: wave-per-trajectory systems): one lane per trajectory copies its
// records, occurrences strided over grid.y; the same bounds and count check (event_pack_run).
__global__ __launch_bounds__(IVP_WAVE) void event_pack_lanes(EventPackArgs p)
{
    const size_t j = (size_t)blockIdx.x * IVP_WAVE + threadIdx.x;
    if (j >= p.cnt) return;
    const bool bad = event_pack_run(p.st_t, p.st_y, p.hits, p.off, p.t, p.y, blockIdx.z, j, (size_t)p.first, p.cnt, (size_t)p.B, p.cap, p.n,
                                    blockIdx.y, gridDim.y);
    if (bad && blockIdx.y == 0) atomicOr(p.err, 1u);
}

}  // namespace

extern "C" int ivp_event_pack_timing_hook(const EventPackArgs *args, size_t args_bytes, void *hip_stream)
{
    if (!args || args_bytes != sizeof(EventPackArgs)) return -1;
    return (int)ivp_event_pack(*args, (hipStream_t)hip_stream);
}

hipError_t ivp_event_pack(const EventPackArgs &p, hipStream_t s)
{
    if (p.cnt == 0 || p.cap == 0 || p.n_events == 0) return hipSuccess;
    if (p.n_events > 65535u) return hipErrorInvalidValue;
    // records per tile: as many as 48 KB of LDS hold, at most 8 (C2, n = 6: 8 records = 29 KB)
    const size_t row_bytes = (size_t)(p.n + 1) * kPackLd * sizeof(double);
    const uint32_t kk = (uint32_t)std::min<size_t>(8, (48u << 10) / row_bytes);
    (void)hipGetLastError();
    if (kk == 0) {
        const dim3 grid((p.cnt + IVP_WAVE - 1) / IVP_WAVE, p.cap < 256u ? p.cap : 256u, p.n_events), block(IVP_WAVE);
        hipLaunchKernelGGL(event_pack_lanes, grid, block, 0, s, p);
        return hipGetLastError();
    }
    const uint32_t ky = std::min<uint32_t>((p.cap + kk - 1) / kk, 64u);
    const dim3 grid((p.cnt + kPackCols - 1) / kPackCols, ky, p.n_events), block(kPackThreads);
    hipLaunchKernelGGL(event_pack_kernel, grid, block, (size_t)kk * row_bytes, s, p, kk);
    return hipGetLastError();
}
