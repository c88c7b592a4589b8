// event_pack.h -- index arithmetic of the CSR event log (include/ivp_hip.h, ivp_event_log_t), shared by the tiled pack
// kernel, its one-lane-per-trajectory fallback (event_pack.hip) and the host test (tests/test_events_csr_cpu.py builds
// this header with `#define IVP_HD inline`).
//
//   source       the bounded block a solve of trajectories [first, first + cnt) wrote (IvpKArgs.t_events / y_events):
//                    t_events[(i * cap + k) * cnt + j]            k-th occurrence of event i on the range's j-th trajectory
//                    y_events[((i * cap + k) * n + c) * cnt + j]  SoA over the range
//   destination  the contiguous run r = i * B + first + j of the batch-wide log (event-major):
//                    t[off[r] + k],  y[(off[r] + k) * n + c]
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef IVP_HD
#error "define IVP_HD (__host__ __device__ __forceinline__ for hipcc, inline for a host build) before including event_pack.h"
#endif

IVP_HD size_t event_src_t(uint32_t i, uint32_t k, size_t j, uint32_t cap, size_t cnt) { return ((size_t)i * cap + k) * cnt + j; }
IVP_HD size_t event_src_y(uint32_t i, uint32_t k, uint32_t c, size_t j, uint32_t cap, uint32_t n, size_t cnt)
{
    return (((size_t)i * cap + k) * n + c) * cnt + j;
}
// run of event i on trajectory first + j of a batch of B, and the range's own count of it ([n_events][cnt])
IVP_HD size_t event_run(uint32_t i, size_t first, size_t j, size_t B) { return (size_t)i * B + first + j; }
IVP_HD size_t event_hits_at(uint32_t i, size_t j, size_t cnt) { return (size_t)i * cnt + j; }
IVP_HD size_t event_dst_t(unsigned long long lo, uint32_t k) { return (size_t)lo + k; }
IVP_HD size_t event_dst_y(unsigned long long lo, uint32_t k, uint32_t c, uint32_t n) { return ((size_t)lo + k) * n + c; }

// records a run receives: never more than the block holds, never past the run's end
IVP_HD uint32_t event_pack_count(uint32_t hits, uint32_t cap, unsigned long long room)
{
    unsigned long long m = hits < cap ? hits : cap;
    m = m < room ? m : room;
    return (uint32_t)m;
}
// the solve that wrote the block did not reproduce the count the run was sized for, or the block did not hold it all
IVP_HD bool event_pack_mismatch(uint32_t hits, uint32_t cap, unsigned long long room) { return hits != room || hits > cap; }

// one run, record by record: the fallback kernel's body (records k = k_first, k_first + k_step, ..) and the host
// test's whole pack (k_first = 0, k_step = 1).  Returns whether the run's count is inconsistent.
IVP_HD bool event_pack_run(const double *st_t, const double *st_y, const uint32_t *hits, const unsigned long long *off, double *t, double *y,
                           uint32_t i, size_t j, size_t first, size_t cnt, size_t B, uint32_t cap, uint32_t n, uint32_t k_first, uint32_t k_step)
{
    const size_t r = event_run(i, first, j, B);
    const unsigned long long lo = off[r], room = off[r + 1] - lo;
    const uint32_t h = hits[event_hits_at(i, j, cnt)], m = event_pack_count(h, cap, room);
    for (uint32_t k = k_first; k < m; k += k_step) {
        t[event_dst_t(lo, k)] = st_t[event_src_t(i, k, j, cap, cnt)];
        for (uint32_t c = 0; c < n; ++c) y[event_dst_y(lo, k, c, n)] = st_y[event_src_y(i, k, c, j, cap, n, cnt)];
    }
    return event_pack_mismatch(h, cap, room);
}
