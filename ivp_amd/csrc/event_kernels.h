// event_kernels.h -- host entry point of event_pack.hip (unbounded batch event output: the bounded block -> CSR runs).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// The event occurrences of trajectories [first, first + cnt) of a batch of B, as a solve of that range left them in its
// bounded block (layout: event_pack.h), into their runs off[i * B + first + j] of the batch-wide CSR log.
struct EventPackArgs {
    const double *st_t;              // [n_events][cap][cnt]
    const double *st_y;              // [n_events][cap][n][cnt]
    const uint32_t *hits;            // [n_events][cnt] occurrences that solve detected
    const unsigned long long *off;   // [n_events * B + 1], batch-wide
    double *t;                       // [total]
    double *y;                       // [total][n]
    uint32_t *err;                   // device word: bit 0 = some count differs from its run's length or exceeds cap
    unsigned long long B, first;
    uint32_t cnt, cap, n, n_events;
};

hipError_t ivp_event_pack(const EventPackArgs &p, hipStream_t s);

// Measurement hook (tools/bench_events_csr.py times the pack kernel alone through it; not part of the C ABI of
// include/ivp_hip.h): ivp_event_pack(*args, stream) when args_bytes == sizeof(EventPackArgs), else -1 without a launch,
// so that a caller whose copy of the struct has gone stale is told instead of passing garbage.
extern "C" int ivp_event_pack_timing_hook(const EventPackArgs *args, size_t args_bytes, void *hip_stream);
