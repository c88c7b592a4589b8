// ivp_csr_plan.h -- the trajectory ranges of a CSR log's filling solve (ivp_csr.cpp).  A plain function of integers, no HIP
// types: tested on the CPU (tests/helpers/csr_plan_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

// One range [first, first + cnt) and the depth `cap` of its bounded block: every trajectory of the range gets `cap` slots
// of `rec` bytes, so the block takes cap * rec * cnt bytes.
struct IvpCsrRange {
    size_t cnt;
    uint32_t cap;   // max(largest need of the range, 1)
};

// The longest range from `first` whose block fits `budget` bytes; need[b]: slots trajectory b fills.  A range always takes
// at least one trajectory, whatever its block costs (the caller checks that against the free memory).  first < B.
inline IvpCsrRange ivp_csr_plan_range(const uint32_t *need, size_t first, size_t B, size_t rec, size_t budget)
{
    IvpCsrRange r = {0, 0};
    while (first + r.cnt < B) {
        const uint32_t one = need[first + r.cnt] > 1u ? need[first + r.cnt] : 1u, cap = one > r.cap ? one : r.cap;
        if (r.cnt > 0 && (size_t)cap * rec * (r.cnt + 1) > budget) break;
        r.cap = cap;
        ++r.cnt;
    }
    return r;
}
