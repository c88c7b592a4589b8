// ivp_balance.h -- balanced bulk rounds: how the attempts of one round are cut into launches so that every wave slot of the
// device steps the same number of attempts per launch.  Plain integer functions, host and device, no HIP types: the
// schedule is a pure function of four numbers and is tested on the CPU (tests/helpers/balance_plan_main.cpp).
//
// A thread-per-trajectory wave saturates the f64 pipe of its SIMD on its own (ivp_kargs.h, `window`), so a launch lasts as
// long as the busiest SIMD's queue: a round of R attempts for nb blocks of 64 list entries on S wave slots cannot take less
// than nb R / S attempt-times, and takes more whenever a launch leaves slots idle.  The plan lays the round's work on a line:
//
//     nb R units; block b owns units [b R, (b + 1) R)          (one unit = one attempt of one block)
//     L launches, quota q = ceil(nb R / (S L)) units per workgroup and launch
//     segment s = units [s q, (s + 1) q); workgroup s / L runs it in launch s % L
//
// Consecutive segments fall into different launches, so a block that meets at most L segments is touched by at most one
// workgroup per launch: its pieces are plain "n more attempts", taken in launch order, and no workgroup ever waits for
// another.  L is the smallest count >= ceil(nb R / (S chunk)) (no launch longer than `chunk` attempts) with
// ceil(R / q) + 1 <= L; q <= chunk <= R then, so a segment meets at most two blocks and a workgroup runs at most two
// pieces, (b1, n1) and (b1 + 1, q - n1).  BASELINE C2 (nb = 1563, R = 192, S = 1024, chunk = 64): L = 5, q = 59, 5087 of the
// 5120 workgroup slots used.
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#ifndef IVP_BAL_HD
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define IVP_BAL_HD __host__ __device__ inline
#else
#define IVP_BAL_HD inline
#endif
#endif

// the plan of one round; L == 0: not applicable (the caller keeps its windows or full launches)
struct IvpBalancePlan {
    uint32_t L;   // launches of the round
    uint32_t q;   // quota: attempts per workgroup and launch
    uint32_t W;   // workgroups per launch (<= S)
};

// The condition under which the launch loop cuts a launch down to whole multiples of one wave per slot (`window`): the list
// holds one to four slot-fulls and its last, ragged wave-round would be less than ~80 % full.  Returns the window in lanes
// (a multiple of 64 S) or 0.
constexpr IVP_BAL_HD uint32_t ivp_balance_window(uint32_t lanes, uint32_t S)
{
    const uint64_t one = (uint64_t)S * 64u;
    if (one == 0u || one > 0xFFFFFFFFull) return 0u;
    const uint64_t full = lanes / one;
    if (full >= 1u && full < 4u && (uint64_t)lanes * 5u < (full + 1u) * one * 4u) return (uint32_t)(full * one);
    return 0u;
}

// nb = ceil(lanes / 64) blocks, R attempts per trajectory in the round, S wave slots, `chunk` = longest launch in attempts.
constexpr IVP_BAL_HD IvpBalancePlan ivp_balance_plan(uint32_t lanes, uint32_t R, uint32_t S, uint32_t chunk)
{
    IvpBalancePlan none = {0u, 0u, 0u};
    if (S == 0u || chunk == 0u || R < chunk || R > 0xFFFFu) return none;
    if (ivp_balance_window(lanes, S) == 0u) return none;
    const uint64_t nb = ((uint64_t)lanes + 63u) / 64u, total = nb * R;
    const uint64_t lower = (total + (uint64_t)S * chunk - 1u) / ((uint64_t)S * chunk);
    for (uint64_t L = lower; L <= 2u * lower && L <= 255u; ++L) {
        const uint64_t q = (total + (uint64_t)S * L - 1u) / ((uint64_t)S * L);
        if ((R + q - 1u) / q + 1u <= L) {
            const uint64_t segs = (total + q - 1u) / q;
            IvpBalancePlan p = {(uint32_t)L, (uint32_t)q, (uint32_t)((segs + L - 1u) / L)};
            return p;
        }
    }
    return none;
}

// One piece: `n` attempts for block `b`; `last`: no later launch of the round touches the block, so this piece appends the
// block's survivors to the round's output list.
struct IvpBalancePiece {
    uint32_t b, n;
    bool last;
};

// the launch (0 .. L - 1) that holds the last piece of block b: the highest s % L over the segments the block meets
constexpr IVP_BAL_HD uint32_t ivp_balance_last_launch(uint32_t b, uint32_t R, uint32_t q, uint32_t L)
{
    const uint64_t s_lo = (uint64_t)b * R / q, s_hi = ((uint64_t)(b + 1u) * R - 1u) / q;
    // at most L consecutive segments: either they wrap past a multiple of L (then one of them sits in launch L - 1) or
    // their launches rise with s
    if (s_lo / L != s_hi / L) return L - 1u;
    return (uint32_t)(s_hi % L);
}

// The pieces of workgroup w in launch l (0, 1 or 2 of them, returned in out[]; the count is the return value).
constexpr IVP_BAL_HD uint32_t ivp_balance_pieces(uint32_t w, uint32_t l, uint32_t nb, uint32_t R, uint32_t q, uint32_t L, IvpBalancePiece out[2])
{
    const uint64_t total = (uint64_t)nb * R;
    uint64_t u = ((uint64_t)w * L + l) * q;
    const uint64_t uend = u + q < total ? u + q : total;
    uint32_t k = 0;
    while (u < uend && k < 2u) {
        const uint64_t b = u / R, bend = (b + 1u) * R;
        const uint64_t n = (uend < bend ? uend : bend) - u;
        out[k].b = (uint32_t)b;
        out[k].n = (uint32_t)n;
        out[k].last = ivp_balance_last_launch((uint32_t)b, R, q, L) == l;
        u += n;
        ++k;
    }
    return k;
}

// The plan's scalars of one launch as the kernel receives them: IvpKArgs.chunk carries q, IvpKArgs.balance this word
// (R << 16 | L << 8 | l; L >= 2 whenever a plan applies, so 0 means "not a balanced launch").
constexpr IVP_BAL_HD uint32_t ivp_balance_pack(uint32_t R, uint32_t L, uint32_t l) { return (R << 16) | (L << 8) | l; }
constexpr IVP_BAL_HD uint32_t ivp_balance_R(uint32_t word) { return word >> 16; }
constexpr IVP_BAL_HD uint32_t ivp_balance_L(uint32_t word) { return (word >> 8) & 0xFFu; }
constexpr IVP_BAL_HD uint32_t ivp_balance_l(uint32_t word) { return word & 0xFFu; }
