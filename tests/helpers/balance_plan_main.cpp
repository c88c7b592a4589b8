// balance_plan_main.cpp -- TEST-ONLY stand-alone program: sweeps the balanced-round plan of ivp_amd/csrc/ivp_balance.h and checks,
// for every plan it declares applicable, the properties the kernel and the launch loop rely on.  Host only, no GPU; built with
// -fsanitize=address,undefined by tests/test_balance_plan_cpu.py.  Prints one line per failure and a summary; exit status 0 = all held.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ivp_amd/csrc/ivp_balance.h"

static long failures = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            if (++failures <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                      \
    } while (0)

// the rules of the plan restated on their own: 0 = not applicable
static uint32_t expected_L(uint64_t lanes, uint64_t R, uint64_t S, uint64_t chunk)
{
    const uint64_t one = 64 * S, full = lanes / one;
    const bool windowed = full >= 1 && full < 4 && lanes * 5 < (full + 1) * one * 4;
    if (!windowed || R < chunk) return 0;
    const uint64_t nb = (lanes + 63) / 64, work = nb * R;
    uint64_t lower = work / (S * chunk);
    if (lower * S * chunk < work) ++lower;
    for (uint64_t L = lower; L <= 2 * lower; ++L) {
        uint64_t q = work / (S * L);
        if (q * S * L < work) ++q;
        uint64_t pieces = R / q;
        if (pieces * q < R) ++pieces;
        if (pieces + 1 <= L) return (uint32_t)L;
    }
    return 0;
}

static void check_plan(uint32_t lanes, uint32_t R, uint32_t S, uint32_t chunk, long &applicable, long &declined)
{
    const IvpBalancePlan p = ivp_balance_plan(lanes, R, S, chunk);
    const uint32_t want = expected_L(lanes, R, S, chunk);
    CHECK(p.L == want, "lanes %u R %u S %u chunk %u: L = %u, the rules give %u", lanes, R, S, chunk, p.L, want);
    if (p.L == 0) { ++declined; CHECK(p.q == 0 && p.W == 0, "a declined plan carries q = %u W = %u", p.q, p.W); return; }
    ++applicable;
    const uint32_t nb = (lanes + 63u) / 64u, L = p.L, q = p.q;
    const uint64_t total = (uint64_t)nb * R;
    CHECK(q >= 1 && q <= chunk && q <= R, "lanes %u R %u S %u chunk %u: q = %u", lanes, R, S, chunk, q);
    CHECK(p.W >= 1 && p.W <= S, "lanes %u R %u S %u chunk %u: W = %u", lanes, R, S, chunk, p.W);
    CHECK((uint64_t)p.W * L * q >= total, "lanes %u R %u S %u chunk %u: %u x %u x %u does not cover %llu", lanes, R, S, chunk, p.W, L, q, (unsigned long long)total);
    CHECK((uint64_t)S * L * (q - 1u) < total, "lanes %u R %u S %u chunk %u: q = %u is not the smallest quota", lanes, R, S, chunk, q);
    CHECK(ivp_balance_R(ivp_balance_pack(R, L, L - 1u)) == R && ivp_balance_L(ivp_balance_pack(R, L, L - 1u)) == L && ivp_balance_l(ivp_balance_pack(R, L, L - 1u)) == L - 1u,
          "lanes %u R %u S %u chunk %u: the packed word loses L = %u", lanes, R, S, chunk, L);

    std::vector<uint32_t> got(nb, 0u), seen_in(nb, 0xFFFFFFFFu), last_launch(nb, 0u), lasts(nb, 0u), highest(nb, 0u);
    for (uint32_t l = 0; l < L; ++l) {
        uint32_t lo = 0xFFFFFFFFu, hi = 0u;
        // one workgroup past the grid as well: it must have nothing to do
        for (uint32_t w = 0; w <= p.W; ++w) {
            IvpBalancePiece pc[2];
            const uint32_t k = ivp_balance_pieces(w, l, nb, R, q, L, pc);
            if (w == p.W) { CHECK(k == 0, "lanes %u R %u S %u chunk %u: work beyond the grid in launch %u", lanes, R, S, chunk, l); continue; }
            uint32_t load = 0;
            for (uint32_t i = 0; i < k; ++i) {
                const uint32_t b = pc[i].b;
                CHECK(b < nb && pc[i].n >= 1, "lanes %u R %u S %u chunk %u: piece (%u, %u)", lanes, R, S, chunk, b, pc[i].n);
                if (b >= nb) continue;
                CHECK(seen_in[b] != l, "lanes %u R %u S %u chunk %u: block %u twice in launch %u", lanes, R, S, chunk, b, l);
                seen_in[b] = l;
                got[b] += pc[i].n;
                highest[b] = l;   // launches are walked in rising order
                if (pc[i].last) { lasts[b] += 1; last_launch[b] = l; }
                load += pc[i].n;
            }
            if (k == 2) CHECK(pc[1].b == pc[0].b + 1u, "lanes %u R %u S %u chunk %u: pieces of blocks %u and %u in one workgroup", lanes, R, S, chunk, pc[0].b, pc[1].b);
            CHECK(load <= q, "lanes %u R %u S %u chunk %u: workgroup %u of launch %u steps %u > q = %u", lanes, R, S, chunk, w, l, load, q);
            // the work line is cut front to back: only the segment that holds its end, and the empty ones behind it, are short,
            // and they all belong to the trailing workgroup
            CHECK(load == q || w == p.W - 1u, "lanes %u R %u S %u chunk %u: workgroup %u of %u steps %u < q = %u in launch %u", lanes, R, S, chunk, w, p.W, load, q, l);
            lo = load < lo ? load : lo;
            hi = load > hi ? load : hi;
        }
        CHECK(hi - lo <= q, "lanes %u R %u S %u chunk %u: loads %u .. %u in launch %u", lanes, R, S, chunk, lo, hi, l);
    }
    for (uint32_t b = 0; b < nb; ++b) {
        CHECK(got[b] == R, "lanes %u R %u S %u chunk %u: block %u gets %u attempts", lanes, R, S, chunk, b, got[b]);
        CHECK(lasts[b] == 1u && last_launch[b] == highest[b] && ivp_balance_last_launch(b, R, q, L) == highest[b],
              "lanes %u R %u S %u chunk %u: block %u: %u last pieces, in launch %u, highest launch %u", lanes, R, S, chunk, b, lasts[b], last_launch[b], highest[b]);
    }
}

int main()
{
    const uint32_t Ss[] = {1, 2, 3, 4, 7, 1024}, Rs[] = {64, 192, 256}, chunks[] = {16, 64};
    long applicable = 0, declined = 0;
    for (uint32_t S : Ss)
        for (uint32_t R : Rs)
            for (uint32_t chunk : chunks)
                for (uint32_t nb = 1; nb <= 6000; ++nb) {
                    check_plan(nb * 64u, R, S, chunk, applicable, declined);
                    check_plan(nb * 64u - 63u, R, S, chunk, applicable, declined);   // a last block with one entry
                }
    // BASELINE C2: 100 000 trajectories on 1024 wave slots, three launches of 64 attempts per poll
    {
        const IvpBalancePlan p = ivp_balance_plan(100000u, 192u, 1024u, 64u);
        CHECK(p.L == 5u && p.q == 59u && p.W == 1018u, "C2: L = %u q = %u W = %u", p.L, p.q, p.W);
        const uint64_t segs = ((uint64_t)1563 * 192 + p.q - 1) / (p.q ? p.q : 1);
        CHECK(segs == 5087u, "C2: %llu segments", (unsigned long long)segs);
    }
    // not applicable, and said so: no window (too few, too many, or a last wave-round that is nearly full), R < chunk, no slots
    CHECK(ivp_balance_plan(63u * 64u, 192u, 1024u, 64u).L == 0u, "below one slot-full");
    CHECK(ivp_balance_plan(4096u * 64u, 192u, 1024u, 64u).L == 0u, "four slot-fulls");
    CHECK(ivp_balance_plan(1900u * 64u, 192u, 1024u, 64u).L == 0u, "a last round more than 80 %% full");
    CHECK(ivp_balance_plan(100000u, 32u, 1024u, 64u).L == 0u, "R < chunk");
    CHECK(ivp_balance_plan(100000u, 192u, 0u, 64u).L == 0u, "S = 0");
    CHECK(ivp_balance_plan(100000u, 192u, 1024u, 0u).L == 0u, "chunk = 0");
    CHECK(ivp_balance_plan(443u, 192u, 4u, 64u).L == 0u, "443 entries on 4 slots: the last round is 87 %% full");
    CHECK(ivp_balance_plan(15u * 64u + 1u, 192u, 4u, 64u).L == 0u, "961 entries on 4 slots");
    CHECK(ivp_balance_plan(443u, 192u, 5u, 64u).L != 0u, "443 entries on 5 slots");
    CHECK(ivp_balance_plan(320u, 192u, 4u, 64u).L != 0u, "320 entries on 4 slots");
    std::printf("balance plan: %ld applicable, %ld not applicable, %ld failures\n", applicable, declined, failures);
    return failures == 0 && applicable > 0 && declined > 0 ? 0 : 1;
}
