// csr_plan_main.cpp -- TEST-ONLY stand-alone program: sweeps the range planner of the CSR logs' filling solve
// (ivp_amd/csrc/ivp_csr_plan.h) and checks the properties that determine the greedy plan uniquely.  Host only, no GPU; built
// with -fsanitize=address,undefined by tests/test_csr_plan_cpu.py.  Prints one line per failure and a summary; exit status
// 0 = all held.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ivp_amd/csrc/ivp_csr_plan.h"

static long failures = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            if (++failures <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                      \
    } while (0)

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// the needs of a batch: 0 all zero, 1 all one, 2 small (0 .. 7), 3 small with one large outlier, 4 a mix of 0, 1, small
// and one large outlier
static std::vector<uint32_t> needs(int pattern, size_t B, uint32_t seed)
{
    std::vector<uint32_t> v(B, 0u);
    for (size_t b = 0; b < B; ++b) {
        const uint32_t r = lcg(seed);
        if (pattern == 1) v[b] = 1;
        if (pattern == 2 || pattern == 3) v[b] = r % 8u;
        if (pattern == 4) v[b] = (r & 3u) == 0u ? 0u : (r & 3u) == 1u ? 1u : (r >> 2) % 40u;
    }
    if (pattern >= 3) v[lcg(seed) % B] = 5000u;
    return v;
}

// all ranges of one batch; returns how many
static long check_batch(const std::vector<uint32_t> &need, size_t rec, size_t budget, int pattern)
{
    const size_t B = need.size();
    long ranges = 0;
    size_t first = 0;
    while (first < B) {
        const IvpCsrRange g = ivp_csr_plan_range(need.data(), first, B, rec, budget);
        CHECK(g.cnt >= 1 && first + g.cnt <= B, "pattern %d B %zu rec %zu budget %zu first %zu: cnt %zu", pattern, B, rec, budget, first, g.cnt);
        if (g.cnt < 1 || first + g.cnt > B) return ranges;   // the ranges no longer tile [0, B)
        const uint32_t most = std::max(*std::max_element(need.begin() + first, need.begin() + first + g.cnt), 1u);
        CHECK(g.cap == most, "pattern %d B %zu rec %zu budget %zu first %zu: cap %u, largest need %u", pattern, B, rec, budget, first, g.cap, most);
        if (g.cnt > 1)
            CHECK((size_t)g.cap * rec * g.cnt <= budget, "pattern %d B %zu rec %zu budget %zu first %zu: %zu trajectories x %u slots", pattern, B, rec,
                  budget, first, g.cnt, g.cap);
        if (first + g.cnt < B) {   // maximal: the next trajectory would not have fitted
            const uint32_t with_next = std::max(most, std::max(need[first + g.cnt], 1u));
            CHECK((size_t)with_next * rec * (g.cnt + 1) > budget, "pattern %d B %zu rec %zu budget %zu first %zu: %zu trajectories, one more fits", pattern,
                  B, rec, budget, first, g.cnt);
        }
        first += g.cnt;   // in order, no gap, no overlap
        ++ranges;
    }
    CHECK(first == B, "pattern %d B %zu rec %zu budget %zu: ranges end at %zu", pattern, B, rec, budget, first);
    return ranges;
}

int main()
{
    const size_t recs[] = {8, 56, 264, 4096};   // one double; 1 event x (6 + 1) doubles; (5 x 6 + 2 + 1) doubles; a wide record
    long cases = 0, ranges = 0, split = 0, whole = 0, singles = 0;
    for (size_t B = 1; B <= 200; ++B)
        for (int pattern = 0; pattern < 5; ++pattern) {
            const std::vector<uint32_t> need = needs(pattern, B, (uint32_t)(B * 5 + pattern));
            const size_t most = std::max(*std::max_element(need.begin(), need.end()), 1u);
            for (size_t rec : recs) {
                const size_t all = most * rec * B;   // the block of the whole batch in one range
                const size_t budgets[] = {1, rec - 1, rec, 3 * rec, all / 7, all / 3, all / 2, all - 1, all, all + 1, 2 * all};
                for (size_t budget : budgets) {
                    if (budget == 0) continue;
                    const long k = check_batch(need, rec, budget, pattern);
                    ++cases;
                    ranges += k;
                    split += k > 1;
                    whole += k == 1;
                    singles += (size_t)k == B;
                    if (budget >= all) CHECK(k == 1, "pattern %d B %zu rec %zu budget %zu: %ld ranges for a batch that fits", pattern, B, rec, budget, k);
                    if (budget < rec) CHECK((size_t)k == B, "pattern %d B %zu rec %zu budget %zu: %ld ranges below one record", pattern, B, rec, budget, k);
                }
            }
        }
    std::printf("csr plan: %ld cases, %ld ranges, %ld split, %ld whole, %ld one-per-trajectory, %ld failures\n", cases, ranges, split, whole, singles, failures);
    return failures == 0 ? 0 : 1;
}
