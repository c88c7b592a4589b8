// ubench_dpp64.hip -- what does moving a double between lanes cost a lone wave on gfx950: one v_mov_b64_dpp
// (row_newbcast, the only lane select the 64-bit form has) against the pair of v_mov_b32_dpp?
// Build: hipcc -O3 --offload-arch=gfx950 tools/ubench_dpp64.hip -o tools/ubench_dpp64 ; run on the MI355X.
// The cooperative tail kernels (ivp_amd/csrc/rk_coop.h) run at most one wave per SIMD, so every instruction of the wave's
// stream -- an s_nop that fills a hazard included -- is an issue slot (tools/ubench_issue.hip, tools/ubench_latency.hip).
// A DPP mov must not read a VGPR within two instructions of the VALU instruction that wrote it; the chains below keep that
// distance with the s_nop the compiler would insert, so the hazard is never violated and the cost of the wait states in
// front of each form is part of what is measured:
//   independent movs             issue cost of the mov itself
//   dependent movs + s_nop 1     a hop that feeds the next hop (broadcast after hop, second half of a group broadcast)
// and the two spellings of rk_coop.h's group broadcast, each followed by a v_add_f64 that feeds the next broadcast (a
// value that was just computed is the usual source in an attempt), compiled from the builtins -- the compiler places the s_nop:
//   quad_perm pair + row_shr/row_shl pair with a bank mask (4 x v_mov_b32_dpp, plus the copies that protect `old`)
//   row_newbcast:i whole row + row_newbcast:8+i upper half (2 x v_mov_b64_dpp)
// Reported: ns per item of ONE wave, for a lone wave (grid 1) and one wave per SIMD (grid 1024).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int ITER = 2000;
#define REP4(X) X X X X
#define REP8(X) REP4(X) REP4(X)
#define REP16(X) REP8(X) REP8(X)
#define REP32(X) REP16(X) REP16(X)

__device__ __forceinline__ double u2d(unsigned long long u) { return __builtin_bit_cast(double, u); }
__device__ __forceinline__ unsigned long long d2u(double d) { return __builtin_bit_cast(unsigned long long, d); }
template <int CTRL, int BANK, bool ALL>
__device__ __forceinline__ double dpp32x2(double old, double src)
{
    const unsigned long long o = d2u(old), s = d2u(src);
    const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)o, (int)(unsigned)s, CTRL, 0xF, BANK, ALL);
    const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(o >> 32), (int)(unsigned)(s >> 32), CTRL, 0xF, BANK, ALL);
    return u2d(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}
// lane 1 of every 8-lane group to its eight lanes, as rk_coop.h spelled it with 32-bit movs ...
__device__ __forceinline__ double grp_bcast_b32(double v)
{
    const double t = dpp32x2<0x55, 0xF, true>(0.0, v);   // quad_perm:[1,1,1,1]
    return dpp32x2<0x114, 0xA, false>(t, t);            // row_shr:4 into lanes 4..7, lanes 0..3 keep t
}
// ... and with the 64-bit row broadcast
__device__ __forceinline__ double grp_bcast_b64(double v)
{
    const double t = __builtin_amdgcn_update_dpp(0.0, v, 0x151, 0xF, 0xF, true);   // row_newbcast:1
    return __builtin_amdgcn_update_dpp(t, v, 0x159, 0xF, 0xC, false);              // row_newbcast:9, lanes 8..15
}

template <int K>
__global__ __launch_bounds__(64) void k_dpp(double *out, double seed)
{
    double a = seed + threadIdx.x * 1e-9, b = a + 1.0, c = 1e-9;
    int al = __double2loint(a), ah = __double2hiint(a), bl = al + 1, bh = ah + 1;   // a double as a register pair, for the 32-bit movs
#define B64 "v_mov_b64_dpp %0, %1 row_newbcast:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
#define B32X2 "v_mov_b32_dpp %0, %2 quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n" \
              "v_mov_b32_dpp %1, %3 quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1"
    for (int it = 0; it < ITER; ++it) {
        if constexpr (K == 0) {          // independent: one v_mov_b64_dpp per double
            REP32(asm volatile(B64 : "=v"(b) : "v"(a));)
        } else if constexpr (K == 1) {   // independent: two v_mov_b32_dpp per double
            REP32(asm volatile(B32X2 : "=&v"(bl), "=&v"(bh) : "v"(al), "v"(ah));)
        } else if constexpr (K == 2) {   // dependent, two wait states in front: s_nop 1 + one v_mov_b64_dpp
            REP32(asm volatile("s_nop 1\n" B64 : "=&v"(b) : "v"(a)); asm volatile("s_nop 1\n" B64 : "=&v"(a) : "v"(b));)
        } else if constexpr (K == 3) {   // dependent, two wait states in front: s_nop 1 + two v_mov_b32_dpp
            REP32(asm volatile("s_nop 1\n" B32X2 : "=&v"(bl), "=&v"(bh) : "v"(al), "v"(ah));
                  asm volatile("s_nop 1\n" B32X2 : "=&v"(al), "=&v"(ah) : "v"(bl), "v"(bh));)
        } else if constexpr (K == 4) {   // group broadcast + v_add_f64, dependent, 32-bit spelling (the compiler places the s_nop)
            REP32(a = grp_bcast_b32(a) + c; asm volatile("" : "+v"(a));)
        } else if constexpr (K == 5) {   // group broadcast + v_add_f64, dependent, 64-bit spelling (the compiler places the s_nop)
            REP32(a = grp_bcast_b64(a) + c; asm volatile("" : "+v"(a));)
        }
    }
#undef B64
#undef B32X2
    if (a + b + al + ah + bl + bh == 12345.678) out[threadIdx.x] = a + b;
}

struct Case { const char *name; void (*fn)(double *, double); int per_iter; };

int main()
{
    double *out;
    CHECK(hipMalloc(&out, 64 * sizeof(double)));
    const Case cases[] = {
        {"1 x v_mov_b64_dpp, independent", k_dpp<0>, 32}, {"2 x v_mov_b32_dpp, independent", k_dpp<1>, 32},
        {"s_nop 1 + 1 x b64, dependent", k_dpp<2>, 64}, {"s_nop 1 + 2 x b32, dependent", k_dpp<3>, 64},
        {"group bcast + add, 4 x b32", k_dpp<4>, 32}, {"group bcast + add, 2 x b64", k_dpp<5>, 32},
    };
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const int grids[] = {1, 1024};
    printf("%-36s", "ns per item, grid =");
    for (int g : grids) printf(" %8d", g);
    printf("\n");
    for (const Case &c : cases) {
        printf("%-36s", c.name);
        for (int grid : grids) {
            hipLaunchKernelGGL(c.fn, dim3(grid), dim3(64), 0, 0, out, 1.0);   // warm
            CHECK(hipDeviceSynchronize());
            CHECK(hipEventRecord(e0));
            hipLaunchKernelGGL(c.fn, dim3(grid), dim3(64), 0, 0, out, 1.0);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float ms = 0;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            printf(" %8.3f", ms * 1e6 / ((double)ITER * c.per_iter));
        }
        printf("\n");
    }
    return 0;
}
