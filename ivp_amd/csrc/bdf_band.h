// bdf_band.h -- banded storage and banded LU for large-n BDF (8 < n <= 512): `jac_storage = Banded{ml, mu}` of the
// reference (src/solve/options.rs:104-108, src/matrix/base.rs:12-15).  Device only; included after bdf_group.h, whose
// `if constexpr (HasBand<R>::v)` hooks call into it.  A functor is banded when it carries SP_ML / SP_MU next to the
// sparsity tables (ivp_jit.cpp writes them for IVP_RHS_BANDED problems).
//
// Layout (LAPACK general band, column-major; KD = ml + mu):
//   J      entry (i, j), j - mu <= i <= j + ml, at  j * WJ + (mu + i - j),       WJ = ml + mu + 1
//   factor entry (i, j), j - KD <= i <= j + ml, at  j * W  + (KD + i - j),       W  = 2 ml + mu + 1
// The ml extra superdiagonals of the factors receive the fill that row exchanges create.  Slots of edge columns that
// correspond to no matrix entry (i < 0 or i >= n) hold +0.0, are never read as pivot candidates and never written after
// form(): every access below is guarded by INDEX (0 <= i, j < n and inside the band), never by value.
//
// Arithmetic: lu_decomp_band / lin_solve_band restate src/matrix/lu.rs:37-125 and src/matrix/linear.rs:55-96 exactly as
// BdfG::lu_decomp / BdfG::lin_solve do, restricted to the band: the pivot search covers rows k..min(k+ml, n-1) (first
// row attaining the maximum, NaNs never win), the trailing columns are k+1..min(k+KD, n-1), the `t_j != 0` guard, the row
// exchange, the negated multipliers, the IVP_MA sites and the divisions are those of the dense code.  Every in-band entry
// therefore sees the dense code's operations on the same operands; what the dense code does outside the band is +-0.
//
// Mapping.  A pivot step touches the (ml+1) x (KD+1) window whose corner is (k, k): one lane per window entry
// (entry e <-> row k + e % (ml+1), column k + e / (ml+1); wider windows take NW = ceil(WS / G) entries per lane).  All of a
// step's operands that do not depend on the pivot row arrive in ONE round trip (the entry, its row's column-k value, its
// column's row-k value); the pivot comes from the DPP group_max + ballot of bdf_group.h; one more round trip brings the
// pivot-row entries; every lane then forms its multiplier itself and writes its entry.  Two round trips and two barriers
// per pivot, no whole-column loads, no segment probes.
// The solves keep b in registers (lane l owns rows l, l + G, ...), broadcast b[k] with lane_bcast and touch only the
// components that can hold rows k+1..k+ml (forward) or k-KD..k-1 (backward).
//
// Residency.  LDS form: the factors and pivots of the group's trajectory stay in LDS for the whole launch and travel
// through the trajectory's global block at launch boundaries (like LDSLU in bdf_group.h), so nlu and every bit are
// independent of chunking.  It is chosen by the host (ivp_jit.cpp: band_lds_fits, the same formula as lds_bytes() below)
// when everything the kernel keeps in LDS fits IVP_BAND_LDS_BUDGET.  Global form: same functions on the global block.
#pragma once

namespace IVP_NS {

template <class R, int G>
struct BdfBand {
    using BG = BdfG<R, G>;
    using GR = GroupRhs<R, G>;
    enum { NT = R::N, C = BG::C, ML = R::SP_ML, MU = R::SP_MU, KD = ML + MU, WJ = ML + MU + 1, W = 2 * ML + MU + 1, NGROUP = IVP_WAVE / G };
    enum { WR = ML + 1, WC = KD + 1, WS = WR * WC, NW = (WS + G - 1) / G };
    enum { JD = WJ * NT, LD = W * NT };   // doubles per trajectory: J, factors
    static_assert(ML >= 0 && MU >= 0 && W < NT, "band as wide as the matrix");
    // what a banded LDS kernel allocates: factors, pivots, fd_jac_sparse's KJ + 1 state copies, GR::scratch(), the event stage
    static constexpr int lds_bytes()
    {
        return NGROUP * NT * (8 * (W + BG::KJ + 1 + 1 + (GR::NE > 0 ? 1 : 0)) + 4);
    }
    static __device__ __forceinline__ int gl() { return GR::gl(); }

    // (I - cJ) into the factor block: every slot of the block is written (fill rows and edge slots: +0.0)
    static __device__ __forceinline__ void form(const double *jac, double *lu, double c)
    {
        constexpr int FB = 4;
#pragma unroll 1
        for (int e0 = 0; e0 < LD; e0 += FB * G) {
            double jv[FB];
            bool live[FB], diag[FB];
#pragma unroll
            for (int u = 0; u < FB; ++u) {
                const int e = e0 + u * G + gl();
                const int col = e / W, off = e - col * W;
                const int i = col + off - KD;
                live[u] = e < LD && off >= ML && i >= 0 && i < NT;
                diag[u] = i == col;
                jv[u] = 0.0;
                if (live[u]) jv[u] = jac[col * WJ + (off - ML)];
            }
#pragma unroll
            for (int u = 0; u < FB; ++u) {
                const int e = e0 + u * G + gl();
                const double v = diag[u] ? IVP_MA(1.0, -c, jv[u]) : -c * jv[u];   // (I - cJ): the diagonal is -c j + 1
                if (e < LD) lu[e] = live[u] ? v : 0.0;
            }
        }
    }

    // lu_decomp (src/matrix/lu.rs:37-125) on the band; pivots to piv[0..NT-2].  false: singular.
    static __device__ __forceinline__ bool lu_decomp_band(double *a, uint32_t *piv)
    {
        int r[NW], q[NW];
#pragma unroll
        for (int s = 0; s < NW; ++s) { const int e = gl() + G * s; q[s] = e / WR; r[s] = e - q[s] * WR; }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < NT - 1; ++k) {
            // first round trip: the entry, the column-k value of its row, the row-k value of its column
            bool ok[NW];
            double v[NW], cr[NW], akj[NW];
#pragma unroll
            for (int s = 0; s < NW; ++s) {
                ok[s] = q[s] < WC && k + r[s] < NT && k + q[s] < NT;
                v[s] = 0.0; cr[s] = 0.0; akj[s] = 0.0;
                if (ok[s]) {
                    const int cj = (k + q[s]) * W + KD - q[s];   // slot of (k, k + q)
                    v[s] = a[cj + r[s]];
                    akj[s] = a[cj];
                    cr[s] = a[k * W + KD + r[s]];
                }
            }
            // first row >= k attaining max |a[row][k]| (NaNs never win): the candidates are the entries of window column 0
            double av[NW], lv = -1.0;
#pragma unroll
            for (int s = 0; s < NW; ++s) {
                const double f = fabs(v[s]);
                av[s] = (ok[s] && q[s] == 0 && f == f) ? f : -1.0;
                lv = av[s] > lv ? av[s] : lv;
            }
            const double akk = BG::lane_bcast(v[0], 0);
            const double vmax = BG::group_max(lv);
            int li = 0;
#pragma unroll
            for (int s = NW - 1; s >= 0; --s) {
                if (G * s >= WR) continue;   // no column-0 entry in this slot
                unsigned long long hit = __ballot(av[s] == vmax);
                if (G < IVP_WAVE) hit = (hit >> BG::wl0()) & ((1ull << (G & 63)) - 1ull);
                if (hit != 0ull) li = G * s + __ffsll((long long)hit) - 1;
            }
            int rm = 0;
            double pivot = akk;
            if (akk == akk && vmax >= 0.0) {   // |a[k][k]| NaN: every `>` of the reference's scan is false
                rm = li;
                double sel = v[0];
#pragma unroll
                for (int s = 1; s < NW; ++s) sel = (G * s < WR && li / G == s) ? v[s] : sel;
                pivot = BG::lane_bcast(sel, li % G);
            }
            const int m = k + rm;
            if (gl() == 0) piv[k] = (uint32_t)m;
            if (pivot == 0.0) return false;
            // second round trip: the pivot-row entry of this entry's column
            double tj[NW];
#pragma unroll
            for (int s = 0; s < NW; ++s) {
                tj[s] = 0.0;
                if (ok[s]) tj[s] = a[(k + q[s]) * W + KD - q[s] + rm];
            }
            const double t = 1.0 / pivot;
            double out[NW];
#pragma unroll
            for (int s = 0; s < NW; ++s) {
                const bool is_m = r[s] == rm, below = r[s] > 0;
                const double mult = below ? -(is_m ? akk : cr[s]) * t : 0.0;   // row m holds row k's entry after the swap
                const double vv = is_m ? akj[s] : v[s];                          // row m receives row k's entry (the swap)
                const double w = IVP_MA(vv, mult, tj[s]);
                const double v2 = (tj[s] != 0.0 && below) ? w : vv;
                const double trail = below ? v2 : tj[s];                         // row k becomes U[k][j]
                const double col0 = below ? mult : pivot;
                out[s] = q[s] == 0 ? col0 : trail;
            }
            __syncthreads();   // every lane has read its operands before any entry of the window changes
#pragma unroll
            for (int s = 0; s < NW; ++s)
                if (ok[s]) a[(k + q[s]) * W + KD - q[s] + r[s]] = out[s];
            __syncthreads();   // the window of pivot k + 1 is complete
        }
        return a[(NT - 1) * W + KD] != 0.0;
    }

    // lin_solve (src/matrix/linear.rs:55-96) on the band: b (this lane's components) <- A^-1 b
    static __device__ __forceinline__ void lin_solve_band(const double *a, const uint32_t *piv, double (&bl)[C])
    {
        uint32_t pv[C];
#pragma unroll
        for (int c = 0; c < C; ++c) pv[c] = BG::gi(c) < NT - 1 ? piv[BG::gi(c)] : 0u;
        constexpr int CF = (ML + G - 1) / G;   // components beyond the block's own that rows k+1..k+ml can reach
        constexpr int CB = (KD + G - 1) / G;   // ... that rows k-KD..k-1 can reach
        // forward: b <- L^-1 P b (row exchange m <-> k, then b[i] += l[i][k] * b[k] for k < i <= k + ml; multipliers are stored negated)
#pragma unroll
        for (int kb = 0; kb < C; ++kb) {
            if (kb * G >= NT - 1) break;
            const int kend = (kb + 1) * G < NT - 1 ? (kb + 1) * G : NT - 1;
#pragma unroll 4
            for (int k = kb * G; k < kend; ++k) {
                const int m = (int)BG::lane_bcast(pv[kb], k - kb * G);
                const double bk_old = BG::lane_bcast(bl[kb], k - kb * G);
                const double t = BG::row_bcast(bl, m, kb);
#pragma unroll
                for (int c = kb; c <= kb + CF && c < C; ++c) {
                    const int i = BG::gi(c);
                    const bool in = i > k && i <= k + ML && i < NT;
                    double l = 0.0;
                    if (in) l = a[k * W + KD + (i - k)];
                    double bi = bl[c];
                    bi = i == m ? bk_old : bi;
                    bi = i == k ? t : bi;
                    bl[c] = in ? IVP_MA(bi, l, t) : bi;
                }
            }
        }
        // backward: b <- U^-1 b (b[k] /= u[k][k], then b[i] -= u[i][k] * b[k] for k - KD <= i < k)
#pragma unroll
        for (int kb = C - 1; kb >= 0; --kb) {
            if (kb * G > NT - 1) continue;
            const int ktop = (kb + 1) * G - 1 < NT - 1 ? (kb + 1) * G - 1 : NT - 1;
#pragma unroll 4
            for (int k = ktop; k >= kb * G; --k) {
                const double bk = BG::lane_bcast(bl[kb], k - kb * G) / a[k * W + KD];
#pragma unroll
                for (int c = (kb - CB > 0 ? kb - CB : 0); c <= kb; ++c) {
                    const int i = BG::gi(c);
                    const bool in = i < k && i >= k - KD;
                    double u = 0.0;
                    if (in) u = a[k * W + KD + (i - k)];
                    const double bi = i == k ? bk : bl[c];
                    bl[c] = in ? IVP_MA(bi, u, -bk) : bi;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) bl[c] = BG::own(c) ? bl[c] : 0.0;
    }
};

}  // namespace IVP_NS
