// radau_band.h -- Radau IIA(5) on a banded Jacobian (8 < n <= 512): J, E1, E2r and E2i stored by bands, E1 factorised and
// solved by BdfBand (bdf_band.h, unchanged), E2 = E2r + i E2i by the band complex LU and solve below.  Device only; included
// after radau_group.h and bdf_band.h.  RadauOps<GroupRhs<R, G>> (radau_group.h) selects RadauOpsBand whenever the functor
// carries SP_ML / SP_MU (HasBand, bdf_group.h); a functor without the two constants never names anything in this file.
//
// Storage.  One contiguous block per trajectory, in bdf_band.h's layouts (KD = ml + mu):
//   J                 entry (i, j) at  j * WJ + (mu + i - j),   WJ = ml + mu + 1        (WJ n doubles)
//   E1, E2r, E2i      entry (i, j) at  j * W  + (KD + i - j),   W  = 2 ml + mu + 1      (W n doubles each)
// (WJ + 3 W) n doubles per trajectory instead of 4 n^2: 15 n for a tridiagonal system.  The pivot rows stay in the global
// [B][2][n] array.  Everything lives ONLY in global memory, as in the wide form: nothing is fetched when a launch begins,
// nothing is written through, so `nlu` and every result bit are independent of how attempts are cut into launches.
// Every slot of the three factor blocks is written at every assembly (+0.0 in the fill rows and in the edge slots that
// correspond to no matrix entry), and every access below is guarded by INDEX, never by value.
//
// Arithmetic.  The assembly multiplies the identity's zeros out as RadauOpsWide::decomp_e1 does, and the complex LU and
// solve are RadauG / RadauW::lu_decomp_complex / lin_solve_complex (lu.rs:178-302, linear.rs:140-217) restricted to the
// band: the pivot is the first row in k..min(k+ml, n-1) attaining max |re| + |im| (NaNs never win, a NaN at [k][k] keeps
// m = k), a zero pivot returns false, the reciprocal is (tr / den, -ti / den), the three multiplier cases use the reference's
// three operation sequences, the trailing columns are k+1..min(k+KD, n-1).  Every in-band entry therefore sees the dense
// code's operations on the same operands; what the dense code does outside the band is +-0.  (The dense code leaves a
// trailing column alone when its pivot-row entry is zero and the exchange moves nothing; here such an entry is rewritten
// with the value it had.)
//
// Mapping: bdf_band.h's.  One lane per entry of the (ml+1) x (KD+1) pivot window, all pivot-independent operands of a step
// in ONE round trip (the entry, its row's column-k value, its column's row-k value -- two doubles each), the pivot by
// group_max + ballot, one more round trip for the pivot-row entries, then every lane forms its multiplier and writes its
// entry: every load of a step is issued before its first store.  The solve keeps both right-hand sides in registers and
// touches only the components that can hold rows k+1..k+ml (forward) or k-KD..k-1 (backward).
// All barriers are workgroup barriers of a ONE-WAVEFRONT workgroup: groups of a wavefront may diverge around them.
//
// Pure ODEs with the identity mass, no event functions, strict arithmetic.
#pragma once

namespace IVP_NS {

template <class R, int G>
struct RadauBand {
    using GR = GroupRhs<R, G>;
    using BG = BdfG<R, G>;
    using BB = BdfBand<R, G>;
    enum { NT = R::N, C = GR::N, NGROUP = IVP_WAVE / G, KD = BB::KD, WJ = BB::WJ, W = BB::W, JD = BB::JD, LD = BB::LD };
    enum { WR = BB::WR, WC = BB::WC, NW = BB::NW, TD = JD + 3 * LD };   // TD: doubles per trajectory
    static __device__ __forceinline__ int gl() { return GR::gl(); }
    static __device__ __forceinline__ int gi(int c) { return GR::gl() + G * c; }
    static __device__ __forceinline__ bool own(int c) { return gi(c) < NT; }

    // f1, f2, f3 of the mass contributions, published once per Newton pass: 3 n doubles per group
    static __device__ __forceinline__ double *fvec()
    {
        __shared__ double ivp_radb_f[NGROUP * 3 * NT];
        return ivp_radb_f + (size_t)((int)threadIdx.x / G) * 3 * NT;
    }

    // lu_decomp_complex on the band pair (ar, ai); pivots to piv[0..NT-2].  false: singular.
    static __device__ __forceinline__ bool lu_decomp_band_complex(double *ar, double *ai, uint32_t *piv)
    {
        int r[NW], q[NW];
#pragma unroll
        for (int s = 0; s < NW; ++s) { const int e = gl() + G * s; q[s] = e / WR; r[s] = e - q[s] * WR; }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < NT - 1; ++k) {
            // first round trip: the entry, the column-k value of its row, the row-k value of its column
            bool ok[NW];
            double vr[NW], vi[NW], crr[NW], cri[NW], kjr[NW], kji[NW];
#pragma unroll
            for (int s = 0; s < NW; ++s) {
                ok[s] = q[s] < WC && k + r[s] < NT && k + q[s] < NT;
                vr[s] = 0.0; vi[s] = 0.0; crr[s] = 0.0; cri[s] = 0.0; kjr[s] = 0.0; kji[s] = 0.0;
                if (ok[s]) {
                    const int cj = (k + q[s]) * W + KD - q[s];   // slot of (k, k + q)
                    vr[s] = ar[cj + r[s]]; vi[s] = ai[cj + r[s]];
                    kjr[s] = ar[cj]; kji[s] = ai[cj];
                    crr[s] = ar[k * W + KD + r[s]]; cri[s] = ai[k * W + KD + r[s]];
                }
            }
            // first row >= k attaining max |re| + |im| (NaNs never win): the candidates are the entries of window column 0
            double av[NW], lv = -1.0;
#pragma unroll
            for (int s = 0; s < NW; ++s) {
                const double f = fabs(vr[s]) + fabs(vi[s]);
                av[s] = (ok[s] && q[s] == 0 && f == f) ? f : -1.0;
                lv = av[s] > lv ? av[s] : lv;
            }
            const double akr = BG::lane_bcast(vr[0], 0), aki = BG::lane_bcast(vi[0], 0);
            const double vkk = fabs(akr) + fabs(aki);
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
            double pr = akr, pi = aki;
            if (vkk == vkk && vmax >= 0.0) {   // a NaN at [k][k]: every `>` of the reference's scan is false
                rm = li;
                double selr = vr[0], seli = vi[0];
#pragma unroll
                for (int s = 1; s < NW; ++s) {
                    selr = (G * s < WR && li / G == s) ? vr[s] : selr;
                    seli = (G * s < WR && li / G == s) ? vi[s] : seli;
                }
                pr = BG::lane_bcast(selr, li % G);
                pi = BG::lane_bcast(seli, li % G);
            }
            const int m = k + rm;
            if (gl() == 0) piv[k] = (uint32_t)m;
            if (fabs(pr) + fabs(pi) == 0.0) return false;
            // second round trip: the pivot-row entry of this entry's column
            double mr[NW], mi[NW];
#pragma unroll
            for (int s = 0; s < NW; ++s) {
                mr[s] = 0.0; mi[s] = 0.0;
                if (ok[s]) {
                    const int at = (k + q[s]) * W + KD - q[s] + rm;
                    mr[s] = ar[at]; mi[s] = ai[at];
                }
            }
            const double den = pr * pr + pi * pi;   // 1 / (tr + i ti) = (tr / den, -ti / den)
            const double tr = pr / den;
            const double ti = -pi / den;
            double outr[NW], outi[NW];
#pragma unroll
            for (int s = 0; s < NW; ++s) {
                const bool is_m = r[s] == rm, below = r[s] > 0;
                // this row's multiplier; row m holds row k's entry after the exchange
                const double er = is_m ? akr : crr[s], ei = is_m ? aki : cri[s];
                const double lr = -(er * tr - ei * ti);
                const double lim = -(ei * tr + er * ti);
                const double xr = is_m ? kjr[s] : vr[s], xi = is_m ? kji[s] : vi[s];   // the row exchange
                double tr_ = xr, ti_ = xi;
                if (fabs(mr[s]) + fabs(mi[s]) != 0.0) {
                    double prod_r, prod_i;
                    if (mi[s] == 0.0) {          // real multiplier
                        prod_r = lr * mr[s];
                        prod_i = lim * mr[s];
                    } else if (mr[s] == 0.0) {   // imaginary multiplier
                        prod_r = -lim * mi[s];
                        prod_i = lr * mi[s];
                    } else {                     // general complex multiplier
                        prod_r = lr * mr[s] - lim * mi[s];
                        prod_i = lim * mr[s] + lr * mi[s];
                    }
                    tr_ = xr + prod_r;
                    ti_ = xi + prod_i;
                }
                const double trailr = below ? tr_ : mr[s], traili = below ? ti_ : mi[s];   // row k becomes U[k][j]
                const double col0r = below ? lr : pr, col0i = below ? lim : pi;
                outr[s] = q[s] == 0 ? col0r : trailr;
                outi[s] = q[s] == 0 ? col0i : traili;
            }
            __syncthreads();   // every lane has read its operands before any entry of the window changes
#pragma unroll
            for (int s = 0; s < NW; ++s)
                if (ok[s]) {
                    const int at = (k + q[s]) * W + KD - q[s] + r[s];
                    ar[at] = outr[s]; ai[at] = outi[s];
                }
            __syncthreads();   // the window of pivot k + 1 is complete
        }
        return fabs(ar[(NT - 1) * W + KD]) + fabs(ai[(NT - 1) * W + KD]) != 0.0;
    }

    // lin_solve_complex on the band: (br + i bi), this lane's components, <- (ar + i ai)^-1 (br + i bi)
    static __device__ __forceinline__ void lin_solve_band_complex(const double *ar, const double *ai, const uint32_t *piv, double (&br)[C], double (&bi)[C])
    {
        uint32_t pv[C];
#pragma unroll
        for (int c = 0; c < C; ++c) pv[c] = gi(c) < NT - 1 ? piv[gi(c)] : 0u;
        constexpr int ML = BB::ML;
        constexpr int CF = (ML + G - 1) / G;   // components beyond the block's own that rows k+1..k+ml can reach
        constexpr int CB = (KD + G - 1) / G;   // ... that rows k-KD..k-1 can reach
        // forward: row exchange m <-> k, then b[i] += l[i][k] * b[k] for k < i <= k + ml
#pragma unroll
        for (int kb = 0; kb < C; ++kb) {
            if (kb * G >= NT - 1) break;
            const int kend = (kb + 1) * G < NT - 1 ? (kb + 1) * G : NT - 1;
#pragma unroll 4
            for (int k = kb * G; k < kend; ++k) {
                const int m = (int)BG::lane_bcast(pv[kb], k - kb * G);
                const double kr = BG::lane_bcast(br[kb], k - kb * G), ki = BG::lane_bcast(bi[kb], k - kb * G);
                const double tr = BG::row_bcast(br, m, kb), ti = BG::row_bcast(bi, m, kb);
#pragma unroll
                for (int c = kb; c <= kb + CF && c < C; ++c) {
                    const int i = gi(c);
                    const bool in = i > k && i <= k + ML && i < NT;
                    double cr = 0.0, ci = 0.0;
                    if (in) { cr = ar[k * W + KD + (i - k)]; ci = ai[k * W + KD + (i - k)]; }
                    double xr = i == m ? kr : br[c], xi = i == m ? ki : bi[c];
                    xr = i == k ? tr : xr;
                    xi = i == k ? ti : xi;
                    const double prod_r = cr * tr - ci * ti;
                    const double prod_i = ci * tr + cr * ti;
                    br[c] = in ? xr + prod_r : xr;
                    bi[c] = in ? xi + prod_i : xi;
                }
            }
        }
        // backward: b[k] /= u[k][k], then b[i] -= u[i][k] * b[k] for k - KD <= i < k
#pragma unroll
        for (int kb = C - 1; kb >= 0; --kb) {
            if (kb * G > NT - 1) continue;
            const int ktop = (kb + 1) * G - 1 < NT - 1 ? (kb + 1) * G - 1 : NT - 1;
#pragma unroll 4
            for (int k = ktop; k >= kb * G; --k) {
                double kr = BG::lane_bcast(br[kb], k - kb * G), ki = BG::lane_bcast(bi[kb], k - kb * G);
                radau_cdiv(ar[k * W + KD], ai[k * W + KD], kr, ki);
                const double tr = -kr, ti = -ki;
#pragma unroll
                for (int c = (kb - CB > 0 ? kb - CB : 0); c <= kb; ++c) {
                    const int i = gi(c);
                    const bool in = i < k && i >= k - KD;
                    double cr = 0.0, ci = 0.0;
                    if (in) { cr = ar[k * W + KD + (i - k)]; ci = ai[k * W + KD + (i - k)]; }
                    const double prod_r = cr * tr - ci * ti;
                    const double prod_i = ci * tr + cr * ti;
                    const double xr = i == k ? kr : br[c], xi = i == k ? ki : bi[c];
                    br[c] = in ? xr + prod_r : xr;
                    bi[c] = in ? xi + prod_i : xi;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) if (!own(c)) { br[c] = 0.0; bi[c] = 0.0; }
    }
};

// The band form of the attempt's policy: J, E1, E2r, E2i by bands in the trajectory's global block ([B][(WJ + 3 W) n]), the
// pivot rows of E1 and of E2 in the global [B][2][n] array, C rows per lane at every group width.  Like the wide form it
// keeps nothing in LDS that outlives an attempt.
template <class R, int G>
struct RadauOpsBand {
    using RB = RadauBand<R, G>;
    using BG = BdfG<R, G>;
    using BB = BdfBand<R, G>;
    enum { NT = RB::NT, C = RB::C, JD = RB::JD, LD = RB::LD, TD = RB::TD, W = RB::W, WJ = RB::WJ, KD = RB::KD, ML = BB::ML };
    static_assert(!HasMassCol<R>::v, "Radau in band storage: pure ODEs with the identity mass");
    static_assert(GroupRhs<R, G>::NE == 0, "Radau in band storage: no event functions");
    double *jac, *fac;     // global: J; E1, E2r, E2i
    uint32_t *piv;         // global: the pivot rows of E1, then of E2
    mutable double ms1[C], ms2[C], ms3[C];   // the mass contributions of this lane's rows, formed on the call for row 0
    struct Factor {};

    static __device__ __forceinline__ void init_piv(const IvpKArgs &a, size_t, uint32_t j)
    {
        for (int e = RB::gl(); e < 2 * NT; e += G) radau_piv(a)[(size_t)j * 2 * NT + e] = 0u;
    }
    static __device__ __forceinline__ void init_mat(const IvpKArgs &a, size_t, uint32_t j)
    {
        double *jac0 = radau_mat(a) + (size_t)j * TD;
        for (int e = RB::gl(); e < JD; e += G) jac0[e] = 0.0;
    }
    static __device__ __forceinline__ double tolst(const IvpKArgs &a, const double (&)[C])   // component 0's, in every lane
    {
        return 0.1 * ivp_pow(a.rtol_dev ? a.rtol_dev[0] : a.rtol[0], 2.0 / 3.0);
    }
    __device__ __forceinline__ uint32_t begin(const IvpKArgs &a, size_t, uint32_t j)
    {
        jac = radau_mat(a) + (size_t)j * TD;
        fac = jac + JD;
        piv = radau_piv(a) + (size_t)j * 2 * NT;
        return a.flags[j];
    }
    static __device__ __forceinline__ uint32_t settle(uint32_t j) { __syncthreads(); return j; }
    __device__ __forceinline__ void end(const IvpKArgs &, size_t, uint32_t) const {}
    static __device__ __forceinline__ bool counts() { return RB::gl() == 0; }

    // grouped forward differences from the pattern's tables, written through BdfG::jac_at into the band
    __device__ __forceinline__ void eval_jac(const IvpKArgs &, uint32_t, double x, const double (&y)[C], const double *p) const { BG::eval_jac(x, y, p, jac); }
    // E1, E2r and E2i are assembled together in one pass over the factor layout (every slot is written: +0.0 in the fill rows
    // and the edge slots), the identity's zeros multiplied out, then E1 is factorised ...
    __device__ __forceinline__ bool decomp_e1(const IvpKArgs &, uint32_t, double fac1, double alphn, double betan, uint32_t &nlu, Factor &) const
    {
        double *e1 = fac, *e2r = fac + LD, *e2i = fac + 2 * LD;
        __syncthreads();   // J is complete; nobody still reads the old factors
        constexpr int FB = 4;
#pragma unroll 1
        for (int e0 = 0; e0 < LD; e0 += FB * G) {
            double jv[FB];
            bool live[FB], diag[FB];
#pragma unroll
            for (int u = 0; u < FB; ++u) {
                const int e = e0 + u * G + RB::gl();
                const int col = e / W, off = e - col * W;
                const int i = col + off - KD;
                live[u] = e < LD && off >= ML && i >= 0 && i < NT;
                diag[u] = i == col;
                jv[u] = 0.0;
                if (live[u]) jv[u] = jac[col * WJ + (off - ML)];
            }
#pragma unroll
            for (int u = 0; u < FB; ++u) {
                const int e = e0 + u * G + RB::gl();
                const double id = diag[u] ? 1.0 : 0.0;   // the identity's zeros are multiplied out: 0.0 * inf is a NaN
                if (e < LD) {
                    e1[e] = live[u] ? id * fac1 - jv[u] : 0.0;
                    e2r[e] = live[u] ? id * alphn - jv[u] : 0.0;
                    e2i[e] = live[u] ? id * betan : 0.0;
                }
            }
        }
        nlu += 1;
        return BB::lu_decomp_band(e1, piv);
    }
    // ... and E2
    __device__ __forceinline__ bool decomp_e2(const IvpKArgs &, uint32_t, double, double, uint32_t &nlu, Factor &, Factor &) const
    {
        nlu += 1;
        return RB::lu_decomp_band_complex(fac + LD, fac + 2 * LD, piv + NT);
    }
    __device__ __forceinline__ void load_e1(const IvpKArgs &, uint32_t, Factor &) const {}
    __device__ __forceinline__ void solve_e1(const Factor &, double (&b)[C]) const { BB::lin_solve_band(fac, piv, b); }
    __device__ __forceinline__ void solve_e2(const IvpKArgs &, uint32_t, double (&br)[C], double (&bi)[C]) const { RB::lin_solve_band_complex(fac + LD, fac + 2 * LD, piv + NT, br, bi); }
    // mass contributions over ALL j, the identity's zeros multiplied out, as in the wide form: published ONCE, on the call
    // for row 0, which sums over all j for every row this lane owns
    __device__ __forceinline__ void mass_row3(const IvpKArgs &, uint32_t, int i, const double (&f1)[C], const double (&f2)[C], const double (&f3)[C],
                                              double &sum1, double &sum2, double &sum3) const
    {
        if (i == 0) {
            double *fv = RB::fvec();
            __syncthreads();
#pragma unroll
            for (int c = 0; c < C; ++c) if (RB::own(c)) { fv[RB::gi(c)] = f1[c]; fv[NT + RB::gi(c)] = f2[c]; fv[2 * NT + RB::gi(c)] = f3[c]; }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < C; ++c) { ms1[c] = 0.0; ms2[c] = 0.0; ms3[c] = 0.0; }
#pragma unroll 2
            for (int jj = 0; jj < NT; ++jj) {
                const double v1 = fv[jj], v2 = fv[NT + jj], v3 = fv[2 * NT + jj];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const double mij = RB::gi(c) == jj ? 1.0 : 0.0;
                    ms1[c] -= mij * v1;
                    ms2[c] -= mij * v2;
                    ms3[c] -= mij * v3;
                }
            }
        }
        sum1 = ms1[i]; sum2 = ms2[i]; sum3 = ms3[i];
    }
    __device__ __forceinline__ double mass_row(const IvpKArgs &, uint32_t, int i, const double (&f)[C]) const
    {
        if (i == 0) {
            double *fv = RB::fvec();
            __syncthreads();
#pragma unroll
            for (int c = 0; c < C; ++c) if (RB::own(c)) fv[RB::gi(c)] = f[c];
            __syncthreads();
#pragma unroll
            for (int c = 0; c < C; ++c) ms1[c] = 0.0;
#pragma unroll 2
            for (int jj = 0; jj < NT; ++jj) {
                const double v = fv[jj];
#pragma unroll
                for (int c = 0; c < C; ++c) ms1[c] += (RB::gi(c) == jj ? 1.0 : 0.0) * v;
            }
        }
        return ms1[i];
    }
};

}  // namespace IVP_NS
