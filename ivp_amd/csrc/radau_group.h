// radau_group.h -- Radau IIA(5) for 8 < n <= 64: one group of G lanes integrates one trajectory, every lane owns exactly ONE
// component and ONE matrix row, the three factors stay in LDS for the whole launch.  Device only.
//
// There is no attempt here: group_init_body / group_chunk_body (rk_group.h, M_RADAU) run radau_core.h's bodies on
// GroupRhs<R, G> -- strict arithmetic only.  This file holds the group form of their policy,
// RadauOps<GroupRhs<R, G>>, over BdfG::eval_jac / lu_decomp / lin_solve (bdf_group.h, unchanged: J and the real factor E1),
// and RadauG: the group's LDS and the complex LU and solve of E2 = E2r + i E2i (lu.rs:178-302, linear.rs:140-217) over lanes.
//
// Why n <= 64.  ivp_group_width(n) gives G = 16 / 32 / 64 >= n, so C == 1: lane gl() owns component and row gl(), lanes with
// gl() >= n idle.  All scalar controller state is computed redundantly by every lane (control flow is group-uniform); what
// crosses lanes -- the right-hand sides, the "mass contribution" sums, the linear solves, the two norms -- goes through LDS
// or lane broadcasts and nothing else does.  The factors take 3 n^2 doubles per trajectory, 96 KB at n = 64 (one group per
// wavefront), 48 KB at n = 32 (two groups), 24 KB at n = 16 (four): they fit the CU's 160 KB beside the group vectors; at
// n = 100 they would need 240 KB.
//
// Memory.  J lives in global memory, column-major, one contiguous block per trajectory, followed by the global copies of
// E1, E2r, E2i (4 n^2 doubles per trajectory); the pivot vectors are uint32_t[n] each.  The LDS factors are column-major
// too: a column operation is one conflict-free access across the owning lanes.  They are written through to the global
// block after every factorisation in which both factors succeed, and fetched again at the start of a launch whenever
// call_decomp is clear -- the only case in which an attempt uses factors it did not compute itself -- so `nlu` and every
// result bit are independent of how attempts are cut into launches.
// All barriers are workgroup barriers of a ONE-WAVEFRONT workgroup: groups of a wavefront may diverge around them.
//
// M y' = f.  A component-form functor with a `mass_col` member (HasMassCol, radau_core.h) makes HasMass<GroupRhs<R, G>> true,
// and the bodies' mass sites and DAE index sets are compiled in.  M is a fifth n^2 block of the trajectory's global block
// (J, E1, E2r, E2i, M: 5 n^2 doubles per trajectory, column-major), filled once by the init body, column c by lane c.  It is
// constant and is read n times per Newton pass, so begin() copies it into the group's LDS on EVERY launch (unlike the
// factors it is always valid) and the assembly and the mass-contribution sums read it from there: NGROUP n^2 doubles more
// LDS, 32 KB at n = 64, paid by the mass instantiations only.  Everything here stays behind `if constexpr (MASS)`: a
// functor without the hook compiles to what it compiled to.
//
// 64 < n <= 512 (the WIDE form, below: RadauW and RadauOpsWide).  G = 64 and lane l owns rows l, l + 64, ...: C = ceil(n / 64)
// up to 8 rows per lane.  Three n x n factors no longer fit LDS (240 KB at n = 100), so J, E1, E2r and E2i live ONLY in the
// trajectory's global block and the pivot rows only in the global [B][2][n] array: nothing is fetched when a launch begins,
// nothing is written through, and `nlu` and every result bit are independent of how attempts are cut into launches by
// construction.  J and E1 go through BdfG::eval_jac / lu_decomp / lin_solve as they are (they work for any C on matrices in
// global memory); RadauW holds the complex LU and solve for C rows per lane, with BdfG::lu_decomp's trailing update: only
// the columns whose pivot-row entry is non-zero, or whose rows k and m differ, are read and written -- a handful per pivot
// for a tridiagonal Jacobian.  Pure ODEs with the identity mass only: a functor with mass_col stays at n <= 64.
// RadauOps<GroupRhs<R, G>> picks the form by C at compile time; the C == 1 form is the code it always was.
//
// Band storage (radau_band.h, included after this header by the modules of the banded call only): a functor that carries
// SP_ML / SP_MU (HasBand, bdf_group.h) takes RadauOpsBand at every width instead -- J and the three factors by bands in
// global memory.  A functor without the two constants compiles to exactly what it compiled to.
#pragma once

namespace IVP_NS {

template <class R, int G>
struct RadauG {
    using GR = GroupRhs<R, G>;
    using BG = BdfG<R, G>;
    enum { NT = R::N, C = GR::N, P = R::P, NGROUP = IVP_WAVE / G, NN = R::N * R::N };
    static_assert(C == 1, "RadauG: every lane owns exactly one component and one matrix row (G >= n)");
    static_assert(NT > 1 && NT <= 64, "RadauG: 8 < n <= 64 (three n x n factors resident in LDS)");
    static __device__ __forceinline__ int gl() { return GR::gl(); }
    static __device__ __forceinline__ bool own() { return GR::gl() < NT; }
    static __device__ __forceinline__ int row() { return GR::gl() < NT ? GR::gl() : NT - 1; }   // idle lanes read a clamped address
    static __device__ __forceinline__ int grp() { return (int)threadIdx.x / G; }

    // this group's LDS: E1, E2r, E2i (column-major, NN doubles each); the pivot rows of E1 and of E2; f1, f2, f3
    static __device__ __forceinline__ double *factors()
    {
        __shared__ double ivp_rad_fac[NGROUP * 3 * NN];
        return ivp_rad_fac + (size_t)grp() * 3 * NN;
    }
    static __device__ __forceinline__ uint32_t *pivots()
    {
        __shared__ uint32_t ivp_rad_piv[NGROUP * 2 * NT];
        return ivp_rad_piv + (size_t)grp() * 2 * NT;
    }
    static __device__ __forceinline__ double *fvec()
    {
        __shared__ double ivp_rad_f[NGROUP * 3 * NT];
        return ivp_rad_f + (size_t)grp() * 3 * NT;
    }
    // ... and, for a functor with mass_col only (nothing else names it), this group's copy of M, column-major
    static __device__ __forceinline__ double *mass()
    {
        __shared__ double ivp_rad_mass[NGROUP * NN];
        return ivp_rad_mass + (size_t)grp() * NN;
    }

    // lu_decomp_complex (src/matrix/lu.rs:178-302) in place on the column-major pair (ar, ai); pivots to piv[0..NT-2].
    // Right-looking, column by column.  The pivot is the FIRST row >= k that attains max |re| + |im| (the reference's strict
    // `>` scan: NaNs never win, a NaN at [k][k] keeps m = k); the reciprocal is (tr / den, -ti / den); the three multiplier
    // cases are the reference's three operation sequences.  Every entry is only ever touched by the lane that owns its row,
    // with the reference's operations in the reference's order, so the factors are bit-identical.
    static __device__ __forceinline__ bool lu_decomp_complex(double *ar, double *ai, uint32_t *piv)
    {
        const int i = gl(), r = row();
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < NT - 1; ++k) {
            const double ckr = ar[k * NT + r], cki = ai[k * NT + r];
            const double v = fabs(ckr) + fabs(cki);
            const double av = (i >= k && i < NT && v == v) ? v : -1.0;
            const double vkk = BG::lane_bcast(v, k);
            const double vmax = BG::group_max(av);
            unsigned long long hit = __ballot(av == vmax);
            if (G < IVP_WAVE) hit = (hit >> BG::wl0()) & ((1ull << (G & 63)) - 1ull);
            int m = k;
            if (vkk == vkk && vmax >= 0.0) m = __ffsll((long long)hit) - 1;
            const double pr = BG::lane_bcast(ckr, m), pi = BG::lane_bcast(cki, m);
            if (i == 0) piv[k] = (uint32_t)m;
            if (fabs(pr) + fabs(pi) == 0.0) return false;
            const double akr = BG::lane_bcast(ckr, k), aki = BG::lane_bcast(cki, k);
            const double den = pr * pr + pi * pi;   // 1 / (tr + i ti) = (tr / den, -ti / den)
            const double tr = pr / den;
            const double ti = -pi / den;
            // this row's multiplier; row m holds row k's entry after the exchange
            const double er = i == m ? akr : ckr, ei = i == m ? aki : cki;
            const double lr = -(er * tr - ei * ti);
            const double li = -(ei * tr + er * ti);
            const bool below = i > k && i < NT;
            if (i == k) { ar[k * NT + i] = pr; ai[k * NT + i] = pi; }
            else if (below) { ar[k * NT + i] = lr; ai[k * NT + i] = li; }
            // trailing columns, JB at a time: all loads of a block are issued before its first store (a lone wavefront pays
            // a full LDS round trip for whatever it waits on)
            constexpr int JB = 4;
#pragma unroll 1
            for (int j0 = k + 1; j0 < NT; j0 += JB) {
                double mr[JB], mi[JB], kr[JB], ki[JB], cr[JB], ci[JB];
#pragma unroll
                for (int b = 0; b < JB; ++b) {
                    const int col = (j0 + b < NT ? j0 + b : NT - 1) * NT;
                    mr[b] = ar[col + m]; mi[b] = ai[col + m];
                    kr[b] = ar[col + k]; ki[b] = ai[col + k];
                    cr[b] = ar[col + r]; ci[b] = ai[col + r];
                }
#pragma unroll
                for (int b = 0; b < JB; ++b) {
                    if (j0 + b >= NT) continue;
                    const int col = (j0 + b) * NT;
                    const double vr = i == m ? kr[b] : cr[b], vi = i == m ? ki[b] : ci[b];   // the row exchange
                    double outr = vr, outi = vi;
                    if (fabs(mr[b]) + fabs(mi[b]) != 0.0) {
                        double prod_r, prod_i;
                        if (mi[b] == 0.0) {          // real multiplier
                            prod_r = lr * mr[b];
                            prod_i = li * mr[b];
                        } else if (mr[b] == 0.0) {   // imaginary multiplier
                            prod_r = -li * mi[b];
                            prod_i = lr * mi[b];
                        } else {                     // general complex multiplier
                            prod_r = lr * mr[b] - li * mi[b];
                            prod_i = li * mr[b] + lr * mi[b];
                        }
                        outr = vr + prod_r;
                        outi = vi + prod_i;
                    }
                    if (i == k) { ar[col + i] = mr[b]; ai[col + i] = mi[b]; }
                    else if (below) { ar[col + i] = outr; ai[col + i] = outi; }
                }
            }
            __syncthreads();   // column k+1 is complete before the next pivot search reads it
        }
        return fabs(ar[(NT - 1) * NT + (NT - 1)]) + fabs(ai[(NT - 1) * NT + (NT - 1)]) != 0.0;
    }

    // lin_solve_complex (src/matrix/linear.rs:140-217): (br + i bi), this lane's entry of the two right-hand sides,
    // <- (ar + i ai)^-1 (br + i bi).  Like BdfG::lin_solve the right-hand sides never leave the registers: each of the 2 n
    // sequential pivot steps broadcasts ONE complex entry and every lane applies one complex column axpy to the row it owns.
    static __device__ __forceinline__ void lin_solve_complex(const double *ar, const double *ai, const uint32_t *piv, double &br, double &bi)
    {
        const int i = gl(), r = row();
#pragma unroll 4
        for (int k = 0; k < NT - 1; ++k) {
            const double cr = ar[k * NT + r], ci = ai[k * NT + r];
            const int m = (int)piv[k];
            const double kr = BG::lane_bcast(br, k), ki = BG::lane_bcast(bi, k);
            const double tr = BG::lane_bcast(br, m), ti = BG::lane_bcast(bi, m);
            double xr = i == m ? kr : br, xi = i == m ? ki : bi;
            xr = i == k ? tr : xr;
            xi = i == k ? ti : xi;
            const double prod_r = cr * tr - ci * ti;
            const double prod_i = ci * tr + cr * ti;
            br = i > k ? xr + prod_r : xr;
            bi = i > k ? xi + prod_i : xi;
        }
#pragma unroll 4
        for (int k = NT - 1; k >= 1; --k) {
            const double cr = ar[k * NT + r], ci = ai[k * NT + r];
            const double dr = ar[k * NT + k], di = ai[k * NT + k];
            double kr = BG::lane_bcast(br, k), ki = BG::lane_bcast(bi, k);
            radau_cdiv(dr, di, kr, ki);
            const double tr = -kr, ti = -ki;
            const double prod_r = cr * tr - ci * ti;
            const double prod_i = ci * tr + cr * ti;
            br = i == k ? kr : (i < k ? br + prod_r : br);
            bi = i == k ? ki : (i < k ? bi + prod_i : bi);
        }
        {
            double kr = BG::lane_bcast(br, 0), ki = BG::lane_bcast(bi, 0);
            radau_cdiv(ar[0], ai[0], kr, ki);
            if (i == 0) { br = kr; bi = ki; }
        }
        if (!own()) { br = 0.0; bi = 0.0; }
    }
};

// the bodies ask HasMass about the functor they run on, GroupRhs<R, G>: it has a mass matrix when R has the column hook
template <class R, int G>
struct HasMass<GroupRhs<R, G>, void> { enum { v = HasMassCol<R>::v }; };

// The group form of the attempt's policy (radau_core.h): J and the write-through copies of the factors in the trajectory's
// global block, the factors and pivots the solves read in the group's LDS, one row per lane.
template <class R, int G>
struct RadauOpsLds {
    using RG = RadauG<R, G>;
    using BG = BdfG<R, G>;
    enum { NT = RG::NT, NN = RG::NN, MASS = HasMassCol<R>::v, NMAT = MASS ? 5 : 4 };   // matrices in a trajectory's global block
    double *jac, *fac_mem, *fac;     // global: J, then E1, E2r, E2i (then M); LDS: E1, E2r, E2i
    uint32_t *piv_mem, *piv;         // global and LDS: the pivot rows of E1, then of E2
    struct Factor {};                // the factors are resident: nothing to hand back

    static __device__ __forceinline__ void init_piv(const IvpKArgs &a, size_t, uint32_t j)
    {
        for (int e = RG::gl(); e < 2 * NT; e += G) radau_piv(a)[(size_t)j * 2 * NT + e] = 0u;
    }
    static __device__ __forceinline__ void init_mat(const IvpKArgs &a, size_t, uint32_t j)
    {
        double *jac0 = radau_mat(a) + (size_t)j * NMAT * NN;
        for (int e = RG::gl(); e < NN; e += G) jac0[e] = 0.0;
    }
    // MASS only: this lane's scal and the group's hhfac, behind cont, h_acc and err_acc (radau_scal_at, slot 5 n + 2)
    static __device__ __forceinline__ void init_scal(const IvpKArgs &a, size_t B, uint32_t j)
    {
        using MAP = typename OutMap<GroupRhs<R, G>>::type;
        if (MAP::own(0)) radau_cont(a)[radau_scal_at<MAP>(0, B, j)] = 0.0;
        radau_cont(a)[(size_t)(5 * NT + 2) * B + j] = 0.0;
    }
    // f.mass() is called once, on a zeroed Matrix (radau.rs:283, :359): M is zeroed by the whole group, then
    // lane c fills columns c, c + G, ... the way BdfG::eval_jac calls jac_col -- entries the hook does not write stay 0.0
    static __device__ __forceinline__ void init_mass(const IvpKArgs &a, size_t, uint32_t j, const double *p)
    {
        double *m0 = radau_mat(a) + ((size_t)j * NMAT + 4) * NN;
        for (int e = RG::gl(); e < NN; e += G) m0[e] = 0.0;
        __syncthreads();   // the zeroes have landed before another lane's column does
        for (int col = RG::gl(); col < NT; col += G) R::mass_col(col, m0 + (size_t)col * NT, p);
        __syncthreads();
    }
    static __device__ __forceinline__ double tolst(const IvpKArgs &a, const double (&)[RG::C])   // component 0's, in every lane
    {
        return 0.1 * ivp_pow(a.rtol_dev ? a.rtol_dev[0] : a.rtol[0], 2.0 / 3.0);
    }
    __device__ __forceinline__ uint32_t begin(const IvpKArgs &a, size_t, uint32_t j)
    {
        const uint32_t flags = a.flags[j];
        jac = radau_mat(a) + (size_t)j * NMAT * NN;
        fac_mem = jac + NN;
        piv_mem = radau_piv(a) + (size_t)j * 2 * NT;
        fac = RG::factors();
        piv = RG::pivots();
        if (!(flags & IVP_RAD_CALLDEC)) {   // factors computed by an earlier launch: fetch them (coalesced)
#pragma unroll 8
            for (int e = RG::gl(); e < 3 * NN; e += G) fac[e] = fac_mem[e];
            for (int e = RG::gl(); e < 2 * NT; e += G) piv[e] = piv_mem[e];
        }
        if constexpr (MASS) {   // M is constant and always valid: every launch brings it in (coalesced)
            double *ms = RG::mass();
            const double *m0 = jac + 4 * NN;
#pragma unroll 8
            for (int e = RG::gl(); e < NN; e += G) ms[e] = m0[e];
        }
        __syncthreads();
        return flags;
    }
    // every lane has read the counters it started from (nstep0, naccpt0) before lane 0 updates them
    static __device__ __forceinline__ uint32_t settle(uint32_t j) { __syncthreads(); return j; }
    __device__ __forceinline__ void end(const IvpKArgs &, size_t, uint32_t) const {}
    static __device__ __forceinline__ bool counts() { return RG::gl() == 0; }

    __device__ __forceinline__ void eval_jac(const IvpKArgs &, uint32_t, double x, const double (&y)[RG::C], const double *p) const { BG::eval_jac(x, y, p, jac); }
    // E1, E2r and E2i are assembled together (one pass over J; lane <-> row: each column is one coalesced load), then E1 is
    // factorised ...  (MASS: e1 = m fac1 - j, e2r = m alphn - j, e2i = m betan with m = M[i][c] from LDS)
    __device__ __forceinline__ bool decomp_e1(const IvpKArgs &, uint32_t, double fac1, double alphn, double betan, uint32_t &nlu, Factor &) const
    {
        double *e1 = fac, *e2r = fac + NN, *e2i = fac + 2 * NN;
        const int i = RG::gl();
        __syncthreads();
        if (RG::own()) {
#pragma unroll 8
            for (int c = 0; c < NT; ++c) {
                const double jv = jac[c * NT + i];
                double id;
                if constexpr (MASS) id = RG::mass()[c * NT + i];
                else id = i == c ? 1.0 : 0.0;
                e1[c * NT + i] = id * fac1 - jv;
                e2r[c * NT + i] = id * alphn - jv;
                e2i[c * NT + i] = id * betan;
            }
        }
        nlu += 1;
        return BG::lu_decomp(e1, piv);
    }
    // ... and E2, after which both factors go to the global block
    __device__ __forceinline__ bool decomp_e2(const IvpKArgs &, uint32_t, double, double, uint32_t &nlu, Factor &, Factor &) const
    {
        const int i = RG::gl();
        nlu += 1;
        if (!RG::lu_decomp_complex(fac + NN, fac + 2 * NN, piv + NT)) return false;
        // write-through: the only attempts that use factors they did not compute follow an acceptance that cleared
        // call_decomp, possibly in another launch -- both factors are current then
        __syncthreads();
#pragma unroll 8
        for (int e = i; e < 3 * NN; e += G) fac_mem[e] = fac[e];
        for (int e = i; e < 2 * NT; e += G) piv_mem[e] = piv[e];
        return true;
    }
    __device__ __forceinline__ void load_e1(const IvpKArgs &, uint32_t, Factor &) const {}
    __device__ __forceinline__ void solve_e1(const Factor &, double (&b)[RG::C]) const { BG::lin_solve(fac, piv, b); }
    __device__ __forceinline__ void solve_e2(const IvpKArgs &, uint32_t, double (&br)[RG::C], double (&bi)[RG::C]) const { RG::lin_solve_complex(fac + NN, fac + 2 * NN, piv + NT, br[0], bi[0]); }
    // mass contributions over ALL j, the identity's zeros multiplied out (MASS: row i of M, one conflict-free LDS read per
    // j across the owning lanes): f1, f2, f3 are published as three n-vectors
    __device__ __forceinline__ void mass_row3(const IvpKArgs &, uint32_t, int, const double (&f1)[RG::C], const double (&f2)[RG::C], const double (&f3)[RG::C],
                                              double &sum1, double &sum2, double &sum3) const
    {
        const int i = RG::gl();
        double *fv = RG::fvec();
        __syncthreads();
        if (RG::own()) { fv[i] = f1[0]; fv[NT + i] = f2[0]; fv[2 * NT + i] = f3[0]; }
        __syncthreads();
        sum1 = 0.0; sum2 = 0.0; sum3 = 0.0;
#pragma unroll 8
        for (int jj = 0; jj < NT; ++jj) {
            double mij;
            if constexpr (MASS) mij = RG::mass()[jj * NT + RG::row()];
            else mij = i == jj ? 1.0 : 0.0;
            sum1 -= mij * fv[jj];
            sum2 -= mij * fv[NT + jj];
            sum3 -= mij * fv[2 * NT + jj];
        }
    }
    __device__ __forceinline__ double mass_row(const IvpKArgs &, uint32_t, int, const double (&f)[RG::C]) const
    {
        const int i = RG::gl();
        double *fv = RG::fvec();
        __syncthreads();
        if (RG::own()) fv[i] = f[0];
        __syncthreads();
        double sum = 0.0;
#pragma unroll 8
        for (int jj = 0; jj < NT; ++jj) {
            if constexpr (MASS) sum += RG::mass()[jj * NT + RG::row()] * fv[jj];
            else sum += (i == jj ? 1.0 : 0.0) * fv[jj];
        }
        return sum;
    }
};

// ---- 64 < n <= 512: C rows per lane, every matrix in global memory ------------------------------------------------------------

template <class R, int G>
struct RadauW {
    using GR = GroupRhs<R, G>;
    using BG = BdfG<R, G>;
    enum { NT = R::N, C = GR::N, NN = R::N * R::N };
    static_assert(G == IVP_WAVE, "RadauW: one wavefront per trajectory");
    static_assert(C > 1 && C <= 8, "RadauW: 64 < n <= 512 (up to 8 rows per lane)");
    static __device__ __forceinline__ int gl() { return GR::gl(); }
    static __device__ __forceinline__ int gi(int c) { return GR::gl() + G * c; }
    static __device__ __forceinline__ bool own(int c) { return gi(c) < NT; }

    // f1, f2, f3 of the mass contributions, published once per Newton pass: 3 n doubles, 12 KB at n = 512
    static __device__ __forceinline__ double *fvec()
    {
        __shared__ double ivp_radw_f[3 * NT];
        return ivp_radw_f;
    }

    // lu_decomp_complex (src/matrix/lu.rs:178-302) in place on the column-major pair (ar, ai) in GLOBAL memory; pivots to
    // piv[0..NT-2].  The pivot search, the reciprocal and the three multiplier operation sequences are RadauG's; the search
    // runs over C slots per lane (one group_max, one ballot per slot, the lowest row wins across slots: BdfG::lu_decomp).
    // Every entry is only ever touched by the lane that owns its row.
    // Trailing update, after BdfG::lu_decomp: a column j > k changes only if its pivot-row entry is non-zero (the reference's
    // guard, |mr| + |mi| != 0) or if the row exchange moves two different values.  One strided load per 64 columns brings
    // rows m and k of the trailing columns (lane <-> column), a ballot turns them into a mask; the pivot-row entry of a
    // flagged column then comes out of those registers by v_readlane -- it is wave-uniform, so which of the three
    // multiplier cases a column takes is a SCALAR branch -- and only flagged columns are read, updated and written, JB at a
    // time, all loads of a block before its first store.
    static __device__ __forceinline__ bool lu_decomp_complex(double *ar, double *ai, uint32_t *piv)
    {
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < NT - 1; ++k) {
            double ckr[C], cki[C], v[C], av[C], lv = -1.0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const size_t at = (size_t)k * NT + (own(c) ? gi(c) : NT - 1);   // rows >= n read a clamped address
                ckr[c] = ar[at]; cki[c] = ai[at];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int i = gi(c);
                v[c] = fabs(ckr[c]) + fabs(cki[c]);
                av[c] = (i >= k && i < NT && v[c] == v[c]) ? v[c] : -1.0;
                lv = av[c] > lv ? av[c] : lv;
            }
            const double vkk = BG::row_bcast(v, k, 0);
            const double vmax = BG::group_max(lv);
            int first = NT;
#pragma unroll
            for (int c = C - 1; c >= 0; --c) {
                const unsigned long long hit = __ballot(av[c] == vmax);
                if (hit != 0ull) first = G * c + __ffsll((long long)hit) - 1;
            }
            int m = k;
            if (vkk == vkk && vmax >= 0.0) m = first;   // a NaN at [k][k]: every `>` of the reference's scan is false
            const double pr = BG::row_bcast(ckr, m, 0), pi = BG::row_bcast(cki, m, 0);
            if (gl() == 0) piv[k] = (uint32_t)m;
            if (fabs(pr) + fabs(pi) == 0.0) return false;
            const double akr = BG::row_bcast(ckr, k, 0), aki = BG::row_bcast(cki, k, 0);
            const double den = pr * pr + pi * pi;   // 1 / (tr + i ti) = (tr / den, -ti / den)
            const double tr = pr / den;
            const double ti = -pi / den;
            double lr[C], li[C];
            bool is_m[C], below[C], is_k[C], in_range[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int i = gi(c);
                is_m[c] = i == m; below[c] = i > k && i < NT; is_k[c] = i == k; in_range[c] = i < NT;
                // this row's multiplier; row m holds row k's entry after the exchange
                const double er = is_m[c] ? akr : ckr[c], ei = is_m[c] ? aki : cki[c];
                lr[c] = -(er * tr - ei * ti);
                li[c] = -(ei * tr + er * ti);
                if (is_k[c]) { ar[(size_t)k * NT + i] = pr; ai[(size_t)k * NT + i] = pi; }
                else if (below[c]) { ar[(size_t)k * NT + i] = lr[c]; ai[(size_t)k * NT + i] = li[c]; }
            }
            // rows m and k of ALL trailing columns first (one round trip), then segment by segment; processing a segment
            // only writes that segment's columns
            constexpr int SEG = C;
            double tmr[SEG], tmi[SEG], tkr[SEG], tki[SEG];
#pragma unroll
            for (int sg = 0; sg < SEG; ++sg) {
                const int jj = k + 1 + sg * G + gl();
                tmr[sg] = 0.0; tmi[sg] = 0.0; tkr[sg] = 0.0; tki[sg] = 0.0;
                if (jj < NT) {
                    tmr[sg] = ar[(size_t)jj * NT + m]; tmi[sg] = ai[(size_t)jj * NT + m];
                    tkr[sg] = ar[(size_t)jj * NT + k]; tki[sg] = ai[(size_t)jj * NT + k];
                }
            }
            constexpr int JB = C <= 4 ? 4 : 2;
#pragma unroll 1
            for (int sg = 0; sg < SEG; ++sg) {
                const int j0 = k + 1 + sg * G;
                if (j0 >= NT) break;
                const int jj = j0 + gl();
                double smr = tmr[0], smi = tmi[0], skr = tkr[0], ski = tki[0];   // select chain instead of a run-time register index
#pragma unroll
                for (int q = 1; q < SEG; ++q) {
                    smr = sg == q ? tmr[q] : smr; smi = sg == q ? tmi[q] : smi;
                    skr = sg == q ? tkr[q] : skr; ski = sg == q ? tki[q] : ski;
                }
                const bool need = jj < NT && (fabs(smr) + fabs(smi) != 0.0 || (m != k && (d2u(smr) != d2u(skr) || d2u(smi) != d2u(ski))));
                unsigned long long todo = __ballot(need);
#pragma unroll 1
                while (todo != 0ull) {
                    int jc[JB];
                    bool act[JB];
                    double mr[JB], mi[JB], kr[JB], ki[JB], cr[JB][C], ci[JB][C];
#pragma unroll
                    for (int b = 0; b < JB; ++b) {
                        act[b] = todo != 0ull;
                        const int bit = act[b] ? __ffsll((long long)todo) - 1 : 0;
                        jc[b] = j0 + bit;
                        todo &= todo - 1ull;
                        mr[b] = BG::lane_bcast(smr, bit); mi[b] = BG::lane_bcast(smi, bit);
                        kr[b] = BG::lane_bcast(skr, bit); ki[b] = BG::lane_bcast(ski, bit);
                    }
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        if (G * c + (G - 1) < k) continue;   // whole slot above the pivot row (scalar test)
#pragma unroll
                        for (int b = 0; b < JB; ++b) {
                            cr[b][c] = 0.0; ci[b][c] = 0.0;
                            if (act[b] && in_range[c]) { cr[b][c] = ar[(size_t)jc[b] * NT + gi(c)]; ci[b][c] = ai[(size_t)jc[b] * NT + gi(c)]; }
                        }
                    }
#pragma unroll
                    for (int b = 0; b < JB; ++b) {
                        if (!act[b]) continue;
                        const bool upd = fabs(mr[b]) + fabs(mi[b]) != 0.0;
                        const int kind = mi[b] == 0.0 ? 0 : (mr[b] == 0.0 ? 1 : 2);   // real, imaginary, general: wave-uniform
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            if (G * c + (G - 1) < k) continue;
                            const double vr = is_m[c] ? kr[b] : cr[b][c], vi = is_m[c] ? ki[b] : ci[b][c];   // the row exchange
                            double outr = vr, outi = vi;
                            if (upd) {
                                double prod_r, prod_i;
                                if (kind == 0) {          // real multiplier
                                    prod_r = lr[c] * mr[b];
                                    prod_i = li[c] * mr[b];
                                } else if (kind == 1) {   // imaginary multiplier
                                    prod_r = -li[c] * mi[b];
                                    prod_i = lr[c] * mi[b];
                                } else {                  // general complex multiplier
                                    prod_r = lr[c] * mr[b] - li[c] * mi[b];
                                    prod_i = li[c] * mr[b] + lr[c] * mi[b];
                                }
                                outr = below[c] ? vr + prod_r : vr;
                                outi = below[c] ? vi + prod_i : vi;
                            }
                            outr = is_k[c] ? mr[b] : outr;
                            outi = is_k[c] ? mi[b] : outi;
                            if (in_range[c]) { ar[(size_t)jc[b] * NT + gi(c)] = outr; ai[(size_t)jc[b] * NT + gi(c)] = outi; }
                        }
                    }
                }
            }
            __syncthreads();   // column k+1 is complete before the next pivot search reads it
        }
        return fabs(ar[(size_t)(NT - 1) * NT + (NT - 1)]) + fabs(ai[(size_t)(NT - 1) * NT + (NT - 1)]) != 0.0;
    }

    // lin_solve_complex (src/matrix/linear.rs:140-217): (br + i bi), this lane's rows of the two right-hand sides,
    // <- (ar + i ai)^-1 (br + i bi).  The right-hand sides never leave the registers; the 2 n pivot steps are walked in blocks
    // of G like BdfG::lin_solve (slots below the block are not touched, the block's own slot is the only one that needs the
    // row mask), the pivot indices sit in registers (one coalesced load) and are read with v_readlane, entries are
    // broadcast by row_bcast, whole columns of the factors are fetched PF steps ahead without masks.
    enum { PF = C <= 2 ? 4 : 2 };
    static __device__ __forceinline__ void lin_solve_complex(const double *ar, const double *ai, const uint32_t *piv, double (&br)[C], double (&bi)[C])
    {
        int row[C];
        uint32_t pv[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            row[c] = own(c) ? gi(c) : NT - 1;
            pv[c] = gi(c) < NT - 1 ? piv[gi(c)] : 0u;
        }
        // forward: row exchange m <-> k, then b[i] += l[i][k] * b[k] for i > k
#pragma unroll
        for (int kb = 0; kb < C; ++kb) {
            const int kend = (kb + 1) * G < NT - 1 ? (kb + 1) * G : NT - 1;
            if (kb * G >= NT - 1) break;
            double qr[PF][C], qi[PF][C];
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int k = kb * G + u < NT ? kb * G + u : NT - 1;
#pragma unroll
                for (int c = kb; c < C; ++c) { qr[u][c] = ar[(size_t)k * NT + row[c]]; qi[u][c] = ai[(size_t)k * NT + row[c]]; }
            }
#pragma unroll 1
            for (int k0 = kb * G; k0 < kend; k0 += PF) {
#pragma unroll
                for (int u = 0; u < PF; ++u) {
                    const int k = k0 + u;
                    if (k < kend) {
                        double cr[C], ci[C];
#pragma unroll
                        for (int c = kb; c < C; ++c) { cr[c] = qr[u][c]; ci[c] = qi[u][c]; }
                        const int kn = k + PF;
                        if (kn < kend) {
#pragma unroll
                            for (int c = kb; c < C; ++c) { qr[u][c] = ar[(size_t)kn * NT + row[c]]; qi[u][c] = ai[(size_t)kn * NT + row[c]]; }
                        }
                        const int m = (int)BG::lane_bcast(pv[kb], k - kb * G);
                        const double kr = BG::lane_bcast(br[kb], k - kb * G), ki = BG::lane_bcast(bi[kb], k - kb * G);
                        const double tr = BG::row_bcast(br, m, kb), ti = BG::row_bcast(bi, m, kb);
                        {
                            const int i = gi(kb);
                            double xr = i == m ? kr : br[kb], xi = i == m ? ki : bi[kb];
                            xr = i == k ? tr : xr;
                            xi = i == k ? ti : xi;
                            const double prod_r = cr[kb] * tr - ci[kb] * ti;
                            const double prod_i = ci[kb] * tr + cr[kb] * ti;
                            br[kb] = i > k ? xr + prod_r : xr;
                            bi[kb] = i > k ? xi + prod_i : xi;
                        }
#pragma unroll
                        for (int c = kb + 1; c < C; ++c) {
                            const double xr = gi(c) == m ? kr : br[c], xi = gi(c) == m ? ki : bi[c];
                            const double prod_r = cr[c] * tr - ci[c] * ti;
                            const double prod_i = ci[c] * tr + cr[c] * ti;
                            br[c] = xr + prod_r;
                            bi[c] = xi + prod_i;
                        }
                    }
                }
            }
        }
        // backward: b[k] /= u[k][k], then b[i] -= u[i][k] * b[k] for i < k
#pragma unroll
        for (int kb = C - 1; kb >= 0; --kb) {
            const int ktop = (kb + 1) * G - 1 < NT - 1 ? (kb + 1) * G - 1 : NT - 1;   // first (highest) row of the block
            const int kbot = kb == 0 ? 1 : kb * G;                                      // last row the loop handles (row 0: below)
            if (kb * G > NT - 1) continue;
            double qr[PF][C], qi[PF][C], dqr[PF], dqi[PF];
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int k = ktop - u >= 0 ? ktop - u : 0;
                dqr[u] = ar[(size_t)k * NT + k]; dqi[u] = ai[(size_t)k * NT + k];
#pragma unroll
                for (int c = 0; c <= kb; ++c) { qr[u][c] = ar[(size_t)k * NT + row[c]]; qi[u][c] = ai[(size_t)k * NT + row[c]]; }
            }
#pragma unroll 1
            for (int k0 = ktop; k0 >= kbot; k0 -= PF) {
#pragma unroll
                for (int u = 0; u < PF; ++u) {
                    const int k = k0 - u;
                    if (k >= kbot) {
                        double cr[C], ci[C];
                        const double dr = dqr[u], di = dqi[u];
#pragma unroll
                        for (int c = 0; c <= kb; ++c) { cr[c] = qr[u][c]; ci[c] = qi[u][c]; }
                        const int kn = k - PF;
                        if (kn >= kbot) {
                            dqr[u] = ar[(size_t)kn * NT + kn]; dqi[u] = ai[(size_t)kn * NT + kn];
#pragma unroll
                            for (int c = 0; c <= kb; ++c) { qr[u][c] = ar[(size_t)kn * NT + row[c]]; qi[u][c] = ai[(size_t)kn * NT + row[c]]; }
                        }
                        double kr = BG::lane_bcast(br[kb], k - kb * G), ki = BG::lane_bcast(bi[kb], k - kb * G);
                        radau_cdiv(dr, di, kr, ki);
                        const double tr = -kr, ti = -ki;
                        {
                            const int i = gi(kb);
                            const double prod_r = cr[kb] * tr - ci[kb] * ti;
                            const double prod_i = ci[kb] * tr + cr[kb] * ti;
                            br[kb] = i == k ? kr : (i < k ? br[kb] + prod_r : br[kb]);
                            bi[kb] = i == k ? ki : (i < k ? bi[kb] + prod_i : bi[kb]);
                        }
#pragma unroll
                        for (int c = 0; c < kb; ++c) {
                            const double prod_r = cr[c] * tr - ci[c] * ti;
                            const double prod_i = ci[c] * tr + cr[c] * ti;
                            br[c] = br[c] + prod_r;
                            bi[c] = bi[c] + prod_i;
                        }
                    }
                }
            }
        }
        {
            double kr = BG::lane_bcast(br[0], 0), ki = BG::lane_bcast(bi[0], 0);
            radau_cdiv(ar[0], ai[0], kr, ki);
            if (gi(0) == 0) { br[0] = kr; bi[0] = ki; }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) if (!own(c)) { br[c] = 0.0; bi[c] = 0.0; }
    }
};

// The wide form of the attempt's policy: J, E1, E2r, E2i in the trajectory's global block ([B][4 n n], column-major), the
// pivot rows of E1 and of E2 in the global [B][2][n] array, C rows per lane.  There is no LDS copy of anything that
// outlives an attempt, so begin() fetches nothing and decomp_e2 writes nothing through.
template <class R, int G>
struct RadauOpsWide {
    using RW = RadauW<R, G>;
    using BG = BdfG<R, G>;
    enum { NT = RW::NT, NN = RW::NN, C = RW::C, NMAT = 4 };
    static_assert(!HasMassCol<R>::v, "Radau for 64 < n <= 512: pure ODEs with the identity mass (mass_col stays at n <= 64)");
    double *jac, *fac;     // global: J; E1, E2r, E2i
    uint32_t *piv;         // global: the pivot rows of E1, then of E2
    mutable double ms1[C], ms2[C], ms3[C];   // the mass contributions of this lane's rows, formed on the call for row 0
    struct Factor {};

    static __device__ __forceinline__ void init_piv(const IvpKArgs &a, size_t, uint32_t j)
    {
        for (int e = RW::gl(); e < 2 * NT; e += G) radau_piv(a)[(size_t)j * 2 * NT + e] = 0u;
    }
    static __device__ __forceinline__ void init_mat(const IvpKArgs &a, size_t, uint32_t j)
    {
        double *jac0 = radau_mat(a) + (size_t)j * NMAT * NN;
        for (int e = RW::gl(); e < NN; e += G) jac0[e] = 0.0;
    }
    static __device__ __forceinline__ double tolst(const IvpKArgs &a, const double (&)[C])   // component 0's, in every lane
    {
        return 0.1 * ivp_pow(a.rtol_dev ? a.rtol_dev[0] : a.rtol[0], 2.0 / 3.0);
    }
    __device__ __forceinline__ uint32_t begin(const IvpKArgs &a, size_t, uint32_t j)
    {
        jac = radau_mat(a) + (size_t)j * NMAT * NN;
        fac = jac + NN;
        piv = radau_piv(a) + (size_t)j * 2 * NT;
        return a.flags[j];
    }
    static __device__ __forceinline__ uint32_t settle(uint32_t j) { __syncthreads(); return j; }
    __device__ __forceinline__ void end(const IvpKArgs &, size_t, uint32_t) const {}
    static __device__ __forceinline__ bool counts() { return RW::gl() == 0; }

    // forward differences keep their KJ state copies where BDF's global-memory form does: in LDS (32 KB at n = 512)
    __device__ __forceinline__ void eval_jac(const IvpKArgs &, uint32_t, double x, const double (&y)[C], const double *p) const { BG::eval_jac(x, y, p, jac); }
    // E1, E2r and E2i are assembled together, element by element over the column-major blocks (coalesced, FB loads in flight
    // per lane), then E1 is factorised ...
    __device__ __forceinline__ bool decomp_e1(const IvpKArgs &, uint32_t, double fac1, double alphn, double betan, uint32_t &nlu, Factor &) const
    {
        double *e1 = fac, *e2r = fac + NN, *e2i = fac + 2 * NN;
        __syncthreads();   // J is complete; nobody still reads the old factors
        constexpr int FB = 8;
#pragma unroll 1
        for (int e0 = 0; e0 < NN; e0 += FB * G) {
            double jv[FB];
#pragma unroll
            for (int u = 0; u < FB; ++u) { const int e = e0 + u * G + RW::gl(); jv[u] = e < NN ? jac[e] : 0.0; }
#pragma unroll
            for (int u = 0; u < FB; ++u) {
                const int e = e0 + u * G + RW::gl();
                const int col = e / NT, r = e - col * NT;
                const double id = r == col ? 1.0 : 0.0;   // the identity's zeros are multiplied out: 0.0 * inf is a NaN
                if (e < NN) {
                    e1[e] = id * fac1 - jv[u];
                    e2r[e] = id * alphn - jv[u];
                    e2i[e] = id * betan;
                }
            }
        }
        nlu += 1;
        return BG::lu_decomp(e1, piv);
    }
    // ... and E2
    __device__ __forceinline__ bool decomp_e2(const IvpKArgs &, uint32_t, double, double, uint32_t &nlu, Factor &, Factor &) const
    {
        nlu += 1;
        return RW::lu_decomp_complex(fac + NN, fac + 2 * NN, piv + NT);
    }
    __device__ __forceinline__ void load_e1(const IvpKArgs &, uint32_t, Factor &) const {}
    __device__ __forceinline__ void solve_e1(const Factor &, double (&b)[C]) const { BG::lin_solve(fac, piv, b); }
    __device__ __forceinline__ void solve_e2(const IvpKArgs &, uint32_t, double (&br)[C], double (&bi)[C]) const { RW::lin_solve_complex(fac + NN, fac + 2 * NN, piv + NT, br, bi); }
    // mass contributions over ALL j, the identity's zeros multiplied out.  The bodies ask row by row (local row i = 0 .. C-1,
    // a constant after unrolling) with the same f1, f2, f3: they are published ONCE, on the call for row 0, and that call
    // sums over all j for every row this lane owns -- one pass over the three n-vectors in LDS.
    __device__ __forceinline__ void mass_row3(const IvpKArgs &, uint32_t, int i, const double (&f1)[C], const double (&f2)[C], const double (&f3)[C],
                                              double &sum1, double &sum2, double &sum3) const
    {
        if (i == 0) {
            double *fv = RW::fvec();
            __syncthreads();
#pragma unroll
            for (int c = 0; c < C; ++c) if (RW::own(c)) { fv[RW::gi(c)] = f1[c]; fv[NT + RW::gi(c)] = f2[c]; fv[2 * NT + RW::gi(c)] = f3[c]; }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < C; ++c) { ms1[c] = 0.0; ms2[c] = 0.0; ms3[c] = 0.0; }
#pragma unroll 2
            for (int jj = 0; jj < NT; ++jj) {
                const double v1 = fv[jj], v2 = fv[NT + jj], v3 = fv[2 * NT + jj];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const double mij = RW::gi(c) == jj ? 1.0 : 0.0;
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
            double *fv = RW::fvec();
            __syncthreads();
#pragma unroll
            for (int c = 0; c < C; ++c) if (RW::own(c)) fv[RW::gi(c)] = f[c];
            __syncthreads();
#pragma unroll
            for (int c = 0; c < C; ++c) ms1[c] = 0.0;
#pragma unroll 2
            for (int jj = 0; jj < NT; ++jj) {
                const double v = fv[jj];
#pragma unroll
                for (int c = 0; c < C; ++c) ms1[c] += (RW::gi(c) == jj ? 1.0 : 0.0) * v;
            }
        }
        return ms1[i];
    }
};

// one row per lane with the factors in LDS (G >= n), or C rows per lane with every matrix in global memory -- or, for a
// functor that carries SP_ML / SP_MU (HasBand, bdf_group.h), band storage at every width (radau_band.h, included after
// this header by the modules of such functors only: nothing else names RadauOpsBand)
template <class R, int G>
struct RadauOpsBand;
template <class R, int G, int FORM>
struct RadauOpsGroupSel { using type = RadauOpsLds<R, G>; };
template <class R, int G>
struct RadauOpsGroupSel<R, G, 1> { using type = RadauOpsWide<R, G>; };
template <class R, int G>
struct RadauOpsGroupSel<R, G, 2> { using type = RadauOpsBand<R, G>; };
template <class R, int G>
struct RadauOps<GroupRhs<R, G>> : RadauOpsGroupSel<R, G, HasBand<R>::v ? 2 : (GroupRhs<R, G>::N > 1 ? 1 : 0)>::type {};

}  // namespace IVP_NS
