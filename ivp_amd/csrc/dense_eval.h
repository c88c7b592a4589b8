// dense_eval.h -- the batch's continuous solution (ContinuousOutput, src/solve/cont.rs:9-153) evaluated from the CSR
// dense-output log of ivp_batch_solve_dense*(): segment search and per-component interpolation, shared by the eval
// kernels (dense_eval.hip) and a host build of the same code (tests).
//
// Include after rk_core.h (interpolate<M, N> and the IVP_NS namespace come from there).
//
// CSR layout (include/ivp_hip.h, ivp_dense_log_t): trajectory b's k-th segment is record q = offsets[b] + k with
//     xold[q], h[q], cont[q * (ncoef * n) + ..]    coefficients in the crate's per-segment order: RK [coef][component],
//                                                  BDF per-state blocks [D0, D1..D5, order] (cont.rs:44-51)
//
// PRECONDITION of the search: a trajectory's run is MONOTONE in its integration direction -- every segment's interval
// starts where the one before it ends, all h of one sign.  That holds for every run the solver writes (segments are
// accepted steps in integration order, forward or backward, or the single constant segment of a zero-length interval),
// and it turns the reference's linear scan (find_segment: the FIRST segment with left - tol <= t <= right + tol,
// cont.rs:104-120) into a binary search with the same answer.  Runs assembled by hand that break it get no defined result.
#pragma once

namespace IVP_NS {

enum { IVP_DENSE_NONE = 0, IVP_DENSE_INSIDE = 1, IVP_DENSE_EXTRAPOLATED = 2 };

// The segment of run [lo, lo + cnt) that ContinuousOutput::evaluate (extrapolate = 0) or evaluate_extrapolate
// (extrapolate != 0, cont.rs:122-153) takes for t.  Returns IVP_DENSE_* and the record in *seg.
IVP_HD int dense_find(const double *xold, const double *h, unsigned long long lo, unsigned long long cnt, double t,
                      int extrapolate, unsigned long long *seg)
{
    const double tol = 1e-12;
    if (cnt == 0) return IVP_DENSE_NONE;
    // Forward runs: right + tol grows with k, so "t <= right + tol" is false, then true; the first k where it holds is the
    // only candidate (every later segment starts even further right).  Backward runs: the same with "t >= left - tol".
    const bool fwd = h[lo] > 0.0;
    unsigned long long a = 0, b = cnt;
    while (a < b) {
        const unsigned long long m = a + (b - a) / 2, q = lo + m;
        const double x0 = xold[q], x1 = x0 + h[q];
        const double left = x0 < x1 ? x0 : x1, right = x0 < x1 ? x1 : x0;
        const bool reached = fwd ? (t <= right + tol) : (t >= left - tol);
        if (reached) b = m; else a = m + 1;
    }
    if (a < cnt) {
        const unsigned long long q = lo + a;
        const double x0 = xold[q], x1 = x0 + h[q];
        const double left = x0 < x1 ? x0 : x1, right = x0 < x1 ? x1 : x0;
        if (t >= left - tol && t <= right + tol) { *seg = q; return IVP_DENSE_INSIDE; }
    }
    if (!extrapolate) return IVP_DENSE_NONE;
    // find_segment_extrapolate: before the first segment's left end -> the first, past the last one's right end -> the last
    const double f0 = xold[lo], f1 = f0 + h[lo];
    const unsigned long long ql = lo + cnt - 1;
    const double l0 = xold[ql], l1 = l0 + h[ql];
    const double first_left = f0 < f1 ? f0 : f1, last_right = l0 < l1 ? l1 : l0;
    if (t < first_left) { *seg = lo; return IVP_DENSE_EXTRAPOLATED; }
    if (t > last_right) { *seg = ql; return IVP_DENSE_EXTRAPOLATED; }
    return IVP_DENSE_NONE;
}

// One component's coefficients of a segment as the container interpolate<M, 1> reads: component i of the block at
// `seg` is seg[i + c * n] for the RK methods ([coef][component]) and seg[7 i + c] for BDF (per-state blocks), so that
// the stepping kernels' own interpolant -- not a copy of it -- evaluates a single component.
struct DenseCompView {
    const double *p;
    int stride;
    IVP_HD double operator[](int c) const { return p[(size_t)c * (size_t)stride]; }
};
template <int M>
IVP_HD DenseCompView dense_comp_view(const double *seg, int n, int i)
{
    if constexpr (M == M_BDF) return DenseCompView{seg + (size_t)7 * (size_t)i, 1};
    else return DenseCompView{seg + i, n};
}
template <int M, class CP>
IVP_HD double dense_component(const CP &view, double t, double xold, double h)
{
    double yi[1] = {0.0};
    interpolate<M, 1>(t, yi, view, xold, h);
    return yi[0];
}

}  // namespace IVP_NS
