// The six dot products of the line search's polynomial fit for a batch on the caller's device buffers
// (gn_linesearch_fit_batched.inc; the elements and the scalar stage: gn_linesearch_fit.hpp): concatenate! (src/enlsip_functions.jl:
// 1635-1659), coefficients_linesearch! (:1665-1689) and the scaling of v1 (:1986-1998), reduced to v0.v0, v0.v1, v0.v2, v1.v1, v1.v2,
// v2.v2 (:1849, :1749-1751).  No vector is materialised and no buffer of the caller is written.
//   k_fit_part    grid problem * nblk + b: the m residual entries by the ordered partial sums of the line-search set-up
//                 (gn_kernels_linesearch_batched.hpp) with six accumulators per thread; six partial sums per workgroup
//   k_fit_total   one wave per problem, four problems per workgroup: the six totals of the partial sums by the fixed-shape
//                 butterfly, then the constraint terms added one by one in list order, active list first (as k_merit_total):
//                 lane i forms the three elements of list position base + i and their six products, and the products are added
//                 to the running sums in position order (v_readlane of lane 0, 1, ...)
// The elements are those of gn_linesearch_fit.hpp, formed with the same unfused operations: an inactive entry is 0 where cx > 0
// (v0, v1: the OLD cx, :1996) or cx_new > 0 (v_buff); v2 = ((vb - v0) / alpha_k - v1) / alpha_k with two IEEE divisions.
// No floating-point atomics: a sum depends on m, l, the lists and the operands alone, never on the slot, the batch or the call.
// The problem index is carried in gridDim.x, so a batch is not bounded by the grid's y limit.  The records (MeritMeta, the two
// lists) are the merit function's, so k_merit_part / k_merit_total run on the same upload when psi of the trial point is wanted.
#pragma once
#include "gn_device_utils.hpp"
#include "gn_kernels_linesearch_batched.hpp"
#include "gn_kernels_penalty_batched.hpp"

namespace gn {

struct FitArgs {
    const MeritMeta* meta;
    const int* act;             // stride t_max: 1-based constraints
    const int* inact;           // stride l
    const double* alpha;        // alpha_k per problem
    double* part;               // 6 * nblk per problem
    double* out;                // 6 per problem
    int count, m, l, t_max, nblk;
    const double* rx;           // stride m
    const double* rx_new;       // stride m
    const double* Jp;           // stride m
    const double* cx;           // stride l
    const double* cx_new;       // stride l
    const double* Ap;           // stride l
    const double* w;            // stride l
};

// the six products of one entry (fit_add_entry of gn_linesearch_fit.hpp, product by product)
__device__ __forceinline__ void fit_products(double v0, double v1, double vb, double al, double (&p)[6]) {
#pragma clang fp contract(off)
    const double v2 = ((vb - v0) / al - v1) / al;                                // :1688
    p[0] = v0 * v0;
    p[1] = v0 * v1;
    p[2] = v0 * v2;
    p[3] = v1 * v1;
    p[4] = v1 * v2;
    p[5] = v2 * v2;
}

__global__ __launch_bounds__(256) void k_fit_part(FitArgs a) {
    __shared__ double ws[6][4];
    const long long k = blockIdx.x / a.nblk;
    const int b = (int)(blockIdx.x % a.nblk);
    if (!a.meta[k].take) return;
    const double* rx = a.rx + k * a.m;
    const double* rn = a.rx_new + k * a.m;
    const double* jp = a.Jp + k * a.m;
    const double al = a.alpha[k];
    ordered_partial_sums<6>(b, a.nblk, a.m, ws, a.part + ((size_t)k * a.nblk + b) * 6, [=](long long i, double (&s)[6]) {
#pragma clang fp contract(off)
        double p[6];
        fit_products(rx[i], jp[i], rn[i], al, p);
#pragma unroll
        for (int q = 0; q < 6; ++q) s[q] = s[q] + p[q];
    });
}

// the terms of `n` list positions added to s one by one: lane i holds position base + i
__device__ __forceinline__ void fit_list_sum(double (&s)[6], const int* list, int n, bool inactive, double al, const double* cx,
                                             const double* cxn, const double* ap, const double* w) {
#pragma clang fp contract(off)
    const int ln = lane_id();
    for (int base = 0; base < n; base += WAVE) {
        const int j = base + ln < n ? list[base + ln] : 0;
        double p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (j != 0) {
            const double sq = sqrt(w[j - 1]);
            const double c = cx[j - 1], cn = cxn[j - 1];
            const bool old_out = inactive && c > 0.0;                            // :1655, :1996: the test is literal
            const double v0 = old_out ? 0.0 : sq * c;
            const double v1 = old_out ? 0.0 : sq * ap[j - 1];
            const double vb = (inactive && cn > 0.0) ? 0.0 : sq * cn;
            fit_products(v0, v1, vb, al, p);
        }
        const int cnt = n - base < WAVE ? n - base : WAVE;
        for (int i = 0; i < cnt; ++i) {
#pragma unroll
            for (int q = 0; q < 6; ++q) s[q] = s[q] + wave_bcast(p[q], i);
        }
    }
}

__global__ __launch_bounds__(256) void k_fit_total(FitArgs a) {
#pragma clang fp contract(off)
    const long long k = (long long)blockIdx.x * 4 + wave_id();
    if (k >= a.count) return;
    const MeritMeta mt = a.meta[k];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (mt.take) {
        if (a.nblk > 0) {
#pragma unroll
            for (int q = 0; q < 6; ++q) s[q] = ordered_partials_total(a.part + (size_t)k * a.nblk * 6, a.nblk, 6, q);
        }
        const double al = a.alpha[k];
        const double* cx = a.cx + k * a.l;
        const double* cxn = a.cx_new + k * a.l;
        const double* ap = a.Ap + k * a.l;
        const double* w = a.w + k * a.l;
        fit_list_sum(s, a.act + k * a.t_max, mt.t, false, al, cx, cxn, ap, w);
        fit_list_sum(s, a.inact + k * a.l, mt.n_inactive, true, al, cx, cxn, ap, w);
    }
    if (lane_id() < 6) {
        double v = s[0];
#pragma unroll
        for (int q = 1; q < 6; ++q) v = lane_id() == q ? s[q] : v;
        a.out[k * 6 + lane_id()] = v;
    }
}

}  // namespace gn
