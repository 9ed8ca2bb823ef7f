// The sums of the Gauss-Newton direction check of a batch on the caller's device buffers (gn_direction_batched.inc; the routines:
// gn_direction_check.hpp): what search_direction_analys (src/enlsip_functions.jl:1222-1231) and check_gn_direction (:943-1030) read
// of b, d, lambda, diag_scale and cx.  The decision itself is made on the host from the downloaded record.  The problem index is
// carried in gridDim.x.
//
// Every sum of a problem belongs to ONE wave, which takes it in the documented order (lane s adds the terms s, s + 64, ... in
// ascending order from +0.0, then the butterfly), so both forms give the bytes of enlsip_gn_direction_sums:
//   general   k_dir_general   one workgroup of four waves per problem.  Wave 0: ONE pass over d, three accumulators (every entry,
//                             j < dimJ2, j < k_prev); wave 1: dot(b1, b1) and the sum over the active list; wave 2: the two
//                             multiplier counts; wave 3: the inactive count.  Each wave's lane 0 writes its own fields of the
//                             record: no LDS, no barrier.
//   wave      k_dir_wave      one wave per problem, four problems per 256-thread workgroup, one launch; the same four bodies one
//                             after the other.  m <= DIR_WAVE_MAX_M, l <= 64, t_max <= 64.
// The index lists are read straight from the uploaded records, one entry per lane.  No floating-point atomics; products and
// additions are rounded on their own (fp contract off where they are formed).
#pragma once
#include "gn_batch_records.hpp"
#include "gn_device_utils.hpp"
#include "gn_direction_check.hpp"
#include "gn_kernels_termination_batched.hpp"

namespace gn {

constexpr int DIR_WAVE_MAX_M = 1024;      // the wave form's bound on m: 16 entries of d per lane.  Not result-changing.

struct DirectionArgs {
    const DirMeta* meta;
    const int* act;             // batch x l
    const int* inact;           // batch x l
    enlsip_gn_dir_sums* out;
    int count, m, l, t_max, scaling;
    const double* b;            // stride t_max
    const double* d;            // stride m
    const double *lambda, *diag_scale;      // stride t_max
    const double* cx_all;       // stride l
};

enum { DIR_G_D = 1, DIR_G_ACTIVE = 2, DIR_G_MULT = 4, DIR_G_INACTIVE = 8, DIR_G_ALL = 15 };

// The groups `groups` of problem k by ONE wave.
__device__ __forceinline__ void dir_wave_sums(const DirectionArgs& a, long long k, const DirMeta& mt, int ln, int groups) {
#pragma clang fp contract(off)
    enlsip_gn_dir_sums* o = a.out + k;
    const int l = a.l, t = mt.t;
    if (groups & DIR_G_D) {
        const double* d = a.d + k * a.m;
        double s_all = 0.0, s_1 = 0.0, s_prev = 0.0;
        for (int j = ln; j < a.m; j += WAVE) {
            const double sq = d[j] * d[j];
            s_all = s_all + sq;
            if (j < mt.dimJ2) s_1 = s_1 + sq;
            if (j < mt.k_prev) s_prev = s_prev + sq;
        }
        s_all = wave_allsum(s_all);
        s_1 = wave_allsum(s_1);
        s_prev = wave_allsum(s_prev);
        if (ln == 0) { o->d_sq = s_all; o->d1_sq = s_1; o->d1_asprev_sq = s_prev; }
    }
    if (groups & DIR_G_ACTIVE) {
        const double* b = a.b + k * a.t_max;
        const int* act = a.act + k * l;
        const double* cxn = a.cx_all + k * l;
        const double bb = wave_ordered_sum(mt.dimA, ln, [=](int i) { return b[i] * b[i]; });
        const double cc = wave_ordered_sum(t, ln, [=](int i) {
            const int r = act[i];
            const double c = r ? cxn[r - 1] : 0.0;
            return c * c;
        });
        if (ln == 0) { o->b1_sq = bb; o->active_c_sum = cc; }
    }
    if (groups & DIR_G_MULT) {
        const double* lam = a.lambda + k * a.t_max;
        const double* ds = a.diag_scale + k * a.t_max;
        long long ge = 0, neg = 0;
        for (int i0 = mt.q; i0 < t; i0 += WAVE) {
            const int i = i0 + ln;
            const bool in = i < t;
            const double li = in ? lam[i] : 0.0;
            const double rows = in ? term_rows(ds[i], a.scaling != 0) : 1.0;
            ge += __popcll(__ballot(in && dir_lm_ge(li, rows)));
            neg += __popcll(__ballot(in && li < 0.0));
        }
        if (ln == 0) { o->n_lm_ge = ge; o->n_lm_neg = neg; }
    }
    if (groups & DIR_G_INACTIVE) {
        const int* ina = a.inact + k * l;
        const double* cxn = a.cx_all + k * l;
        const int cnt = l - t;
        long long lt = 0;
        for (int i0 = 0; i0 < cnt; i0 += WAVE) {
            const int i = i0 + ln;
            const int r = i < cnt ? ina[i] : 0;
            const double c = r ? cxn[r - 1] : 1.0;
            lt += __popcll(__ballot(r != 0 && c < GN_DIR_DELTA));
        }
        if (ln == 0) o->n_inactive_lt_delta = lt;
    }
}

// grid: count workgroups
__global__ __launch_bounds__(256) void k_dir_general(DirectionArgs a) {
    const long long k = blockIdx.x;
    const DirMeta mt = a.meta[k];
    if (!mt.take) return;
    dir_wave_sums(a, k, mt, lane_id(), 1 << wave_id());
}

// grid: ceil(count / 4) workgroups
__global__ __launch_bounds__(256) void k_dir_wave(DirectionArgs a) {
    const long long k = (long long)blockIdx.x * 4 + wave_id();
    if (k >= a.count) return;
    const DirMeta mt = a.meta[k];
    if (!mt.take) return;
    dir_wave_sums(a, k, mt, lane_id(), DIR_G_ALL);
}

}  // namespace gn
