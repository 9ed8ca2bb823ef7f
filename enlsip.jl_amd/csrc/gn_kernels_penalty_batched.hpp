// The penalty weights and the merit function of a batch on the caller's device buffers (gn_penalty_batched.inc):
//   k_penalty       penalty_weight_update (src/enlsip_functions.jl:1545-1629, gn_penalty_weights.hpp) per taken problem, with the
//                   division active_Ap ./ diag_scale of :2231-2233 in front of it, psi(0) of :2243 and atwa of :2268 behind it
//   k_merit_part,   psi of :1307-1340 on a batch of trial points whose rx and cx are already evaluated: rx.rx by the ordered partial
//   k_merit_total   sums of the line-search set-up (gn_kernels_linesearch_batched.hpp), the constraint sums in list order
// The problem index is carried in gridDim.x, so a batch is not bounded by the grid's y limit.
//
// k_penalty, one group of TPP threads per problem (256 / TPP problems per workgroup), four steps between workgroup barriers that
// every thread reaches whatever its problem is:
//   1  the group gathers the t active entries of w_old, K[4], cx and the t entries of active_Ap (divided by diag_scale where
//      scaling is on) into LDS; its first thread reads w_old[i1] and K[1..4][1] of the max-norm arm
//   2  the first thread runs penalty_weights_active on the LDS copies and leaves the branch, the scalars and K[1..4][1]
//   3  the group copies the l entries w = K[4] (branches 1-3, :1383) or w = w_old (otherwise; skipped where dw == dw_old)
//   4  the group scatters the t new weights and, under the Euclidean norm, runs assort! (:1344-1360) for one active entry per
//      thread on K[1..4][k] in global memory; an entry of K that does not move is not written
// Step 1 has read everything step 3 and 4 overwrite, so dw == dw_old is legal.  Two forms, chosen by the shape alone (t_max <= 64
// && l <= 64: TPP = 64, one wave per problem, four problems per workgroup; otherwise TPP = 256).  The serial part is the same
// code on the same values in both, so they give the same bits.  A problem that is not taken has no byte written.
//
// k_merit_total, one wave per problem: lane i forms the term of list position base + i (w[j] * (cx[j] * cx[j]), 0.0 for padding and
// for an inactive entry that fails cx[j] < 0), and the terms are added to the running sum one by one in list order (v_readlane of
// lane 0, 1, ...): active list first, then inactive, as :1322-1337.  No floating-point atomics anywhere.
#pragma once
#include "gn_batch_records.hpp"
#include "gn_device_utils.hpp"
#include "gn_kernels_linesearch_batched.hpp"
#include "gn_penalty_weights.hpp"

namespace gn {

struct PenaltyArgs {
    const PenaltyMeta* meta;
    const int* list;            // stride t_max: 1-based constraints, 0 padding
    PenaltyOut* out;
    int count, l, t_max, norm_code, scaling;
    const double* w_old;        // stride l
    const double* active_Ap;    // stride t_max
    const double* diag_scale;   // stride t_max
    const double* cx;           // stride l
    double* K;                  // stride 4 l, row ii at + ii * l
    double* w;                  // stride l
};

constexpr int PW_MAX_T = 1024;      // the LDS copies of the general form

template <int TPP, int CAP>
__global__ __launch_bounds__(256) void k_penalty(PenaltyArgs a) {
    constexpr int PPB = 256 / TPP;
    __shared__ double sw[PPB][CAP], sap[PPB][CAP], scx[PPB][CAP], sk3[PPB][CAP], sy[PPB][CAP];
    __shared__ int spos[PPB][CAP], sact[PPB][CAP];
    __shared__ double skf[PPB][4];
    __shared__ int sbranch[PPB], smoved[PPB];
    const int g = threadIdx.x / TPP, tid = threadIdx.x % TPP;
    const long long k = (long long)blockIdx.x * PPB + g;
    PenaltyMeta mt{};
    if (k < a.count) mt = a.meta[k];
    const bool live = k < a.count && mt.take != 0;
    const int t = mt.t, l = a.l;
    const bool euclid = a.norm_code != 0;
    const double* w_old = a.w_old + k * l;
    double* Kk = a.K + k * 4 * (long long)l;
    double* w = a.w + k * l;
    double w_first = 0.0;
    if (live) {
        const int* list = a.list + k * a.t_max;
        const double* cx = a.cx + k * l;
        for (int i = tid; i < t; i += TPP) {
            const int j = list[i] - 1;
            sact[g][i] = j;
            sw[g][i] = w_old[j];
            scx[g][i] = cx[j];
            if (euclid) sk3[g][i] = Kk[3 * (long long)l + j];
            double ap = a.active_Ap[k * a.t_max + i];
            if (a.scaling) ap = ap / a.diag_scale[k * a.t_max + i];              // :2231-2233, an IEEE division
            sap[g][i] = ap;
        }
        if (tid == 0 && !euclid && l > 0) {
            w_first = w_old[t > 0 ? list[0] - 1 : 0];                            // :1515-1517: active[1] == 0 reads w[1]
            for (int ii = 0; ii < 4; ++ii) skf[g][ii] = Kk[ii * (long long)l];
        }
    }
    __syncthreads();
    if (live && tid == 0) {
        bool moved = false;
        PenaltyOut o{};
        o.branch = penalty_weights_active(t, mt.dimA, a.norm_code, sw[g], sap[g], scx[g], sk3[g], sy[g], spos[g], mt.sums[0],
                                          mt.sums[1], mt.sums[2], l > 0, w_first, skf[g], &moved, o.scalars);
        sbranch[g] = o.branch;
        smoved[g] = moved;
        a.out[k] = o;
    }
    __syncthreads();
    if (live) {
        const double* base = penalty_base_is_K4(sbranch[g]) ? Kk + 3 * (long long)l : w_old;
        if (base != w)
            for (int j = tid; j < l; j += TPP) w[j] = base[j];
    }
    __syncthreads();
    if (live) {
        for (int i = tid; i < t; i += TPP) {
            const int j = sact[g][i];
            const double wk = sw[g][i];
            w[j] = wk;
            if (euclid) {
                double kk[4];
#pragma unroll
                for (int ii = 0; ii < 4; ++ii) kk[ii] = Kk[ii * (long long)l + j];
                double was[4] = {kk[0], kk[1], kk[2], kk[3]};
                if (penalty_assort_entry(wk, kk)) {
#pragma unroll
                    for (int ii = 0; ii < 4; ++ii)
                        if (__double_as_longlong(kk[ii]) != __double_as_longlong(was[ii])) Kk[ii * (long long)l + j] = kk[ii];
                }
            }
        }
        if (tid == 0 && smoved[g]) {
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) Kk[ii * (long long)l] = skf[g][ii];
        }
    }
}

// ---- the merit function ----------------------------------------------------------------------------------------------------------
struct MeritArgs {
    const MeritMeta* meta;
    const int* act;             // stride t_max: 1-based constraints, 0 padding
    const int* inact;           // stride l
    double* part;               // nblk per problem
    double* out;                // psi per problem
    int count, m, l, t_max, nblk;
    const double* rx;           // stride m
    const double* cx;           // stride l
    const double* w;            // stride l
};

__global__ __launch_bounds__(256) void k_merit_part(MeritArgs a) {
    __shared__ double ws[1][4];
    const long long k = blockIdx.x / a.nblk;
    const int b = (int)(blockIdx.x % a.nblk);
    if (!a.meta[k].take) return;
    const double* rx = a.rx + k * a.m;
    ordered_partial_sums<1>(b, a.nblk, a.m, ws, a.part + (size_t)k * a.nblk + b, [=](long long i, double (&s)[1]) {
        const double y = rx[i];
        s[0] += y * y;
    });
}

// the terms of `n` list positions added to s one by one: lane i holds position base + i
__device__ __forceinline__ double merit_list_sum(double s, const int* list, int n, bool only_negative, const double* cx, const double* w) {
#pragma clang fp contract(off)
    const int ln = lane_id();
    for (int base = 0; base < n; base += WAVE) {
        const int j = base + ln < n ? list[base + ln] : 0;
        double term = 0.0;
        if (j != 0) {
            const double c = cx[j - 1];
            if (!only_negative || c < 0.0) term = w[j - 1] * (c * c);            // :1324, :1331-1333: the test is literal
        }
        const int cnt = n - base < WAVE ? n - base : WAVE;
        for (int i = 0; i < cnt; ++i) s = s + wave_bcast(term, i);
    }
    return s;
}

__global__ __launch_bounds__(256) void k_merit_total(MeritArgs a) {
#pragma clang fp contract(off)
    const long long k = (long long)blockIdx.x * 4 + wave_id();
    if (k >= a.count) return;
    const MeritMeta mt = a.meta[k];
    double psi = 0.0;
    if (mt.take) {
        const double rr = a.nblk > 0 ? ordered_partials_total(a.part + (size_t)k * a.nblk, a.nblk, 1, 0) : 0.0;
        const double* cx = a.cx + k * a.l;
        const double* w = a.w + k * a.l;
        double s = 0.0;
        s = merit_list_sum(s, a.act + k * a.t_max, mt.t, false, cx, w);
        s = merit_list_sum(s, a.inact + k * a.l, mt.n_inactive, true, cx, w);
        psi = 0.5 * (rr + s);                                                    // :1339
    }
    if (lane_id() == 0) a.out[k] = psi;
}

}  // namespace gn
