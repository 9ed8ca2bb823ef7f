// The step between the stages of the batched update_working_set, on the caller's device buffers (gn_deletion_batched.inc):
//   k_delete_*    check_constraint_deletion (src/enlsip_functions.jl:574-603) on lambda, diag_scale, grad_res of every taken problem,
//                 then where s != 0 the removal of row s from C.A, C.cx, C.diag_scale and lambda (:708-719, :748-756, :776-785) in
//                 the padded ragged layout, with the record of :708-711 saved for the undo
//   k_restore_*   the re-insertion after a failed feasibility test (:731-739): the exact inverse
// A' is stored n x t column-major, so row s of C.A is column s - 1 of the block.  Every thread owns fixed rows of the block and
// walks its columns in ascending order (descending for the restore): the in-place shift needs no barrier and is coalesced along
// the rows.  The vectors are shifted through registers (wave form) or LDS copies (general form).  Nothing between rows n and
// ldat, past column t_max, or of a problem that is not edited is written.
//
// Two forms, chosen by the shape alone (n <= 64 && t_max <= 64: wave per problem).  They must give the same s:
//   general   one workgroup per problem; one lane runs deletion_check (gn_deletion_test.hpp) on LDS copies.
//   wave      four problems per 256-thread workgroup, lane i holds entry i, no LDS, no barrier.  The sequential loop of :591-597
//             keeps e = min of the candidates v_i = row_i * lambda_i (q < i <= t) that pass v_i <= sq_rel, because e starts at
//             sq_rel and only ever takes such a v_i that is <= e; and s is the LAST i with v_i == e, because both tests are <=.
//             So: a ballot for "some candidate passes", a wave minimum, a ballot of v_i == e and its highest lane.  v_i == e
//             holds for -0.0 against +0.0 exactly where <= held in the loop; a NaN v_i passes neither.  A NaN anywhere in
//             lambda[0:t) makes sq_rel NaN in the loop, so nothing passes and the gate of :598 is false: s = 0, by one ballot.
#pragma once
#include "gn_batch_records.hpp"
#include "gn_device_utils.hpp"
#include "gn_deletion_test.hpp"

namespace gn {

struct DeletionArgs {
    const DeletionMeta* meta;
    int* s_out;                 // delete: the decision per problem
    int count, n, t_max, scaling;
    double* lambda;             // stride t_max
    double* diag_scale;         // stride t_max
    const double* grad_res;     // stride 1, null: 0.0 for every problem (the second-order test, :747 / :775)
    double* At; long long ldat, strideAt;
    double* cx;                 // stride t_max
    double* saved;              // stride n + 3: A_s (n), cx_s, lambda_s, diag_scale_s (:708-711); delete: may be null
};

__global__ __launch_bounds__(256) void k_delete_wave(DeletionArgs a) {
    const int ln = lane_id();
    const long long k = (long long)blockIdx.x * 4 + wave_id();
    if (k >= a.count) return;
    const DeletionMeta mt = a.meta[k];
    const int t = mt.t, q = mt.q, n = a.n;
    double* lam = a.lambda + k * a.t_max;
    double* ds = a.diag_scale + k * a.t_max;
    double* cx = a.cx + k * a.t_max;
    const bool in = ln < t;
    int s = 0;
    double li = 0.0, di = 1.0;
    if (mt.take && t > q) {
        li = in ? lam[ln] : 0.0;
        di = in ? ds[ln] : 1.0;
        if (!__ballot(in && li != li)) {
            const double sq_rel = GN_DELETION_SQRT_EPS * wave_allmax(in ? fabs(li) : 0.0);      // :585-586
            const double row_i = a.scaling ? 1.0 / di : di;                                      // :592
            const double v = row_i * li;
            const bool pass = in && ln >= q && v <= sq_rel;
            if (__ballot(pass)) {
                const double e = -wave_allmax(pass ? -v : -INFINITY);
                s = 64 - __builtin_clzll(__ballot(pass && v == e));
                const double gr = a.grad_res ? a.grad_res[k] : 0.0;
                if (gr > -e * 10.0) s = 0;                                                       // :598-600
            }
        }
    }
    if (ln == 0) a.s_out[k] = s;
    if (s == 0) return;
    const double ci = in ? cx[ln] : 0.0;
    double* sv = a.saved ? a.saved + k * (n + 3) : nullptr;
    if (ln < n) {
        double* row = a.At + k * a.strideAt + ln;
        if (sv) sv[ln] = row[(size_t)(s - 1) * a.ldat];
        for (int c = s - 1; c < t - 1; ++c) row[(size_t)c * a.ldat] = row[(size_t)(c + 1) * a.ldat];
        row[(size_t)(t - 1) * a.ldat] = 0.0;
    }
    if (sv && ln == s - 1) { sv[n] = ci; sv[n + 1] = li; sv[n + 2] = di; }
    const double lnx = __shfl_down(li, 1), dnx = __shfl_down(di, 1), cnx = __shfl_down(ci, 1);
    if (ln >= s - 1 && in) {
        const bool last = ln == t - 1;
        lam[ln] = last ? 0.0 : lnx;
        ds[ln] = last ? 1.0 : dnx;
        cx[ln] = last ? 0.0 : cnx;
    }
}

__global__ __launch_bounds__(256) void k_delete_general(DeletionArgs a) {
    __shared__ double sl[1024], sd[1024], sc[1024];
    __shared__ int sh_s;
    const long long k = blockIdx.x;
    const int tid = threadIdx.x;
    const DeletionMeta mt = a.meta[k];
    const int t = mt.t, q = mt.q, n = a.n;
    if (!mt.take || t <= q) {
        if (tid == 0) a.s_out[k] = 0;
        return;
    }
    double* lam = a.lambda + k * a.t_max;
    double* ds = a.diag_scale + k * a.t_max;
    double* cx = a.cx + k * a.t_max;
    for (int i = tid; i < t; i += 256) { sl[i] = lam[i]; sd[i] = ds[i]; sc[i] = cx[i]; }
    __syncthreads();
    if (tid == 0) sh_s = (int)deletion_check(q, t, sl, sd, a.scaling != 0, a.grad_res ? a.grad_res[k] : 0.0);
    __syncthreads();
    const int s = sh_s;
    if (tid == 0) a.s_out[k] = s;
    if (s == 0) return;
    double* sv = a.saved ? a.saved + k * (n + 3) : nullptr;
    for (int r = tid; r < n; r += 256) {
        double* row = a.At + k * a.strideAt + r;
        if (sv) sv[r] = row[(size_t)(s - 1) * a.ldat];
        for (int c = s - 1; c < t - 1; ++c) row[(size_t)c * a.ldat] = row[(size_t)(c + 1) * a.ldat];
        row[(size_t)(t - 1) * a.ldat] = 0.0;
    }
    if (sv && tid == 0) { sv[n] = sc[s - 1]; sv[n + 1] = sl[s - 1]; sv[n + 2] = sd[s - 1]; }
    for (int i = s - 1 + tid; i < t; i += 256) {
        const bool last = i == t - 1;
        lam[i] = last ? 0.0 : sl[i + 1];
        ds[i] = last ? 1.0 : sd[i + 1];
        cx[i] = last ? 0.0 : sc[i + 1];
    }
}

// meta.t: the count after the deletion (t < t_max where s != 0), meta.s in 1 .. t + 1
__global__ __launch_bounds__(256) void k_restore_wave(DeletionArgs a) {
    const int ln = lane_id();
    const long long k = (long long)blockIdx.x * 4 + wave_id();
    if (k >= a.count) return;
    const DeletionMeta mt = a.meta[k];
    const int t = mt.t, s = mt.s, n = a.n;
    if (s == 0) return;
    double* lam = a.lambda + k * a.t_max;
    double* ds = a.diag_scale + k * a.t_max;
    double* cx = a.cx + k * a.t_max;
    const double* sv = a.saved + k * (n + 3);
    const bool in = ln < t;
    const double li = in ? lam[ln] : 0.0, di = in ? ds[ln] : 0.0, ci = in ? cx[ln] : 0.0;
    if (ln < n) {
        double* row = a.At + k * a.strideAt + ln;
        for (int c = t - 1; c >= s - 1; --c) row[(size_t)(c + 1) * a.ldat] = row[(size_t)c * a.ldat];
        row[(size_t)(s - 1) * a.ldat] = sv[ln];
    }
    const double lpv = __shfl_up(li, 1), dpv = __shfl_up(di, 1), cpv = __shfl_up(ci, 1);
    if (ln >= s - 1 && ln <= t) {
        const bool first = ln == s - 1;
        lam[ln] = first ? sv[n + 1] : lpv;
        ds[ln] = first ? sv[n + 2] : dpv;
        cx[ln] = first ? sv[n] : cpv;
    }
}

__global__ __launch_bounds__(256) void k_restore_general(DeletionArgs a) {
    __shared__ double sl[1024], sd[1024], sc[1024];
    const long long k = blockIdx.x;
    const int tid = threadIdx.x;
    const DeletionMeta mt = a.meta[k];
    const int t = mt.t, s = mt.s, n = a.n;
    if (s == 0) return;
    double* lam = a.lambda + k * a.t_max;
    double* ds = a.diag_scale + k * a.t_max;
    double* cx = a.cx + k * a.t_max;
    const double* sv = a.saved + k * (n + 3);
    for (int i = tid; i < t; i += 256) { sl[i] = lam[i]; sd[i] = ds[i]; sc[i] = cx[i]; }
    __syncthreads();
    for (int r = tid; r < n; r += 256) {
        double* row = a.At + k * a.strideAt + r;
        for (int c = t - 1; c >= s - 1; --c) row[(size_t)(c + 1) * a.ldat] = row[(size_t)c * a.ldat];
        row[(size_t)(s - 1) * a.ldat] = sv[r];
    }
    for (int i = s - 1 + tid; i <= t; i += 256) {
        const bool first = i == s - 1;
        lam[i] = first ? sv[n + 1] : sl[i - 1];
        ds[i] = first ? sv[n + 2] : sd[i - 1];
        cx[i] = first ? sv[n] : sc[i - 1];
    }
}

}  // namespace gn
