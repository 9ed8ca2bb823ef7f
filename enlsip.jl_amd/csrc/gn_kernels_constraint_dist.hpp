// Helpers of the constraint stage with MANY constraints (t > 64, matrices beyond one workgroup's LDS): F_A = qr(C.A', ColumnNorm())
// and F_L11 = qr(F_A.R', ColumnNorm()) (src/enlsip_functions.jl:700, :769) run through the distributed pivoted QR of
// gn_kernels_qrcp_dist.hpp (one launch per pivot step over all column groups and problems) instead of one workgroup walking
// the whole matrix in L2 (measured: 293 ms for the 1000 x 998 matrix of the reference's chained-Rosenbrock test).
#pragma once
#include "gn_device_utils.hpp"

namespace gn {

// plist (every kernel of this file with a problem per grid row): device list of problem indices, NULL = row y is problem y
// dst[r + c * ldd] = src[r + c * lds], r < rows, c < cols, per problem
__global__ __launch_bounds__(256) void k_copy_cols(double* __restrict__ dst, long long ldd, long long sD, const double* __restrict__ src,
                                                   long long lds, long long sS, int rows, int cols, const int* __restrict__ plist) {
    const int c = blockIdx.x;
    const int prob = listed_prob(plist, blockIdx.y, 0);
    if (c >= cols) return;
    double* d = dst + prob * sD + (size_t)c * ldd;
    const double* s = src + prob * sS + (size_t)c * lds;
    for (int r = threadIdx.x; r < rows; r += 256) d[r] = s[r];
}

// b_buff[i] = -cx[F_A.p[i]]   (src/enlsip_functions.jl:131 / :141)
__global__ __launch_bounds__(256) void k_bbuff(double* __restrict__ out, long long sOut, const double* __restrict__ cx, long long sCx,
                                               const long long* __restrict__ jpvt, long long sJ, int t,
                                               const int* __restrict__ plist) {
    const int prob = listed_prob(plist, blockIdx.y, 0);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < t) out[prob * sOut + i] = -cx[prob * sCx + jpvt[prob * sJ + i] - 1];
}

// per-problem stand-in records for the distributed QR (it reads kp = steps and n2 = columns from a ProbState)
__global__ __launch_bounds__(256) void k_fake_state(ProbState* st, int batch, int kp, int n2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < batch) {
        ProbState s{};
        s.rankA = 0; s.n2 = n2; s.kp = kp;
        st[i] = s;
    }
}

// ---- ragged batch (enlsip_gn_solve_batched_ragged): problem prob has tk[prob] <= t constraints, kA = min(n, tk) ---------------
// mode 0 (F_A): columns c < tk of src (rows `rows`, ld ldd), columns tk <= c < cols_max zero — the identity padding of F_A
// mode 1 (F_L11): the tk x kA factor with the problem's own leading dimension tk (the rows past tk of the padded factorisation
//                 are zero and carry nothing)
// mode 2 (F_L11.Q' b_buff): column kA of src (the carried column sits right of the problem's own kA columns), tk rows
__global__ __launch_bounds__(256) void k_copy_cols_ragged(double* __restrict__ dst, long long ldd, long long sD,
                                                          const double* __restrict__ src, long long lds, long long sS, int rows,
                                                          int cols_max, int n, const int* __restrict__ tk, int mode,
                                                          const int* __restrict__ plist) {
    const int c = blockIdx.x;
    const int prob = listed_prob(plist, blockIdx.y, 0);
    const int t = tk[prob], kA = n < t ? n : t;
    if (mode == 0) {
        if (c >= cols_max) return;
        double* d = dst + prob * sD + (size_t)c * ldd;
        const double* s = src + prob * sS + (size_t)c * lds;
        for (int r = threadIdx.x; r < rows; r += 256) d[r] = (c < t) ? s[r] : 0.0;
    } else if (mode == 1) {
        if (c >= kA) return;
        double* d = dst + prob * sD + (size_t)c * t;
        const double* s = src + prob * sS + (size_t)c * lds;
        for (int r = threadIdx.x; r < t; r += 256) d[r] = s[r];
    } else {
        if (c != 0) return;
        double* d = dst + prob * sD;
        const double* s = src + prob * sS + (size_t)kA * lds;
        for (int r = threadIdx.x; r < t; r += 256) d[r] = s[r];
    }
}

// b_buff[i] = -cx[F_A.p[i]] for i < tk, 0 up to t (the padded rows of the F_L11 factorisation must be zero)
__global__ __launch_bounds__(256) void k_bbuff_ragged(double* __restrict__ out, long long sOut, const double* __restrict__ cx,
                                                      long long sCx, const long long* __restrict__ jpvt, long long sJ, int t,
                                                      const int* __restrict__ tk, const int* __restrict__ plist) {
    const int prob = listed_prob(plist, blockIdx.y, 0);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < t) out[prob * sOut + i] = (i < tk[prob]) ? -cx[prob * sCx + jpvt[prob * sJ + i] - 1] : 0.0;
}

// stand-in records with each problem's own sizes: F_A has tk columns (kp = min(n, tk) steps), F_L11 kA = min(n, tk)
__global__ __launch_bounds__(256) void k_fake_state_ragged(ProbState* st, int batch, int n, const int* __restrict__ tk, int for_L) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < batch) {
        const int t = tk[i], kA = n < t ? n : t;
        ProbState s{};
        s.rankA = 0; s.n2 = for_L ? kA : t; s.kp = kA;
        st[i] = s;
    }
}

}  // namespace gn
