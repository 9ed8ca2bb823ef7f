// Products of one row shard J_g (m x n, column-major, ld >= m) of a row-sharded Jacobian with the shard's rx_g: what the
// consumers around the subproblem need of J once its rows live on several devices (enlsip_gn_tsqr_products*).
//   k_tp_rows     Jp = J_g p                                                       (src/enlsip_functions.jl:2226)
//   k_tp_cols     per chunk of TP_CH rows: partial[chunk][c] = sum over the chunk's rows of J[r, c] v[r], v = rx + Jp (or rx),
//                 and the chunk's parts of dot(rx,rx), dot(Jp,Jp), dot(Jp,rx)       (:2690, :1561-1584)
//   k_tp_reduce   message body[c] = sum of partial[chunk][c] over the chunks, ascending; header
//   k_tp_combine  the G gathered messages added in rank order, 0 first, and the check of their headers
//   k_tp_qt       x = F_A.Q' x on an n-vector (second multiplier estimate: J1' w = (F_A.Q' (J' w))[1:t], :526-529)
//
// Order of summation (fixed by m, n, ld and the operands alone: not by the grid, the CU count, the handle or what ran before).
//   Jp[r]: wave w of the row's workgroup adds columns w, w + 4, ... ascending from +0.0; the four parts as (s0 + s1) + (s2 + s3).
//   A chunk's column sum: lane l adds rows l, l + 64, ... of the chunk ascending from +0.0, then the butterfly (wave_allsum), the
//   order of the Hessian sums (gn_hessian_sums.hpp).  Chunks ascending from +0.0.  Ranks ascending, rank 0's value first.
// No floating-point atomics.  Loads are 8 bytes per lane, consecutive lanes on consecutive rows (512 contiguous bytes per wave and
// load): nothing assumes more than the 8-byte alignment of a double, so a shard that starts at an odd row of a larger matrix
// (ld = that matrix's height) runs the same instructions, in the same order, as a copy of its rows.  No thread reads or writes a
// row >= m of any column: the last chunk and the last 64-row group are guarded, a guarded row contributes an exact +0.0 product.
// These kernels stream J from HBM: k_tp_rows and k_tp_cols each read it once (two passes when p is given, one otherwise).
#pragma once
#include "gn_device_utils.hpp"
#include "gn_wg_linalg.hpp"

namespace gn {

constexpr int TP_CH = 1024;              // chunk height of the transposed product (rows); the tests read it from here
constexpr int TP_RPL = TP_CH / 64;       // rows of a chunk per lane
constexpr int TP_CPW = 8;                // columns per wave of k_tp_cols: a workgroup of four waves serves 32 columns of a chunk
constexpr int TP_CPG = 4 * TP_CPW;
constexpr int TP_HDR = 4;                // message header, doubles: [0] rank of the sender + 1 (0: not stated), [1] the rank count it
                                         // believes in (0: not stated), [2] n, [3] spare (zero); then g (n), then the three sums
constexpr int TP_SUMS = 3;               // dot(rx,rx), dot(Jp,Jp), dot(Jp,rx)
static_assert(TP_CH % 64 == 0 && TP_HDR % 2 == 0, "whole strides of a wave per chunk; the body starts on a 16-byte granule");

__host__ __device__ inline long long tp_msg_len(long long n) { return (TP_HDR + n + TP_SUMS + 1) & ~1LL; }

// Jp[r] = sum_c J[r + c ld] p[c]: 64 rows per workgroup, lanes along rows, the columns dealt to the four waves
__global__ __launch_bounds__(256) void k_tp_rows(const double* __restrict__ J, long long ld, int m, int n,
                                                 const double* __restrict__ p, double* __restrict__ Jp) {
    __shared__ double part[4][64];
    const int ln = lane_id(), w = wave_id();
    const long long r = (long long)blockIdx.x * 64 + ln;
    double s = 0.0;
    if (r < m) {
        const double* row = J + r;
#pragma unroll 8
        for (int c = w; c < n; c += 4) s += row[(size_t)c * ld] * p[c];
    }
    part[w][ln] = s;
    __syncthreads();
    if (w == 0 && r < m) Jp[r] = (part[0][ln] + part[1][ln]) + (part[2][ln] + part[3][ln]);
}

// blockIdx.x: chunk; blockIdx.y: group of TP_CPG columns, and one more workgroup (y == gridDim.y - 1) for the three sums.
// partial: gridDim.x rows of n + TP_SUMS.  Jp NULL: v = rx and the sums that involve Jp are +0.0.
__global__ __launch_bounds__(256) void k_tp_cols(const double* __restrict__ J, long long ld, int m, int n,
                                                 const double* __restrict__ rx, const double* __restrict__ Jp,
                                                 double* __restrict__ partial) {
    const int ln = lane_id(), w = wave_id();
    const long long r0 = (long long)blockIdx.x * TP_CH;
    const int rows = (int)((m - r0) < TP_CH ? (m - r0) : TP_CH);
    double* out = partial + (size_t)blockIdx.x * (n + TP_SUMS);
    double xr[TP_RPL], xj[TP_RPL];
#pragma unroll
    for (int i = 0; i < TP_RPL; ++i) {
        const int r = ln + 64 * i;
        xr[i] = r < rows ? rx[r0 + r] : 0.0;
        xj[i] = (Jp && r < rows) ? Jp[r0 + r] : 0.0;
    }
    if (blockIdx.y == gridDim.y - 1) {
        if (w != 0) return;
        double srr = 0.0, sjj = 0.0, sjr = 0.0;
#pragma unroll
        for (int i = 0; i < TP_RPL; ++i) {
            srr += xr[i] * xr[i];
            sjj += xj[i] * xj[i];
            sjr += xj[i] * xr[i];
        }
        srr = wave_allsum(srr);
        sjj = wave_allsum(sjj);
        sjr = wave_allsum(sjr);
        if (ln == 0) {
            out[n] = srr;
            out[n + 1] = sjj;
            out[n + 2] = sjr;
        }
        return;
    }
    if (Jp) {
#pragma unroll
        for (int i = 0; i < TP_RPL; ++i) xr[i] += xj[i];      // v = rx + Jp
    }
    const int c0 = blockIdx.y * TP_CPG + w * TP_CPW;
    const bool full = rows == TP_CH;                            // uniform over the workgroup
    // one column at a time: its TP_RPL loads are in flight together; unrolling over columns only costs the registers that
    // more waves per SIMD need
#pragma unroll 1
    for (int k = 0; k < TP_CPW; ++k) {
        const int c = c0 + k;
        if (c >= n) break;
        const double* col = J + (size_t)c * ld + r0;
        double s = 0.0;
        if (full) {
#pragma unroll
            for (int i = 0; i < TP_RPL; ++i) s += col[ln + 64 * i] * xr[i];
        } else {
#pragma unroll
            for (int i = 0; i < TP_RPL; ++i) {
                const int r = ln + 64 * i;
                const double a = r < rows ? col[r] : 0.0;
                s += a * xr[i];
            }
        }
        s = wave_allsum(s);
        if (ln == 0) out[c] = s;
    }
}

// one thread per entry of the body: the chunks' partials ascending; the header and the padding by thread 0
__global__ __launch_bounds__(256) void k_tp_reduce(const double* __restrict__ partial, long long nchunks, int n, double* __restrict__ msg,
                                                   double rank_tag, double ranks) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int w = n + TP_SUMS;
    if (j < w) {
        double s = 0.0;
        for (long long ch = 0; ch < nchunks; ++ch) s += partial[(size_t)ch * w + j];
        msg[TP_HDR + j] = s;
    }
    if (j == 0) {
        msg[0] = rank_tag;
        msg[1] = ranks;
        msg[2] = (double)n;
        msg[3] = 0.0;
        for (long long i = TP_HDR + w; i < tp_msg_len(n); ++i) msg[i] = 0.0;
    }
}

// out[j] = msg_0[j] + msg_1[j] + ... + msg_{G-1}[j], j < n + TP_SUMS, in that order; out[n + TP_SUMS] = number of messages whose
// header names another n, another rank count than G (0: not stated) or another slot than the one it lies in (0: not stated)
__global__ __launch_bounds__(256) void k_tp_combine(const double* __restrict__ msgs, long long msg_len, int G, int n,
                                                    double* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int w = n + TP_SUMS;
    if (j < w) {
        double s = msgs[TP_HDR + j];
        for (int g = 1; g < G; ++g) s += msgs[(size_t)g * msg_len + TP_HDR + j];
        out[j] = s;
    }
    if (j == 0) {
        double bad = 0.0;
        for (int g = 0; g < G; ++g) {
            const double* hd = msgs + (size_t)g * msg_len;
            const bool ok = hd[2] == (double)n && (hd[1] == (double)G || hd[1] == 0.0) && (hd[0] == (double)(g + 1) || hd[0] == 0.0);
            if (!ok) bad += 1.0;
        }
        out[w] = bad;
    }
}

// x = F_A.Q' x, one wave
__global__ __launch_bounds__(64) void k_tp_qt(const double* FA, int n, const double* tauA, int kA, double* x) {
    wave_apply_reflectors<true>(FA, n, tauA, kA, n, x);
}

}  // namespace gn
