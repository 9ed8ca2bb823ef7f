// Cholesky of ONE n2 x n2 matrix spread over the device (gn_tsqr_newton.inc): the Newton direction on a row-sharded J has a single
// sW22 of up to 1024 columns, for which one workgroup (k_newton_chol_batched) is one compute unit of 256.  Right-looking, panel
// width NWB_NB = 32, the matrix in global memory (ld n2), two launches per panel step and NOTHING that waits inside a kernel: the
// kernel boundary is the only synchronisation.
//   k_nw_panel   one wave per 64-row strip of the panel rows j0 .. n2.  Every workgroup stages the 32 x 32 diagonal block in LDS
//                and factors it, lane r holding row r in registers, the column of the step broadcast by v_readlane: the same
//                arithmetic in the same order in every workgroup, so every workgroup holds the same L11 bit for bit and no launch
//                of its own is needed for it.  Every lane whose row lies below the block solves its row of L21 = A21 L11^-T in
//                registers and stores it, and its mirror into the upper triangle (as k_newton_chol_batched does: the back
//                substitution reads U = L' as stored).  L11 itself: the other strips may still be reading A11, so strip 0 of a
//                panel of several strips leaves it in the 32 x 32 side buffer D and block (0, 0) of the syrk launch that follows
//                puts it in place; the one strip of a panel of at most 64 rows stores it directly.
//   k_nw_syrk    A22 -= L21 L21' on v_mfma_f64_16x16x4, lower triangle only; a workgroup of four waves owns a 64 x 64 block, its two
//                64 x 32 strips of L21 go through LDS (ld NW_LDS), wave w the rows 16 w .. 16 w + 15 of the block.
//   k_nw_finish  one workgroup: the two triangular solves and p = F_A.Q [p1; p2], or p = 0 and status 1.
// A pivot <= 0 or NaN (dpotrf's test, the one of k_newton_chol_batched) sets *flag; the panel and syrk kernels read the flag first
// and return when it is set, so an indefinite matrix costs empty launches and no host round trip.  Nothing is read or written
// outside n2 x n2 for any n2 >= 1; a guarded lane contributes an exact +0.0.  No atomics: every entry of A22 is updated once per
// panel step, by one lane, in an order that depends on n2 alone.
#pragma once
#include "gn_kernels_newton_batched.hpp"

namespace gn {

constexpr int NW_STRIP = 64;     // rows of a panel strip = edge of a syrk block
// leading dimension of a 32 x 64 strip image in LDS (doubles): ds_read_b64 serves lanes 0-31 and 32-63 in one LDS cycle each, and
// the MFMA operand read has lanes (lr, lq) at (k0 + lq) * 80 + lr: 160 dwords between lq and lq + 1 = 32 banks of 64, no conflict
constexpr int NW_LDS = 80;

struct NewtonWideArgs {
    int n2;
    double* A;       // sW22 on entry, L (and L' above the diagonal) on exit; ld n2
    double* D;       // 32 x 32: L11 of a panel of several strips, from its k_nw_panel to its k_nw_syrk
    int* flag;       // zero before the first panel; set: not positive definite
};

__global__ __launch_bounds__(64) void k_nw_panel(NewtonWideArgs a, int j0) {
    constexpr int NB = NWB_NB, LDB = NB + 1;
    __shared__ double blk[NB * LDB];
    if (*a.flag) return;
    const int n2 = a.n2, ld = n2, ln = threadIdx.x;
    const int nb = (n2 - j0) < NB ? (n2 - j0) : NB;
    double* A = a.A;
    // the diagonal block: its lower triangle as stored, zeros above, the identity where the last panel is narrower than 32
    for (int e = ln; e < NB * NB; e += 64) {
        const int r = e % NB, c = e / NB;
        double v = (r == c) ? 1.0 : 0.0;
        if (r < nb && c < nb) v = (r >= c) ? A[(j0 + r) + (size_t)(j0 + c) * ld] : 0.0;
        blk[r + c * LDB] = v;
    }
    __syncthreads();
    const int rr = ln & 31;      // both halves of the wave carry the block: every lane takes every step
    double row[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) row[c] = blk[rr + c * LDB];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const double akk = readlane_f64(row[k], k);
        if (!(akk > 0.0)) { bad = true; break; }
        const double l = sqrt(akk);
        const double lrk = (rr == k) ? l : row[k] / l;
        row[k] = lrk;
#pragma unroll
        for (int c = k + 1; c < NB; ++c) row[c] -= lrk * readlane_f64(lrk, c);
    }
    if (bad) {
        if (blockIdx.x == 0 && ln == 0) *a.flag = 1;
        return;
    }
    __syncthreads();
    if (ln < NB) {
#pragma unroll
        for (int c = 0; c < NB; ++c) blk[ln + c * LDB] = row[c];
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        const bool direct = gridDim.x == 1;      // no other workgroup reads A11
        for (int e = ln; e < nb * nb; e += 64) {
            const int r = e % nb, c = e / nb;
            if (r < c) continue;
            const double v = blk[r + c * LDB];
            if (direct) {
                A[(j0 + r) + (size_t)(j0 + c) * ld] = v;
                A[(j0 + c) + (size_t)(j0 + r) * ld] = v;
            } else {
                a.D[r + c * NB] = v;
            }
        }
    }
    // a row below the block exists only under a full panel (j0 + 32 < n2): all 32 columns are inside the matrix
    const int gr = j0 + NW_STRIP * (int)blockIdx.x + ln;
    if (gr < j0 + NB || gr >= n2) return;
    double x[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) x[c] = A[gr + (size_t)(j0 + c) * ld];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
#pragma unroll
        for (int k = 0; k < c; ++k) x[c] -= x[k] * blk[c + k * LDB];
        x[c] /= blk[c + c * LDB];
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        A[gr + (size_t)(j0 + c) * ld] = x[c];
        A[(j0 + c) + (size_t)gr * ld] = x[c];
    }
}

// grid (nbk, nbk), nbk = ceil((n2 - j0 - 32) / 64); a block above the diagonal exits.  The product is formed transposed, the MFMA's
// A operand from the block's COLUMN strip and its B operand from the ROW strip (fragment maps: A[i = l & 15][k = l >> 4],
// B[k = l >> 4][j = l & 15], D[i = (l >> 4) + 4 r][j = l & 15]), so that D's j, the lane's low bits, runs along a column of A22:
// 16 consecutive doubles per store.
__global__ __launch_bounds__(256) void k_nw_syrk(NewtonWideArgs a, int j0) {
    constexpr int NB = NWB_NB;
    __shared__ double sR[NB * NW_LDS], sC[NB * NW_LDS];
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    if (*a.flag) return;
    const int n2 = a.n2, ld = n2, t0 = j0 + NB;
    const int R0 = t0 + NW_STRIP * bi, C0 = t0 + NW_STRIP * bj;
    double* A = a.A;
    if (bi == 0 && n2 - j0 > NW_STRIP) {      // the panel had several strips: its L11 waits in D (nobody reads A11 in this launch)
        for (int e = threadIdx.x; e < NB * NB; e += 256) {
            const int r = e % NB, c = e / NB;
            if (r < c) continue;
            const double v = a.D[r + c * NB];
            A[(j0 + r) + (size_t)(j0 + c) * ld] = v;
            A[(j0 + c) + (size_t)(j0 + r) * ld] = v;
        }
    }
    for (int e = threadIdx.x; e < NB * NW_STRIP; e += 256) {
        const int i = e & (NW_STRIP - 1), k = e / NW_STRIP;
        sR[k * NW_LDS + i] = (R0 + i < n2) ? A[(R0 + i) + (size_t)(j0 + k) * ld] : 0.0;
        sC[k * NW_LDS + i] = (C0 + i < n2) ? A[(C0 + i) + (size_t)(j0 + k) * ld] : 0.0;
    }
    __syncthreads();
    const int w = wave_id(), ln = lane_id(), lr = ln & 15, lq = ln >> 4;
    nwb_d4 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = nwb_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k0 = 0; k0 < NB; k0 += 4) {
        const double bv = sR[(k0 + lq) * NW_LDS + 16 * w + lr];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const double av = sC[(k0 + lq) * NW_LDS + 16 * ct + lr];
            acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[ct], 0, 0, 0);
        }
    }
    const int row = R0 + 16 * w + lr;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = C0 + 16 * ct + lq + 4 * r;
            if (row < n2 && col < n2 && row >= col) A[row + (size_t)col * ld] -= acc[ct][r];
        }
    }
}

// The tail of k_newton_chol_batched<256> for slot 0 of `a` on the factor the panel steps left in a.X (n2 > 0).
__global__ __launch_bounds__(256) void k_nw_finish(NewtonBatchArgs a) {
    __shared__ double blk[64 * 65];
    __shared__ double y[1024], pb[1024];
    __shared__ int sh;
    const int tid = threadIdx.x;
    const ProbState st = a.state[0];
    const int n = a.n, rankA = st.rankA, n2 = st.n2;
    if (*a.flag) {        // :417-420: p = zeros, error = true
        for (int i = tid; i < n; i += 256) a.p_out[i] = 0.0;
        if (tid == 0) a.status_out[0] = 1;
        return;
    }
    if (tid == 0) sh = 0;
    for (int i = tid; i < n2; i += 256) y[i] = a.rhs[i];
    __syncthreads();
    wg_trsv<true>(a.X, n2, n2, y, blk, &sh);
    wg_trsv<false>(a.X, n2, n2, y, blk, &sh);
    for (int i = tid; i < rankA; i += 256) pb[i] = a.p1[i];
    for (int i = tid; i < n2; i += 256) pb[rankA + i] = y[i];
    __syncthreads();
    if (wave_id() == 0) wave_apply_reflectors<false>(a.FA, n, a.tauA, a.kA, n, pb);
    __syncthreads();
    for (int i = tid; i < n; i += 256) a.p_out[i] = pb[i];
    if (tid == 0) a.status_out[0] = 0;
}

}  // namespace gn
