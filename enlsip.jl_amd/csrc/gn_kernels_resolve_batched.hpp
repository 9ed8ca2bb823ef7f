// Batched subspace re-solve (gn_resolve_batched.inc): sub_search_direction (src/enlsip_functions.jl:116-153) for a range of the
// resident batch with per-problem dimA / dimJ2 / code, on the RESIDENT factors — nothing is factored again.  Stages:
//   k_resolve_head            b, p1 from F_A / F_L11 (:131-133 / :141-144)
//   k_dtemp_batched           d_temp = -J1 p1 - rx (:134 / :145)
//   k_caqr_vec_batched        Q0' d_temp, one launch per (panel, level) of the CAQR plan for the whole range
//   k_vec_reflectors_batched  Qt' on the leading kp entries
//   k_resolve_tail            triangular solve with dimJ2, scatter, p = F_A.Q [p1; p2], outputs (:136-137 / :147-151)
// Every kernel reads the per-slot request (ResolveDims) and leaves a skipped slot's buffers and state alone.
#pragma once
#include "gn_kernels_caqr.hpp"
#include "gn_kernels_final.hpp"

namespace gn {

constexpr int RESOLVE_HOLD = ENLSIP_GN_DIM_HOLD;

// request of one slot: code 0 or status != 0 = leave the problem alone; dimJ2 == HOLD = stop after Q3' d_temp (b, d written);
// dimA == HOLD = start from the resident p1 and Q3' d_temp of such a call
struct ResolveDims {
    int dimA, dimJ2, code, status;
};
__device__ __forceinline__ bool resolve_skip(const ResolveDims& d) { return d.code == 0 || d.status != 0; }
__device__ __forceinline__ bool resolve_skip_head(const ResolveDims& d) { return resolve_skip(d) || d.dimA == RESOLVE_HOLD; }

// all pointers address slot 0 of the segment (problem k0 of the handle)
struct ResolveBatchArgs {
    int m, n, t, kA, ldw, ldr;      // t, kA: the batch's (t_max of a ragged batch)
    int nv;                         // LDS vector length (>= max(n, t))
    int blkd;                       // LDS doubles of the triangular solves' diagonal block: 65 min(64, max(n, t))
    const ResolveDims* dims;
    const int* tk;                  // ragged batch: each problem's own t, else NULL
    ProbState* state;
    const double* cx;    long long scx;
    const double* rx;
    const double* FA;    long long sFA;
    const double* tauA;  long long sTauA;
    const long long* jpvtA; long long sJA;
    const double* FL;    long long sFL;
    const double* tauL;  long long sTauL;
    const long long* jpvtL; long long sJL;
    const double* qb;    long long sQb;      // distributed constraint route: the resident F_L11.Q' b_buff, else NULL
    double* p1;          long long sP1;
    double* bvec;        long long sB;
    const double* W;     long long sW;
    double* vec;         long long sVec;
    const double* Rt;    long long sRt;
    const double* tauJ;  long long sTauJ;
    const long long* jpvtJ; long long sJJ;
    double* p_out;       // n per slot, may be NULL
    double* b_out;       // t per slot
    double* d_out;       // m per slot
    enlsip_gn_info* info_out;
    int* status_out;
};

inline size_t resolve_lds_bytes(int nv, int blkd) { return (size_t)(2 * nv + blkd + 8) * 8; }

// wg_trsv<LOWER = true> on the transpose of an upper-triangular factor: solves R' x = y with R (ld) as it is stored
__device__ inline void wg_trsv_upper_t(const double* __restrict__ R, int ld, int dim, double* y, double* blk, int* status) {
    const int ln = lane_id();
    const int w = wave_id();
    const int nblk = (dim + 63) / 64;
    for (int bi = 0; bi < nblk; ++bi) {
        const int i0 = bi * 64;
        const int nb = (dim - i0) < 64 ? (dim - i0) : 64;
        for (int e = threadIdx.x; e < nb * nb; e += blockDim.x) {
            const int c = e % nb, r = e / nb;       // L[r][c] = R[c][r]
            blk[r + c * 65] = R[(i0 + c) + (size_t)(i0 + r) * ld];
        }
        __syncthreads();
        if (w == 0) {
            const double di = (ln < nb) ? blk[ln + ln * 65] : 1.0;
            if (di == 0.0) atomicOr(status, 1);
            const double ri = 1.0 / di;
            double yi = (ln < nb) ? y[i0 + ln] / di : 0.0;
            for (int kk = 0; kk < nb; ++kk) {
                const double xk = wave_bcast(yi, kk);
                if (ln > kk && ln < nb) yi -= (blk[ln + kk * 65] * ri) * xk;
            }
            if (ln < nb) y[i0 + ln] = yi;
        }
        __syncthreads();
        for (int r = i0 + nb + threadIdx.x; r < dim; r += blockDim.x) {
            double s = 0.0;
            for (int c = 0; c < nb; ++c) s += R[(i0 + c) + (size_t)r * ld] * y[i0 + c];
            y[r] -= s;
        }
        __syncthreads();
    }
}

// b and p1 of one problem per workgroup from the resident F_A / F_L11 (the b / p1 part of constraint_body, no factorisation).
// NTH = 64: one wave per problem (n, t_max <= 64); NTH = 256: the general form.
template <int NTH>
__global__ __launch_bounds__(NTH) void k_resolve_head(ResolveBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* ybuf = smem;
    double* blk = ybuf + 2 * a.nv;
    int* sh_i = reinterpret_cast<int*>(blk + a.blkd);
    const int j = blockIdx.x;
    const ResolveDims dm = a.dims[j];
    if (resolve_skip_head(dm)) return;
    const int n = a.n;
    const int t = a.tk ? a.tk[j] : a.t;
    const int kA = n < t ? n : t;
    const double* cx = a.cx + j * a.scx;
    const double* FA = a.FA + j * a.sFA;
    const long long* jpvtA = a.jpvtA + j * a.sJA;
    const double* FL = a.FL + j * a.sFL;
    const double* tauL = a.tauL + j * a.sTauL;
    const long long* jpvtL = a.jpvtL + j * a.sJL;
    double* p1 = a.p1 + j * a.sP1;
    double* bvec = a.bvec + j * a.sB;
    const int tid = threadIdx.x;
    const int dimA = dm.dimA < kA ? dm.dimA : kA;
    if (tid == 0) sh_i[0] = 0;
    for (int i = tid; i < t; i += NTH) ybuf[i] = -cx[jpvtA[i] - 1];      // b_buff = -cx[F_A.p]
    __syncthreads();
    if (dm.code == 1) {
        // b = b_buff; p1 = LowerTriangular(F_A.R') \ b        (:132-133)
        for (int i = tid; i < t; i += NTH) bvec[i] = ybuf[i];
        __syncthreads();
        wg_trsv_upper_t(FA, n, t, ybuf, blk, &sh_i[0]);
        for (int i = tid; i < t; i += NTH) p1[i] = ybuf[i];
    } else {
        // b = F_L11.Q' b_buff; dp1 = U(R_L[1:dimA, 1:dimA]) \ b[1:dimA]; p1 = ([dp1; 0][invperm(F_L11.p)])[1:rankA]   (:141-144)
        if (a.qb) {
            for (int i = tid; i < t; i += NTH) ybuf[i] = a.qb[j * a.sQb + i];
        } else if (wave_id() == 0) wave_apply_reflectors<true>(FL, t, tauL, kA, t, ybuf);
        __syncthreads();
        for (int i = tid; i < t; i += NTH) bvec[i] = ybuf[i];
        __syncthreads();
        wg_trsv<false>(FL, t, dimA, ybuf, blk, &sh_i[0]);
        for (int i = tid; i < t; i += NTH) p1[i] = 0.0;
        __syncthreads();
        for (int i = tid; i < kA; i += NTH) p1[(int)jpvtL[i] - 1] = (i < dimA) ? ybuf[i] : 0.0;
    }
    if (tid == 0) {
        a.state[j].code = dm.code;
        a.state[j].dimA = dimA;
    }
}

// k_dtemp for the range: vec[0:m] = -J1 p1 - rx, rows m .. ldw-1 zero
__global__ __launch_bounds__(256) void k_dtemp_batched(ResolveBatchArgs a) {
    const int j = blockIdx.y;
    if (resolve_skip_head(a.dims[j])) return;
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= a.ldw) return;
    const int rankA = a.state[j].rankA;
    const double* W = a.W + j * a.sW;
    const double* p1 = a.p1 + j * a.sP1;
    double s = 0.0;
    if (row < a.m) {
        for (int c = 0; c < rankA; ++c) s += W[row + (size_t)c * a.ldw] * p1[c];
        s = -s - a.rx[(size_t)j * a.m + row];
    }
    a.vec[j * a.sVec + row] = s;
}

typedef double rb_d2 __attribute__((ext_vector_type(2)));

// Q' of ONE group (tile or tree node) of (panel, level) applied to the vector C of every problem of the range: the vector form of
// k_caqr_update_refl (same geometry, same masks).  Thread p of the 16 F threads owns the row pair (block p >> 4, rows 2 (p & 15),
// + 1): V is read once, 16 bytes per lane and column, non-temporal; every wave works on rows.  A group with a full T factor gets
// the block form  w = V' c, w = T' w, c -= V w  (three barriers); the last narrow panel whose right-hand side rode through the
// factorisation has only diag(T) = tau (caqr_factor_core, GRAM = false) — exactly when T has no off-diagonal entry, where the
// block form with a genuine T would be the same product — and gets its reflectors one after the other (one barrier each).
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_caqr_vec_batched(CaqrArgs a, const ResolveDims* dims) {
    constexpr int NT = 64 * NW;
    __shared__ double Tsh[PB * (PB + 1)];
    __shared__ double wred[NW][PB];
    __shared__ double wsum[PB], zsh[PB];
    __shared__ double red[2][NW];
    if (resolve_skip_head(dims[blockIdx.y])) return;
    const int prob = blockIdx.y + a.prob0;
    const ProbState st = a.state[prob];
    const int r0 = a.panel * PB;
    if (r0 >= st.kp) return;
    const int bw = (st.kp - r0) < PB ? (st.kp - r0) : PB;
    const int col0 = st.rankA + r0;
    const int g = blockIdx.x;
    const double* W = a.W + prob * a.sW;
    const double* T = a.Tbuf + prob * a.sT + (a.tOff + g) * (long long)(PB * PB);
    double* Cv = a.C + prob * a.sC;
    const bool tri = a.level > 0;
    const int tid = threadIdx.x, ln = lane_id(), w = wave_id();
    const int q = tid >> 4, rb = (tid & 15) * 2;
    const long long bidx = (long long)g * a.F + q;
    const bool bval = bidx < a.nblocks && q >= a.skip;
    const bool dns = a.mode == 2 && ((bidx + 1) & 1) == 0;
    const long long row = caqr_block_row(a, bidx) + rb;
    const int dsh = 32 * a.skip;
    const int s0 = q * 32 + rb;          // slot of the pair's first row in the group

    int nz = 0;
    for (int e = tid; e < PB * PB; e += NT) {
        const int r = e & 31, c = e >> 5;
        const double tv = T[e];
        Tsh[r + c * (PB + 1)] = tv;
        if (r != c && r < bw && c < bw && tv != 0.0) nz = 1;
    }
    const bool blocked = __syncthreads_or(nz) != 0;

    rb_d2 c = {0.0, 0.0};
    if (bval) c = *reinterpret_cast<const rb_d2*>(Cv + row);
    const bool ldv = bval && !(tri && q == 0);
    double v0[PB], v1[PB];
#pragma unroll
    for (int jj = 0; jj < PB; ++jj) {
        rb_d2 x = {0.0, 0.0};
        if (jj < bw && ldv && (tri || s0 + 1 > jj + dsh)) x = __builtin_nontemporal_load(reinterpret_cast<const rb_d2*>(W + row + (size_t)(col0 + jj) * a.ldw));
        double a0, a1;
        if (!tri) {
            a0 = s0 > jj + dsh ? x.x : (s0 == jj + dsh ? 1.0 : 0.0);
            a1 = s0 + 1 > jj + dsh ? x.y : (s0 + 1 == jj + dsh ? 1.0 : 0.0);
        } else if (q == 0) {
            a0 = rb == jj ? 1.0 : 0.0;
            a1 = rb + 1 == jj ? 1.0 : 0.0;
        } else {
            a0 = (dns || rb <= jj) ? x.x : 0.0;
            a1 = (dns || rb + 1 <= jj) ? x.y : 0.0;
        }
        const bool on = jj < bw && bval;
        v0[jj] = on ? a0 : 0.0;
        v1[jj] = on ? a1 : 0.0;
    }

    if (blocked) {
        double wp[PB];
#pragma unroll
        for (int jj = 0; jj < PB; ++jj) wp[jj] = v0[jj] * c.x + v1[jj] * c.y;
#pragma unroll
        for (int b8 = 0; b8 < PB / 8; ++b8) {
            double d8[8], o8[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) d8[i] = wp[8 * b8 + i];
            wave_allsum8(d8, o8);
#pragma unroll
            for (int i = 0; i < 8; ++i) wp[8 * b8 + i] = o8[i];
        }
        if (ln == 0) {
#pragma unroll
            for (int jj = 0; jj < PB; ++jj) wred[w][jj] = wp[jj];
        }
        __syncthreads();
        if (tid < PB) {
            double s = 0.0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) s += wred[ww][tid];
            wsum[tid] = s;
        }
        __syncthreads();
        if (tid < PB) {          // (T' w)[tid] = sum_{i <= tid} T[i][tid] w[i]
            double z = 0.0;
            if (tid < bw)
                for (int i = 0; i <= tid; ++i) z += Tsh[i + tid * (PB + 1)] * wsum[i];
            zsh[tid] = z;
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < PB; ++jj) {
            const double z = zsh[jj];
            c.x -= v0[jj] * z;
            c.y -= v1[jj] * z;
        }
    } else {
        int par = 0;
#pragma unroll
        for (int jj = 0; jj < PB; ++jj) {
            if (jj >= bw) continue;
            const double tj = Tsh[jj + jj * (PB + 1)];
            if (tj == 0.0) continue;
            double d = wave_allsum(v0[jj] * c.x + v1[jj] * c.y);
            if (ln == 0) red[par][w] = d;
            __syncthreads();
            d = 0.0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) d += red[par][ww];
            par ^= 1;
            d *= tj;
            c.x -= d * v0[jj];
            c.y -= d * v1[jj];
        }
    }
    if (bval) *reinterpret_cast<rb_d2*>(Cv + row) = c;
}

// x <- Qt' x on the leading kp entries of every problem's vector (k_vec_reflectors for the range), one wave per problem
__global__ __launch_bounds__(64) void k_vec_reflectors_batched(ResolveBatchArgs a) {
    const int j = blockIdx.x;
    if (resolve_skip_head(a.dims[j])) return;
    const int kp = a.state[j].kp;
    if (kp > 0) wave_apply_reflectors<true>(a.Rt + j * a.sRt, a.ldr, a.tauJ + j * a.sTauJ, kp, kp, a.vec + j * a.sVec);
}

// The solve part of k_pivot_solve (refactor = 0) with each problem's own dimJ2, and the outputs.  RPL = 0: n beyond 512.
template <int RPL, int NTH>
__global__ __launch_bounds__(NTH) void k_resolve_tail(ResolveBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* ybuf = smem;
    double* pbuf = ybuf + a.nv;
    double* blk = pbuf + a.nv;
    int* sh_i = reinterpret_cast<int*>(blk + a.blkd);
    const int j = blockIdx.x;
    const ResolveDims dm = a.dims[j];
    const int tid = threadIdx.x;
    if (dm.code != 0 && a.status_out && tid == 0) a.status_out[j] = dm.status;
    if (resolve_skip(dm)) return;
    ProbState* stp = a.state + j;
    const int rankA = stp->rankA, n2 = stp->n2, kp = stp->kp;
    const int n = a.n, m = a.m;
    const double* dv = a.vec + j * a.sVec;
    const double* Rt = a.Rt + j * a.sRt;
    const long long* jpvtJ = a.jpvtJ + j * a.sJJ;
    const double* p1 = a.p1 + j * a.sP1;
    const double* bvec = a.bvec + j * a.sB;
    if (a.b_out)
        for (int i = tid; i < a.t; i += NTH) a.b_out[(size_t)j * a.t + i] = bvec[i];
    if (a.d_out)
        for (int i = tid; i < m; i += NTH) a.d_out[(size_t)j * m + i] = dv[i];
    if (dm.dimJ2 == RESOLVE_HOLD) {
        if (a.info_out && tid == 0) a.info_out[j] = {stp->rankA, stp->rankJ2, stp->code, stp->dimA, stp->dimJ2, stp->status};
        return;
    }
    const int dimJ2 = dm.dimJ2 < kp ? dm.dimJ2 : kp;
    if (tid == 0) sh_i[0] = 0;
    for (int i = tid; i < n2; i += NTH) ybuf[i] = (i < dimJ2) ? dv[i] : 0.0;
    __syncthreads();
    wg_trsv<false>(Rt, a.ldr, dimJ2, ybuf, blk, &sh_i[0]);
    for (int i = tid; i < rankA; i += NTH) pbuf[i] = p1[i];
    for (int i = tid; i < n2; i += NTH) pbuf[rankA + (int)jpvtJ[i] - 1] = (i < dimJ2) ? ybuf[i] : 0.0;
    __syncthreads();
    if (wave_id() == 0) {
        const double* FA = a.FA + j * a.sFA;
        const double* tauA = a.tauA + j * a.sTauA;
        if constexpr (RPL > 0) wave_apply_reflectors_reg<false, RPL>(FA, n, tauA, a.kA, n, pbuf);
        else wave_apply_reflectors<false>(FA, n, tauA, a.kA, n, pbuf);
    }
    __syncthreads();
    if (a.p_out)
        for (int i = tid; i < n; i += NTH) a.p_out[(size_t)j * n + i] = pbuf[i];
    if (tid == 0) {
        stp->dimJ2 = dimJ2;
        stp->status |= sh_i[0];
        if (a.info_out) a.info_out[j] = {stp->rankA, stp->rankJ2, stp->code, stp->dimA, dimJ2, stp->status};
    }
}

// diag(F.R) of every problem of the range into out (stride doubles per slot), zeros past each problem's own length
__global__ __launch_bounds__(64) void k_diag_gather(ResolveBatchArgs a, int which, double* out, long long stride) {
    const int j = blockIdx.x;
    const int t = a.tk ? a.tk[j] : a.t;
    const int kA = a.n < t ? a.n : t;
    const double* F;
    int ld, kd;
    if (which == ENLSIP_GN_FACTOR_A) { F = a.FA + j * a.sFA; ld = a.n; kd = kA; }
    else if (which == ENLSIP_GN_FACTOR_L11) { F = a.FL + j * a.sFL; ld = t; kd = t < kA ? t : kA; }
    else { F = a.Rt + j * a.sRt; ld = a.ldr; kd = a.state[j].kp; }
    for (long long i = threadIdx.x; i < stride; i += 64) out[j * stride + i] = i < kd ? F[i + (size_t)i * ld] : 0.0;
}

}  // namespace gn
