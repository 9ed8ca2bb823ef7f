// One-call subspace minimisation (gn_subspace_batched.inc): lines :1251-1253 of search_direction_analys with the dimension choice
// of choose_subspace_dimensions (src/enlsip_functions.jl:1118-1176) on the device, between the stages of the batched re-solve
// (gn_kernels_resolve_batched.hpp), which run unchanged:
//   k_subspace_head           b (:1251), dimA by determine_solving_dim (:1144-1150) on b in LDS, p1(dimA) (:1156-1157)
//   k_dtemp_batched, k_caqr_vec_batched, k_vec_reflectors_batched      d = F_J2.Q' (-(rx + J1 p1)) (:1158-1163)
//   k_subspace_dimj2          dimJ2 (:1165-1169), the max with the previous dimensions (:1171-1174), range checks; writes the
//                             request of the closing pass
//   [b, p1, d again with the final dimA where the max raised it: sub_search_direction (:1253) is called with the final pair]
//   k_resolve_tail            p (:1253) and the outputs
// The choice itself is gn_subspace_choice.hpp, run by one lane on LDS copies of the vector and the diagonal; the other lanes /
// waves load those and reduce the norms.  No scratch.
#pragma once
#include "gn_kernels_resolve_batched.hpp"
#include "gn_subspace_choice.hpp"

namespace gn {

enum { SS_OUT_OF_BOUNDS = CHOICE_OUT_OF_BOUNDS };

struct SubspaceArgs {
    ResolveDims* dims;       // first pass: code / status in, the chosen dimA (and a status 5) out
    ResolveDims* dims2;      // closing pass, written by k_subspace_dimj2: dimA = HOLD where b, p1 and d stand, the final dimA where
                             // they are computed again; status 1 / 2 / 5 where the problem is flagged
    const enlsip_gn_subspace_prev* prev;
    int nc;                  // LDS length of the dimA choice (>= min(n, t_max))
    int nr;                  // LDS length of the dimJ2 choice (>= min(m, n))
};

inline size_t subspace_head_lds_bytes(int nv, int blkd, int nc) { return resolve_lds_bytes(nv, blkd) + (size_t)3 * nc * 8; }
inline size_t subspace_dimj2_lds_bytes(int nr) { return (size_t)(4 * nr + 16) * 8; }

// k_resolve_head's code = -1 branch with the choice of dimA between b and the substitution.  A problem whose choice would index
// out of bounds in the reference gets status 5 in its request and nothing of it is written.
template <int NTH>
__global__ __launch_bounds__(NTH) void k_subspace_head(ResolveBatchArgs a, SubspaceArgs c) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* ybuf = smem;
    double* blk = ybuf + 2 * a.nv;
    int* sh_i = reinterpret_cast<int*>(blk + a.blkd);
    double* tau = blk + a.blkd + 8;
    double* rho = tau + c.nc;
    double* dg = rho + c.nc;
    const int j = blockIdx.x;
    const ResolveDims dm = c.dims[j];
    if (resolve_skip(dm)) return;
    const int n = a.n;
    const int t = a.tk ? a.tk[j] : a.t;
    const int kA = n < t ? n : t;
    const double* cx = a.cx + j * a.scx;
    const long long* jpvtA = a.jpvtA + j * a.sJA;
    const double* FL = a.FL + j * a.sFL;
    const double* tauL = a.tauL + j * a.sTauL;
    const long long* jpvtL = a.jpvtL + j * a.sJL;
    double* p1 = a.p1 + j * a.sP1;
    double* bvec = a.bvec + j * a.sB;
    const int tid = threadIdx.x;
    const int rankA = a.state[j].rankA < kA ? a.state[j].rankA : kA;
    const enlsip_gn_subspace_prev pv = c.prev[j];
    if (tid == 0) { sh_i[0] = 0; sh_i[1] = 0; sh_i[2] = 0; }
    for (int i = tid; i < t; i += NTH) ybuf[i] = -cx[jpvtA[i] - 1];      // b_buff = -cx[F_A.p]
    for (int i = tid; i < rankA; i += NTH) dg[i] = FL[i + (size_t)i * t];
    __syncthreads();
    if (a.qb) {
        for (int i = tid; i < t; i += NTH) ybuf[i] = a.qb[j * a.sQb + i];
    } else if (wave_id() == 0) wave_apply_reflectors<true>(FL, t, tauL, kA, t, ybuf);      // b = F_L11.Q' b_buff (:1251)
    __syncthreads();
    if (wave_id() == 0 && rankA > 0) {      // rankA <= 0: dimA = 0, previous_dimA = 0 (:1136-1138)
        const long long pd = pv.previous_dimA;
        const int ln = lane_id();
        double s_all = 0.0, s_prev = 0.0;
        for (int i = ln; i < t; i += WAVE) {
            const double v = ybuf[i] * ybuf[i];
            s_all += v;
            if (i < pd) s_prev += v;
        }
        s_all = wave_allsum(s_all);
        s_prev = wave_allsum(s_prev);
        if (ln == 0) {
            long long dimA = 0;
            int st = pd > t ? SS_OUT_OF_BOUNDS : 0;      // b[1:previous_dimA] (:1145)
            if (!st)
                st = choice_determine_solving_dim(pd, rankA, sqrt(s_all), pv.constraint_progress, sqrt(s_prev), dg, 1, ybuf,
                                                  pv.previous_alpha, pv.restart != 0, tau, rho, &dimA, nullptr);
            sh_i[1] = (int)dimA;
            sh_i[2] = st;
        }
    }
    __syncthreads();
    const int dimA = sh_i[1];
    if (sh_i[2]) {
        if (tid == 0) c.dims[j].status = sh_i[2];
        return;
    }
    for (int i = tid; i < t; i += NTH) bvec[i] = ybuf[i];
    __syncthreads();
    // dp1 = U(R_L[1:dimA, 1:dimA]) \ b[1:dimA]; p1 = ([dp1; 0][invperm(F_L11.p)])[1:rankA]   (:1156-1157)
    wg_trsv<false>(FL, t, dimA, ybuf, blk, &sh_i[0]);
    for (int i = tid; i < t; i += NTH) p1[i] = 0.0;
    __syncthreads();
    for (int i = tid; i < kA; i += NTH) p1[(int)jpvtL[i] - 1] = (i < dimA) ? ybuf[i] : 0.0;
    if (tid == 0) c.dims[j].dimA = dimA;
}

// dimJ2 from d = F_J2.Q' d_temp and diag(F_J2.R), then the final pair and its checks.  One workgroup per problem: every wave
// reduces ||d|| and ||d[1:previous_dimJ2]|| over the m entries, one lane runs the choice.
template <int NTH>
__global__ __launch_bounds__(NTH) void k_subspace_dimj2(ResolveBatchArgs a, SubspaceArgs c) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NW = NTH / WAVE;
    double* yl = smem;
    double* dg = yl + c.nr;
    double* tau = dg + c.nr;
    double* rho = tau + c.nr;
    double* red = rho + c.nr;                 // 2 NW partial sums
    int* sh_i = reinterpret_cast<int*>(red + 8);
    const int j = blockIdx.x;
    const int tid = threadIdx.x;
    const ResolveDims dm = c.dims[j];
    if (resolve_skip(dm)) {
        if (tid == 0) c.dims2[j] = {RESOLVE_HOLD, 0, dm.code, dm.status};      // dimA = HOLD: nothing of this problem was touched
        return;
    }
    ProbState* stp = a.state + j;
    const int m = a.m, n = a.n;
    const int t = a.tk ? a.tk[j] : a.t;
    const int rankA = stp->rankA, kp = stp->kp;
    const int rankJ2 = stp->rankJ2 < kp ? stp->rankJ2 : kp;
    const enlsip_gn_subspace_prev pv = c.prev[j];
    const long long pd = pv.previous_dimJ2;
    const double* dv = a.vec + j * a.sVec;
    const double* Rt = a.Rt + j * a.sRt;
    double s_all = 0.0, s_prev = 0.0;
    for (int i = tid; i < m; i += NTH) {
        const double v = dv[i] * dv[i];
        s_all += v;
        if (i < pd) s_prev += v;
    }
    s_all = wave_allsum(s_all);
    s_prev = wave_allsum(s_prev);
    if (lane_id() == 0) { red[wave_id()] = s_all; red[NW + wave_id()] = s_prev; }
    for (int i = tid; i < rankJ2; i += NTH) {
        yl[i] = dv[i];
        dg[i] = Rt[i + (size_t)i * a.ldr];
    }
    __syncthreads();
    if (tid == 0) {
        s_all = 0.0; s_prev = 0.0;
        for (int w = 0; w < NW; ++w) { s_all += red[w]; s_prev += red[NW + w]; }
        long long dimJ2 = 0;
        int st = pd > m ? SS_OUT_OF_BOUNDS : 0;      // d[1:previous_dimJ2] (:1166)
        if (!st)
            st = choice_determine_solving_dim(pd, rankJ2, sqrt(s_all), pv.residual_progress, sqrt(s_prev), dg, 1, yl,
                                              pv.previous_alpha, pv.restart != 0, tau, rho, &dimJ2, nullptr);
        const int dimA0 = dm.dimA;
        long long dimA = dimA0;
        if (!st && choice_keeps_previous(pv.previous_alpha, pv.restart != 0)) {      // :1171-1174
            const long long pa = rankA > 0 ? pv.previous_dimA : 0;
            dimA = dimA > pa ? dimA : pa;
            dimJ2 = dimJ2 > pd ? dimJ2 : pd;
        }
        const int tmax = n < t ? n : t;
        if (!st && (dimA < 0 || dimA > tmax)) st = 1;
        if (!st && (dimJ2 < 0 || dimJ2 > kp)) st = 2;
        // b, p1 and d stand for dimA0: the record says so until the closing pass rewrites them
        stp->code = -1;
        stp->dimA = dimA0;
        const long long big = 0x7fffffff;
        const int dA = (int)(dimA < big ? dimA : big), dJ = (int)(dimJ2 < big ? dimJ2 : big);
        c.dims2[j] = {(!st && dA == dimA0) ? RESOLVE_HOLD : (st == SS_OUT_OF_BOUNDS ? dimA0 : dA), dJ, -1, st};
        if ((st == 1 || st == 2) && a.info_out) a.info_out[j] = {rankA, stp->rankJ2, -1, dimA, dimJ2, stp->status};
        sh_i[0] = st;
    }
    __syncthreads();
    const int st = sh_i[0];
    if (st == 1 || st == 2) {      // no p; b and the d the choice of dimJ2 read
        const double* bvec = a.bvec + j * a.sB;
        if (a.b_out)
            for (int i = tid; i < a.t; i += NTH) a.b_out[(size_t)j * a.t + i] = bvec[i];
        if (a.d_out)
            for (int i = tid; i < m; i += NTH) a.d_out[(size_t)j * m + i] = dv[i];
    }
}

}  // namespace gn
