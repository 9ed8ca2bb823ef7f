// Batched Newton direction (gn_newton_batched.inc): newton_search_direction (src/enlsip_functions.jl:348-423) after its Hessian
// sums for a range of the resident batch, on the RESIDENT factors — no pass over J, nothing factored again.  With
// F_J2: J2 Pi = Q R (R the kp x n2 upper trapezoid in Rt, Pi from jpvtJ) and d = F_J2.Q' d_temp, d_temp = -(rx + J1 p1):
//     J2'J2            = Pi R'R Pi'
//     -W21 p1 - J2'rx  = -E21 p1 + J2' d_temp = -E21 p1 + Pi R' d[1:kp]
// Stages, one launch each over (work, problem) grids; a slot whose request is not 1 exits at once:
//   k_newton_side<false>    X = F_A.Q' Gamma     the kA reflectors of F_A applied to 8 columns per workgroup        (:398)
//   k_newton_side<true>     E = X F_A.Q          the same reflectors applied to 8 rows per workgroup
//   k_newton_w22            sW22 = sym(E22) + Pi R'R Pi' on v_mfma_f64_16x16x4 (tiles of the upper triangle of R'R, scattered
//                           by jpvtJ to both triangles), E read through F_L11.p where t > rankA (:396-399); rhs   (:405-411)
//   k_newton_chol_batched   blocked right-looking Cholesky (panel 32, trailing update on MFMA), the two triangular solves,
//                           p = F_A.Q [p1; p2]                                                                      (:414-421)
#pragma once
#include "gn_kernels_resolve_batched.hpp"

namespace gn {

typedef double nwb_d4 __attribute__((ext_vector_type(4)));

constexpr int NWB_VEC = 8;       // vectors (columns or rows of the n x n matrix) per workgroup of k_newton_side, 2 per wave
constexpr int NWB_NB = 32;       // panel width of the Cholesky factorisation

// all pointers address slot 0 of the segment (problem k0 of the handle)
struct NewtonBatchArgs {
    int n, t, kA, ldr;              // t, kA: the batch's (t_max of a ragged batch)
    const int* req;                 // per slot: 0 leave alone, 1 take the step, 2 rank-deficient working set with t < n (status only)
    const int* tk;                  // ragged batch: each problem's own t, else NULL
    const ProbState* state;
    const double* FA;    long long sFA;
    const double* tauA;  long long sTauA;
    const long long* jpvtL; long long sJL;
    const double* p1;    long long sP1;
    const double* vec;   long long sVec;     // F_J2.Q' d_temp of the default p1 (the call's own buffer, not the resident vec)
    const double* Rt;    long long sRt;
    const long long* jpvtJ; long long sJJ;
    const double* Gamma; long long ldg, strideG;
    double* X;           long long sX;       // n x n per slot: F_A.Q' Gamma, later sW22 and its factor (ld n2)
    double* E;                               // n x n per slot (stride sX)
    double* rhs;                             // n per slot
    double* p_out;                           // n per slot
    int* status_out;                         // 1 per slot
    int* flag;                               // set when some slot of the segment is flagged
};

inline size_t newton_side_lds(int n) { return (size_t)NWB_VEC * (n + 1) * 8; }

// ROWS = false: X[:, c] = F_A.Q' Gamma[:, c] for the workgroup's 8 columns.  ROWS = true: E[r, :] = (F_A.Q' X[r, :]')' for its 8 rows,
// i.e. E = X F_A.Q.  The vectors sit in LDS (ld n + 1); a wave applies every reflector to its two vectors, lane l owning the
// entries l + 64 i of both, so a reflector is fetched once per pair and no lane reads what another lane wrote.  Every element
// of the source is read once and every element of the destination written once.
template <bool ROWS>
__global__ __launch_bounds__(256) void k_newton_side(NewtonBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int j = blockIdx.y;
    if (a.req[j] != 1 || a.state[j].n2 == 0) return;
    const int n = a.n, ldx = n + 1;
    const int v0 = blockIdx.x * NWB_VEC;
    const int nv = (n - v0) < NWB_VEC ? (n - v0) : NWB_VEC;
    const int tid = threadIdx.x;
    const double* src = ROWS ? a.X + j * a.sX : a.Gamma + j * a.strideG;
    double* dst = ROWS ? a.E + j * a.sX : a.X + j * a.sX;
    if (ROWS) {
        for (int e = tid; e < NWB_VEC * n; e += 256) {
            const int i = e % NWB_VEC, c = e / NWB_VEC;
            smem[i * ldx + c] = (i < nv) ? src[(v0 + i) + (size_t)c * n] : 0.0;
        }
    } else {
        for (int e = tid; e < NWB_VEC * n; e += 256) {
            const int i = e / n, r = e % n;
            smem[i * ldx + r] = (i < nv) ? src[r + (size_t)(v0 + i) * a.ldg] : 0.0;
        }
    }
    __syncthreads();
    const int w = wave_id(), ln = lane_id();
    if (2 * w < nv) {
        double* x0 = smem + (2 * w) * ldx;
        double* x1 = x0 + ldx;
        const double* FA = a.FA + j * a.sFA;
        const double* tauA = a.tauA + j * a.sTauA;
        for (int k = 0; k < a.kA; ++k) {      // Q' = H_{kA-1} ... H_0: H_0 first
            const double tj = tauA[k];
            if (tj == 0.0) continue;
            const double* v = FA + (size_t)k * n;
            double d[2] = {0.0, 0.0}, o[2];
            for (int r = (k & ~63) + ln; r < n; r += 64) {
                const double vr = (r > k) ? v[r] : (r == k ? 1.0 : 0.0);
                d[0] += vr * x0[r];
                d[1] += vr * x1[r];
            }
            wave_allsumN(d, o);
            const double s0 = o[0] * tj, s1 = o[1] * tj;
            for (int r = (k & ~63) + ln; r < n; r += 64) {
                const double vr = (r > k) ? v[r] : (r == k ? 1.0 : 0.0);
                x0[r] -= s0 * vr;
                x1[r] -= s1 * vr;
            }
        }
    }
    __syncthreads();
    if (ROWS) {
        for (int e = tid; e < NWB_VEC * n; e += 256) {
            const int i = e % NWB_VEC, c = e / NWB_VEC;
            if (i < nv) dst[(v0 + i) + (size_t)c * n] = smem[i * ldx + c];
        }
    } else {
        for (int e = tid; e < NWB_VEC * n; e += 256) {
            const int i = e / n, r = e % n;
            if (i < nv) dst[r + (size_t)(v0 + i) * n] = smem[i * ldx + r];
        }
    }
}

// grid x: nt * nt tile blocks (nt = ceil(n / 16); a block below the diagonal or beyond the problem's n2 exits), then
// ceil(n / 64) right-hand-side blocks; one wave each.  MFMA f64 16x16x4 fragment maps: A[i = l & 15][k = l >> 4],
// B[k = l >> 4][j = l & 15], D[i = (l >> 4) + 4 r][j = l & 15].  Tile (I, J), I <= J, of G = R'R sums over k <= 16 I + 15 only
// (R is upper trapezoidal; what Rt holds below the diagonal are reflectors and is masked).
__global__ __launch_bounds__(64) void k_newton_w22(NewtonBatchArgs a) {
    const int j = blockIdx.y;
    if (a.req[j] != 1) return;
    const ProbState st = a.state[j];
    const int n = a.n, rankA = st.rankA, n2 = st.n2, kp = st.kp, ldr = a.ldr;
    if (n2 == 0) return;
    const int nt = (n + 15) / 16;
    const int t = a.tk ? a.tk[j] : a.t;
    const bool perm = t != rankA;             // E[F_L11.p, F_L11.p] (:396-399; t >= n here)
    const long long* pl = a.jpvtL + j * a.sJL;
    const long long* pj = a.jpvtJ + j * a.sJJ;
    const double* E = a.E + j * a.sX;
    const double* R = a.Rt + j * a.sRt;
    double* W = a.X + j * a.sX;               // sW22, ld n2 (X is dead after the second side)
    auto pe = [&](int x) { return perm ? (int)pl[x] - 1 : x; };
    const int ln = threadIdx.x, lr = ln & 15, lq = ln >> 4;
    const int bx = blockIdx.x;
    if (bx < nt * nt) {
        const int I = bx / nt, J = bx % nt;
        if (J < I || 16 * J >= n2) return;
        const int ia = 16 * I + lr, jb = 16 * J + lr;
        const int kmax = kp < 16 * I + 16 ? kp : 16 * I + 16;
        nwb_d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < kmax; k0 += 4) {
            const int k = k0 + lq;
            const double av = (k < kp && ia < n2 && k <= ia) ? R[k + (size_t)ia * ldr] : 0.0;
            const double bv = (k < kp && jb < n2 && k <= jb) ? R[k + (size_t)jb * ldr] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
        if (jb < n2) {
            const int cb = (int)pj[jb] - 1, eb = pe(rankA + cb);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ii = 16 * I + lq + 4 * r;
                if (ii >= n2) continue;
                const int ca = (int)pj[ii] - 1, ea = pe(rankA + ca);
                const double val = acc[r] + 0.5 * (E[ea + (size_t)eb * n] + E[eb + (size_t)ea * n]);
                W[ca + (size_t)cb * n2] = val;
                if (I != J) W[cb + (size_t)ca * n2] = val;
            }
        }
    } else {
        // rhs[Pi i] = (R' d)[i] - (E21 p1)[Pi i]
        const int i = (bx - nt * nt) * 64 + ln;
        if (i >= n2) return;
        const double* dv = a.vec + j * a.sVec;
        const double* p1 = a.p1 + j * a.sP1;
        const int ke = i < kp - 1 ? i : kp - 1;
        double s = 0.0;
        for (int k = 0; k <= ke; ++k) s += R[k + (size_t)i * ldr] * dv[k];
        const int ca = (int)pj[i] - 1, ea = pe(rankA + ca);
        double e = 0.0;
        for (int c = 0; c < rankA; ++c) e += E[ea + (size_t)pe(c) * n] * p1[c];
        a.rhs[(size_t)j * n + ca] = s - e;
    }
}

// Cholesky of sW22 (LAPACK dpotrf semantics: a pivot <= 0 or NaN = not positive definite, which is what isposdef reports), the
// two triangular solves and p = F_A.Q [p1; p2]; one workgroup per problem, the matrix stays in global memory (L2) and only the
// 32 x 32 diagonal block of a panel step is factored out of LDS.  NTH = 64: one wave per problem (n <= 64); NTH = 256: general.
// L is mirrored into the upper triangle as it is produced, so that the second solve reads U = L' as stored.
template <int NTH>
__global__ __launch_bounds__(NTH) void k_newton_chol_batched(NewtonBatchArgs a) {
    constexpr int NB = NWB_NB, LDB = NB + 1, NVEC = NTH == 64 ? 64 : 1024;
    __shared__ double blk[64 * 65];       // the panel's diagonal block (ld 33), then the blocks of wg_trsv
    __shared__ double y[NVEC], pb[NVEC];
    __shared__ int sh[2];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int rq = a.req[j];
    if (rq == 0) return;
    if (rq == 2) {
        if (tid == 0) { a.status_out[j] = 2; atomicOr(a.flag, 1); }
        return;
    }
    const ProbState st = a.state[j];
    const int n = a.n, rankA = st.rankA, n2 = st.n2;
    const double* p1 = a.p1 + j * a.sP1;
    double* pout = a.p_out + (size_t)j * n;
    if (n2 == 0) {        // :374-376: p1 as it is
        for (int i = tid; i < n; i += NTH) pout[i] = p1[i];
        if (tid == 0) a.status_out[j] = 0;
        return;
    }
    double* A = a.X + j * a.sX;
    const int ld = n2;
    const int ln = lane_id(), lr = ln & 15, lq = ln >> 4;
    if (tid == 0) { sh[0] = 0; sh[1] = 0; }
    __syncthreads();
    for (int j0 = 0; j0 < n2; j0 += NB) {
        const int nb = (n2 - j0) < NB ? (n2 - j0) : NB;
        for (int e = tid; e < nb * nb; e += NTH) {
            const int r = e % nb, c = e / nb;
            blk[r + c * LDB] = A[(j0 + r) + (size_t)(j0 + c) * ld];
        }
        __syncthreads();
        if (wave_id() == 0) {
            for (int k = 0; k < nb; ++k) {
                const double akk = uniform_f64(blk[k + k * LDB]);
                if (!(akk > 0.0)) {
                    if (ln == 0) sh[0] = 1;
                    break;
                }
                const double l = sqrt(akk);
                double lrk = 0.0;
                if (ln >= k && ln < nb) {
                    lrk = (ln == k) ? l : blk[ln + k * LDB] / l;
                    blk[ln + k * LDB] = lrk;
                }
                wave_mem_sync();
                for (int c = k + 1; c < nb; ++c)
                    if (ln >= c && ln < nb) blk[ln + c * LDB] -= lrk * blk[c + k * LDB];
                wave_mem_sync();
            }
        }
        __syncthreads();
        if (sh[0]) break;
        for (int e = tid; e < nb * nb; e += NTH) {
            const int r = e % nb, c = e / nb;
            if (r < c) continue;
            const double v = blk[r + c * LDB];
            A[(j0 + r) + (size_t)(j0 + c) * ld] = v;
            A[(j0 + c) + (size_t)(j0 + r) * ld] = v;
        }
        // rows below the block: X L' = A[rows, panel], one row per thread, 8 columns at a time (the earlier columns of the row
        // are read back from where this thread stored them)
        for (int r = j0 + nb + tid; r < n2; r += NTH) {
            for (int cb = 0; cb < nb; cb += 8) {
                double x[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = (cb + i < nb) ? A[r + (size_t)(j0 + cb + i) * ld] : 0.0;
                for (int k = 0; k < cb; ++k) {
                    const double xk = A[r + (size_t)(j0 + k) * ld];
#pragma unroll
                    for (int i = 0; i < 8; ++i) x[i] -= xk * blk[(cb + i) + k * LDB];
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (cb + i >= nb) continue;
#pragma unroll
                    for (int k = 0; k < i; ++k) x[i] -= x[k] * blk[(cb + i) + (cb + k) * LDB];
                    x[i] /= blk[(cb + i) + (cb + i) * LDB];
                    A[r + (size_t)(j0 + cb + i) * ld] = x[i];
                    A[(j0 + cb + i) + (size_t)r * ld] = x[i];
                }
            }
        }
        __syncthreads();
        // trailing update of the lower triangle, 16 x 16 tiles dealt to the waves: A[R, C] -= P[R, :] P[C, :]'
        const int t0 = j0 + nb;
        const int nrt = (n2 - t0 + 15) / 16;
        const int ntl = nrt * (nrt + 1) / 2;
        for (int tile = wave_id(); tile < ntl; tile += NTH / 64) {
            int ti = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
            while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
            while (ti * (ti + 1) / 2 > tile) --ti;
            const int tj = tile - ti * (ti + 1) / 2;
            const int R0 = t0 + 16 * ti, C0 = t0 + 16 * tj;
            nwb_d4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < nb; k0 += 4) {
                const int k = k0 + lq;
                const double av = (k < nb && R0 + lr < n2) ? A[(R0 + lr) + (size_t)(j0 + k) * ld] : 0.0;
                const double bv = (k < nb && C0 + lr < n2) ? A[(C0 + lr) + (size_t)(j0 + k) * ld] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
            const int col = C0 + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = R0 + lq + 4 * r;
                if (col < n2 && row < n2 && row >= col) A[row + (size_t)col * ld] -= acc[r];
            }
        }
        __syncthreads();
    }
    if (sh[0]) {          // :417-420: p = zeros, error = true
        for (int i = tid; i < n; i += NTH) pout[i] = 0.0;
        if (tid == 0) { a.status_out[j] = 1; atomicOr(a.flag, 1); }
        return;
    }
    for (int i = tid; i < n2; i += NTH) y[i] = a.rhs[(size_t)j * n + i];
    __syncthreads();
    wg_trsv<true>(A, ld, n2, y, blk, &sh[1]);
    wg_trsv<false>(A, ld, n2, y, blk, &sh[1]);
    for (int i = tid; i < rankA; i += NTH) pb[i] = p1[i];
    for (int i = tid; i < n2; i += NTH) pb[rankA + i] = y[i];
    __syncthreads();
    if (wave_id() == 0) wave_apply_reflectors<false>(a.FA + j * a.sFA, n, a.tauA + j * a.sTauA, a.kA, n, pb);
    __syncthreads();
    for (int i = tid; i < n; i += NTH) pout[i] = pb[i];
    if (tid == 0) a.status_out[j] = 0;
}

}  // namespace gn
