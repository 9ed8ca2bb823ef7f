// Batched forms of the consumers of a solve (gn_lagrange_batched.inc): J' v, J p (+ x0) and the two multiplier estimates over a
// contiguous range of the resident problems, one launch per stage whatever the range size.  The problem index comes from the grid;
// slot j of every buffer holds problem k0 + j of the handle (the caller offsets the bases), strides are those of the batched solve
// with t = t_max, and each problem uses its own t (ragged batch: tk != nullptr).
//
// The products keep the per-problem kernels' summation order lane for lane (k_gemv_t, k_gemv_n_add), so their results are bitwise
// those of enlsip_gn_gradient / enlsip_gn_jacobian_times.  The general estimate runs lagrange_wg_body, the body of k_lagrange, on
// one workgroup per problem (bitwise the per-problem estimate).  The wave-per-problem estimate (n <= 64, t_max <= 64) does a whole
// problem in one wave with no barrier, four problems per workgroup.
#pragma once
#include "gn_kernels_lagrange.hpp"

namespace gn {

// One column of A' x in the order of k_gemv_t: lane ln adds rows ln, ln + 64, ... in ascending order, then the wave all-reduce.
// Every lane returns the sum.  Shared with the termination call (gn_kernels_termination_batched.hpp), whose gradient is these bits.
__device__ __forceinline__ double gemv_t_column(const double* __restrict__ col, const double* __restrict__ x, int rows, int ln) {
    double s = 0.0;
#pragma unroll 8
    for (int r = ln; r < rows; r += WAVE) s += col[r] * x[r];
    return wave_allsum(s);
}

// y_j[c] = sum_r A_j[r + c*ld] * x_j[r] for c < ncols_j (ncols_j = tk ? tk[j] : ncols), y_j[c] = 0 for ncols_j <= c < ncols.
// grid (ceil(ncols / 4), count): one wave per column, lanes along rows, the order of k_gemv_t.
__global__ __launch_bounds__(256) void k_gemv_t_batched(const double* __restrict__ A, long long ld, long long sA, int rows, int ncols,
                                                        const int* __restrict__ tk, const double* __restrict__ x, long long sx,
                                                        double* __restrict__ y, long long sy) {
    const int c = blockIdx.x * 4 + wave_id();
    if (c >= ncols) return;
    const long long j = blockIdx.y;
    const int ln = lane_id();
    const int nc = tk ? tk[j] : ncols;
    double* yj = y + j * sy;
    if (c >= nc) {
        if (ln == 0) yj[c] = 0.0;
        return;
    }
    const double* col = A + j * sA + (size_t)c * ld;
    const double* xj = x + j * sx;
    const double s = gemv_t_column(col, xj, rows, ln);
    if (ln == 0) yj[c] = s;
}

// y_j[r] = x0_j[r] + sum_c A_j[r + c*ld] * p_j[c], r < rows (x0 may be null): grid (ceil(rows / 256), count), the order of k_gemv_n_add
__global__ __launch_bounds__(256) void k_gemv_n_add_batched(const double* __restrict__ A, long long ld, long long sA, int rows,
                                                            int ncols, const double* __restrict__ p, long long sp,
                                                            const double* __restrict__ x0, long long sx0, double* __restrict__ y,
                                                            long long sy) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const long long j = blockIdx.y;
    const double* Aj = A + j * sA;
    const double* pj = p + j * sp;
    double s = x0 ? x0[j * sx0 + r] : 0.0;
#pragma unroll 8
    for (int c = 0; c < ncols; ++c) s += Aj[r + (size_t)c * ld] * pj[c];
    y[j * sy + r] = s;
}

struct LagrangeBatchArgs {
    int mode;                   // 1: first estimate (vec: grad, stride n), 2: second estimate (vec: J1'(rx + J p), stride t_max)
    int count, n, t_max;
    const int* tk;              // each problem's t (ragged batch), null: t_max for all
    const ProbState* state;     // rankA of the solve (mode 2)
    const double* FA; long long sFA;
    const double* tauA; long long sTauA;
    const long long* jpvtA; long long sJA;
    const double* cx; long long scx;      // mode 1
    const double* vec; long long svec;
    const double* diag_scale;   // stride t_max, may be null
    double eps_rank;
    double* lambda;             // stride t_max; entries past the problem's t are set to 0
    double* grad_res;           // mode 1, may be null
    int* status;                // 0, 1 (singular triangular system) or 2 (pseudo-rank beyond the solve's rank), may be null
    int* flag;                  // OR of every status != 0 of the launch (one int)
};

// ||x[0:n)|| summed in order with a correctly rounded square root: the per-problem entry point's host sum for t = 0
__device__ __forceinline__ double serial_norm(const double* x, int n) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += x[i] * x[i];
    return sqrt(s);
}

__device__ __forceinline__ int lagrange_status_code(int bits) { return (bits & 2) ? 2 : ((bits & 1) ? 1 : 0); }

// General form: one workgroup per problem (grid count), the body of k_lagrange.  LDS as k_lagrange (~57 KB).
__global__ __launch_bounds__(256) void k_lagrange_batched(LagrangeBatchArgs b) {
    __shared__ double bq[1024], v[1024], u[1024];
    __shared__ double blk[64 * 65];
    __shared__ double red[4];
    __shared__ int sh[2];
    const long long j = blockIdx.x;
    const int tid = threadIdx.x;
    const int t = b.tk ? b.tk[j] : b.t_max;
    double* lam = b.lambda + j * b.t_max;
    for (int i = t + tid; i < b.t_max; i += 256) lam[i] = 0.0;
    if (t == 0) {      // no active constraint: lambda is empty, grad_res = ||grad|| (Q = I, prankA = 0)
        if (tid == 0) {
            if (b.mode == 1 && b.grad_res) b.grad_res[j] = serial_norm(b.vec + j * b.svec, b.n);
            if (b.status) b.status[j] = 0;
        }
        return;
    }
    LagrangeArgs a{};
    a.mode = b.mode; a.n = b.n; a.t = t; a.kA = min(b.n, t); a.rank_solve = b.state[j].rankA;
    a.FA = b.FA + j * b.sFA; a.tauA = b.tauA + j * b.sTauA; a.jpvtA = b.jpvtA + j * b.sJA;
    a.cx = b.cx ? b.cx + j * b.scx : nullptr;
    a.vec = b.vec + j * b.svec;
    a.diag_scale = b.diag_scale ? b.diag_scale + j * b.t_max : nullptr;
    a.eps_rank = b.eps_rank;
    a.lambda = lam;
    lagrange_wg_body(a, bq, v, u, blk, red, sh, b.grad_res ? b.grad_res + j : &red[0]);     // (red[0]: a sink for no grad_res)
    if (tid == 0) {
        const int code = lagrange_status_code(sh[1]);
        if (b.status) b.status[j] = code;
        if (code) atomicOr(b.flag, 1);
    }
}

// Wave-per-problem form, n <= 64 and t_max <= 64: lane i owns entry i of every vector.  Q' grad by the register form of
// wave_apply_reflectors, the pseudo-rank by one ballot, both triangular systems by the row-scaled substitution of wg_trsv with the
// rows of R read from L2 (the two back substitutions share one pass), then the inverse permutation and diag_scale.  No barrier;
// four problems per 256-thread workgroup, 2 KB of LDS for the reflector vector.
__global__ __launch_bounds__(256) void k_lagrange_wave(LagrangeBatchArgs b) {
    __shared__ double xs[4][WAVE];
    const int ln = lane_id(), w = wave_id();
    const long long j = (long long)blockIdx.x * 4 + w;
    if (j >= b.count) return;
    const int n = b.n, tmax = b.t_max;
    const int t = b.tk ? b.tk[j] : tmax;
    double* lam = b.lambda + j * tmax;
    const double* vec = b.vec + j * b.svec;
    if (t == 0) {
        if (ln < tmax) lam[ln] = 0.0;
        if (ln == 0) {
            if (b.mode == 1 && b.grad_res) b.grad_res[j] = serial_norm(vec, n);
            if (b.status) b.status[j] = 0;
        }
        return;
    }
    const int kA = min(n, t);
    const double* FA = b.FA + j * b.sFA;
    const long long* jp = b.jpvtA + j * b.sJA;
    // pseudo-rank (pseudo_rank_serial): the first i < kA with |R_ii| not above tol, kA if none; 0 if |R_00| < eps_rank
    const double d0 = fabs(FA[0]);
    int pr = 0;
    if (!(d0 < b.eps_rank)) {
        const double tol = d0 * sqrt((double)kA) * b.eps_rank;
        const double dl = (ln < kA) ? FA[ln + (size_t)ln * n] : 0.0;
        const unsigned long long stop = __ballot(ln < kA && !(fabs(dl) > tol));
        pr = stop ? __builtin_ctzll(stop) : kA;
    }
    int bits = 0;
    double bi;
    if (b.mode == 1) {
        xs[w][ln] = (ln < n) ? vec[ln] : 0.0;
        wave_apply_reflectors_reg<true, 1>(FA, n, b.tauA + j * b.sTauA, kA, n, xs[w]);       // b = F.Q' * grad
        bi = (ln < n) ? xs[w][ln] : 0.0;
        const double s = wave_allsum((ln >= pr && ln < n) ? bi * bi : 0.0);                  // ||b[prankA+1 : n]||
        if (ln == 0 && b.grad_res) b.grad_res[j] = (n > pr) ? sqrt(s) : 0.0;
    } else {
        bi = (ln < t) ? vec[ln] : 0.0;
        if (pr > b.state[j].rankA) bits |= 2;       // columns rank_solve .. pr-1 of J1 were overwritten by the factorisation of J2
    }
    double v = 0.0, u = 0.0;
    if (pr > 0) {
        const bool own = ln < pr;
        const double di = own ? FA[ln + (size_t)ln * n] : 1.0;
        if (__ballot(di == 0.0)) bits |= 1;
        const double ri = 1.0 / di;
        double yv = own ? bi / di : 0.0;
        double yu = 0.0;
        if (b.mode == 1) {
            // LowerTriangular(R'[1:pr,1:pr]) y = -cx[p]: row ln of R' is column ln of R
            const int pj = own ? (int)jp[ln] - 1 : -1;
            yu = ((unsigned)pj < (unsigned)t) ? -b.cx[j * b.scx + pj] / di : 0.0;
            for (int kk = 0; kk < pr; ++kk) {
                const double xk = wave_bcast(yu, kk);
                if (ln > kk && own) yu -= (FA[kk + (size_t)ln * n] * ri) * xk;
            }
            yu = own ? yu / di : 0.0;        // the row-scaled right-hand side of the back substitution below
        }
        // U(R[1:pr,1:pr]) [v u] = [b y]
        for (int kk = pr - 1; kk >= 0; --kk) {
            const double xv = wave_bcast(yv, kk);
            const double xu = wave_bcast(yu, kk);
            if (ln < kk) {
                const double r = FA[ln + (size_t)kk * n] * ri;
                yv -= r * xv;
                yu -= r * xu;
            }
        }
        v = own ? yv : 0.0;
        u = own ? yu : 0.0;
    }
    // lambda = (v + u)[invperm(p)], then the row-scaling back-transform; the slots past t are 0
    if (ln < t) {
        const int dst = (int)jp[ln] - 1;
        double l = v + u;
        if ((unsigned)dst < (unsigned)t) {
            if (b.diag_scale) l *= b.diag_scale[j * tmax + dst];
            lam[dst] = l;
        }
    } else if (ln < tmax) {
        lam[ln] = 0.0;
    }
    if (ln == 0) {
        const int code = lagrange_status_code(bits);
        if (b.status) b.status[j] = code;
        if (code) atomicOr(b.flag, 1);
    }
}

}  // namespace gn
