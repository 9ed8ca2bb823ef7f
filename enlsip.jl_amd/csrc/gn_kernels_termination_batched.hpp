// The termination test of a batch on the caller's device buffers (gn_termination_batched.inc; the routines: gn_termination.hpp):
// grad = J' rx, rx_sum and every other scalar check_termination_criteria (src/enlsip_functions.jl:2399-2517) and
// minmax_lagrangian_mult (:540-564) read, with whsum and progress of :2279-2280.  The decision itself is made on the host from the
// downloaded record.  The problem index is carried in gridDim.x.
//
// Two forms, chosen by the shape alone (n <= 64 && l <= 64: wave per problem).  They give the same bytes except rx_sum, which
// follows the form of the line-search set-up:
//   general   k_term_grad      one wave per (column, problem): gemv_t_column, the statement of k_gemv_t_batched, so dgrad is bitwise
//                              what enlsip_gn_gradient_batched_dev returns.  The one launch that moves real bytes.
//             k_term_rx_part   ordered_partial_sums of the line-search set-up on rx alone: nblk partials per problem.
//             k_term_short     one workgroup per problem.  Every short reduction belongs to ONE wave, which takes it in the
//                              documented order (lane s adds terms s, s + 64, ... ascending, then the butterfly): wave 0 the norms
//                              of p, x_prev - x and x; wave 1 the norm of the gradient just written and dot(d1, d1); wave 2 the sums
//                              over the active list, sigma_min / lambda_abs_max, the total of the rx partials and progress; wave 3
//                              the two counts over the inactive list.  Then At * cx_active: cx_active in LDS (broadcast reads), the
//                              256 lanes along the rows of At (column-major reads coalesce), 1024 rows at a time into LDS, whose
//                              squares wave 0 adds to its strided partials in ascending row order.  The index lists are read
//                              straight from the records, one entry per lane: an inactive entry once, an active entry twice (the
//                              penalty sum and whsum, by the same lane, the second read from L1/L2); an LDS copy would save that
//                              one repeated read of at most 4 KB per problem and cost a barrier, so none is made.
//   wave      k_term_wave      four problems per 256-thread workgroup, one launch, no LDS, no barrier.  J' rx column by column by
//                              gemv_t_column; rx_sum as k_ls_wave forms it; the short reductions by the same body as the general
//                              form's waves (every strided partial is one term); lane j owns row j of At.
// No floating-point atomics.  Outside the two statements shared with existing kernels (J' rx, rx.rx: fused multiply-adds there and
// here) products and additions are rounded on their own (fp contract off where they are formed).
#pragma once
#include "gn_batch_records.hpp"
#include "gn_device_utils.hpp"
#include "gn_kernels_lagrange_batched.hpp"
#include "gn_kernels_linesearch_batched.hpp"
#include "gn_termination.hpp"

namespace gn {

struct TerminationArgs {
    const TermMeta* meta;
    const int* act;             // batch x l
    const int* inact;           // batch x l
    enlsip_gn_term_sums* out;
    double* part;               // general form: nblk per problem
    int count, m, n, l, t_max, scaling;
    int nblk, col_blocks;       // general form: partial-sum workgroups per problem (<= 64, 0 when m == 0); ceil(n / 4)
    const double* J; long long ldj, strideJ;
    const double* rx;           // stride m
    const double* cx_all;       // stride l
    const double *x, *x_prev, *p, *d_gn;      // stride n
    const double *lambda, *cx_active, *diag_scale;      // stride t_max
    const double* At; long long ldat, strideAt;
    const double* w;            // stride l
    double* grad;               // stride n
};

constexpr int TERM_ROWS = 1024;         // rows of At * cx_active held in LDS at a time (a multiple of 64)

// one sum in the documented order: lane ln adds term(j) for j = ln, ln + 64, ... from +0.0, then the butterfly.  Every lane of the
// wave calls it and returns the sum.
template <class Term>
__device__ __forceinline__ double wave_ordered_sum(int count, int ln, Term term) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int j = ln; j < count; j += WAVE) s = s + term(j);
    return wave_allsum(s);
}

// dot(rx, rx) as k_ls_wave forms it
__device__ __forceinline__ double wave_rx_sum(const double* __restrict__ rx, int m, int ln) {
    double rr = 0.0;
    for (int i = ln; i < m; i += WAVE) {
        const double y = rx[i];
        rr += y * y;
    }
    return wave_allsum(rr);
}

enum { TERM_G_STEP = 1, TERM_G_GRAD = 2, TERM_G_ACTIVE = 4, TERM_G_INACTIVE = 8, TERM_G_ALL = 15 };

// The short reductions of problem k by ONE wave: the groups of `groups`.  rx_sum: the problem's dot(rx, rx), formed before.
__device__ __forceinline__ void term_wave_sums(const TerminationArgs& a, long long k, const TermMeta& mt, int ln, int groups,
                                               double rx_sum) {
#pragma clang fp contract(off)
    enlsip_gn_term_sums* o = a.out + k;
    const int n = a.n, l = a.l, t = mt.t;
    if (groups & TERM_G_STEP) {
        const double* p = a.p + k * n;
        const double* x = a.x + k * n;
        const double* xp = a.x_prev + k * n;
        const double pp = wave_ordered_sum(n, ln, [=](int j) { return p[j] * p[j]; });
        const double dd = wave_ordered_sum(n, ln, [=](int j) { const double d = xp[j] - x[j]; return d * d; });
        const double xx = wave_ordered_sum(n, ln, [=](int j) { return x[j] * x[j]; });
        if (ln == 0) { o->p_nrm = sqrt(pp); o->x_diff = sqrt(dd); o->x_nrm = sqrt(xx); }
    }
    if (groups & TERM_G_GRAD) {
        const double* g = a.grad + k * n;
        const double* d = a.d_gn + k * n;
        const double gg = wave_ordered_sum(n, ln, [=](int j) { return g[j] * g[j]; });
        const double d1 = wave_ordered_sum(mt.dimJ2, ln, [=](int j) { return d[j] * d[j]; });
        if (ln == 0) { o->grad_nrm = sqrt(gg); o->d1_sq = d1; }
    }
    if (groups & TERM_G_ACTIVE) {
        const int* act = a.act + k * l;
        const double* cxa = a.cx_active + k * a.t_max;
        const double* cxn = a.cx_all + k * l;
        const double* w = a.w + k * l;
        const double cc = wave_ordered_sum(t, ln, [=](int i) { return cxa[i] * cxa[i]; });
        const double ww = wave_ordered_sum(t, ln, [=](int i) {
            const int r = act[i];
            const double wi = r ? w[r - 1] : 0.0;
            return wi * wi;
        });
        const double wh = wave_ordered_sum(t, ln, [=](int i) {
            const int r = act[i];
            if (!r) return 0.0;
            const double c = cxn[r - 1];
            const double sq = c * c;
            return w[r - 1] * sq;
        });
        double mx = 0.0, mn = INFINITY;                                            // :550-551
        if (t > mt.q) {                                                           // :553
            const double* lam = a.lambda + k * a.t_max;
            const double* ds = a.diag_scale + k * a.t_max;
            bool nan = false;
            for (int i = ln; i < t; i += WAVE) {
                const double li = lam[i];
                const double ab = fabs(li);
                if (ab != ab) nan = true;
                else mx = fmax(mx, ab);                                           // :554
                if (i >= mt.q && term_sigma_candidate(li, term_rows(ds[i], a.scaling != 0)) && li < mn) mn = li;     // :558
            }
            mx = wave_allmax(mx);
            if (__ballot(nan)) mx = __builtin_nan("");
            mn = -wave_allmax(-mn);
        }
        if (ln == 0) {
            o->active_cx_nrm = sqrt(cc);
            o->active_penalty_sum = ww;
            o->whsum = wh;
            o->sigma_min = mn;
            o->lambda_abs_max = mx;
            o->rx_sum = rx_sum;
            o->progress = (2 * mt.psi0 - rx_sum) - wh;                            // :2280
        }
    }
    if (groups & TERM_G_INACTIVE) {
        const int* ina = a.inact + k * l;
        const double* cxn = a.cx_all + k * l;
        const int cnt = l - t;
        long long nonpos = 0, le0 = 0;
        for (int i0 = 0; i0 < cnt; i0 += WAVE) {
            const int i = i0 + ln;
            const int r = i < cnt ? ina[i] : 0;
            const double c = r ? cxn[r - 1] : 1.0;
            nonpos += __popcll(__ballot(r != 0 && !(c > 0.0)));
            le0 += __popcll(__ballot(r != 0 && c <= 0.0));
        }
        if (ln == 0) { o->n_inactive_nonpos = nonpos; o->n_inactive_le0 = le0; }
    }
}

// grid: count * col_blocks workgroups, one wave per column of J
__global__ __launch_bounds__(256) void k_term_grad(TerminationArgs a) {
    const long long k = blockIdx.x / a.col_blocks;
    const int c = (int)(blockIdx.x % a.col_blocks) * 4 + wave_id();
    if (c >= a.n || !a.meta[k].take) return;
    const int ln = lane_id();
    const double s = gemv_t_column(a.J + k * a.strideJ + (size_t)c * a.ldj, a.rx + k * a.m, a.m, ln);
    if (ln == 0) a.grad[k * a.n + c] = s;
}

// grid: count * nblk workgroups (m > 0)
__global__ __launch_bounds__(256) void k_term_rx_part(TerminationArgs a) {
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

// At * cx_active of the rows j0 .. j0 + TERM_ROWS - 1 into sv, the 256 lanes along the rows
__device__ __forceinline__ void term_at_rows(const double* __restrict__ At, long long ldat, int n, int t, int j0, const double* scx,
                                             double* sv) {
#pragma clang fp contract(off)
    for (int jj = threadIdx.x; jj < TERM_ROWS && j0 + jj < n; jj += 256) {
        const double* row = At + j0 + jj;
        double s = 0.0;
        for (int c = 0; c < t; ++c) s = s + row[(size_t)c * ldat] * scx[c];
        sv[jj] = s;
    }
}

// grid: count workgroups
__global__ __launch_bounds__(256) void k_term_short(TerminationArgs a) {
    __shared__ double scx[BATCH_MAX_T];
    __shared__ double sv[TERM_ROWS];
    const long long k = blockIdx.x;
    const TermMeta mt = a.meta[k];
    if (!mt.take) return;
    const int ln = lane_id(), w = wave_id(), n = a.n, t = mt.t;
    const double rx_sum = a.m > 0 ? ordered_partials_total(a.part + (size_t)k * a.nblk, a.nblk, 1, 0) : 0.0;
    term_wave_sums(a, k, mt, ln, 1 << w, rx_sum);
    for (int c = threadIdx.x; c < t; c += 256) scx[c] = a.cx_active[k * a.t_max + c];
    __syncthreads();
    double acc = 0.0;
    for (int j0 = 0; j0 < n; j0 += TERM_ROWS) {
        term_at_rows(a.At + k * a.strideAt, a.ldat, n, t, j0, scx, sv);
        __syncthreads();
        if (w == 0) {
#pragma clang fp contract(off)
            const int rows = n - j0 < TERM_ROWS ? n - j0 : TERM_ROWS;
            for (int jj = ln; jj < rows; jj += WAVE) {
                const double sq = sv[jj] * sv[jj];
                acc = acc + sq;
            }
        }
        __syncthreads();
    }
    if (w == 0) {
        const double s = wave_allsum(acc);
        if (ln == 0) a.out[k].Atcx_nrm = sqrt(s);
    }
}

// lane j's entry of At * cx_active (n <= 64, t <= 64) squared and summed over the wave
__device__ __forceinline__ double term_wave_atcx(const double* __restrict__ At, long long ldat, int n, int t, const double* cxa, int ln) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int c = 0; c < t; ++c) {
        const double v = ln < n ? At[ln + (size_t)c * ldat] : 0.0;
        s = s + v * cxa[c];
    }
    const double sq = s * s;
    return wave_allsum(sq);
}

__global__ __launch_bounds__(256) void k_term_wave(TerminationArgs a) {
    const int ln = lane_id();
    const long long k = (long long)blockIdx.x * 4 + wave_id();
    if (k >= a.count) return;
    const TermMeta mt = a.meta[k];
    if (!mt.take) return;
    const int n = a.n;
    const double* J = a.J + k * a.strideJ;
    const double* rx = a.rx + k * a.m;
    double mine = 0.0;
    for (int c = 0; c < n; ++c) {
        const double g = gemv_t_column(J + (size_t)c * a.ldj, rx, a.m, ln);
        if (ln == c) mine = g;
    }
    if (ln < n) a.grad[k * n + ln] = mine;      // lane j reads its own entry back below
    const double rx_sum = wave_rx_sum(rx, a.m, ln);
    term_wave_sums(a, k, mt, ln, TERM_G_ALL, rx_sum);
    const double s = term_wave_atcx(a.At + k * a.strideAt, a.ldat, n, mt.t, a.cx_active + k * a.t_max, ln);
    if (ln == 0) a.out[k].Atcx_nrm = sqrt(s);
}

}  // namespace gn
