// The finite-difference Hessian sums of the Newton branch for a batch on the caller's device buffers (gn_hessian_batched.inc; the
// routines: gn_hessian_sums.hpp): the stencil points of hessian_res! / hessian_cons! (src/enlsip_functions.jl:259-265) and the two
// contractions with their divisions (:268-272, :317-322), written straight into Gamma = r_mat - c_mat (:393) where the batched
// Newton direction reads it.  The evaluations between the two kernels are the caller's.  The problem index is carried in
// gridDim.x, the pair range in gridDim.y (strided where the range has more blocks than a grid dimension admits).
//
//   k_hessian_points   one thread per entry of dX (count, npairs, 4, n): consecutive threads write consecutive addresses, so a
//                      row of n entries and the rows behind it go out coalesced.  A thread decodes its pair from the pair index
//                      (hess_decode: integer arithmetic around a first guess) and forms its entry by hess_point_entry.
//   k_hessian_sums     ONE wave owns one (problem, pair), four pairs per 256-thread workgroup.  The wave streams the four
//                      residual rows and rx once, 8 bytes per lane and load, four strides of 64 per iteration (20 loads of a
//                      lane in flight before the first addition: at m = 256 that is the whole row), then the four constraint
//                      rows through the active list.  Lane s adds its terms s, s + 64, ... in ascending order from +0.0 whatever
//                      the unrolling, then the butterfly (wave_allsum): the bytes of hess_sums.  Lane 0 writes the two entries
//                      of Gamma.  No LDS, no barrier, no floating-point atomics.
// Products, differences and sums are rounded on their own (fp contract off where they are formed).
#pragma once
#include "gn_batch_records.hpp"
#include "gn_device_utils.hpp"
#include "gn_hessian_sums.hpp"

namespace gn {

constexpr int HESS_PAIRS_PER_WG = 4;          // waves of a workgroup, one pair each
constexpr int HESS_UNROLL = 4;                // strides of 64 whose loads are issued together.  Not result-changing.
constexpr unsigned HESS_MAX_GRID_Y = 65535;

struct HessianPointsArgs {
    int n;
    long long pair0, npairs;
    double eps1;
    const double* x;            // count x n
    double* X;                  // count x npairs x 4 x n
};

struct HessianSumsArgs {
    const HessMeta* meta;
    const int* act;             // count x l
    int m, n, l, t_max;
    long long pair0, npairs;
    double eps1;
    const double* x;            // stride n
    const double* F;            // stride npairs * 4 * m
    const double* rx;           // stride m
    const double* G;            // stride npairs * 4 * l
    const double* lambda;       // stride t_max
    double* Gamma;              // slot * strideG
    long long ldg, strideG;
};

// grid: (count, blocks over npairs * 4 * n entries)
__global__ __launch_bounds__(256) void k_hessian_points(HessianPointsArgs a) {
    const long long k = blockIdx.x;
    const long long total = a.npairs * 4 * a.n;
    const double* x = a.x + k * a.n;
    double* X = a.X + k * total;
    for (long long e = (long long)blockIdx.y * 256 + threadIdx.x; e < total; e += (long long)gridDim.y * 256) {
        const long long row = e / a.n;
        const long long i = e - row * a.n;
        long long kk, jj;
        hess_decode(a.pair0 + (row >> 2), &kk, &jj);
        X[e] = hess_point_entry(x, i, kk, jj, (int)(row & 3), a.eps1);
    }
}

// pair q of the range, problem k, by ONE wave
__device__ __forceinline__ void hess_wave_pair(const HessianSumsArgs& a, long long k, const HessMeta& mt, long long q, int ln) {
#pragma clang fp contract(off)
    long long kk, jj;
    hess_decode(a.pair0 + q, &kk, &jj);
    const double* x = a.x + k * a.n;
    const double ek = hess_eps(x[kk], a.eps1), ej = hess_eps(x[jj], a.eps1);
    const long long m = a.m;
    const double* f1 = a.F + (k * a.npairs + q) * 4 * m;
    const double *f2 = f1 + m, *f3 = f2 + m, *f4 = f3 + m;
    const double* rx = a.rx + k * m;
    double s = 0.0;
    long long i = ln;
    for (; i + (HESS_UNROLL - 1) * WAVE < m; i += HESS_UNROLL * WAVE) {
        double v1[HESS_UNROLL], v2[HESS_UNROLL], v3[HESS_UNROLL], v4[HESS_UNROLL], w[HESS_UNROLL];
#pragma unroll
        for (int u = 0; u < HESS_UNROLL; ++u) {
            const long long c = i + u * WAVE;
            v1[u] = f1[c]; v2[u] = f2[c]; v3[u] = f3[c]; v4[u] = f4[c]; w[u] = rx[c];
        }
#pragma unroll
        for (int u = 0; u < HESS_UNROLL; ++u) s = s + hess_term(v1[u], v2[u], v3[u], v4[u], w[u]);
    }
    for (; i < m; i += WAVE) s = s + hess_term(f1[i], f2[i], f3[i], f4[i], rx[i]);
    const double r = hess_div_res(wave_allsum(s), ej, ek);
    double c = 0.0;
    if (mt.t > 0) {
        const long long l = a.l;
        const double* g1 = a.G + (k * a.npairs + q) * 4 * l;
        const double *g2 = g1 + l, *g3 = g2 + l, *g4 = g3 + l;
        const int* act = a.act + k * l;
        const double* lam = a.lambda + k * a.t_max;
        double sc = 0.0;
        for (int j = ln; j < mt.t; j += WAVE) {
            const int row = act[j];
            const double term = row ? hess_term(g1[row - 1], g2[row - 1], g3[row - 1], g4[row - 1], lam[j]) : 0.0;
            sc = sc + term;
        }
        c = hess_div_cons(wave_allsum(sc), ej, ek);
    }
    if (ln == 0) {
        double* Gam = a.Gamma + (long long)mt.slot * a.strideG;
        const double v = r - c;
        Gam[kk + jj * a.ldg] = v;
        Gam[jj + kk * a.ldg] = v;
    }
}

// grid: (count, blocks of four pairs)
__global__ __launch_bounds__(256) void k_hessian_sums(HessianSumsArgs a) {
    const long long k = blockIdx.x;
    const HessMeta mt = a.meta[k];
    if (mt.slot < 0) return;
    const int ln = lane_id();
    for (long long q = (long long)blockIdx.y * HESS_PAIRS_PER_WG + wave_id(); q < a.npairs; q += (long long)gridDim.y * HESS_PAIRS_PER_WG)
        hess_wave_pair(a, k, mt, q, ln);
}

}  // namespace gn
