// The working-set additions of a batch and the rebuild of its active constraints on the caller's device buffers
// (gn_addition_batched.inc; the routines: gn_violated_constraints.hpp): evaluate_violated_constraints
// (src/enlsip_functions.jl:608-650) on the full cx of every walked problem, then active_C.cx / active_C.A of :2854-2855 with
// evaluate_scaling! (src/structures.jl:160-178) written as the padded slot of the ragged solve: columns 0..t-1 of the n x t_max
// column-major A' block gathered (and scaled), columns t..t_max-1 zero in rows 0..n-1, cx 0.0 and diag_scale 1.0 behind t.
// Nothing between rows n and ldat, behind ldat * t_max, of a problem that is not taken, or of any input is written.
//
// Two forms, chosen by the shape alone (n <= 64 && l <= 64: wave per problem).  They give the same lists and the same bytes:
//   general   k_add_walk: one workgroup per problem, one lane runs addition_walk on LDS copies of the lists and of cx and leaves
//             t and the lists in the device records.  k_add_gather: one workgroup per (64-column tile of A', problem) reads t and
//             the list from those records.  Lane c of every wave owns column c of the tile: a load of 64 lanes reads A at rows
//             active[c0 .. c0+63] of ONE column j of A (l x n column-major), contiguous wherever the sorted list is; the four waves
//             take j = w, w+4, ...  The 64 x 64 chunk goes through a padded LDS tile and is written with the lanes along the rows
//             of A', 512 contiguous bytes per column.  The strided partial s = j mod 64 of a column's sum of squares belongs to
//             exactly one thread (lane c, wave s mod 4), which adds it up in registers in ascending j; the 64 partials of a column
//             are then added by one wave all-reduce, the butterfly gather_butterfly restates.  With scaling the columns are read
//             twice (norms, then the scaled copy: the second read comes from L2).
//   wave      four problems per 256-thread workgroup, one launch, no LDS.  Lane i holds active[i], inactive[i] and cx[i + 1]; i
//             and t are wave-uniform.  The worst active inequality is a wave maximum over the candidates and the LOWEST lane that
//             holds it (the first maximum of the strict > loop; a NaN or -Inf is no candidate, as in the loop); an insertion is a
//             ballot of "entry <= v" whose highest lane + 1 is the position of the insertion from the back, and a one-lane shift.
//             The rebuild walks the columns with the lanes along the rows of A': n <= 64 makes every strided partial one square,
//             so the all-reduce of the squares is the documented order.
// No floating-point atomics.  The squares are rounded on their own (fp contract off where they are formed).
#pragma once
#include "gn_batch_records.hpp"
#include "gn_device_utils.hpp"
#include "gn_violated_constraints.hpp"

namespace gn {

struct AdditionArgs {
    const AdditionMeta* meta;
    int* act;                   // batch x l, in and out
    int* inact;                 // batch x l, in and out
    AdditionOut* out;
    int count, n, l, t_max, scaling, tiles;
    const double* A; long long lda, strideA;
    const double* cx_all;       // stride l
    double* At; long long ldat, strideAt;
    double* cx;                 // stride t_max
    double* diag_scale;         // stride t_max
};

__global__ __launch_bounds__(256) void k_add_wave(AdditionArgs a) {
#pragma clang fp contract(off)
    const int ln = lane_id();
    const long long k = (long long)blockIdx.x * 4 + wave_id();
    if (k >= a.count) return;
    const AdditionMeta mt = a.meta[k];
    if (!mt.take) return;
    const int l = a.l, n = a.n, q = mt.q;
    int* gact = a.act + k * l;
    int* gina = a.inact + k * l;
    int act = ln < l ? gact[ln] : 0;
    int ina = ln < l ? gina[ln] : 0;
    const double cxl = ln < l ? a.cx_all[k * l + ln] : 0.0;
    int t = mt.t, added = 0, status = 0;
    if (mt.take == 1) {
        const int bnd = l < n ? l : n;
        const int cap = (l + 1) * (l + 1);
        int passes = 0, i = 1;
        while (i <= l - t) {
            if (++passes > cap) { status = 2; break; }
            const int kk = __shfl(ina, i - 1);
            const double ck = __shfl(cxl, kk ? kk - 1 : 0);
            if (kk == 0 || !addition_violated(ck, kk == mt.index_alpha_upp)) { ++i; continue; }
            if (t >= bnd) {
                const double mine = __shfl(cxl, act ? act - 1 : 0);
                const bool cand = ln >= q && ln < t && act != 0 && mine > -INFINITY;
                if (!__ballot(cand)) { ++i; continue; }
                const double mx = wave_allmax(cand ? mine : -INFINITY);
                const int wl = (int)__builtin_ctzll(__ballot(cand && mine == mx));
                if (!(mx > ck)) { ++i; continue; }
                const int v = __shfl(act, wl);
                const int cnt = l - t;
                const unsigned long long le = __ballot(ln < cnt && ina <= v);
                const int p = le ? 64 - (int)__builtin_clzll(le) : 0;
                if (p == i - 1) { status = 1; break; }
                const int up = __shfl_up(ina, 1);
                if (ln > p && ln <= cnt) ina = up;
                else if (ln == p) ina = v;
                const int dn = __shfl_down(act, 1);
                if (ln >= wl && ln < t - 1) act = dn;
                else if (ln == t - 1) act = 0;
                --t;
            }
            const int v = __shfl(ina, i - 1);
            const unsigned long long le = __ballot(ln < t && act <= v);
            const int p = le ? 64 - (int)__builtin_clzll(le) : 0;
            const int up = __shfl_up(act, 1);
            if (ln > p && ln <= t) act = up;
            else if (ln == p) act = v;
            const int cnt = l - t;
            const int dn = __shfl_down(ina, 1);
            if (ln >= i - 1 && ln < cnt - 1) ina = dn;
            else if (ln == cnt - 1) ina = 0;
            ++t;
            added = 1;
        }
        if (ln < l) { gact[ln] = act; gina[ln] = ina; }
    }
    if (ln == 0) a.out[k] = {t, added, status, 0};
    // the rebuild: lanes along the rows of A'
    const double* A = a.A + k * a.strideA;
    double* At = a.At + k * a.strideAt;
    double my_ds = 1.0, my_cx = 0.0;
    for (int c = 0; c < a.t_max; ++c) {
        const int r = c < t ? __shfl(act, c) : 0;
        const double v = (r && ln < n) ? A[(size_t)(r - 1) + (size_t)ln * a.lda] : 0.0;
        const double sq = v * v;
        const double sum = wave_allsum(sq);
        double dsv;
        const double div = gather_divisor(sum, a.scaling != 0, &dsv);
        const double cv = __shfl(cxl, r ? r - 1 : 0);
        if (ln < n) At[(size_t)c * a.ldat + ln] = c < t ? (a.scaling ? v / div : v) : 0.0;
        if (ln == c && c < t) {
            my_ds = dsv;
            my_cx = r ? (a.scaling ? cv / div : cv) : 0.0;
        }
    }
    if (ln < a.t_max) {
        a.diag_scale[k * a.t_max + ln] = my_ds;
        a.cx[k * a.t_max + ln] = my_cx;
    }
}

__global__ __launch_bounds__(256) void k_add_walk(AdditionArgs a) {
    __shared__ int sa[BATCH_MAX_T], si[BATCH_MAX_T];
    __shared__ double sc[BATCH_MAX_T];
    const long long k = blockIdx.x;
    const int tid = threadIdx.x;
    const AdditionMeta mt = a.meta[k];
    if (!mt.take) return;
    if (mt.take != 1) {      // rebuild only: the lists stand as given
        if (tid == 0) a.out[k] = {mt.t, 0, 0, 0};
        return;
    }
    const int l = a.l;
    int* gact = a.act + k * l;
    int* gina = a.inact + k * l;
    for (int i = tid; i < l; i += 256) { sa[i] = gact[i]; si[i] = gina[i]; sc[i] = a.cx_all[k * l + i]; }
    __syncthreads();
    if (tid == 0) {
        long long t = mt.t;
        int added = 0;
        const int status = addition_walk<int>(l, a.n, mt.q, &t, sa, si, sc, mt.index_alpha_upp, &added);
        a.out[k] = {(int)t, added, status, 0};
    }
    __syncthreads();
    for (int i = tid; i < l; i += 256) { gact[i] = sa[i]; gina[i] = si[i]; }
}

// grid: count * tiles workgroups, tile = 64 columns of A'
__global__ __launch_bounds__(256) void k_add_gather(AdditionArgs a) {
#pragma clang fp contract(off)
    __shared__ double T[64][65];      // the transposed chunk, then the partials [column][s]
    __shared__ double ssum[64];
    const long long k = blockIdx.x / a.tiles;
    const int c0 = (int)(blockIdx.x % a.tiles) * 64;
    const AdditionMeta mt = a.meta[k];
    if (!mt.take) return;
    const int ln = lane_id(), w = wave_id(), n = a.n;
    const int t = a.out[k].t;
    const int ncol = a.t_max - c0 < 64 ? a.t_max - c0 : 64;      // columns of this tile inside the slot
    const int c = c0 + ln;
    const bool live = c < t;
    const int r = live ? a.act[k * a.l + c] : 0;
    const bool scaling = a.scaling != 0;
    const double* src = a.A + k * a.strideA + (r ? r - 1 : 0);
    double* At = a.At + k * a.strideAt;
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    double div = 1.0;
    for (int pass = scaling ? 0 : 1; pass < 2; ++pass) {
        const bool accum = scaling ? pass == 0 : true;
        const bool write = pass == 1;
        for (int j0 = 0; j0 < n; j0 += 64) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int jl = w + 4 * i, j = j0 + jl;
                const double v = (r && j < n) ? src[(size_t)j * a.lda] : 0.0;
                if (accum) {
                    const double sq = v * v;
                    acc[i] = acc[i] + sq;
                }
                if (write) T[jl][ln] = scaling ? v / div : v;
            }
            if (write) {
                __syncthreads();
                const int j = j0 + ln;
                if (j < n)
                    for (int cc = w; cc < ncol; cc += 4) At[(size_t)(c0 + cc) * a.ldat + j] = T[ln][cc];
                __syncthreads();
            }
        }
        if (accum) {
#pragma unroll
            for (int i = 0; i < 16; ++i) T[ln][w + 4 * i] = acc[i];
            __syncthreads();
            for (int cc = w * 16; cc < w * 16 + 16; ++cc) {
                const double sum = wave_allsum(T[cc][ln]);
                if (ln == 0) ssum[cc] = sum;
            }
            __syncthreads();
            double dsv;
            div = gather_divisor(ssum[ln], scaling, &dsv);
            if (w == 0 && ln < ncol) {
                const double cv = r ? a.cx_all[k * a.l + r - 1] : 0.0;
                a.diag_scale[k * a.t_max + c] = live ? dsv : 1.0;
                a.cx[k * a.t_max + c] = live ? (scaling ? cv / div : cv) : 0.0;
            }
        }
    }
}

}  // namespace gn
