// The line-search set-up of a batch on the caller's device buffers (gn_linesearch_batched.inc): Ap = A * p with the FULL constraint
// Jacobian (src/enlsip_functions.jl:2227), upper_bound_steplength on it (:2149-2178, gn_steplength_bound.hpp) and the three sums
// dot(Jp,Jp), dot(Jp,rx), dot(rx,rx) through which Jp enters penalty_weight_update (:1561-1584) and the predicted reduction (:2269).
// The problem index is carried in gridDim.x, so a batch is not bounded by the grid's y limit.
//
// Two forms, chosen by the shape alone (n <= 64 && l <= 64: wave per problem).  They must name the same row:
//   general   k_ls_product   one thread per row, lanes along rows (column-major reads coalesce), p in LDS (broadcast reads), block
//                            id = problem * row_blocks + row_block.  The sum over the columns is k_gemv_n_add's statement in its
//                            order, so Ap is bitwise what enlsip_gn_full_constraints_times returns for the problem.
//             k_ls_sums_part grid problem * nblk + b: workgroup b of a problem adds entries b*256 + tid + i*nblk*256 per thread, the
//                            wave butterfly, its four waves in order, and stores three partial sums.  No floating-point atomics.
//             k_ls_bound     one workgroup per problem.  Thread i takes list positions i, i + 256, ... in ascending order and keeps
//                            (alpha, position) under the strict < of :2169; the workgroup reduces the 256 pairs lexicographically,
//                            the smaller position winning on equal alpha.  The sequential loop names the FIRST position that attains
//                            the minimum of alpha_j over the rows passing steplength_candidate (a later equal alpha_j fails the
//                            strict <), and that is the lexicographic minimum of (alpha_j, position).  Its first wave then adds the
//                            problem's nblk <= 64 partial sums, lane b holding partial b, by the fixed-shape butterfly.
//   wave      k_ls_wave      four problems per 256-thread workgroup, no LDS, no barrier, one launch.  Lane j owns row j of A and
//                            sums its columns in ascending order, p broadcast from lane c's register.  Lane i then owns list position
//                            i: Ap of its row comes from the owning lane by a shuffle, the minimum of alpha over the passing lanes by
//                            a wave minimum and the first position that attains it by a ballot.  The sums: a lane-strided loop over
//                            m and the butterfly.
// A sum depends on m and the operands only, never on the slot, the batch size or the arrival order.
#pragma once
#include "gn_batch_records.hpp"
#include "gn_device_utils.hpp"
#include "gn_steplength_bound.hpp"

namespace gn {

struct LinesearchArgs {
    const LsMeta* meta;
    const int* list;            // stride l: 1-based rows, 0 padding
    LsOut* out;
    int count, n, l, m;         // m == 0: no sums
    int row_blocks, nblk;       // general form: ceil(l / 256); partial-sum workgroups per problem (<= 64)
    const double* p;            // stride n
    const double* A; long long lda, strideA;
    const double* cx;           // stride l
    const double* Jp;           // stride m
    const double* rx;           // stride m
    double* Ap;                 // stride l
    double* part;               // general form: 3 * nblk per problem
};

constexpr int LS_MAX_N = 1024;          // p in LDS (general form)

__global__ __launch_bounds__(256) void k_ls_product(LinesearchArgs a) {
    __shared__ double sp[LS_MAX_N];
    const long long k = blockIdx.x / a.row_blocks;
    const int r = (int)(blockIdx.x % a.row_blocks) * 256 + threadIdx.x;
    const int n = a.n;
    const double* pk = a.p + k * n;
    for (int c = threadIdx.x; c < n; c += 256) sp[c] = pk[c];
    __syncthreads();
    if (r >= a.l) return;
    const double* Ak = a.A + k * a.strideA;
    double s = 0.0;
#pragma unroll 8
    for (int c = 0; c < n; ++c) s += Ak[r + (size_t)c * a.lda] * sp[c];
    a.Ap[k * a.l + r] = s;
}

// The ordered partial sums, shared with the merit function (gn_kernels_penalty_batched.hpp).  Workgroup b of a problem's nblk: every
// thread walks entries b*256 + tid + i*nblk*256 and `add(i, acc)` adds entry i's products to the thread's Q sums; then the wave
// butterfly, the four waves in order, and Q partial sums at out[0:Q).  ws: Q x 4 doubles of LDS.  All 256 threads call it.
template <int Q, class Add>
__device__ __forceinline__ void ordered_partial_sums(int b, int nblk, long long m, double (*ws)[4], double* out, Add add) {
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
    for (long long i = (long long)b * 256 + threadIdx.x; i < m; i += (long long)nblk * 256) add(i, acc);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        acc[q] = wave_allsum(acc[q]);
        if (lane_id() == 0) ws[q][wave_id()] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < Q) {
        const double* w = ws[threadIdx.x];
        out[threadIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
    }
}

// ... and their sum: lane b of one wave holds partial b of sum q (nblk <= 64, stride Q), added by the fixed-shape butterfly
__device__ __forceinline__ double ordered_partials_total(const double* pt, int nblk, int Q, int q) {
    const int ln = lane_id();
    return wave_allsum(ln < nblk ? pt[ln * Q + q] : 0.0);
}

__global__ __launch_bounds__(256) void k_ls_sums_part(LinesearchArgs a) {
    __shared__ double ws[3][4];
    const long long k = blockIdx.x / a.nblk;
    const int b = (int)(blockIdx.x % a.nblk);
    const double* jp = a.Jp + k * a.m;
    const double* rx = a.rx + k * a.m;
    ordered_partial_sums<3>(b, a.nblk, a.m, ws, a.part + ((size_t)k * a.nblk + b) * 3, [=](long long i, double (&s)[3]) {
        const double x = jp[i], y = rx[i];
        s[0] += x * x;
        s[1] += x * y;
        s[2] += y * y;
    });
}

__global__ __launch_bounds__(256) void k_ls_bound(LinesearchArgs a) {
    __shared__ double sa[256];
    __shared__ int spos[256];
    const long long k = blockIdx.x;
    const int tid = threadIdx.x;
    const LsMeta mt = a.meta[k];
    const int* list = a.list + k * a.l;
    const double* cx = a.cx + k * a.l;
    const double* Ap = a.Ap + k * a.l;
    double best = INFINITY;
    int pos = 0x7fffffff;
    for (int i = tid; i < mt.n_inactive; i += 256) {
        double al;
        if (steplength_candidate(list[i], mt.index_del, cx, Ap, &al) && al < best) {
            best = al;
            pos = i;
        }
    }
    sa[tid] = best;
    spos[tid] = pos;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const double oa = sa[tid + s];
            const int op = spos[tid + s];
            if (oa < sa[tid] || (oa == sa[tid] && op < spos[tid])) {
                sa[tid] = oa;
                spos[tid] = op;
            }
        }
        __syncthreads();
    }
    LsOut* o = a.out + k;
    if (tid == 0) {
        const bool any = spos[0] != 0x7fffffff;
        o->alpha_upp = (any && sa[0] < GN_STEPLENGTH_CAP) ? sa[0] : GN_STEPLENGTH_CAP;
        o->index_alpha_upp = any ? list[spos[0]] : 0;
    }
    if (a.m > 0 && tid < WAVE) {
        const double* pt = a.part + (size_t)k * a.nblk * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double t = ordered_partials_total(pt, a.nblk, 3, q);
            if (tid == 0) o->sums[q] = t;
        }
    }
}

__global__ __launch_bounds__(256) void k_ls_wave(LinesearchArgs a) {
    const int ln = lane_id();
    const long long k = (long long)blockIdx.x * 4 + wave_id();
    if (k >= a.count) return;
    const int n = a.n, l = a.l;
    LsOut* o = a.out + k;
    double alpha = GN_STEPLENGTH_CAP;
    int index = 0;
    if (l > 0) {
        const LsMeta mt = a.meta[k];
        const bool own = ln < l;
        const double pl = ln < n ? a.p[k * n + ln] : 0.0;
        const double* row = a.A + k * a.strideA + (own ? ln : 0);
        double ap = 0.0;
        for (int c = 0; c < n; ++c) {
            const double pc = wave_bcast(pl, c);
            const double v = own ? row[(size_t)c * a.lda] : 0.0;
            ap += v * pc;
        }
        if (own) a.Ap[k * l + ln] = ap;
        const int j = ln < mt.n_inactive ? a.list[k * l + ln] : 0;
        const bool look = j != 0 && j != mt.index_del;                           // :2163, :2166
        const double g = __shfl(ap, look ? j - 1 : 0);
        const double c = look ? a.cx[k * l + j - 1] : 0.0;
        double al = INFINITY;
        const bool pass = steplength_row_test(c, g, &al) && look;
        if (__ballot(pass)) {
            const double e = -wave_allmax(pass ? -al : -INFINITY);
            const int first = (int)__builtin_ctzll(__ballot(pass && al == e));
            index = __builtin_amdgcn_readlane(j, first);
            alpha = e < GN_STEPLENGTH_CAP ? e : GN_STEPLENGTH_CAP;
        }
    }
    if (ln == 0) {
        o->alpha_upp = alpha;
        o->index_alpha_upp = index;
    }
    if (a.m > 0) {
        const double* jp = a.Jp + k * a.m;
        const double* rx = a.rx + k * a.m;
        double jj = 0.0, jr = 0.0, rr = 0.0;
        for (int i = ln; i < a.m; i += WAVE) {
            const double x = jp[i], y = rx[i];
            jj += x * x;
            jr += x * y;
            rr += y * y;
        }
        jj = wave_allsum(jj);
        jr = wave_allsum(jr);
        rr = wave_allsum(rr);
        if (ln == 0) { o->sums[0] = jj; o->sums[1] = jr; o->sums[2] = rr; }
    }
}

}  // namespace gn
