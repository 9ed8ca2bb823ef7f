// Magnitudes beyond the range of plain sums of squares (entries outside 2^+-400, the band GN_RESCALE_BAND): LAPACK's behaviour on
// the same inputs.  The reference's qr(., ColumnNorm()) (src/enlsip_functions.jl:223, :700, :769) runs dgeqp3, whose column norms (dnrm2)
// and reflectors (dlarfg with its safmin loop) scale internally and never overflow or underflow; the kernels of this library
// square plainly.  Instead of a scaled norm at every one of their norm sites, the rare case is DETECTED on the result and the
// problem is solved again on a copy of its inputs scaled by a power of two — exact, so every factor comes out as
// 2^shift x (what LAPACK computes on the unscaled data), the reflectors and pivots as they are — and the resident factors and the
// outputs are scaled back (enlsip_gn.hip: "rescale").  The absolute first test of pseudo_rank (:17-31) is taken against
// 2^shift eps_rank (pseudo_rank_abs_threshold).  Costs one tiny launch per solve on the normal path (k_extreme_flags).
#pragma once
#include "gn_device_utils.hpp"

namespace gn {

constexpr int GN_FLAG_NONFINITE = 1 << 29;     // ProbState::status bits, host-internal: cleared before the caller sees status
                                               // (NONFINITE: |R[0]| above 2^440, Inf or NaN; TINY: below 2^-440)
constexpr int GN_FLAG_TINY = 1 << 30;
constexpr int GN_RESCALE_BAND = 400;           // inputs with 2^-400 <= max |entry| <= 2^400 are never rescaled

// first diagonal entries of F_A.R and F_J2.R: the largest column norm of each factorisation (pivoting puts it first).  Not
// finite: a sum of squares overflowed (or the inputs held NaN / Inf).  Above 2^440 (the same threshold for both factors): the
// largest column norm squared may still be finite, but other plain sums of squares need not be — the column norms of
// L11 = R_A', which are the ROW norms of R_A, reach sqrt(t) |R_A[0]|; ||rx||^2 may exceed every column norm of J.  Below 2^-440
// (zero included): the squares of the largest column sit at the bottom of the exponent range (or J / A is zero).  All three only
// nominate the problem: the host looks at the magnitudes of its inputs before anything is redone, and no input with
// |R[0]| beyond 2^+-440 that is worth redoing lies inside the band 2^+-400.
// RAGGED: F_A of problem k has min(kA, tk[k]) reflectors — a problem without constraints has none to look at
template <bool RAGGED>
__device__ __forceinline__ void extreme_flags_body(ProbState* state, const double* Rt, long long sRt, const double* FA, long long sFA,
                                                   int kA, int n2cap, int batch, const int* tk, const int* plist) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= batch) return;
    const int k = listed_prob(plist, idx, 0);
    const ProbState st = state[k];
    if (n2cap > 0 && st.n2 > n2cap) return;            // redone by the caller (second attempt): nothing of it is final yet
    const double tiny = 0x1p-440, huge = 0x1p440;
    int f = 0;
    if (RAGGED ? (kA > 0 && tk[k] > 0) : kA > 0) {
        const double a = fabs(FA[k * sFA]);
        if (!(a <= huge)) f |= GN_FLAG_NONFINITE;       // NaN and Inf included
        else if (a < tiny) f |= GN_FLAG_TINY;
    }
    if (Rt && st.kp > 0) {
        const double r = fabs(Rt[k * sRt]);
        if (!(r <= huge)) f |= GN_FLAG_NONFINITE;
        else if (r < tiny) f |= GN_FLAG_TINY;
    }
    if (f) state[k].status = st.status | f;
}
__global__ __launch_bounds__(256) void k_extreme_flags(ProbState* state, const double* Rt, long long sRt, const double* FA, long long sFA,
                                                       int kA, int n2cap, int batch, const int* plist) {
    extreme_flags_body<false>(state, Rt, sRt, FA, sFA, kA, n2cap, batch, nullptr, plist);
}
__global__ __launch_bounds__(256) void k_extreme_flags_ragged(ProbState* state, const double* Rt, long long sRt, const double* FA,
                                                              long long sFA, int kA, int n2cap, int batch, const int* tk, const int* plist) {
    extreme_flags_body<true>(state, Rt, sRt, FA, sFA, kA, n2cap, batch, tk, plist);
}

// The same nomination for the local stage of a row shard (gn_tsqr.inc).  Its R is unpivoted, so no entry of it is "the largest
// column norm": the maximum of |x| (bit patterns, as k_amax_bits takes it) runs over the whole n2 x n2 upper triangle of R in W
// (rows < kp) and over the whole carried column d (all m rows: its tail can be huge while z is not).  ||R[:, j]|| <= sqrt(n) amax(R)
// keeps every plain sum of squares of the stage in range when nothing is flagged.  F_A is replicated and pivoted: its first
// diagonal entry is looked at as k_extreme_flags does.  acc: [0] the running maximum, [1] workgroups done; the last workgroup
// decides and leaves both words zero for the next launch.
__global__ __launch_bounds__(256) void k_tsqr_flags(ProbState* state, const double* W, int ldw, int n, int m, const double* FA, int kA,
                                                    int n2cap, unsigned long long* acc) {
    const ProbState st = *state;
    const int rankA = st.rankA, n2 = st.n2, kp = st.kp;
    // wider than launched: redone by the caller (second attempt), nothing of it is final yet
    const bool skip = n2 > n2cap || rankA < 0 || n2 < 0 || rankA + n2 > n || kp < 0 || kp > m || kp > n2;
    unsigned long long mx = 0ull;
    if (!skip) {
        for (int c = blockIdx.x; c < n2; c += gridDim.x) {
            const double* col = W + (size_t)(rankA + c) * ldw;
            const int rows = c + 1 < kp ? c + 1 : kp;
            for (int i = threadIdx.x; i < rows; i += 256) {
                const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(col[i]));
                mx = b > mx ? b : mx;
            }
        }
        const double* d = W + (size_t)n * ldw;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += (long long)gridDim.x * 256) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(d[i]));
            mx = b > mx ? b : mx;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(acc, mx);
    __syncthreads();
    if (threadIdx.x != 0) return;
    __threadfence();
    if (atomicAdd(acc + 1, 1ull) != (unsigned long long)gridDim.x - 1) return;
    __threadfence();
    const unsigned long long bits = atomicExch(acc, 0ull);
    atomicExch(acc + 1, 0ull);
    if (skip) return;
    const double tiny = 0x1p-440, huge = 0x1p440;
    int f = 0;
    if (kA > 0) {
        const double a = fabs(FA[0]);
        if (!(a <= huge)) f |= GN_FLAG_NONFINITE;
        else if (a < tiny) f |= GN_FLAG_TINY;
    }
    const double r = __longlong_as_double((long long)bits);
    if (!(r <= huge)) f |= GN_FLAG_NONFINITE;             // NaN and Inf included (a NaN outranks every number as a bit pattern)
    else if (r < tiny && kp > 0) f |= GN_FLAG_TINY;        // zero included; without a row of R there is nothing to redo
    if (f) state->status = st.status | f;
}

__global__ __launch_bounds__(256) void k_clear_status_bits(ProbState* state, int bits, int batch, const int* plist) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < batch) state[listed_prob(plist, idx, 0)].status &= ~bits;
}

// dst[plist[i]] = src[i]: the info records of the listed problems of a changed-problems solve into the caller's device array
__global__ __launch_bounds__(256) void k_scatter_info(enlsip_gn_info* dst, const enlsip_gn_info* src, const int* plist, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) dst[plist[i]] = src[i];
}

// bits of max |x| over a rows x cols matrix (non-negative doubles order like their bit patterns; a NaN outranks everything, so
// the host sees it); one workgroup per column
__global__ __launch_bounds__(256) void k_amax_bits(const double* A, long long ld, int rows, int cols, unsigned long long* out) {
    const int c = blockIdx.x;
    if (c >= cols) return;
    const double* col = A + (size_t)c * ld;
    unsigned long long mx = 0ull;
    for (int r = threadIdx.x; r < rows; r += 256) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(col[r]));
        mx = b > mx ? b : mx;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(out, mx);
}

// dst = src * 2^shift (exact unless an entry leaves the exponent range: such entries are below 2^-1000 of the largest one)
__global__ __launch_bounds__(256) void k_scale_copy(double* dst, long long ldd, const double* src, long long lds, int rows, int cols, int shift) {
    const int c = blockIdx.y;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < rows; r += gridDim.x * 256) dst[r + (size_t)c * ldd] = __builtin_ldexp(src[r + (size_t)c * lds], shift);
}

// in place: X *= 2^shift on a rows x cols region; upper = 1: only the entries on and above the diagonal (the R part of compact
// LAPACK factors: the reflector vectors below it do not depend on the scale of the data)
__global__ __launch_bounds__(256) void k_scale_region(double* X, long long ld, int rows, int cols, int shift, int upper) {
    const int c = blockIdx.y;
    if (c >= cols) return;
    const int rmax = upper ? (c + 1 < rows ? c + 1 : rows) : rows;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < rmax; r += gridDim.x * 256) X[r + (size_t)c * ld] = __builtin_ldexp(X[r + (size_t)c * ld], shift);
}

}  // namespace gn
