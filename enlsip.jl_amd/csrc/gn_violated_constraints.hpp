// The working-set additions after a step and the rebuild of the active constraints, one body for host and device:
//   addition_walk     evaluate_violated_constraints (src/enlsip_functions.jl:608-650) with add_constraint! / remove_constraint!
//                     (src/structures.jl:234-267)
//   gather_active     active_C.cx = cx[active], active_C.A = A[active, :] (:2854-2855) followed by evaluate_scaling!
//                     (src/structures.jl:160-178), written as the n x t column-major A' block of the ragged solve
//
// The walk, line for line against the reference:
//   - eps = sqrt(eps(Float64)) = 2^-26, delta = 0.1, bnd = min(l, n) (:615-617);
//   - inactive[i] = k is violated when cx[k] < eps || (k == index_alpha_upp && cx[k] < delta) (:623): a NaN is never violated.
//     An entry 0 (padding inside the used part; the reference would fail on it) is never violated either and never a candidate
//     of the search below, so nothing outside cx is read;
//   - at capacity (t >= bnd) the worst active inequality is the FIRST maximum of cx[active[j]] over the positions q+1..t, by a
//     strict > against -Inf (:626-634): a NaN or -Inf never wins, and with no winner nothing is swapped;
//   - the swap happens only when worst_val > cx[k] (:635), otherwise the walk moves on;
//   - remove_constraint! appends the removed constraint to the inactive list and sorts it, so after the removal inactive[i] may
//     be another constraint than k: add_constraint!(W, i) adds inactive[i] WHATEVER IT NOW IS (:642).  That is the reference's
//     behaviour, quirk included;
//   - both sorts act on a sorted list with one new last entry: each is ONE insertion from the back (entries greater than the
//     new one move up by one).  On sorted lists that is what sort! gives.
// status:
//   0  the walk ended as the reference's does;
//   1  at capacity the constraint the swap removes would be sorted into position i of the inactive list and be put straight
//      back: (active, inactive, t, i) after the pass equals what it was before it, and the reference repeats that pass for
//      ever.  The routine stops BEFORE that pass: the lists are left in the unchanged state
//      and `added` holds what earlier passes set;
//   2  more than (l + 1)^2 passes of the while loop: a defensive cap, so that the loop is bounded even if a longer cycle than
//      the one-pass cycle of status 1 exists.  None has been observed (not proved); the lists are left as they are at the cap.
// Single-threaded: on the device one lane runs it on LDS copies (gn_kernels_addition_batched.hpp, general form); the
// wave-per-problem form there makes the same moves by cross-lane operations.
//
// The rebuild: column c of At is row active[c] of A (l x n column-major, lda); an entry 0 of the list gathers a row of zeros.
// row_i = sqrt(sum of squares) in ONE fixed order that depends on n alone and that a wave can form: partial s (0 <= s < 64) is
// the sum of a[j]^2 over j = s, s + 64, s + 128, ... in ascending j, starting from +0.0; the 64 partials are then added by the
// butterfly of the wave all-reduce, level after level x[s] += x[s ^ mask] for mask = 1, 2, 7, 15, 16, 32 (every lane of a level
// adds the same two partial sums, so all 64 end with the same bits: row_i is x[0]).  Products and additions are rounded
// separately (fp contract off), the square root and the divisions are IEEE.  Plain sums of squares: covered for entries inside the
// 2^+-400 band, as the sums of the line-search set-up.
//   scaling == 0: diag_scale = row_i, the row and cx are copied;
//   scaling != 0: row_i < DBL_EPSILON gives the divisor 1.0, the row and cx are divided by the divisor and diag_scale = 1.0 / divisor.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GN_HD __host__ __device__
#else
#define GN_HD
#endif

namespace gn {

#define GN_ADDITION_SQRT_EPS 1.4901161193847656e-08      // sqrt(eps(Float64)) = 2^-26 (:615)
#define GN_ADDITION_DELTA 0.1                            // :616
#define GN_ADDITION_EPS 2.220446049250313e-16            // eps(Float64) of evaluate_scaling!

// cx[k] < eps || (k == index_alpha_upp && cx[k] < delta) (:623)
GN_HD inline bool addition_violated(double c, bool is_alpha_upp) {
    return c < GN_ADDITION_SQRT_EPS || (is_alpha_upp && c < GN_ADDITION_DELTA);
}

// where v goes when it is appended to the sorted list[0:cnt) and sorted in by one insertion from the back
template <class I>
GN_HD inline long long addition_insert_pos(const I* list, long long cnt, I v) {
    long long p = cnt;
    while (p > 0 && list[p - 1] > v) --p;
    return p;
}
template <class I>
GN_HD inline void addition_insert(I* list, long long cnt, long long p, I v) {
    for (long long j = cnt; j > p; --j) list[j] = list[j - 1];
    list[p] = v;
}

// evaluate_violated_constraints.  active, inactive: l entries each, the first *t / l - *t used, 0 behind; cx: l entries.
// Returns the status; *t, the lists and *added (0 / 1) are updated.
template <class I>
GN_HD inline int addition_walk(long long l, long long n, long long q, long long* t_io, I* active, I* inactive, const double* cx,
                               long long index_alpha_upp, int* added) {
    const long long bnd = l < n ? l : n;                                          // :617
    const long long cap = (l + 1) * (l + 1);
    long long t = *t_io, passes = 0;
    int status = 0;
    *added = 0;                                                                   // :618
    long long i = 1;                                                              // :620
    while (i <= l - t) {                                                          // :621 (false at once when l <= t, :619)
        if (++passes > cap) { status = 2; break; }
        const long long k = (long long)inactive[i - 1];                           // :622
        if (k == 0 || !addition_violated(cx[k - 1], k == index_alpha_upp)) {      // :623
            ++i;                                                                  // :645
            continue;
        }
        if (t >= bnd) {                                                           // :624
            long long worst_k = 0;                                                // :626
            double worst_val = -INFINITY;                                         // :627
            for (long long j = q + 1; j <= t; ++j) {                              // :628
                const long long jj = (long long)active[j - 1];
                if (jj != 0 && cx[jj - 1] > worst_val) {                          // :630
                    worst_val = cx[jj - 1];
                    worst_k = j;
                }
            }
            if (!(worst_k > 0 && worst_val > cx[k - 1])) {                        // :635
                ++i;                                                              // :638
                continue;
            }
            // remove_constraint!(W, worst_k): the removed constraint goes to the inactive list, sorted in
            const I v = active[worst_k - 1];
            const long long p = addition_insert_pos(inactive, l - t, v);
            if (p == i - 1) { status = 1; break; }                                // it would come straight back: the reference spins
            addition_insert(inactive, l - t, p, v);
            for (long long j = worst_k; j < t; ++j) active[j - 1] = active[j];
            active[t - 1] = 0;
            --t;
        }
        // add_constraint!(W, i)
        const I v = inactive[i - 1];
        addition_insert(active, t, addition_insert_pos(active, t, v), v);
        for (long long j = i; j < l - t; ++j) inactive[j - 1] = inactive[j];
        inactive[l - t - 1] = 0;
        ++t;
        *added = 1;                                                               // :643
    }
    *t_io = t;
    return status;
}

// the 64 strided partials of the squares of `count` entries a[0], a[stride], ... (x[s] from +0.0, ascending j)
GN_HD inline void gather_partials(const double* a, long long stride, long long count, double* x) {
#pragma clang fp contract(off)
    for (int s = 0; s < 64; ++s) x[s] = 0.0;
    for (long long j = 0; j < count; ++j) {
        const double v = a[j * stride];
        const double sq = v * v;
        x[j & 63] = x[j & 63] + sq;
    }
}
// the butterfly over the 64 partials, in place; the sum is x[0] (and every other entry)
GN_HD inline double gather_butterfly(double* x) {
#pragma clang fp contract(off)
    const int masks[6] = {1, 2, 7, 15, 16, 32};
    for (int lv = 0; lv < 6; ++lv) {
        const int mk = masks[lv];
        for (int s = 0; s < 64; ++s) {
            const int o = s ^ mk;
            if (s < o) {
                const double sum = x[s] + x[o];
                x[s] = sum;
                x[o] = sum;
            }
        }
    }
    return x[0];
}
// the divisor of a row and its diag_scale from the sum of squares
GN_HD inline double gather_divisor(double sumsq, bool scaling, double* diag_scale) {
    double row = sqrt(sumsq);
    if (!scaling) {
        *diag_scale = row;
        return 1.0;
    }
    if (fabs(row) < GN_ADDITION_EPS) row = 1.0;
    *diag_scale = 1.0 / row;
    return row;
}

// the rebuild on host data.  At: n x t column-major, ldat; nothing between rows n and ldat is written
template <class I>
GN_HD inline void gather_active(long long n, long long t, const I* active, const double* A, long long lda, const double* cx,
                                bool scaling, double* At, long long ldat, double* cx_active, double* diag_scale) {
    double x[64];
    for (long long c = 0; c < t; ++c) {
        const long long r = (long long)active[c];
        const double* row = r ? A + (r - 1) : A;
        gather_partials(row, lda, r ? n : 0, x);
        const double div = gather_divisor(gather_butterfly(x), scaling, diag_scale + c);
        double* col = At + c * ldat;
        const double cv = r ? cx[r - 1] : 0.0;
        if (scaling) {
            for (long long j = 0; j < n; ++j) col[j] = (r ? row[j * lda] : 0.0) / div;
            cx_active[c] = cv / div;
        } else {
            for (long long j = 0; j < n; ++j) col[j] = r ? row[j * lda] : 0.0;
            cx_active[c] = cv;
        }
    }
}

}  // namespace gn
