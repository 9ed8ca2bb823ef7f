// The upper bound of the steplength, one body for host and device: upper_bound_steplength (src/enlsip_functions.jl:2149-2178) on
// a product Ap = A * p that has already been formed.  Line for line against the reference:
//   - the inactive list is walked in list order and only its first n_inactive entries (1:l-t, :2164); a 0 entry is padding and is
//     skipped, so an all-zero list looks at nothing (:2163);
//   - the entry j == index_del is skipped (:2166);
//   - alpha_j = -cx[j] / Ap[j] is an IEEE division (:2168), formed before the test as the reference does;
//   - the test is cx[j] > 0 && Ap[j] < 0 && alpha_j < alpha_upper with a strict < (:2169): among equal minima the FIRST list position
//     wins, a comparison with a NaN is false (the row is skipped), and alpha_j = +Inf never beats the initial +Inf;
//   - alpha_upp = min(3.0, alpha_upper) (:2176) while index_alpha_upp stays the minimising row even when its alpha_j is 3 or more.
// steplength_candidate is the test of one list position; the kernels (gn_kernels_linesearch_batched.hpp) evaluate it per position
// and reduce (alpha, position) lexicographically, which names the row the sequential loop names (the proof is next to them).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GN_HD __host__ __device__
#else
#define GN_HD
#endif

namespace gn {

#define GN_STEPLENGTH_CAP 3.0      // :2176

// :2168-2169 of one row with c = cx[j], g = Ap[j], against alpha_upper = +Inf: true and *alpha = alpha_j when the row could ever
// be taken, i.e. c > 0 && g < 0 && alpha_j < +Inf
GN_HD inline bool steplength_row_test(double c, double g, double* alpha) {
    const double a = -c / g;                                                     // :2168
    *alpha = a;
    return c > 0.0 && g < 0.0 && a < (double)INFINITY;                           // :2169
}

// One list entry j (1-based, 0: padding, in 0..l) of :2165-2169
GN_HD inline bool steplength_candidate(long long j, long long index_del, const double* cx, const double* Ap, double* alpha) {
    if (j == 0 || j == index_del) return false;                                  // :2163, :2166
    return steplength_row_test(cx[j - 1], Ap[j - 1], alpha);
}

// upper_bound_steplength (:2149-2178).  inactive: n_inactive entries in 0..l; cx, Ap: l entries.
template <class Int>
GN_HD inline void steplength_bound(long long n_inactive, const Int* inactive, long long index_del, const double* cx,
                                   const double* Ap, double* alpha_upp, Int* index_alpha_upp) {
    double alpha_upper = (double)INFINITY;                                       // :2161
    Int index = 0;                                                               // :2162
    for (long long i = 0; i < n_inactive; ++i) {                                 // :2164
        double a;
        if (steplength_candidate(inactive[i], index_del, cx, Ap, &a) && a < alpha_upper) {      // :2169
            alpha_upper = a;                                                     // :2170
            index = inactive[i];                                                 // :2171
        }
    }
    *alpha_upp = alpha_upper < GN_STEPLENGTH_CAP ? alpha_upper : GN_STEPLENGTH_CAP;             // :2176
    *index_alpha_upp = index;
}

}  // namespace gn
