// The analysis of the Gauss-Newton direction, host side (no GPU; the kernels: gn_kernels_direction_batched.hpp):
//   dir_decide         check_gn_direction (src/enlsip_functions.jl:943-1030) on scalars only (the batched call runs it on the
//                      downloaded sums: the decision has this one implementation)
//   dir_status         what the call reports besides the code: 1 the reference would index d past its end, 2 a prefix of d reaches
//                      past n - rankA
//   dir_sums           every scalar the decision reads, from host arrays of one problem, in the order the kernels use
//                      (enlsip_gn_direction_sums)
//
// The decision keeps the reference's statements and their order.  The four norms are sqrt of the sums (one IEEE square root
// each), beta = sqrt(d1nrm * d1nrm + b1nrm * b1nrm) with d1nrm^2 as d1nrm * d1nrm (Julia's literal power), products and additions
// rounded on their own.  any(>=(-sqr_eps), lambda .* rows) && any(<(0), lambda) of :1004 is n_lm_ge > 0 && n_lm_neg > 0 and is
// looked at only when q < t; any(<(delta), inact_c) of :1009 is n_inactive_lt_delta > 0 and is looked at only when l - t > 0.
//
// Sums: the order of gn_termination.hpp.  Partial s (0 <= s < 64) adds the terms j = s, s + 64, ... in ascending j from +0.0, and
// the 64 partials are added by the butterfly of the wave all-reduce (masks 1, 2, 7, 15, 16, 32); products and additions are
// rounded separately.  A prefix sum (d1_sq, d1_asprev_sq, b1_sq) is the same statement over fewer terms, so the kernels may form
// the three sums over d in one pass under two predicates.  Norms are a plain sum of squares: covered for operands inside the
// 2^+-400 band.  A NaN passes none of the three comparisons behind the counts; a list entry 0
// (padding inside the used part) contributes nothing.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/enlsip_gn.h"
#include "gn_termination.hpp"

namespace gn {

#define GN_DIR_DELTA 1e-1       // delta of :964, the bound of the inactive test (:1009)

// :1001-1004 for one multiplier: lambda_i * rows_i >= -sqrt(eps)
GN_HD inline bool dir_lm_ge(double lam, double rows) {
#pragma clang fp contract(off)
    const double prod = lam * rows;
    return prod >= -GN_TERM_SQRT_EPS;
}

// k of d_gn[1:k] at :1230-1231 (the callers keep prev_t in 0..l and |prev_dimJ2| <= 2^31: no overflow)
inline long long dir_k_prev(const enlsip_gn_dir_state& s) { return s.prev_dimJ2 + s.prev_t - s.t - 1; }

inline long long dir_status(const enlsip_gn_dir_state& s, long long m, long long n) {
    const long long kp = dir_k_prev(s);
    if (kp > m) return 1;                                                         // BoundsError at :1231
    const long long reach = s.dimJ2 > kp ? s.dimJ2 : kp;
    return reach > 0 && reach > n - s.rankA ? 2 : 0;
}

inline void dir_decide(const enlsip_gn_dir_state& s, const enlsip_gn_dir_sums& v, long long m, long long n, long long* method_code,
                       double* beta) {
#pragma clang fp contract(off)
    const double b1nrm = sqrt(v.b1_sq);                                           // :1222
    const double d1nrm = sqrt(v.d1_sq);                                           // :1228
    const double d1nrm_as_km1 = sqrt(v.d1_asprev_sq);                             // :1231
    const double dnrm = sqrt(v.d_sq);                                             // :1227
    const double active_c_sum = v.active_c_sum;
    const double c1 = 0.5, c2 = 0.1, c3 = 4.0, c4 = 10.0, c5 = 0.05;              // :965
    const double eps_rel = DBL_EPSILON;                                           // :966
    const double beta_k = sqrt(d1nrm * d1nrm + b1nrm * b1nrm);                    // :967
    long long code = 1;                                                           // :969
    const bool constraint_added = s.add != 0, constraint_deleted = s.del != 0;
    const bool newton_or_restart = s.prev_code == 2 || s.restart != 0;            // :974
    const bool first_iter = s.iter_number == 0;                                   // :981
    const bool submin_prev_iter = s.prev_code == -1;                              // :982
    const bool add_or_del = constraint_added || constraint_deleted;               // :983
    const bool convergence_lower_c1 = beta_k < c1 * s.prev_beta;                  // :984
    const bool progress_not_close = (s.prev_progress > c2 * s.prev_predicted_reduction) && (dnrm <= c3 * beta_k);      // :985
    if (newton_or_restart || (!first_iter && (submin_prev_iter || !(add_or_del || convergence_lower_c1 || progress_not_close)))) {
        code = -1;                                                                // :993
        const double non_linearity_k = sqrt(d1nrm * d1nrm + active_c_sum);        // :994
        const double non_linearity_km1 = sqrt(d1nrm_as_km1 * d1nrm_as_km1 + active_c_sum);      // :995
        bool to_reduce = false;                                                   // :997
        if (s.q < s.t) {                                                          // :998
            const bool lagrange_mult_cond = v.n_lm_ge > 0 && v.n_lm_neg > 0;      // :1004
            to_reduce = to_reduce || lagrange_mult_cond;                          // :1005
        }
        if (s.l - s.t > 0) to_reduce = to_reduce || v.n_inactive_lt_delta > 0;    // :1007-1010
        const bool newton_previously = s.prev_code == 2 && !constraint_deleted;   // :1012
        const bool cond4 = active_c_sum > c2;                                     // :1013
        const bool cond5 = constraint_deleted || constraint_added || to_reduce || (s.t == n && s.t == s.rankA);      // :1015
        const double eps = fmax(1e-2, 10.0 * eps_rel);                            // :1017
        const bool cond6 = !((s.l == s.q) || (s.rankA <= s.t)) && !((beta_k < eps * dnrm) || (b1nrm < eps && m == n - s.t));     // :1018
        if (newton_previously || !(cond4 || cond5 || cond6)) {                    // :1019
            const bool cond7 = (s.prev_alpha < c5 && non_linearity_km1 < c2 * non_linearity_k) || m == n - s.t;      // :1020
            const bool cond8 = !(dnrm <= c4 * beta_k);                            // :1021
            if (newton_previously || cond7 || cond8) code = 2;                    // :1023-1025
        }
    }
    *method_code = code;
    *beta = beta_k;
}

struct DirHostArgs {
    long long m, l;
    const int64_t *active, *inactive;
    const double *b, *d, *lambda, *diag_scale, *cx_all;
    bool scaling;
};

// the caller has excluded dir_status == 1: k_prev <= m
inline void dir_sums(const enlsip_gn_dir_state& s, const DirHostArgs& a, enlsip_gn_dir_sums* out) {
#pragma clang fp contract(off)
    enlsip_gn_dir_sums v;
    const long long t = s.t, kp = dir_k_prev(s);
    auto dsq = [&](long long j) { return a.d[j] * a.d[j]; };
    v.b1_sq = term_ordered_sum(s.dimA, [&](long long i) { return a.b[i] * a.b[i]; });      // :1222
    v.d_sq = term_ordered_sum(a.m, dsq);                                          // :1227
    v.d1_sq = term_ordered_sum(s.dimJ2, dsq);                                     // :1228
    v.d1_asprev_sq = term_ordered_sum(kp > 0 ? kp : 0, dsq);                      // :1231
    v.active_c_sum = term_ordered_sum(t, [&](long long i) {                       // :2701 / :2785
        const long long r = a.active[i];
        const double c = r ? a.cx_all[r - 1] : 0.0;
        return c * c;
    });
    long long ge = 0, neg = 0, lt = 0;
    for (long long i = s.q; i < t; ++i) {                                         // :1001-1004
        const double li = a.lambda[i];
        ge += dir_lm_ge(li, term_rows(a.diag_scale[i], a.scaling));
        neg += li < 0.0;
    }
    for (long long j = 0; j < a.l - t; ++j) {                                     // :1008-1009
        const long long r = a.inactive[j];
        if (r == 0) continue;
        lt += a.cx_all[r - 1] < GN_DIR_DELTA;
    }
    v.n_lm_ge = ge;
    v.n_lm_neg = neg;
    v.n_inactive_lt_delta = lt;
    *out = v;
}

}  // namespace gn
