// The termination test of the outer iteration, one body for host and device wherever the device needs it:
//   term_minmax        minmax_lagrangian_mult (src/enlsip_functions.jl:540-564)
//   term_decide        check_termination_criteria (:2420-2516) on scalars only (host; the batched call runs it on the downloaded sums)
//   term_sums          every scalar the decision reads, from host arrays, in the orders the kernels of
//                      gn_kernels_termination_batched.hpp use (enlsip_gn_termination_sums)
//
// minmax, line for line: t <= q gives (+Inf, 0.0) (:550-553).  Otherwise lambda_abs_max = maximum(abs, lambda) over ALL t entries
// (:554) and sigma_min is the smallest lambda_i over the positions q+1..t, in order, that pass
// lambda_i * rows_i <= -sqrt(DBL_EPSILON) && lambda_i < sigmin (strict <, :558), rows_i = 1.0 / diag_scale_i (IEEE) with scaling,
// diag_scale_i without (:555).  A NaN never passes the test.  The value the ordered walk ends with is the minimum of the passing
// entries, whatever the order (equal minima are the same bits: a passing entry is never a zero), so the device takes it as a wave
// minimum.  A NaN IN lambda: Julia's maximum and NumPy's max both return NaN, and so does this routine: lambda_abs_max is the
// quiet NaN 0x7ff8000000000000 as soon as one of the t entries is a NaN, on the host and in both kernel forms.
//
// The decision keeps the reference's statements and their order: the preliminary condition, the necessary conditions, the four
// convergence codes 10000 / 2000 / 300 / 40, the feas negation of :2471-2481, then the abnormal elseif chain -2, error_code
// (-3..-5), -9, -6, -10, -11.  The negation is unreachable in the reference as it stands: necessary_crit already demands every
// inactive cx > 0 (:2434), so no inactive cx <= 0 can be left at :2475.  It is restated all the same, from a count of its own
// (n_inactive_le0; the necessary condition reads n_inactive_nonpos, and a NaN separates the two).  eps_rel^2 is eps_rel * eps_rel,
// as Julia's literal power.  alfnoi = eps / (norm_p + eps), eps = DBL_EPSILON.
//
// Sums.  Every n-, t- and l-length sum is taken in ONE fixed order that depends on its length alone, the order of
// gn_violated_constraints.hpp: partial s (0 <= s < 64) adds the terms j = s, s + 64, ... in ascending j from +0.0, and the 64
// partials are added by the butterfly of the wave all-reduce (masks 1, 2, 7, 15, 16, 32).  Products and additions are rounded
// separately (fp contract off).  Entry j of At * cx_active is a matrix-vector product: its t terms in ascending column order from
// +0.0, one running sum per row (the lanes of the kernels run along the rows of At), then the norm over j in the order above.
// Norms are a plain sum of squares and one IEEE square root, not BLAS nrm2's scaled form: covered for operands inside the 2^+-400
// band, as the sums of the line-search set-up and the gather (5.12).
// Two values are pinned to existing kernels instead and are NOT restated bit for bit here: grad = J' rx follows k_gemv_t (a fused
// multiply-add per term on the device), rx_sum the dot(rx, rx) of the line-search set-up.  term_sums takes both as optional
// inputs (grad_in, rx_sum_in: what the device formed) and otherwise forms them in the strided order with separate roundings.
// A list entry 0 (padding inside the used part; the reference would fail on it) contributes nothing to a sum or a count.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/enlsip_gn.h"
#include "gn_violated_constraints.hpp"

namespace gn {

#define GN_TERM_SQRT_EPS 1.4901161193847656e-08      // sqrt(eps(Float64)) = 2^-26 (:549)
#define GN_TERM_EPS 2.220446049250313e-16            // eps(Float64) (:2421)

// the factor of :555
GN_HD inline double term_rows(double diag_scale, bool scaling) { return scaling ? 1.0 / diag_scale : diag_scale; }
// the test of :558 without its strict < (the caller keeps the minimum)
GN_HD inline bool term_sigma_candidate(double lam, double rows) {
#pragma clang fp contract(off)
    const double prod = lam * rows;
    return prod <= -GN_TERM_SQRT_EPS;
}

inline void term_minmax(long long q, long long t, const double* lambda, const double* diag_scale, bool scaling, double* sigma_min,
                        double* lambda_abs_max) {
    double lam_abs_max = 0.0;                                                     // :550
    double sigmin = INFINITY;                                                     // :551
    if (t > q) {                                                                  // :553
        bool nan = false;
        for (long long i = 0; i < t; ++i) {                                       // :554
            const double a = fabs(lambda[i]);
            if (a != a) nan = true;
            else if (a > lam_abs_max) lam_abs_max = a;
        }
        if (nan) lam_abs_max = (double)NAN;
        for (long long i = q + 1; i <= t; ++i) {                                  // :556
            const double li = lambda[i - 1];                                      // :557
            if (term_sigma_candidate(li, term_rows(diag_scale[i - 1], scaling)) && li < sigmin) sigmin = li;     // :558-559
        }
    }
    *sigma_min = sigmin;
    *lambda_abs_max = lam_abs_max;
}

inline long long term_decide(const enlsip_gn_term_state& s, const enlsip_gn_term_sums& v, const enlsip_gn_term_tol& tol) {
#pragma clang fp contract(off)
    long long exit_code = 0;                                                      // :2420
    const double rel_tol = GN_TERM_EPS;                                           // :2421
    const double alfnoi = rel_tol / (v.p_nrm + rel_tol);                          // :2422
    const bool preliminary_cond = !(s.restart != 0 || (s.code == -1 && alfnoi <= 0.25));     // :2425
    if (preliminary_cond) {                                                       // :2427
        bool necessary_crit = s.del == 0 && v.active_cx_nrm < tol.eps_c && s.grad_res < sqrt(tol.eps_rel) * (1 + v.grad_nrm);     // :2430
        if (s.l - s.t > 0) necessary_crit = necessary_crit && v.n_inactive_nonpos == 0;     // :2431-2435
        if (s.t > s.q) {                                                          // :2437
            double factor = 0.0;
            if (s.t == 1) factor = 1 + v.rx_sum;                                  // :2438-2439
            else if (s.t > 1) factor = v.lambda_abs_max;                          // :2440-2441
            necessary_crit = necessary_crit && v.sigma_min >= tol.eps_rel * factor;     // :2443
        }
        if (necessary_crit) {                                                     // :2446
            if (v.d1_sq <= v.rx_sum * (tol.eps_rel * tol.eps_rel)) exit_code += 10000;      // :2452
            if (v.rx_sum <= tol.eps_abs * tol.eps_abs) exit_code += 2000;         // :2456
            if (v.x_diff < tol.eps_x * v.x_nrm) exit_code += 300;                 // :2460
            if (alfnoi > 0.25) exit_code += 40;                                   // :2464
            if (exit_code > 0 && s.l - s.t > 0) {                                 // :2471 (unreachable with feas = -1, see above)
                const long long feas = v.n_inactive_le0 > 0 ? -1 : 1;             // :2472-2479
                exit_code *= feas;                                                // :2480
            }
        }
    }
    if (exit_code == 0) {                                                         // :2485
        const double active_penalty_sum = s.t == 0 ? 0.0 : v.active_penalty_sum;  // :2489
        if (s.nb_iter >= tol.max_iter) exit_code = -2;                            // :2492
        else if (-5 <= s.error_code && s.error_code <= -3) exit_code = s.error_code;     // :2496
        else if (s.nb_newton_steps > 5) exit_code = -9;                           // :2500
        else if (s.psi_error == -1) exit_code = -6;                               // :2503
        else if (v.x_diff <= 10.0 * tol.eps_x && v.Atcx_nrm <= 10.0 * tol.eps_c && active_penalty_sum >= 1.0) exit_code = -10;     // :2507
        else if (s.delta_time > 0) exit_code = -11;                               // :2511
    }
    return exit_code;
}

// one sum in the documented order: term(j) for j = 0 .. count-1
template <class Term>
inline double term_ordered_sum(long long count, Term term) {
#pragma clang fp contract(off)
    double x[64];
    for (int s = 0; s < 64; ++s) x[s] = 0.0;
    for (long long j = 0; j < count; ++j) x[j & 63] = x[j & 63] + term(j);
    return gather_butterfly(x);
}

struct TermHostArgs {
    long long m, n, l, t, q, dimJ2;
    double psi0;
    const int64_t *active, *inactive;
    const double* J; long long ldj;
    const double *rx, *cx_all, *x, *x_prev, *p, *d_gn, *lambda, *cx_active, *diag_scale;
    const double* At; long long ldat;
    const double* w;
    bool scaling;
    const double* grad_in;        // the gradient as formed elsewhere (the device's dgrad), or NULL
    const double* rx_sum_in;      // likewise rx_sum
    double* grad_out;             // n entries, or NULL
};

// `scratch`: n doubles (the gradient, then At * cx_active)
inline void term_sums(const TermHostArgs& a, double* scratch, enlsip_gn_term_sums* out) {
#pragma clang fp contract(off)
    enlsip_gn_term_sums v;
    const long long n = a.n, t = a.t, l = a.l;
    double* g = scratch;
    for (long long c = 0; c < n; ++c)
        g[c] = a.grad_in ? a.grad_in[c] : term_ordered_sum(a.m, [&](long long r) { return a.J[r + c * a.ldj] * a.rx[r]; });
    if (a.grad_out) for (long long c = 0; c < n; ++c) a.grad_out[c] = g[c];
    v.rx_sum = a.rx_sum_in ? *a.rx_sum_in : term_ordered_sum(a.m, [&](long long r) { return a.rx[r] * a.rx[r]; });
    v.grad_nrm = sqrt(term_ordered_sum(n, [&](long long j) { return g[j] * g[j]; }));
    v.p_nrm = sqrt(term_ordered_sum(n, [&](long long j) { return a.p[j] * a.p[j]; }));
    v.active_cx_nrm = sqrt(term_ordered_sum(t, [&](long long i) { return a.cx_active[i] * a.cx_active[i]; }));
    long long nonpos = 0, le0 = 0;
    for (long long i = 0; i < l - t; ++i) {
        const long long r = a.inactive[i];
        if (r == 0) continue;
        const double c = a.cx_all[r - 1];
        nonpos += !(c > 0.0);
        le0 += c <= 0.0;
    }
    v.n_inactive_nonpos = nonpos;
    v.n_inactive_le0 = le0;
    term_minmax(a.q, t, a.lambda, a.diag_scale, a.scaling, &v.sigma_min, &v.lambda_abs_max);
    v.d1_sq = term_ordered_sum(a.dimJ2, [&](long long j) { return a.d_gn[j] * a.d_gn[j]; });
    v.x_diff = sqrt(term_ordered_sum(n, [&](long long j) { const double d = a.x_prev[j] - a.x[j]; return d * d; }));
    v.x_nrm = sqrt(term_ordered_sum(n, [&](long long j) { return a.x[j] * a.x[j]; }));
    for (long long j = 0; j < n; ++j) {
        double s = 0.0;
        for (long long c = 0; c < t; ++c) s = s + a.At[j + c * a.ldat] * a.cx_active[c];
        g[j] = s;
    }
    v.Atcx_nrm = sqrt(term_ordered_sum(n, [&](long long j) { return g[j] * g[j]; }));
    v.active_penalty_sum = term_ordered_sum(t, [&](long long i) {
        const long long r = a.active[i];
        const double wi = r ? a.w[r - 1] : 0.0;
        return wi * wi;
    });
    v.whsum = term_ordered_sum(t, [&](long long i) {
        const long long r = a.active[i];
        if (!r) return 0.0;
        const double c = a.cx_all[r - 1];
        const double sq = c * c;
        return a.w[r - 1] * sq;
    });
    v.progress = (2 * a.psi0 - v.rx_sum) - v.whsum;                               // :2279-2280
    *out = v;
}

}  // namespace gn
