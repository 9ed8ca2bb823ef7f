// The polynomial fit of the line search (linesearch_constrained, src/enlsip_functions.jl:1940-2143) between two callback
// evaluations, restated from the reference with IEEE arithmetic where a scripting language would raise:
//   linesearch_coefficients   concatenate! (:1635-1659), coefficients_linesearch! (:1665-1689) and the scaling of v1 = [Jp; Ap]
//                             (:1986-1998), reduced to the six dot products minrm (:1849) and parameters_rm (:1749-1751) take
//   linesearch_fit            minrm (:1841-1862) with parameters_rm (:1739-1786), bounds (:1788-1792), newton_raphson (:1794-1813),
//                             one_root (:1817-1820), two_roots (:1823-1839) and the choice of :2023-2026
//   linesearch_minrn          minrn (:1708-1735) with minimize_quadratic (:1692-1702)
//   linesearch_check_reduction  check_reduction (:1870-1886)
// Plain C++, host only, nothing of HIP; the entry points of gn_linesearch_fit_batched.inc export them without a handle and without a
// GPU.  Every body switches contraction off.
//
// The six sums.  No vector is materialised; the elements are formed literally, entry by entry:
//   residual i          v0 = rx[i], v1 = Jp[i], vb = rx_new[i]
//   active k            v0 = sqrt(w[k]) * cx[k], v1 = sqrt(w[k]) * Ap[k], vb = sqrt(w[k]) * cx_new[k]
//   inactive k          the same, but v0 = 0 and v1 = 0 when cx[k] > 0 (v1 reads the OLD cx, :1996), vb = 0 when cx_new[k] > 0
//   v2 = ((vb - v0) / alpha_k - v1) / alpha_k, two IEEE divisions; alpha_k == 0 is not special-cased
// and sums = v0.v0, v0.v1, v0.v2, v1.v1, v1.v2, v2.v2.  The order of summation is part of the contract: the m residual terms in
// index order, then the active list in list order, then the inactive list in list order, each product rounded and then added.  (The
// reference's dot is BLAS's and sums in constraint-number order inside [m, m + l); the difference is a reordering of a sum.)  The
// reference scales JpAp in place (:1986); this routine writes neither Jp nor Ap, so it can be called again on the same buffers
// (:2078-2092 does call it again, on the already scaled v1: there the caller hands the unscaled Ap once more).
//
// The scalar stage.  s = [v0.v0 / 2, v0.v1, v0.v2 + v1.v1 / 2, v1.v2, v2.v2 / 2] in increasing degree, ds and dds its derivatives.
// Polynomials are evaluated by Horner's rule, unfused, starting from 0.0; Polynomials.jl's evalpoly may fuse
// (muladd), which moves a value by a rounding.  Quirks kept as written:
//   - d starts as the sentinel 1.0 (:1747) and is only overwritten on the analytic arm, so the Newton arm always ends in
//     beta_hat = alpha_hat (:1781-1783)
//   - (a3, a2, a1) = coeffs(ds) / (2 normv2) destructures the FIRST three coefficients of ds, those of degree 0, 1, 2 (:1757)
//   - the test alpha_old == beta_hat compares the UNCLAMPED alpha_hat after bounds has run on it (:1854-1856)
//   - the Newton loop runs while (error > 1e-4 || iter < 3) && iter < 50, and leaves on |dds(alpha)| < eps (:1801-1805)
//   - dds_best * eta < 2 Dm hm, d < 0, d >= 0, x_min <= beta2, c <= 0 and the choice alpha_kp1 != beta && p_beta < pk &&
//     beta <= alpha_k keep their strictness
// a^2 and a^3 are a*a and a*a*a as Julia lowers literal powers; (-b/3)^(3/2) is pow, and pow, acos and cos are the host libm's;
// cbrt is the libm's with one correction step (fit_cbrt).
// min and max read min(a, b) = b < a ? b : a, max(a, b) = b > a ? b : a: a NaN in the first place stays.  Where the Julia would
// throw (or a scripting language's division would raise), the IEEE value is taken: ds(x_min) / dds_best with dds_best == 0, the division
// by 2 normv2 == 0 on the analytic arm (the coefficients become +-Inf or NaN and so does the step), acos of an argument that
// rounding pushed past 1 (NaN), sort of a triple with a NaN (the triple is ordered by `<` with a three-element network).  The Newton
// loop is bounded by its 50 iterations, so a NaN input ends the routine; nothing loops on a value.
#pragma once
#include <math.h>
#include <stdint.h>

namespace gn {

#define GN_FIT_EPS 2.220446049250313e-16        // eps(Float64), :1803
#define GN_FIT_SQRT_EPS 1.4901161193847656e-08  // sqrt(eps(Float64)), :1717

inline double fit_min(double a, double b) { return b < a ? b : a; }
inline double fit_max(double a, double b) { return b > a ? b : a; }

// the six products of one entry added to the six sums
inline void fit_add_entry(double v0, double v1, double vb, double alpha_k, double* s) {
#pragma clang fp contract(off)
    const double v2 = ((vb - v0) / alpha_k - v1) / alpha_k;                      // :1688
    s[0] = s[0] + v0 * v0;
    s[1] = s[1] + v0 * v1;
    s[2] = s[2] + v0 * v2;
    s[3] = s[3] + v1 * v1;
    s[4] = s[4] + v1 * v2;
    s[5] = s[5] + v2 * v2;
}

// the three elements of constraint k (0-based): v0, v1, vb.  An inactive entry is 0 where the constraint is satisfied (:1655,
// :1996 for v1 on the OLD cx, :1655 through :1680 for v_buff on cx_new)
inline void fit_constraint_elements(bool inactive, double wk, double cxk, double cxnk, double apk, double* v0, double* v1, double* vb) {
#pragma clang fp contract(off)
    const double sq = sqrt(wk);
    const bool old_out = inactive && cxk > 0.0;
    *v0 = old_out ? 0.0 : sq * cxk;
    *v1 = old_out ? 0.0 : sq * apk;
    *vb = (inactive && cxnk > 0.0) ? 0.0 : sq * cxnk;
}

inline void linesearch_coefficients(int64_t m, int64_t t, const int64_t* active, int64_t n_inactive, const int64_t* inactive,
                                    const double* rx, const double* rx_new, const double* Jp, const double* cx, const double* cx_new,
                                    const double* Ap, const double* w, double alpha_k, double* sums) {
#pragma clang fp contract(off)
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = 0; i < m; ++i) fit_add_entry(rx[i], Jp[i], rx_new[i], alpha_k, s);
    for (int pass = 0; pass < 2; ++pass) {
        const int64_t* list = pass ? inactive : active;
        const int64_t n = pass ? n_inactive : t;
        for (int64_t i = 0; i < n; ++i) {
            const int64_t k = list[i] - 1;
            double v0, v1, vb;
            fit_constraint_elements(pass != 0, w[k], cx[k], cx_new[k], Ap[k], &v0, &v1, &vb);
            fit_add_entry(v0, v1, vb, alpha_k, s);
        }
    }
    for (int q = 0; q < 6; ++q) sums[q] = s[q];
}

// Horner from 0.0 over `n` coefficients in increasing degree, unfused
inline double fit_polyval(const double* c, int n, double x) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int i = n - 1; i >= 0; --i) s = s * x + c[i];
    return s;
}

inline double fit_newton_raphson(double x_min, double Dm, const double* ds, const double* dds) {
#pragma clang fp contract(off)
    double a = x_min, err = 1.0;
    int it = 0;
    while ((err > 1e-4 || it < 3) && it < 50) {                                  // :1801
        const double cc = fit_polyval(dds, 3, a);
        if (fabs(cc) < GN_FIT_EPS) break;                                        // :1803
        const double h = -fit_polyval(ds, 4, a) / cc;
        a = a + h;
        err = (2.0 * Dm * (h * h)) / fabs(cc);                                   // :1808
        ++it;
    }
    return a;
}

// cbrt to the last place: the libm's value and one Newton correction on its residual x - y^3, formed without rounding error by
// explicit fma calls.  one_root adds two cube roots of opposite sign and subtracts a / 3, so an ulp of a cube root is many ulps of
// the step; a libm whose cbrt is an ulp off in every other argument (glibc's) would show there.
inline double fit_cbrt(double x) {
#pragma clang fp contract(off)
    const double y = cbrt(x);
    if (y == 0.0 || !(fabs(y) <= 1.7976931348623157e308)) return y;
    const double y2 = y * y, e2 = fma(y, y, -y2);
    const double y3 = y2 * y, e3 = fma(y2, y, -y3);
    const double r = ((x - y3) - e3) - e2 * y;
    return y + r / (3.0 * y2);
}

inline double fit_one_root(double cc, double d, double a) {
#pragma clang fp contract(off)
    const double arg1 = -cc / 2.0 + sqrt(d), arg2 = -cc / 2.0 - sqrt(d);         // :1818
    return (fit_cbrt(arg1) + fit_cbrt(arg2)) - a / 3.0;
}

inline void fit_two_roots(double b, double cc, double a, double x_min, double* alpha_hat, double* beta_hat) {
#pragma clang fp contract(off)
    const double pi = 3.141592653589793;
    const double phi = acos(fabs(cc / 2.0) / pow(-b / 3.0, 1.5));                // :1824
    const double tt = cc <= 0.0 ? 2.0 * sqrt(-b / 3.0) : -2.0 * sqrt(-b / 3.0);  // :1825
    double b1 = tt * cos(phi / 3.0) - a / 3.0;
    double b2 = tt * cos((phi + 2.0 * pi) / 3.0) - a / 3.0;
    double b3 = tt * cos((phi + 4.0 * pi) / 3.0) - a / 3.0;
    double sw;
    if (b2 < b1) { sw = b1; b1 = b2; b2 = sw; }                                  // :1834
    if (b3 < b2) { sw = b2; b2 = b3; b3 = sw; }
    if (b2 < b1) { sw = b1; b1 = b2; b2 = sw; }
    if (x_min <= b2) { *alpha_hat = b1; *beta_hat = b3; }                        // :1837
    else { *alpha_hat = b3; *beta_hat = b1; }
}

// minrm and the choice.  out = alpha_kp1, pk, alpha_hat, s_alpha, beta_hat, s_beta (the last four as minrm returns them, before
// the choice); *arm: 0 Newton-Raphson, 1 one root, 2 two roots
inline void linesearch_fit(const double* sums, double alpha_k, double x_min, double alpha_min, double alpha_max, double* out, int* arm) {
#pragma clang fp contract(off)
    const double v0v0 = sums[0], v0v1 = sums[1], v0v2 = sums[2], v1v1 = sums[3], v1v2 = sums[4], v2v2 = sums[5];
    const double s[5] = {0.5 * v0v0, v0v1, v0v2 + 0.5 * v1v1, v1v2, 0.5 * v2v2}; // :1849
    const double ds[4] = {1.0 * s[1], 2.0 * s[2], 3.0 * s[3], 4.0 * s[4]};
    const double dds[3] = {1.0 * ds[1], 2.0 * ds[2], 3.0 * ds[3]};
    // parameters_rm (:1739-1786)
    const double dds_best = fit_polyval(dds, 3, x_min);
    const double eta = 0.1;
    double d = 1.0;                                                              // :1747, the sentinel
    const double normv2 = v2v2;
    const double h0 = fabs(fit_polyval(ds, 4, x_min) / dds_best);
    const double Dm = fabs(6.0 * v1v2 + 12.0 * x_min * normv2) + 24.0 * h0 * normv2;
    const double hm = fit_max(h0, 1.0);
    double alpha_hat, beta_hat = 0.0;
    int which = 0;
    if (dds_best * eta < 2.0 * Dm * hm) {                                        // :1754
        const double den = 2.0 * normv2;
        const double a3 = ds[0] / den, a2 = ds[1] / den, a1 = ds[2] / den;       // :1757: the FIRST three coefficients
        const double b = a2 - (a1 * a1) / 3.0;
        const double a13 = a1 / 3.0;
        const double cc = a3 - a1 * a2 / 3.0 + 2.0 * (a13 * a13 * a13);
        const double c2 = cc / 2.0, b3 = b / 3.0;
        d = c2 * c2 + b3 * b3 * b3;                                              // :1761
        if (d < 0.0) {
            fit_two_roots(b, cc, a1, x_min, &alpha_hat, &beta_hat);
            which = 2;
        } else {
            alpha_hat = fit_one_root(cc, d, a1);
            which = 1;
        }
    } else {
        alpha_hat = fit_newton_raphson(x_min, Dm, ds, dds);
    }
    if (d >= 0.0) beta_hat = alpha_hat;                                          // :1781
    // minrm (:1852-1861)
    const double alpha_old = alpha_hat;
    alpha_hat = fit_max(fit_min(alpha_hat, alpha_max), alpha_min);               // bounds, :1788-1792
    const double s_alpha = fit_polyval(s, 5, alpha_hat);
    double s_beta;
    if (alpha_old == beta_hat) {                                                 // :1856: the unclamped value
        beta_hat = alpha_hat;
        s_beta = fit_polyval(s, 5, alpha_hat);
    } else {
        beta_hat = fit_max(fit_min(beta_hat, alpha_max), alpha_min);
        s_beta = fit_polyval(s, 5, beta_hat);
    }
    double alpha_kp1 = alpha_hat, pk = s_alpha;
    if (alpha_kp1 != beta_hat && s_beta < pk && beta_hat <= alpha_k) {           // :2023-2026
        alpha_kp1 = beta_hat;
        pk = s_beta;
    }
    out[0] = alpha_kp1; out[1] = pk; out[2] = alpha_hat; out[3] = s_alpha; out[4] = beta_hat; out[5] = s_beta;
    *arm = which;
}

inline void linesearch_minrn(double x1, double y1, double x2, double y2, double x3, double y3, double alpha_min, double alpha_max,
                             double p_max, double* alpha, double* p_alpha) {
#pragma clang fp contract(off)
    const double eps = GN_FIT_SQRT_EPS / p_max;                                  // :1717
    if (fabs(x1 - x2) < eps || fabs(x3 - x1) < eps || fabs(x3 - x2) < eps) {     // :1719
        *alpha = 0.0;
        *p_alpha = 0.0;
        return;
    }
    const double d1 = y2 - y1, d2 = y3 - y1;                                     // minimize_quadratic, :1692-1702
    const double sn = (x3 - x1) * (x3 - x1) * d1 - (x2 - x1) * (x2 - x1) * d2;
    const double q = 2.0 * ((x2 - x1) * d2 - (x3 - x1) * d1);
    const double u = x1 - sn / q;
    const double a = fit_min(fit_max(u, alpha_min), alpha_max);                  // :1726
    const double t1 = (a - x1) * (a - x2) * y3 / ((x3 - x1) * (x3 - x2));
    const double t2 = (a - x3) * (a - x2) * y1 / ((x1 - x3) * (x1 - x2));
    const double t3 = (a - x3) * (a - x2) * y2 / ((x2 - x1) * (x2 - x3));
    *alpha = a;
    *p_alpha = t1 + t2 + t3;
}

inline int linesearch_check_reduction(double psi_alpha, double psi_k, double approx_k, double eta, double diff_psi) {
#pragma clang fp contract(off)
    const double delta = 0.2;                                                    // :1878
    if (psi_alpha - approx_k >= eta * diff_psi) return !((psi_alpha - psi_k < eta * diff_psi) && (psi_k > delta * psi_alpha));
    return 0;
}

}  // namespace gn
