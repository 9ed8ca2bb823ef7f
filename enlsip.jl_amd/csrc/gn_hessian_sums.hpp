// The two finite-difference Hessian sums of the Newton branch, hessian_res! and hessian_cons! (src/enlsip_functions.jl:243-328),
// around the caller's evaluations: one body for host and device wherever the device needs it (the kernels:
// gn_kernels_hessian_batched.hpp).
//   hess_decode        pair index P = k (k + 1) / 2 + j  ->  (k, j), 0 <= j <= k: the reference's loop order `for k in 1:n, j in 1:k`
//   hess_eps           eps_k = max(|x[k]|, 1.0) * eps1 (:256-257), eps1 = eps(Float64)^(1/3) formed ONCE on the host (hess_eps1)
//   hess_point_entry   entry i of x_work before evaluation f_{s+1} of pair (k, j) (:259-265)
//   hess_points        the 4 npairs stencil points of a pair range (enlsip_gn_hessian_points)
//   hess_sums          Gamma[k, j] = Gamma[j, k] = r - c of a pair range from the evaluations (enlsip_gn_hessian_sums)
//
// Points.  x_work starts as a copy of x; entry j gets +-eps_j FIRST, then entry k gets +-eps_k, signs (+,+), (-,+), (+,-), (-,-) in
// the order (j, k) for s = 0..3.  On the diagonal k == j these are two successive roundings of the same entry: f2 is
// (x[k] - eps) + eps, which need not be x[k], and f1 is (x[k] + eps) + eps, which need not be x[k] + 2 eps.  Entry by entry this
// is: start from x[i], apply the j step when i == j, then the k step when i == k; the kernel writes every entry that way.
// max(|x|, 1.0) is Julia's: a NaN in x[k] gives a NaN step (fmax would give 1.0).
//
// Sums, per pair, every operation rounded on its own (fp contract off), exactly as the reference writes them:
//   s_r = sum_{i < m} (((f1[i] - f2[i]) - f3[i]) + f4[i]) * rx[i]                   :268-271
//   r   = s_r / ((4 * eps_j) * eps_k)                                              :272
//   s_c = sum_{i < t} (((g1[a] - g2[a]) - g3[a]) + g4[a]) * lambda[i], a = active[i] - 1     :317-321
//   c   = s_c / ((4.0 * eps_k) * eps_j)                                            :322   (the OTHER association: both are kept)
//   Gamma[k, j] = Gamma[j, k] = r - c                                              :393
// The two sums are taken in the order of gn_termination.hpp (term_ordered_sum / wave_ordered_sum): partial s adds the terms
// s, s + 64, ... ascending from +0.0, then the butterfly.  That is NOT the reference's left-to-right order; the difference is
// bounded by the usual summation bound.  An active entry 0 contributes nothing.  With t == 0 no term and no
// divisor of the constraint sum is formed: c = +0.0.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "gn_termination.hpp"

namespace gn {

// eps(Float64)^(1/3) of :252 / :299.  The device has no pow in this library: the kernels take the value as an argument.
inline double hess_eps1() { return pow(DBL_EPSILON, 1.0 / 3.0); }

// pairs of an n x n lower triangle
GN_HD inline long long hess_pairs(long long n) { return n * (n + 1) / 2; }

// P -> (k, j).  The floating square root is a first guess only; the two integer loops make it exact for every P < 2^61.
GN_HD inline void hess_decode(long long P, long long* k_out, long long* j_out) {
    long long k = (long long)((sqrt(8.0 * (double)P + 1.0) - 1.0) * 0.5);
    if (k < 0) k = 0;
    while (k * (k + 1) / 2 > P) --k;
    while ((k + 1) * (k + 2) / 2 <= P) ++k;
    *k_out = k;
    *j_out = P - k * (k + 1) / 2;
}

GN_HD inline double hess_eps(double xk, double eps1) {
#pragma clang fp contract(off)
    const double a = fabs(xk);
    const double mx = a > 1.0 ? a : (a != a ? a : 1.0);      // Julia's max(abs(x[k]), 1.0): a NaN stays a NaN
    return mx * eps1;
}

GN_HD inline double hess_point_entry(const double* x, long long i, long long k, long long j, int s, double eps1) {
#pragma clang fp contract(off)
    double v = x[i];
    if (i == j) {
        const double ej = hess_eps(x[j], eps1);
        v = (s & 1) ? v - ej : v + ej;
    }
    if (i == k) {
        const double ek = hess_eps(x[k], eps1);
        v = (s & 2) ? v - ek : v + ek;
    }
    return v;
}

// one term of s_r (f = residual rows, w = rx[i]) or of s_c (f = constraint rows, w = lambda[i])
GN_HD inline double hess_term(double f1, double f2, double f3, double f4, double w) {
#pragma clang fp contract(off)
    const double a = f1 - f2;
    const double b = a - f3;
    const double c = b + f4;
    return c * w;
}

GN_HD inline double hess_div_res(double s, double ej, double ek) {      // :272
#pragma clang fp contract(off)
    const double d = 4.0 * ej;
    return s / (d * ek);
}
GN_HD inline double hess_div_cons(double s, double ej, double ek) {     // :322
#pragma clang fp contract(off)
    const double d = 4.0 * ek;
    return s / (d * ej);
}

// X: (npairs, 4, n)
inline void hess_points(long long n, long long pair0, long long npairs, const double* x, double eps1, double* X) {
    for (long long q = 0; q < npairs; ++q) {
        long long k, j;
        hess_decode(pair0 + q, &k, &j);
        for (int s = 0; s < 4; ++s)
            for (long long i = 0; i < n; ++i) X[(q * 4 + s) * n + i] = hess_point_entry(x, i, k, j, s, eps1);
    }
}

struct HessHostArgs {
    long long m, n, l, t, pair0, npairs;
    const int64_t* active;      // t entries used, 1-based, 0 = padding
    const double* x;            // n
    const double* F;            // (npairs, 4, m)
    const double* rx;           // m
    const double* G;            // (npairs, 4, l)
    const double* lambda;       // t
};

// Gamma: column-major, ldg >= n; only the (k, j) and (j, k) entries of the pairs in the range are written
inline void hess_sums(const HessHostArgs& a, double eps1, double* Gamma, long long ldg) {
#pragma clang fp contract(off)
    for (long long q = 0; q < a.npairs; ++q) {
        long long k, j;
        hess_decode(a.pair0 + q, &k, &j);
        const double ek = hess_eps(a.x[k], eps1), ej = hess_eps(a.x[j], eps1);
        const double* f = a.F + q * 4 * a.m;
        const double sr = term_ordered_sum(a.m, [&](long long i) {
            return hess_term(f[i], f[a.m + i], f[2 * a.m + i], f[3 * a.m + i], a.rx[i]);
        });
        const double r = hess_div_res(sr, ej, ek);
        double c = 0.0;
        if (a.t > 0) {
            const double* g = a.G + q * 4 * a.l;
            const double sc = term_ordered_sum(a.t, [&](long long i) {
                const long long row = a.active[i];
                if (!row) return 0.0;
                return hess_term(g[row - 1], g[a.l + row - 1], g[2 * a.l + row - 1], g[3 * a.l + row - 1], a.lambda[i]);
            });
            c = hess_div_cons(sc, ej, ek);
        }
        const double v = r - c;
        Gamma[k + j * ldg] = v;
        Gamma[j + k * ldg] = v;
    }
}

}  // namespace gn
