// The constraint deletion test of update_working_set, one body for host and device: check_constraint_deletion
// (src/enlsip_functions.jl:574-603).  Line for line against the reference:
//   - lambda_max is maximum(abs, lambda) over ALL t entries (:585) and propagates a NaN as Julia's maximum does: with a NaN in
//     lambda sq_rel is NaN, every comparison of :593 is false and so is the gate of :598, hence s = 0;
//   - row_i is an IEEE division when scaling is on and the product row_i * lambda[i] is formed after it (:592-593), so the
//     decision is that of the host on the same bytes;
//   - both tests of :593 are <=: among equal minima the LAST index wins.
// Single-threaded: on the device one lane runs it on LDS copies of lambda and diag_scale (gn_kernels_deletion_batched.hpp, general
// form); the wave-per-problem form there reaches the same s by reductions (the proof is next to it).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GN_HD __host__ __device__
#else
#define GN_HD
#endif

namespace gn {

// sqrt(eps(Float64)) = 2^-26 (:586)
#define GN_DELETION_SQRT_EPS 1.4901161193847656e-08

// maximum(abs, lambda) of :585, 1.0 for an empty lambda; a NaN stays
GN_HD inline double deletion_lambda_max(const double* lambda, long long t) {
    if (t <= 0) return 1.0;
    double mx = fabs(lambda[0]);
    for (long long i = 1; i < t; ++i) {
        const double v = fabs(lambda[i]);
        if (mx != mx) break;
        if (v != v || v > mx) mx = v;
    }
    return mx;
}

// check_constraint_deletion (:574-603): the 1-based index of the constraint to delete, 0 for none.  lambda, diag_scale: t entries
// (not read when t <= q).
GN_HD inline long long deletion_check(long long q, long long t, const double* lambda, const double* diag_scale, bool scaling,
                                      double grad_res) {
    const double delta = 10.0;                                                   // :583
    long long s = 0;                                                             // :587
    if (t > q) {                                                                 // :589
        // lambda_max and sq_rel are read inside this branch only: they are formed here
        const double lambda_max = deletion_lambda_max(lambda, t);                // :585
        const double sq_rel = GN_DELETION_SQRT_EPS * lambda_max;                 // :586
        double e = sq_rel;                                                       // :590
        for (long long i = q + 1; i <= t; ++i) {                                 // :591
            const double row_i = scaling ? 1.0 / diag_scale[i - 1] : diag_scale[i - 1];      // :592
            const double v = row_i * lambda[i - 1];
            if (v <= sq_rel && v <= e) {                                         // :593
                e = v;                                                           // :594
                s = i;                                                           // :595
            }
        }
        if (grad_res > -e * delta) s = 0;                                        // :598-600
    }
    return s;
}

}  // namespace gn
