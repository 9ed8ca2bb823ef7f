// The dimension choice of the subspace-minimisation branch, one body for host and device: determine_solving_dim
// (src/enlsip_functions.jl:1041-1113) with gn_previous_step (:909-932) and subspace_min_previous_step (:864-904), and the lines of
// choose_subspace_dimensions (:1118-1176) that go around them.  Line for line against the reference, except that
//   - eta (:1055, :1104-1109) is not computed: its only caller discards it (:1150, :1169) — so a restart reads nothing of tau,
//     also where the reference's eta would (previous_dimR - 1 > rankR);
//   - where Julia would throw a BoundsError the routine returns CHOICE_OUT_OF_BOUNDS BEFORE the read;
//   - y and diag(R) are scaled by exact powers of two in the psi loop (:1077-1086) so that sqrt(dsum) * |R[i,i]| neither
//     overflows nor underflows for data far from 1 (the rescue route's problems); the decisions are those of the unscaled data.
// Single-threaded: on the device one lane runs it on LDS copies of y and diag(R) (gn_kernels_subspace_batched.hpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GN_HD __host__ __device__
#else
#define GN_HD
#endif

namespace gn {

enum { CHOICE_OK = 0, CHOICE_OUT_OF_BOUNDS = 5 };

// norm([a, b]) of :1067-1068
GN_HD inline double choice_norm2(double a, double b) { return hypot(a, b); }

// gn_previous_step (:909-932); tau, rho: 0-based arrays of pseudo_rank entries, every index it reads lies in 1 .. pseudo_rank - 1
GN_HD inline long long choice_gn_previous_step(const double* tau, double tau_prk, long long mindim, const double* rho, double rho_prk,
                                               long long pseudo_rank) {
    const double tau_max = 2e-1, rho_min = 5e-1;                                             // :918
    const long long pm1 = pseudo_rank - 1;
    if (mindim > pm1) return mindim;                                                         // :920-921
    long long k = pm1;
    while ((tau[k - 1] >= tau_max * tau_prk || rho[k - 1] <= rho_min * rho_prk) && k > mindim) --k;      // :924-926
    return k > mindim ? k : (mindim > pm1 ? mindim : pm1);                                   // :928
}

// subspace_min_previous_step (:864-904), entered with previous_dimR > 0 and != pseudo_rk; tau, rho have pseudo_rk entries.
// *bad_step (may be null): whether the test of :879-881 held
GN_HD inline int choice_subspace_min_previous_step(const double* tau, const double* rho, double rho_prk, double c1, long long pseudo_rk,
                                                   long long previous_dimR, double progress, double predicted_linear_progress,
                                                   double prelin_previous_dim, double previous_alpha, long long* suggested_dim,
                                                   int* bad_step) {
    const double stepb = 2e-1, pgb1 = 3e-1, pgb2 = 1e-1, predb = 7e-1, rlenb = 2.0, c2 = 1e2;      // :878
    const bool bad = previous_alpha < stepb && progress <= pgb1 * predicted_linear_progress * predicted_linear_progress &&
                     progress <= pgb2 * prelin_previous_dim * prelin_previous_dim;                  // :879-881
    if (bad_step) *bad_step = bad ? 1 : 0;
    if (bad) {
        const long long dim = previous_dimR - 1 > 1 ? previous_dimR - 1 : 1;                       // :884
        if (previous_dimR > 1) {
            if (dim > pseudo_rk) return CHOICE_OUT_OF_BOUNDS;                                       // rho[dim], :885
            if (rho[dim - 1] > c1 * rho_prk) { *suggested_dim = dim; return CHOICE_OK; }
        }
    }
    const long long dim = previous_dimR;                                                            // :890
    if (previous_dimR < pseudo_rk && ((rho[dim - 1] > predb * rho_prk && rlenb * tau[dim - 1] < tau[dim]) ||
                                      c2 * tau[dim - 1] < tau[dim])) {                              // :891-893
        *suggested_dim = dim;
        return CHOICE_OK;
    }
    const long long i1 = previous_dimR - 1;                                                         // :895
    if (i1 <= 0) { *suggested_dim = pseudo_rk; return CHOICE_OK; }                                  // :896-897
    if (previous_dimR > pseudo_rk) return CHOICE_OUT_OF_BOUNDS;      // the comprehension of :899 reads rho[i1 .. previous_dimR], all of them
    *suggested_dim = pseudo_rk;
    for (long long i = i1; i <= previous_dimR; ++i)
        if (rho[i - 1] > predb * rho_prk) { *suggested_dim = i; break; }                            // minimum(buff), :899-900
    return CHOICE_OK;
}

// 2^-e with e the exponent of the largest |x[i*s]|, i < len (1 when that is 0 or not finite): an exact scaling to about 1
GN_HD inline double choice_pow2_scale(const double* x, long long s, long long len) {
    double mx = 0.0;
    for (long long i = 0; i < len; ++i) mx = fmax(mx, fabs(x[i * s]));
    if (!(mx > 0.0) || !(mx <= 1.7976931348623157e308)) return 1.0;
    return scalbn(1.0, -ilogb(mx));
}

// determine_solving_dim (:1041-1113).  diagR: R[i,i] at diagR[i*sR]; y: at least rankR entries; tau, rho: workspace of rankR
// doubles each (l_estim_sd, l_estim_righthand).  branch (may be null): 0 none (rankR == 0), 1 gn_previous_step, 2
// subspace_min_previous_step with the bad-step test false, 3 with it true, 4 restart.
GN_HD inline int choice_determine_solving_dim(long long previous_dimR, long long rankR, double predicted_linear_progress,
                                              double obj_progress, double prelin_previous_dim, const double* diagR, long long sR,
                                              const double* y, double previous_alpha, bool restart, double* tau, double* rho,
                                              long long* newdim, int* branch) {
    const double c1 = 0.1;                                                                          // :1053
    *newdim = rankR;                                                                                // :1054
    long long mindim = 1;                                                                           // :1056
    if (branch) *branch = 0;
    if (rankR <= 0) return CHOICE_OK;                                                               // :1058
    tau[0] = fabs(y[0]);                                                                            // :1060
    rho[0] = fabs(y[0] / diagR[0]);                                                                 // :1061
    for (long long i = 1; i < rankR; ++i) {                                                         // :1064-1069
        rho[i] = choice_norm2(rho[i - 1], y[i] / diagR[i * sR]);
        tau[i] = choice_norm2(tau[i - 1], y[i]);
    }
    const double nrm_sd = tau[rankR - 1], nrm_rh = rho[rankR - 1];                                  // :1072-1073
    // lowest possible dimension (:1077-1086); a strict > keeps the first maximiser
    const double sy = choice_pow2_scale(tau, 1, rankR), sr = choice_pow2_scale(diagR, sR, rankR);
    double dsum = 0.0, psimax = 0.0;
    for (long long i = 0; i < rankR; ++i) {
        const double l = tau[i] * sy;
        dsum += l * l;
        const double psi = sqrt(dsum) * fabs(diagR[i * sR] * sr);
        if (psi > psimax) { psimax = psi; mindim = i + 1; }
    }
    if (!restart) {                                                                                 // :1089
        long long suggested = rankR;
        if (previous_dimR == rankR || previous_dimR <= 0) {                                         // :1090-1092
            suggested = choice_gn_previous_step(tau, nrm_sd, mindim, rho, nrm_rh, rankR);
            if (branch) *branch = 1;
        } else {                                                                                    // :1094-1098
            int bad = 0;
            const int rc = choice_subspace_min_previous_step(tau, rho, nrm_rh, c1, rankR, previous_dimR, obj_progress,
                                                             predicted_linear_progress, prelin_previous_dim, previous_alpha, &suggested, &bad);
            if (branch) *branch = bad ? 3 : 2;
            if (rc) return rc;
        }
        *newdim = mindim > suggested ? mindim : suggested;                                          // :1100
    } else {
        const long long lo = rankR < previous_dimR ? rankR : previous_dimR;
        *newdim = lo > 0 ? lo : 0;                                                                  // :1103
        if (branch) *branch = 4;
    }
    return CHOICE_OK;
}

// Whether the choice is certain to run out of bounds, from what the host knows before any launch (the remaining case,
// previous_dimR == rankR + 1 after a short step, depends on the bad-step test and is found where the data are)
GN_HD inline bool choice_certainly_out_of_bounds(long long previous_dimR, long long rankR, double previous_alpha, bool restart) {
    if (restart || rankR <= 0 || previous_dimR <= rankR) return false;
    return previous_dimR > rankR + 1 || !(previous_alpha < 2e-1);
}

// the max of :1171-1174
GN_HD inline bool choice_keeps_previous(double previous_alpha, bool restart) { return !restart && previous_alpha >= 0.2; }      // alpha_low, :1133

}  // namespace gn
