// The penalty weights of the line search, one body for host and device: penalty_weight_update (src/enlsip_functions.jl:1545-1629)
// with max_norm_weight_update! (:1504-1539), euclidean_norm_weight_update (:1429-1497), min_norm_w! (:1374-1423) and assort!
// (:1344-1360), plus psi(0) of :2243 and atwa of :2268 on the new weights.
//
// The routine works on the t ACTIVE entries only, gathered in list order: position i stands for the constraint k = active[i], so
// w[i] is w[k], cxa[i] is cx[k], K3[i] is K[4][k] and ap[i] is active_Ap[i].  Nothing of the reference reads any other entry of
// those vectors except the two whole-vector copies (w = w_old[:] at :1607 / :1443, w[:] = K[4] at :1383), which the callers do:
// the host entry point in a loop, the kernels with the whole workgroup (gn_kernels_penalty_batched.hpp).  The entries of a working
// set are distinct; with a repeated entry the gathered form and the reference differ, and which copy is scattered last is open.
//
// One stated deviation: Jp and rx enter through the sums JpJp, Jprx, rxrx alone.  nrm_Jp = sqrt(JpJp), nrm_Jp^2 is nrm_Jp * nrm_Jp
// as in the Julia, Jp_rx = Jprx instead of the dot of the two normalised vectors multiplied back (:1567-1584); nrm_rx is then
// unused.  Everything on the t-vectors is literal, including the divide by nrm_Ap / nrm_cx (:1572-1582) and the multiply back at
// :1610.  All sums run in index order.  Only + - * / and sqrt are used, and every function body switches contraction off, so host
// and device give the same bits.  maximum / max / norm(., Inf) propagate a NaN as Julia's do.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GN_HD __host__ __device__
#else
#define GN_HD
#endif

namespace gn {

#define GN_PENALTY_DELTA 0.25                      // :1555
#define GN_PENALTY_EPS 2.220446049250313e-16       // eps(Float64), :1598 and :1388

// Julia's max(a, b): a NaN on either side stays
GN_HD inline double penalty_max(double a, double b) {
    if (a != a) return a;
    if (b != b) return b;
    return a > b ? a : b;
}

// x / nrm where the reference scaled the vector (nrm != 0; a NaN norm divides too), x otherwise (:1572-1582)
GN_HD inline double penalty_scaled(double x, double nrm) { return nrm != 0.0 ? x / nrm : x; }

// min_norm_w! (:1374-1423) after its w[:] = w_old (:1383), which the caller has done on w.  w, w_old: t entries by position;
// y: t entries of which the first nb_pos are set and the rest zero; pos: the positions of those (the reference keeps the
// constraint numbers k there, :1458 / :1476 / :1490, and uses them only to index w and w_old).
GN_HD inline void penalty_min_norm_w(int ctrl, double* w, const double* w_old, double* y, int t, double tau, int* pos, int nb_pos) {
#pragma clang fp contract(off)
    if (nb_pos <= 0) return;                                                     // :1384
    double y_sum = 0.0;
    for (int i = 0; i < t; ++i) y_sum = y_sum + y[i] * y[i];                     // :1385
    const double y_norm = sqrt(y_sum);                                           // :1386: sqrt of the same index-ordered sum
    if (y_norm != 0.0)                                                           // :1388-1390
        for (int i = 0; i < t; ++i) y[i] = y[i] / y_norm;
    double tau_new = tau, s = 0.0;                                               // :1391-1392
    int n_runch = nb_pos;                                                        // :1393
    bool terminated = false;
    while (!terminated) {                                                        // :1396
        tau_new = tau_new - s;                                                   // :1397
        // norm(y, Inf) over ALL t entries, the stale ones the shifts of :1412-1415 leave behind included (:1398)
        double y_inf = 0.0;
        for (int i = 0; i < t; ++i) y_inf = penalty_max(y_inf, fabs(y[i]));
        const double c = y_inf <= GN_PENALTY_EPS ? 1.0 : tau_new / y_sum;        // :1398: <=, and c = 1 for a vanishing y
        y_sum = 0.0;                                                             // :1399
        s = 0.0;
        const int i_stop = n_runch;                                              // :1400
        int k = 0;
        while (k < n_runch) {                                                    // :1402
            const int i = pos[k];
            const double buff = (c * y[k]) * y_norm;                             // :1404
            if (buff >= w_old[i]) {                                              // :1405: >=, a tie takes buff
                w[i] = buff;
                y_sum = y_sum + y[k] * y[k];
                ++k;
            } else {
                s = s + (w_old[i] * y[k]) * y_norm;                              // :1410
                --n_runch;
                for (int j = k; j < n_runch; ++j) {                              // :1412-1415; w[i] keeps what an earlier pass wrote
                    pos[j] = pos[j + 1];
                    y[j] = y[j + 1];
                }
            }
        }
        y_sum = y_sum * (y_norm * y_norm);                                       // :1418
        terminated = n_runch <= 0 || ctrl == 2 || i_stop == n_runch;             // :1419
    }
}

// assort! (:1344-1360) for one constraint: kk = K[1..4][k].  There is no break after an insertion, so the inner loop goes on
// comparing w with the entries it has just moved down (:1351-1357): a w above K[ii][k] fills every place from ii on.
GN_HD inline bool penalty_assort_entry(double wk, double* kk) {
    bool moved = false;
    for (int ii = 0; ii < 4; ++ii)
        if (wk > kk[ii]) {                                                       // :1352: strict
            for (int j = 3; j > ii; --j) kk[j] = kk[j - 1];
            kk[ii] = wk;
            moved = true;
        }
    return moved;
}

// What the whole-vector copy of the caller starts w from, by branch: K[4] in the three arms that call min_norm_w! (:1383), w_old
// otherwise (:1443, :1607)
GN_HD inline bool penalty_base_is_K4(int branch) { return branch >= 1 && branch <= 3; }

// penalty_weight_update (:1545-1629) on the gathered entries.  In: w = w_old at the active positions, ap = active_Ap (after the
// division of :2231-2233), cxa = cx at the active positions, K3 = K[4] there (norm_code 2; not read otherwise).  Out: w = the new
// weights at the active positions, scalars = dpsi0, psi0, atwa.  y, pos: scratch of t entries.  Max-norm arm (norm_code 0): it
// reads and writes K[ii][1] and reads w[i1], i1 = active[1] or 1 where that is 0 (:1515-1518), whatever the working set is:
// have_first says those exist (l > 0), w_first = w_old[i1], Kf = K[1..4][1] in and out, *Kf_moved whether :1526-1537 placed mu.
// With l == 0 the reference would throw at :1516; here w stays empty and K untouched.  Returns the branch:
//   0 norm_code 0, or t == 0;  1 ztw >= mu && dimA < t;  2 ztw < mu && dimA < t;  3 ztw < mu && dimA == t (ctrl = 1);
//   4 otherwise: nothing changes w, assort! still runs (:1493).
GN_HD inline int penalty_weights_active(int t, int dimA, int norm_code, double* w, const double* ap, const double* cxa,
                                        const double* K3, double* y, int* pos, double JpJp, double Jprx, double rxrx,
                                        bool have_first, double w_first, double* Kf, bool* Kf_moved, double* scalars) {
#pragma clang fp contract(off)
    const double delta = GN_PENALTY_DELTA;
    double apap = 0.0;
    for (int i = 0; i < t; ++i) apap = apap + ap[i] * ap[i];
    const double nrm_Ap = sqrt(apap);                                            // :1557
    double nrm_cx = 0.0;                                                         // :1558, over the first dimA active entries
    if (dimA > 0) {
        double mx = fabs(cxa[0]);
        for (int i = 1; i < dimA; ++i) mx = penalty_max(mx, fabs(cxa[i]));
        nrm_cx = penalty_max(0.0, mx);
    }
    const double nrm_Jp = sqrt(JpJp);                                            // :1559
    const double nrm_Jp2 = nrm_Jp * nrm_Jp;                                      // nrm_Jp^2 of :1598-1602
    const double Jp_rx = Jprx;                                                   // :1584, the stated deviation
    double AtwA = 0.0, BtwA = 0.0;                                               // :1587-1596
    for (int i = 0; i < dimA; ++i) {
        const double a = penalty_scaled(ap[i], nrm_Ap), c = penalty_scaled(cxa[i], nrm_cx);
        AtwA = AtwA + w[i] * (a * a);
        BtwA = BtwA + (w[i] * a) * c;
    }
    AtwA = AtwA * (nrm_Ap * nrm_Ap);
    BtwA = BtwA * (nrm_Ap * nrm_cx);
    double alpha_w = 1.0;                                                        // :1598-1601
    if (fabs(AtwA + nrm_Jp2) > GN_PENALTY_EPS) alpha_w = (-BtwA - Jp_rx) / (AtwA + nrm_Jp2);
    const double rmy = (fabs(Jp_rx + nrm_Jp2) / delta) - nrm_Jp2;                // :1603
    int branch = 0;
    *Kf_moved = false;
    if (norm_code == 0) {                                                        // :1606-1608, max_norm_weight_update! (:1504-1539)
        if (have_first) {
            const double mu = fabs(alpha_w - 1.0) <= delta ? 0.0 : rmy / nrm_Ap; // :1514: <=, and an IEEE division, also by zero
            const double previous_w = w_first;                                   // :1517
            const double nu = penalty_max(mu, Kf[3]);                            // :1518: K[4][1], whatever the active set
            for (int i = 0; i < t; ++i) w[i] = nu;                               // :1519-1522
            if (mu > previous_w)                                                 // :1524: strict
                for (int ii = 0; ii < 4; ++ii)
                    if (mu > Kf[ii]) {                                           // :1528: strict; placed once (:1533)
                        for (int j = 3; j > ii; --j) Kf[j] = Kf[j - 1];
                        Kf[ii] = mu;
                        *Kf_moved = true;
                        break;
                    }
        }
    } else if (t != 0) {                                                         // euclidean_norm_weight_update (:1429-1497)
        const double mu = rmy;
        double ztw = 0.0;                                                        // :1451: dot(z, K[4][active])
        for (int i = 0; i < t; ++i) {
            const double v = penalty_scaled(ap[i], nrm_Ap) * nrm_Ap;             // vA = Ap * nrm_Ap (:1610)
            ztw = ztw + (v * v) * K3[i];
        }
        if (ztw >= mu && dimA < t) {                                             // :1453
            branch = 1;
            int nb_pos = 0;
            double gamma = 0.0;
            for (int i = 0; i < t; ++i) {
                const double v = penalty_scaled(ap[i], nrm_Ap) * nrm_Ap, c = penalty_scaled(cxa[i], nrm_cx) * nrm_cx;
                const double y_elem = v * (v + c);                               // :1462
                y[i] = 0.0;                                                      // nb_pos <= i: a set entry is never cleared
                if (y_elem > 0) {                                                // :1463: strict
                    pos[nb_pos] = i;
                    y[nb_pos] = y_elem;
                    ++nb_pos;
                } else {
                    gamma = gamma - y_elem * K3[i];                              // :1468
                }
            }
            for (int i = 0; i < t; ++i) w[i] = K3[i];                            // :1383: from K[4], not from previous_w
            penalty_min_norm_w(2, w, K3, y, t, gamma, pos, nb_pos);
        } else if (ztw < mu && dimA < t) {                                       // :1472
            branch = 2;
            int nb_pos = 0;
            double tau = mu;
            for (int i = 0; i < t; ++i) {
                const double v = penalty_scaled(ap[i], nrm_Ap) * nrm_Ap, c = penalty_scaled(cxa[i], nrm_cx) * nrm_cx;
                const double e_elem = (-v) * c;                                  // :1479
                y[i] = 0.0;
                if (e_elem > 0) {                                                // :1480: strict
                    pos[nb_pos] = i;
                    y[nb_pos] = e_elem;
                    ++nb_pos;
                } else {
                    tau = tau - e_elem * K3[i];                                  // :1485
                }
            }
            for (int i = 0; i < t; ++i) w[i] = K3[i];                            // :1383
            penalty_min_norm_w(2, w, K3, y, t, tau, pos, nb_pos);
        } else if (ztw < mu && dimA == t) {                                      // :1489: ctrl = 1 on z itself
            branch = 3;
            for (int i = 0; i < t; ++i) {
                const double v = penalty_scaled(ap[i], nrm_Ap) * nrm_Ap;
                y[i] = v * v;
                pos[i] = i;
            }
            for (int i = 0; i < t; ++i) w[i] = K3[i];                            // :1383
            penalty_min_norm_w(1, w, K3, y, t, mu, pos, t);
        } else {
            branch = 4;                                                          // w = previous_w; assort! follows (:1493)
        }
    }
    BtwA = 0.0;                                                                  // :1614-1626
    double psi_sum = 0.0, atwa = 0.0;
    for (int i = 0; i < t; ++i) {
        const double a = penalty_scaled(ap[i], nrm_Ap), c = penalty_scaled(cxa[i], nrm_cx);
        BtwA = BtwA + (w[i] * a) * c;
        psi_sum = psi_sum + w[i] * (cxa[i] * cxa[i]);                            // :2243
        atwa = atwa + w[i] * (ap[i] * ap[i]);                                    // :2268
    }
    BtwA = BtwA * (nrm_Ap * nrm_cx);
    scalars[0] = BtwA + Jp_rx;                                                   // :1628
    scalars[1] = 0.5 * (rxrx + psi_sum);
    scalars[2] = atwa;
    return branch;
}

}  // namespace gn
