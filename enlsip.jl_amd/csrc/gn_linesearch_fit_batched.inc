// The polynomial fit of the line search (linesearch_constrained, src/enlsip_functions.jl:1940-2143): the host routines of
// gn_linesearch_fit.hpp exported without a handle and without a GPU, and the batched call on the caller's device buffers (kernels:
// gn_kernels_linesearch_fit_batched.hpp).  The batched call forms the six sums per taken problem on the device, brings them down in
// the one copy and runs the scalar stage on the HOST: cbrt, acos, cos and pow of the host libm and of the device library differ in
// the last place and the routine branches on their results, so a device copy could not be pinned to the host routine, and the
// step length has to reach the host for the next callback evaluation anyway.  With psi_new the merit kernels of
// gn_kernels_penalty_batched.hpp run on (drx_new, dcx_new, dw) from the same uploaded records.  The call needs or touches nothing
// resident: the handle lends its device, its stream and its record scratch, in which the call places the layout of the merit call
// with the fit's arrays (MeritScratch with fit).  Included at the end of enlsip_gn.hip.

extern "C" {

int enlsip_gn_linesearch_coefficients(int64_t m, int64_t l, int64_t t, const int64_t* active, const int64_t* inactive,
                                      int64_t n_inactive, const double* rx, const double* rx_new, const double* Jp, const double* cx,
                                      const double* cx_new, const double* Ap, const double* w, double alpha_k, double* sums) {
    if (!sums || m < 0 || m > 0x7fffffff || l < 0 || l > 0x3fffffff || t < 0 || t > l || n_inactive < 0 || n_inactive > l) return -2;
    if (m > 0 && (!rx || !rx_new || !Jp)) return -4;
    if (l > 0 && (!cx || !cx_new || !Ap || !w)) return -4;
    if ((t > 0 && !active) || (n_inactive > 0 && !inactive)) return -4;
    if (t + n_inactive != l) return -5;
    for (int64_t i = 0; i < t; ++i)
        if (active[i] < 1 || active[i] > l) return -6;
    for (int64_t i = 0; i < n_inactive; ++i)
        if (inactive[i] < 1 || inactive[i] > l) return -6;
    linesearch_coefficients(m, t, active, n_inactive, inactive, rx, rx_new, Jp, cx, cx_new, Ap, w, alpha_k, sums);
    return 0;
}

int enlsip_gn_linesearch_fit(const double* sums, double alpha_k, double x_min, double alpha_min, double alpha_max, double* out,
                             int* arm) {
    if (!out || !arm) return -2;
    if (!sums) return -4;
    double o[6];
    int which = 0;
    linesearch_fit(sums, alpha_k, x_min, alpha_min, alpha_max, o, &which);
    for (int q = 0; q < 6; ++q) out[q] = o[q];
    *arm = which;
    return 0;
}

int enlsip_gn_minrn(double x1, double y1, double x2, double y2, double x3, double y3, double alpha_min, double alpha_max,
                    double p_max, double* alpha, double* p_alpha) {
    if (!alpha || !p_alpha) return -2;
    linesearch_minrn(x1, y1, x2, y2, x3, y3, alpha_min, alpha_max, p_max, alpha, p_alpha);
    return 0;
}

int enlsip_gn_check_reduction(double psi_alpha, double psi_k, double approx_k, double eta, double diff_psi, int* likely) {
    if (!likely) return -2;
    *likely = linesearch_check_reduction(psi_alpha, psi_k, approx_k, eta, diff_psi);
    return 0;
}

int enlsip_gn_linesearch_fit_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t l, int64_t t_max, const int64_t* t,
                                         const int64_t* active, const int64_t* inactive, const int64_t* n_inactive,
                                         const int64_t* take, const double* alpha_k, const double* x_min, const double* alpha_min,
                                         const double* alpha_max, const double* drx, const double* drx_new, const double* dJp,
                                         const double* dcx, const double* dcx_new, const double* dAp, const double* dw, double* sums,
                                         double* out, int* arm, double* psi_new) {
    if (!h) return -1;
    GN_TRY
    int rc = check_shape(h->err, batch, l, t_max);
    if (rc) return rc;
    if ((rc = check_m(h->err, m))) return rc;
    if (!t || !n_inactive || !alpha_k || !x_min || !alpha_min || !alpha_max || !sums || !out || !arm) {
        h->err = "t, n_inactive, alpha_k, x_min, alpha_min, alpha_max, sums, out and arm are host arrays of batch (6 x batch) entries";
        return -4;
    }
    if (m > 0 && (!drx || !drx_new || !dJp)) { h->err = "drx, drx_new and dJp are required when m > 0"; return -4; }
    if (l > 0 && (!dcx || !dcx_new || !dAp || !dw || !inactive)) {
        h->err = "dcx, dcx_new, dAp, dw and inactive are required when l > 0";
        return -4;
    }
    if (t_max > 0 && !active) { h->err = "active is required when t_max > 0"; return -4; }
    for (int64_t k = 0; k < batch; ++k) {
        if ((rc = check_count(h->err, -5, "t", k, t[k], {0, t_max, "0..t_max"})) ||
            (rc = check_count(h->err, -5, "n_inactive", k, n_inactive[k], {0, l, "0..l"}))) return rc;
        if (t[k] + n_inactive[k] != l) { h->err = "t[" + std::to_string(k) + "] + n_inactive[" + std::to_string(k) + "] != l"; return -5; }
    }
    for (int64_t k = 0; k < batch; ++k)      // entries from 1, as enlsip_gn_linesearch_coefficients asks: the used entries are the l constraints
        if ((rc = check_list(h->err, -6, "active", k, active + k * t_max, t[k], {1, l, "1..l"})) ||
            (rc = check_list(h->err, -6, "inactive", k, inactive + k * l, n_inactive[k], {1, l, "1..l"}))) return rc;
    const int64_t nblk = sum_blocks(m);
    if (!grid_fits(batch, nblk)) { h->err = "batch * partial-sum workgroups exceeds the grid"; return -2; }
    GN_HIP(hipSetDevice(h->device));
    MeritScratch D, H;
    if ((rc = place_records(h, D, H, nblk, batch, t_max, l, true))) return rc;
    for (int64_t k = 0; k < batch; ++k) H.meta[k] = {(int)t[k], (int)n_inactive[k], take_flag(take, k), 0};
    pack_rows(H.act, active, t, batch, t_max);
    pack_rows(H.inact, inactive, n_inactive, batch, l);
    std::copy(alpha_k, alpha_k + batch, H.alpha);
    FitArgs a{};
    a.meta = D.meta; a.act = D.act; a.inact = D.inact; a.alpha = D.alpha; a.part = D.part; a.out = D.sums;
    a.count = (int)batch; a.m = (int)m; a.l = (int)l; a.t_max = (int)t_max; a.nblk = (int)nblk;
    a.rx = drx; a.rx_new = drx_new; a.Jp = dJp; a.cx = dcx; a.cx_new = dcx_new; a.Ap = dAp; a.w = dw;
    auto launch = [&](hipStream_t st) {
        if (nblk > 0) hipLaunchKernelGGL(k_fit_part, dim3((unsigned)(batch * nblk)), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_fit_total, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
        if (psi_new) launch_merit(st, {D.meta, D.act, D.inact, D.mpart, D.psi, a.count, a.m, a.l, a.t_max, a.nblk, drx_new, dcx_new, dw});
    };
    if ((rc = round_trip(h, D, H, launch, H.sums, D.sums, H.down_bytes - (psi_new ? 0 : H.psi_bytes)))) return rc;
    for (int64_t k = 0; k < batch; ++k) {
        double* o = out + 6 * k;
        double* s = sums + 6 * k;
        arm[k] = 0;
        if (H.meta[k].take) {
            for (int q = 0; q < 6; ++q) s[q] = H.sums[6 * k + q];
            linesearch_fit(s, alpha_k[k], x_min[k], alpha_min[k], alpha_max[k], o, &arm[k]);
        } else {
            for (int q = 0; q < 6; ++q) s[q] = o[q] = 0.0;
        }
    }
    if (psi_new) std::copy(H.psi, H.psi + batch, psi_new);
    return 0;
    GN_CATCH(h)
}

}  // extern "C"
