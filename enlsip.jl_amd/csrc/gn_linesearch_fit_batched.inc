// The polynomial fit of the line search (linesearch_constrained, src/enlsip_functions.jl:1940-2143): the host routines of
// gn_linesearch_fit.hpp exported without a handle and without a GPU, and the batched call on the caller's device buffers (kernels:
// gn_kernels_linesearch_fit_batched.hpp).  The batched call forms the six sums per taken problem on the device, brings them down in
// the one copy and runs the scalar stage on the HOST: cbrt, acos, cos and pow of the host libm and of the device library differ in
// the last place and the routine branches on their results, so a device copy could not be pinned to the host routine, and the
// step length has to reach the host for the next callback evaluation anyway.  With psi_new the merit kernels of
// gn_kernels_penalty_batched.hpp run on (drx_new, dcx_new, dw) from the same uploaded records.  The call needs or touches nothing
// resident: the handle lends its device, its stream and the scratch of the merit call.  Included at the end of enlsip_gn.hip.

namespace {

// one call's records: up goes [meta | act | inact | alpha] in one copy, down comes [sums | psi] in one copy; the partial sums stay
// on the device (the pinned side has none)
struct FitScratch {
    MeritMeta* meta = nullptr;
    int *act = nullptr, *inact = nullptr;
    double *alpha = nullptr, *sums = nullptr, *psi = nullptr, *part = nullptr, *mpart = nullptr;
    void carve(Carver& c, int64_t batch, int64_t t_max, int64_t l, int64_t nblk) {
        c.take(meta, "meta", (size_t)batch, 8);
        c.take(act, "act", (size_t)batch * (size_t)t_max);
        c.take(inact, "inact", (size_t)batch * (size_t)l);
        c.take(alpha, "alpha", (size_t)batch);
        c.take(sums, "sums", (size_t)batch * 6);
        c.take(psi, "psi", (size_t)batch);
        c.take(part, "part", (size_t)batch * (size_t)nblk * 6);
        c.take(mpart, "mpart", (size_t)batch * (size_t)nblk);
    }
    // meta .. alpha are adjacent in both layouts (the padding in front of alpha is the same on both sides)
    size_t up_bytes(int64_t batch) const { return (size_t)((const char*)(alpha + batch) - (const char*)meta); }
};

}  // namespace

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
    int rc = penalty_check_shape(h, batch, l, t_max);
    if (rc) return rc;
    if (m < 0 || m > 0x7fffffff) { h->err = "m must be in 0..2^31-1"; return -3; }
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
        if (t[k] < 0 || t[k] > t_max) { h->err = "t[" + std::to_string(k) + "] outside 0..t_max"; return -5; }
        if (n_inactive[k] < 0 || n_inactive[k] > l) { h->err = "n_inactive[" + std::to_string(k) + "] outside 0..l"; return -5; }
        if (t[k] + n_inactive[k] != l) { h->err = "t[" + std::to_string(k) + "] + n_inactive[" + std::to_string(k) + "] != l"; return -5; }
    }
    for (int64_t k = 0; k < batch; ++k) {
        const int64_t* ra = active + k * t_max;
        for (int64_t i = 0; i < t[k]; ++i)
            if (ra[i] < 1 || ra[i] > l) {
                h->err = "active[" + std::to_string(k) + "][" + std::to_string(i) + "] outside 1..l";
                return -6;
            }
        const int64_t* ri = inactive + k * l;
        for (int64_t i = 0; i < n_inactive[k]; ++i)
            if (ri[i] < 1 || ri[i] > l) {
                h->err = "inactive[" + std::to_string(k) + "][" + std::to_string(i) + "] outside 1..l";
                return -6;
            }
    }
    const int64_t nblk = std::min<int64_t>(LS_MAX_NBLK, (m + LS_SUM_ROWS - 1) / LS_SUM_ROWS);
    if (batch * std::max<int64_t>(nblk, 1) > 0x7fffffff) { h->err = "batch * partial-sum workgroups exceeds the grid"; return -2; }
    GN_HIP(hipSetDevice(h->device));
    FitScratch D, H;
    rc = place_dev(h, h->pen_scr, D, batch, t_max, l, nblk);
    if (rc) return rc;
    rc = place_pinned(h, h->h_pen, H, batch, t_max, l, (int64_t)0);
    if (rc) return rc;
    for (int64_t k = 0; k < batch; ++k) {
        H.meta[k] = {(int)t[k], (int)n_inactive[k], (take && take[k] == 0) ? 0 : 1, 0};
        int* da = H.act + k * t_max;
        for (int64_t i = 0; i < t_max; ++i) da[i] = i < t[k] ? (int)active[k * t_max + i] : 0;
        int* di = H.inact + k * l;
        for (int64_t i = 0; i < l; ++i) di[i] = i < n_inactive[k] ? (int)inactive[k * l + i] : 0;
        H.alpha[k] = alpha_k[k];
    }
    hipStream_t st = h->stream;
    GN_HIP(hipMemcpyAsync(D.meta, H.meta, H.up_bytes(batch), hipMemcpyHostToDevice, st));
    FitArgs a{};
    a.meta = D.meta; a.act = D.act; a.inact = D.inact; a.alpha = D.alpha; a.part = D.part; a.out = D.sums;
    a.count = (int)batch; a.m = (int)m; a.l = (int)l; a.t_max = (int)t_max; a.nblk = (int)nblk;
    a.rx = drx; a.rx_new = drx_new; a.Jp = dJp; a.cx = dcx; a.cx_new = dcx_new; a.Ap = dAp; a.w = dw;
    const unsigned waves = (unsigned)((batch + 3) / 4);
    if (nblk > 0) hipLaunchKernelGGL(k_fit_part, dim3((unsigned)(batch * nblk)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_fit_total, dim3(waves), dim3(256), 0, st, a);
    if (psi_new) {
        MeritArgs ma{};
        ma.meta = D.meta; ma.act = D.act; ma.inact = D.inact; ma.part = D.mpart; ma.out = D.psi;
        ma.count = (int)batch; ma.m = (int)m; ma.l = (int)l; ma.t_max = (int)t_max; ma.nblk = (int)nblk;
        ma.rx = drx_new; ma.cx = dcx_new; ma.w = dw;
        if (nblk > 0) hipLaunchKernelGGL(k_merit_part, dim3((unsigned)(batch * nblk)), dim3(256), 0, st, ma);
        hipLaunchKernelGGL(k_merit_total, dim3(waves), dim3(256), 0, st, ma);
    }
    GN_HIP(hipGetLastError());
    // sums and psi are adjacent in both layouts: one copy
    GN_HIP(hipMemcpyAsync(H.sums, D.sums, (size_t)batch * (psi_new ? 7 : 6) * sizeof(double), hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));
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
