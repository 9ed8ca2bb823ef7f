// The penalty weights and the merit function of a batch on the caller's device buffers (kernels: gn_kernels_penalty_batched.hpp;
// the routine: gn_penalty_weights.hpp): penalty_weight_update (src/enlsip_functions.jl:1545-1629) with psi(0) of :2243 and atwa of
// :2268, and psi of :1307-1340 on evaluated trial points.  Neither call needs or touches anything resident: the handle lends its
// device, its stream and its record scratch, in which each call places the host records, the partial sums and the scalars
// (PenaltyScratch, MeritScratch).  Included at the end of enlsip_gn.hip.

namespace {

bool penalty_wave_form(int64_t t_max, int64_t l) { return t_max <= 64 && l <= 64; }

static_assert(PW_MAX_T == BATCH_MAX_T, "check_t_max bounds t_max by the LDS copies of k_penalty");

// psi of (a.rx, a.cx, a.w) on uploaded records: the launch pair of the merit call and of the fit call's psi_new
void launch_merit(hipStream_t st, const MeritArgs& a) {
    if (a.nblk > 0) hipLaunchKernelGGL(k_merit_part, dim3((unsigned)((int64_t)a.count * a.nblk)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_merit_total, dim3((unsigned)((a.count + 3) / 4)), dim3(256), 0, st, a);
}

}  // namespace

extern "C" {

int enlsip_gn_penalty_weight_update(int64_t l, int64_t t, const int64_t* active, int64_t dimA, int norm_code, const double* w_old,
                                    const double* active_Ap, const double* cx, double JpJp, double Jprx, double rxrx, double* K,
                                    double* w, double* scalars, int* branch) {
    if (!scalars || !branch || l < 0 || l > 0x3fffffff || t < 0 || t > l || dimA < 0 || dimA > t || (norm_code != 0 && norm_code != 2))
        return -2;
    if (l > 0 && (!K || !w)) return -2;
    if (l > 0 && !w_old) return -4;
    if (t > 0 && (!active || !active_Ap || !cx)) return -4;
    for (int64_t i = 0; i < t; ++i)
        if (active[i] < 1 || active[i] > l) return -5;
    try {
        std::vector<double> buf((size_t)t * 5);
        std::vector<int> pos((size_t)t);
        double *wa = buf.data(), *ap = wa + t, *cxa = ap + t, *K3 = cxa + t, *y = K3 + t;
        const bool euclid = norm_code != 0;
        for (int64_t i = 0; i < t; ++i) {
            const int64_t j = active[i] - 1;
            wa[i] = w_old[j];
            ap[i] = active_Ap[i];
            cxa[i] = cx[j];
            K3[i] = euclid ? K[3 * l + j] : 0.0;
        }
        double Kf[4] = {0.0, 0.0, 0.0, 0.0};
        double w_first = 0.0;
        if (!euclid && l > 0) {
            w_first = w_old[t > 0 ? active[0] - 1 : 0];                          // :1515-1517: active[1] == 0 reads w[1]
            for (int ii = 0; ii < 4; ++ii) Kf[ii] = K[ii * l];
        }
        bool moved = false;
        const int br = penalty_weights_active((int)t, (int)dimA, norm_code, wa, ap, cxa, K3, y, pos.data(), JpJp, Jprx, rxrx, l > 0,
                                              w_first, Kf, &moved, scalars);
        const double* base = penalty_base_is_K4(br) ? K + 3 * l : w_old;         // :1383 / :1443, :1607
        if (base != w)
            for (int64_t j = 0; j < l; ++j) w[j] = base[j];
        for (int64_t i = 0; i < t; ++i) {
            const int64_t j = active[i] - 1;
            w[j] = wa[i];
            if (euclid) {                                                        // assort! (:1493)
                double kk[4] = {K[j], K[l + j], K[2 * l + j], K[3 * l + j]};
                if (penalty_assort_entry(wa[i], kk))
                    for (int ii = 0; ii < 4; ++ii) K[ii * l + j] = kk[ii];
            }
        }
        if (moved)
            for (int ii = 0; ii < 4; ++ii) K[ii * l] = Kf[ii];
        *branch = br;
    } catch (...) {
        return 998;
    }
    return 0;
}

int enlsip_gn_penalty_weights_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t l, int64_t t_max, const int64_t* t,
                                          const int64_t* dimA, const int64_t* active, const int64_t* take, int norm_code, int scaling,
                                          const double* dw_old, const double* dactive_Ap, const double* ddiag_scale,
                                          const double* dcx, double* dK, const double* sums, double* dw, double* scalars,
                                          int* branch) {
    if (!h) return -1;
    GN_TRY
    int rc = check_shape(h->err, batch, l, t_max);
    if (rc) return rc;
    if (norm_code != 0 && norm_code != 2) { h->err = "norm_code must be 0 or 2"; return -3; }
    if (!t || !dimA || !sums || !scalars || !branch) {
        h->err = "t, dimA, sums, scalars and branch are host arrays of batch (3 x batch) entries";
        return -4;
    }
    if (l > 0 && (!dw_old || !dK || !dw)) { h->err = "dw_old, dK and dw are required when l > 0"; return -4; }
    if (t_max > 0 && (!active || !dactive_Ap || !dcx)) { h->err = "active, dactive_Ap and dcx are required when t_max > 0"; return -4; }
    if (t_max > 0 && scaling != 0 && !ddiag_scale) { h->err = "ddiag_scale is required when scaling is on and t_max > 0"; return -4; }
    for (int64_t k = 0; k < batch; ++k)      // every t[k] before any dimA[k] or list
        if ((rc = check_count(h->err, -5, "t", k, t[k], {0, t_max, "0..t_max"}))) return rc;
    for (int64_t k = 0; k < batch; ++k)      // entries from 1: the kernel gathers w_old[j - 1] for every used entry
        if ((rc = check_count(h->err, -6, "dimA", k, dimA[k], {0, t[k], "0..t[k]"})) ||
            (rc = check_list(h->err, -6, "active", k, active + k * t_max, t[k], {1, l, "1..l"}))) return rc;
    const bool wave = penalty_wave_form(t_max, l);
    h->form[FORM_PENALTY] = wave ? 1 : 0;
    GN_HIP(hipSetDevice(h->device));
    PenaltyScratch D, H;
    if ((rc = place_records(h, D, H, 0, batch, t_max))) return rc;
    for (int64_t k = 0; k < batch; ++k)
        H.meta[k] = {{sums[3 * k], sums[3 * k + 1], sums[3 * k + 2]}, (int)t[k], (int)dimA[k], take_flag(take, k), 0};
    pack_rows(H.list, active, t, batch, t_max);
    PenaltyArgs a{};
    a.meta = D.meta; a.list = D.list; a.out = D.out;
    a.count = (int)batch; a.l = (int)l; a.t_max = (int)t_max; a.norm_code = norm_code; a.scaling = scaling != 0;
    a.w_old = dw_old; a.active_Ap = dactive_Ap; a.diag_scale = ddiag_scale; a.cx = dcx; a.K = dK; a.w = dw;
    auto launch = [&](hipStream_t st) {
        if (wave) hipLaunchKernelGGL((k_penalty<64, 64>), dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_penalty<256, PW_MAX_T>), dim3((unsigned)batch), dim3(256), 0, st, a);
    };
    if ((rc = round_trip(h, D, H, launch, H.out, D.out, H.down_bytes))) return rc;
    for (int64_t k = 0; k < batch; ++k) {
        const bool taken = H.meta[k].take != 0;
        for (int q = 0; q < 3; ++q) scalars[3 * k + q] = taken ? H.out[k].scalars[q] : 0.0;
        branch[k] = taken ? H.out[k].branch : 0;
    }
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_get_penalty_form(enlsip_gn_handle h, int* form) { return get_form(h, FORM_PENALTY, form); }

int enlsip_gn_merit_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t l, int64_t t_max, const int64_t* t,
                                const int64_t* active, const int64_t* inactive, const int64_t* n_inactive, const int64_t* take,
                                const double* drx, const double* dcx, const double* dw, double* psi) {
    if (!h) return -1;
    GN_TRY
    int rc = check_shape(h->err, batch, l, t_max);
    if (rc) return rc;
    if ((rc = check_m(h->err, m))) return rc;
    if (!t || !n_inactive || !psi) { h->err = "t, n_inactive and psi are host arrays of batch entries"; return -4; }
    if (m > 0 && !drx) { h->err = "drx is required when m > 0"; return -4; }
    if (l > 0 && (!dcx || !dw || !inactive)) { h->err = "dcx, dw and inactive are required when l > 0"; return -4; }
    if (t_max > 0 && !active) { h->err = "active is required when t_max > 0"; return -4; }
    for (int64_t k = 0; k < batch; ++k)
        if ((rc = check_count(h->err, -5, "t", k, t[k], {0, t_max, "0..t_max"})) ||
            (rc = check_count(h->err, -5, "n_inactive", k, n_inactive[k], {0, l, "0..l"}))) return rc;
    for (int64_t k = 0; k < batch; ++k)      // entries from 0: a 0 is padding to k_merit_total
        if ((rc = check_list(h->err, -6, "active", k, active + k * t_max, t[k], {0, l, "0..l"})) ||
            (rc = check_list(h->err, -6, "inactive", k, inactive + k * l, n_inactive[k], {0, l, "0..l"}))) return rc;
    const int64_t nblk = sum_blocks(m);
    if (!grid_fits(batch, nblk)) { h->err = "batch * partial-sum workgroups exceeds the grid"; return -2; }
    GN_HIP(hipSetDevice(h->device));
    MeritScratch D, H;
    if ((rc = place_records(h, D, H, nblk, batch, t_max, l, false))) return rc;
    for (int64_t k = 0; k < batch; ++k) H.meta[k] = {(int)t[k], (int)n_inactive[k], take_flag(take, k), 0};
    pack_rows(H.act, active, t, batch, t_max);
    pack_rows(H.inact, inactive, n_inactive, batch, l);
    const MeritArgs a{D.meta, D.act, D.inact, D.mpart, D.psi, (int)batch, (int)m, (int)l, (int)t_max, (int)nblk, drx, dcx, dw};
    if ((rc = round_trip(h, D, H, [&](hipStream_t st) { launch_merit(st, a); }, H.psi, D.psi, H.down_bytes))) return rc;
    std::copy(H.psi, H.psi + batch, psi);
    return 0;
    GN_CATCH(h)
}

}  // extern "C"
