// The penalty weights and the merit function of a batch on the caller's device buffers (kernels: gn_kernels_penalty_batched.hpp;
// the routine: gn_penalty_weights.hpp): penalty_weight_update (src/enlsip_functions.jl:1545-1629) with psi(0) of :2243 and atwa of
// :2268, and psi of :1307-1340 on evaluated trial points.  Neither call needs or touches anything resident: the handle lends its
// device, its stream and a scratch for the host records, the partial sums and the scalars.  Included at the end of enlsip_gn.hip.

namespace {

// one call's records: up goes [meta | list] in one copy, down comes out in one copy
struct PenaltyScratch {
    PenaltyMeta* meta = nullptr;
    int* list = nullptr;
    PenaltyOut* out = nullptr;
    void carve(Carver& c, int64_t batch, int64_t t_max) {
        c.take(meta, "meta", (size_t)batch);
        c.take(list, "list", (size_t)batch * (size_t)t_max);
        c.take(out, "out", (size_t)batch, 8);
    }
    size_t up_bytes(int64_t batch, int64_t t_max) const {
        return (size_t)batch * sizeof(PenaltyMeta) + (size_t)batch * (size_t)t_max * sizeof(int);
    }
};

// the same for the merit function: [meta | act | inact] up, out down; part stays on the device (the pinned side has none)
struct MeritScratch {
    MeritMeta* meta = nullptr;
    int *act = nullptr, *inact = nullptr;
    double *out = nullptr, *part = nullptr;
    void carve(Carver& c, int64_t batch, int64_t t_max, int64_t l, int64_t nblk) {
        c.take(meta, "meta", (size_t)batch);
        c.take(act, "act", (size_t)batch * (size_t)t_max);
        c.take(inact, "inact", (size_t)batch * (size_t)l);
        c.take(out, "out", (size_t)batch, 8);
        c.take(part, "part", (size_t)batch * (size_t)nblk);
    }
    size_t up_bytes(int64_t batch, int64_t t_max, int64_t l) const {
        return (size_t)batch * sizeof(MeritMeta) + (size_t)batch * (size_t)(t_max + l) * sizeof(int);
    }
};

bool penalty_wave_form(int64_t t_max, int64_t l) { return t_max <= 64 && l <= 64; }

// the shape checks both calls share
int penalty_check_shape(enlsip_gn_handle h, int64_t batch, int64_t l, int64_t t_max) {
    if (batch < 1 || batch > 0x7fffffff) { h->err = "batch must be in 1..2^31-1"; return -2; }
    if (l < 0 || l > (1LL << 27)) { h->err = "l must be in 0..2^27"; return -3; }
    if (t_max < 0 || t_max > PW_MAX_T) { h->err = "t_max must be in 0..1024 in this build"; return -3; }
    if (t_max > l) { h->err = "t_max > l"; return -3; }
    return 0;
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
    int rc = penalty_check_shape(h, batch, l, t_max);
    if (rc) return rc;
    if (norm_code != 0 && norm_code != 2) { h->err = "norm_code must be 0 or 2"; return -3; }
    if (!t || !dimA || !sums || !scalars || !branch) {
        h->err = "t, dimA, sums, scalars and branch are host arrays of batch (3 x batch) entries";
        return -4;
    }
    if (l > 0 && (!dw_old || !dK || !dw)) { h->err = "dw_old, dK and dw are required when l > 0"; return -4; }
    if (t_max > 0 && (!active || !dactive_Ap || !dcx)) { h->err = "active, dactive_Ap and dcx are required when t_max > 0"; return -4; }
    if (t_max > 0 && scaling != 0 && !ddiag_scale) { h->err = "ddiag_scale is required when scaling is on and t_max > 0"; return -4; }
    for (int64_t k = 0; k < batch; ++k)
        if (t[k] < 0 || t[k] > t_max) { h->err = "t[" + std::to_string(k) + "] outside 0..t_max"; return -5; }
    for (int64_t k = 0; k < batch; ++k) {
        if (dimA[k] < 0 || dimA[k] > t[k]) { h->err = "dimA[" + std::to_string(k) + "] outside 0..t[k]"; return -6; }
        const int64_t* row = active + k * t_max;
        for (int64_t i = 0; i < t[k]; ++i)
            if (row[i] < 1 || row[i] > l) {
                h->err = "active[" + std::to_string(k) + "][" + std::to_string(i) + "] outside 1..l";
                return -6;
            }
    }
    const bool wave = penalty_wave_form(t_max, l);
    h->penalty_form = wave ? 1 : 0;
    GN_HIP(hipSetDevice(h->device));
    PenaltyScratch D, H;
    rc = place_dev(h, h->pen_scr, D, batch, t_max);
    if (rc) return rc;
    rc = place_pinned(h, h->h_pen, H, batch, t_max);
    if (rc) return rc;
    for (int64_t k = 0; k < batch; ++k) {
        H.meta[k] = {{sums[3 * k], sums[3 * k + 1], sums[3 * k + 2]}, (int)t[k], (int)dimA[k], (take && take[k] == 0) ? 0 : 1, 0};
        const int64_t* row = active + k * t_max;
        int* dst = H.list + k * t_max;
        for (int64_t i = 0; i < t[k]; ++i) dst[i] = (int)row[i];
        for (int64_t i = t[k]; i < t_max; ++i) dst[i] = 0;
    }
    hipStream_t st = h->stream;
    // meta and list are adjacent in both layouts (int-aligned records): one copy
    GN_HIP(hipMemcpyAsync(D.meta, H.meta, H.up_bytes(batch, t_max), hipMemcpyHostToDevice, st));
    PenaltyArgs a{};
    a.meta = D.meta; a.list = D.list; a.out = D.out;
    a.count = (int)batch; a.l = (int)l; a.t_max = (int)t_max; a.norm_code = norm_code; a.scaling = scaling != 0;
    a.w_old = dw_old; a.active_Ap = dactive_Ap; a.diag_scale = ddiag_scale; a.cx = dcx; a.K = dK; a.w = dw;
    if (wave) hipLaunchKernelGGL((k_penalty<64, 64>), dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_penalty<256, PW_MAX_T>), dim3((unsigned)batch), dim3(256), 0, st, a);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(H.out, D.out, (size_t)batch * sizeof(PenaltyOut), hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));
    for (int64_t k = 0; k < batch; ++k) {
        const bool taken = H.meta[k].take != 0;
        for (int q = 0; q < 3; ++q) scalars[3 * k + q] = taken ? H.out[k].scalars[q] : 0.0;
        branch[k] = taken ? H.out[k].branch : 0;
    }
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_get_penalty_form(enlsip_gn_handle h, int* form) {
    GN_GETTER_CHECK(h, form)
    *form = h->penalty_form;
    return 0;
}

int enlsip_gn_merit_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t l, int64_t t_max, const int64_t* t,
                                const int64_t* active, const int64_t* inactive, const int64_t* n_inactive, const int64_t* take,
                                const double* drx, const double* dcx, const double* dw, double* psi) {
    if (!h) return -1;
    GN_TRY
    int rc = penalty_check_shape(h, batch, l, t_max);
    if (rc) return rc;
    if (m < 0 || m > 0x7fffffff) { h->err = "m must be in 0..2^31-1"; return -3; }
    if (!t || !n_inactive || !psi) { h->err = "t, n_inactive and psi are host arrays of batch entries"; return -4; }
    if (m > 0 && !drx) { h->err = "drx is required when m > 0"; return -4; }
    if (l > 0 && (!dcx || !dw || !inactive)) { h->err = "dcx, dw and inactive are required when l > 0"; return -4; }
    if (t_max > 0 && !active) { h->err = "active is required when t_max > 0"; return -4; }
    for (int64_t k = 0; k < batch; ++k) {
        if (t[k] < 0 || t[k] > t_max) { h->err = "t[" + std::to_string(k) + "] outside 0..t_max"; return -5; }
        if (n_inactive[k] < 0 || n_inactive[k] > l) { h->err = "n_inactive[" + std::to_string(k) + "] outside 0..l"; return -5; }
    }
    for (int64_t k = 0; k < batch; ++k) {
        const int64_t* ra = active + k * t_max;
        for (int64_t i = 0; i < t[k]; ++i)
            if (ra[i] < 0 || ra[i] > l) {
                h->err = "active[" + std::to_string(k) + "][" + std::to_string(i) + "] outside 0..l";
                return -6;
            }
        const int64_t* ri = inactive + k * l;
        for (int64_t i = 0; i < n_inactive[k]; ++i)
            if (ri[i] < 0 || ri[i] > l) {
                h->err = "inactive[" + std::to_string(k) + "][" + std::to_string(i) + "] outside 0..l";
                return -6;
            }
    }
    const int64_t nblk = std::min<int64_t>(LS_MAX_NBLK, (m + LS_SUM_ROWS - 1) / LS_SUM_ROWS);
    if (batch * std::max<int64_t>(nblk, 1) > 0x7fffffff) { h->err = "batch * partial-sum workgroups exceeds the grid"; return -2; }
    GN_HIP(hipSetDevice(h->device));
    MeritScratch D, H;
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
    }
    hipStream_t st = h->stream;
    // meta, act and inact are adjacent in both layouts (int-aligned records): one copy
    GN_HIP(hipMemcpyAsync(D.meta, H.meta, H.up_bytes(batch, t_max, l), hipMemcpyHostToDevice, st));
    MeritArgs a{};
    a.meta = D.meta; a.act = D.act; a.inact = D.inact; a.part = D.part; a.out = D.out;
    a.count = (int)batch; a.m = (int)m; a.l = (int)l; a.t_max = (int)t_max; a.nblk = (int)nblk;
    a.rx = drx; a.cx = dcx; a.w = dw;
    if (nblk > 0) hipLaunchKernelGGL(k_merit_part, dim3((unsigned)(batch * nblk)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_merit_total, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(H.out, D.out, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));
    std::copy(H.out, H.out + batch, psi);
    return 0;
    GN_CATCH(h)
}

}  // extern "C"
