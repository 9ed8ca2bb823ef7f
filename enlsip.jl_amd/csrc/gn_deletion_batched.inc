// The deletion test and the working-set edit of a batch on the caller's device buffers (kernels: gn_kernels_deletion_batched.hpp; the
// test: gn_deletion_test.hpp): check_constraint_deletion (src/enlsip_functions.jl:574-603) with the removal of :708-719 / :748-756 /
// :776-785, and the re-insertion of :731-739.  Neither call needs or touches anything resident: the handle lends its device, its
// stream and a small scratch for t / q / take / s.  Included at the end of enlsip_gn.hip.

namespace {

enum { DEL_MAX_T = 1024 };      // t_max of this build: the LDS copies of the general form.  n is not bounded: rows are strided by thread

// the per-problem records of one call in pinned memory and on the device, the decisions behind them (hs, ds: may be null, the
// restore has none); grown, never shrunk (grow, grow_pinned)
struct DeletionScratch {
    DeletionMeta* meta = nullptr;
    int* s = nullptr;
    void carve(Carver& c, int64_t batch) { c.take(meta, "meta", (size_t)batch); c.take(s, "s", (size_t)batch); }
};
int deletion_scratch(enlsip_gn_handle h, int64_t batch, DeletionMeta** hmeta, int** hs, DeletionMeta** dmeta, int** ds) {
    DeletionScratch D, H;
    int rc = place_dev(h, h->del_scr, D, batch);
    if (rc) return rc;
    rc = place_pinned(h, h->h_del, H, batch);
    if (rc) return rc;
    *hmeta = H.meta;
    *dmeta = D.meta;
    if (hs) *hs = H.s;
    if (ds) *ds = D.s;
    return 0;
}

// the checks both calls share; anything wrong is reported before a launch
int deletion_check_shape(enlsip_gn_handle h, int64_t batch, int64_t n, int64_t t_max, const int64_t* t, const double* dlambda,
                         const double* ddiag_scale, const double* dAt, int64_t ldat, int64_t strideAt, const double* dcx) {
    if (batch < 1 || batch > 0x7fffffff) { h->err = "batch must be in 1..2^31-1"; return -2; }
    if (n < 1 || n > 0x3fffffff) { h->err = "n must be at least 1"; return -3; }
    if (t_max < 0 || t_max > DEL_MAX_T) { h->err = "t_max must be in 0..1024 in this build"; return -3; }
    if (!t) { h->err = "t is a host array of batch entries"; return -4; }
    if (t_max > 0 && (!dlambda || !ddiag_scale || !dAt || !dcx)) {
        h->err = "dlambda, ddiag_scale, dAt and dcx are required when t_max > 0";
        return -4;
    }
    if (ldat < n) { h->err = "ldat < n"; return -9; }
    if (strideAt < ldat * t_max) { h->err = "strideAt < ldat * t_max"; return -10; }
    return 0;
}

bool deletion_wave_form(int64_t n, int64_t t_max) { return n <= 64 && t_max <= 64; }

DeletionArgs deletion_args(int64_t batch, int64_t n, int64_t t_max, int scaling, double* dlambda, double* ddiag_scale,
                           const double* dgrad_res, double* dAt, int64_t ldat, int64_t strideAt, double* dcx, double* dsaved) {
    DeletionArgs a{};
    a.count = (int)batch; a.n = (int)n; a.t_max = (int)t_max; a.scaling = scaling != 0;
    a.lambda = dlambda; a.diag_scale = ddiag_scale; a.grad_res = dgrad_res;
    a.At = dAt; a.ldat = ldat; a.strideAt = strideAt; a.cx = dcx; a.saved = dsaved;
    return a;
}

}  // namespace

extern "C" {

int enlsip_gn_check_constraint_deletion(int64_t q, int64_t t, const double* lambda, const double* diag_scale, int scaling,
                                        double grad_res, int64_t* s) {
    if (!s || t < 0 || q < 0 || q > t) return -2;
    if (t > q && (!lambda || !diag_scale)) return -4;
    *s = deletion_check(q, t, lambda, diag_scale, scaling != 0, grad_res);
    return 0;
}

int enlsip_gn_delete_constraints_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t n, int64_t t_max, const int64_t* t,
                                             const int64_t* q, const int64_t* take, int scaling, double* dlambda,
                                             double* ddiag_scale, const double* dgrad_res, double* dAt, int64_t ldat,
                                             int64_t strideAt, double* dcx, double* dsaved, int64_t* s) {
    if (!h) return -1;
    GN_TRY
    int rc = deletion_check_shape(h, batch, n, t_max, t, dlambda, ddiag_scale, dAt, ldat, strideAt, dcx);
    if (rc) return rc;
    if (!q || !s) { h->err = "q and s are host arrays of batch entries"; return -4; }
    for (int64_t k = 0; k < batch; ++k) {
        if (t[k] < 0 || t[k] > t_max) { h->err = "t[" + std::to_string(k) + "] outside 0..t_max"; return -5; }
        if (q[k] < 0 || q[k] > t[k]) { h->err = "q[" + std::to_string(k) + "] outside 0..t[k]"; return -6; }
    }
    if (t_max == 0) {      // no constraint anywhere: nothing to test
        std::fill(s, s + batch, (int64_t)0);
        return 0;
    }
    GN_HIP(hipSetDevice(h->device));
    DeletionMeta *hm, *dm;
    int *hs, *dsd;
    rc = deletion_scratch(h, batch, &hm, &hs, &dm, &dsd);
    if (rc) return rc;
    for (int64_t k = 0; k < batch; ++k) hm[k] = {(int)t[k], (int)q[k], (take && take[k] == 0) ? 0 : 1, 0};
    hipStream_t st = h->stream;
    GN_HIP(hipMemcpyAsync(dm, hm, (size_t)batch * sizeof(DeletionMeta), hipMemcpyHostToDevice, st));
    DeletionArgs a = deletion_args(batch, n, t_max, scaling, dlambda, ddiag_scale, dgrad_res, dAt, ldat, strideAt, dcx, dsaved);
    a.meta = dm; a.s_out = dsd;
    const bool wave = deletion_wave_form(n, t_max);
    h->deletion_form = wave ? 1 : 0;
    if (wave) hipLaunchKernelGGL(k_delete_wave, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_delete_general, dim3((unsigned)batch), dim3(256), 0, st, a);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(hs, dsd, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));
    for (int64_t k = 0; k < batch; ++k) s[k] = hs[k];
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_restore_constraints_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t n, int64_t t_max, const int64_t* t,
                                              const int64_t* s, double* dlambda, double* ddiag_scale, double* dAt, int64_t ldat,
                                              int64_t strideAt, double* dcx, const double* dsaved) {
    if (!h) return -1;
    GN_TRY
    int rc = deletion_check_shape(h, batch, n, t_max, t, dlambda, ddiag_scale, dAt, ldat, strideAt, dcx);
    if (rc) return rc;
    if (!s) { h->err = "s is a host array of batch entries"; return -4; }
    bool any = false;
    for (int64_t k = 0; k < batch; ++k) {
        const int64_t hi = s[k] != 0 ? t_max - 1 : t_max;
        if (t[k] < 0 || t[k] > hi) {
            h->err = "t[" + std::to_string(k) + "] outside 0..t_max (0..t_max-1 where a row comes back)";
            return -5;
        }
        if (s[k] < 0 || s[k] > t[k] + 1) { h->err = "s[" + std::to_string(k) + "] outside 0..t[k]+1"; return -7; }
        any = any || s[k] != 0;
    }
    if (!any) return 0;
    if (!dsaved) { h->err = "dsaved is NULL while some s[k] != 0"; return -12; }
    GN_HIP(hipSetDevice(h->device));
    DeletionMeta *hm, *dm;
    rc = deletion_scratch(h, batch, &hm, nullptr, &dm, nullptr);
    if (rc) return rc;
    for (int64_t k = 0; k < batch; ++k) hm[k] = {(int)t[k], 0, 1, (int)s[k]};
    hipStream_t st = h->stream;
    GN_HIP(hipMemcpyAsync(dm, hm, (size_t)batch * sizeof(DeletionMeta), hipMemcpyHostToDevice, st));
    DeletionArgs a = deletion_args(batch, n, t_max, 0, dlambda, ddiag_scale, nullptr, dAt, ldat, strideAt, dcx, (double*)dsaved);
    a.meta = dm;
    const bool wave = deletion_wave_form(n, t_max);
    h->deletion_form = wave ? 1 : 0;
    if (wave) hipLaunchKernelGGL(k_restore_wave, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_restore_general, dim3((unsigned)batch), dim3(256), 0, st, a);
    GN_HIP(hipGetLastError());
    GN_HIP(hipStreamSynchronize(st));
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_get_deletion_form(enlsip_gn_handle h, int* form) {
    GN_GETTER_CHECK(h, form)
    *form = h->deletion_form;
    return 0;
}

}  // extern "C"
