// The deletion test and the working-set edit of a batch on the caller's device buffers (kernels: gn_kernels_deletion_batched.hpp; the
// test: gn_deletion_test.hpp): check_constraint_deletion (src/enlsip_functions.jl:574-603) with the removal of :708-719 / :748-756 /
// :776-785, and the re-insertion of :731-739.  Neither call needs or touches anything resident: the handle lends its device, its
// stream and its record scratch, in which each call places t / q / take / s for itself (DeletionScratch: the records up, the
// decisions down; the restore brings nothing down).  Included at the end of enlsip_gn.hip.

namespace {

// the checks both calls share; anything wrong is reported before a launch.  n is not bounded: rows are strided by thread
int deletion_check_shape(enlsip_gn_handle h, int64_t batch, int64_t n, int64_t t_max, const int64_t* t, const double* dlambda,
                         const double* ddiag_scale, const double* dAt, int64_t ldat, int64_t strideAt, const double* dcx) {
    int rc;
    if ((rc = check_batch(h->err, batch)) || (rc = check_n(h->err, n)) || (rc = check_t_max(h->err, t_max))) return rc;
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
    for (int64_t k = 0; k < batch; ++k)      // per problem: the lower k wins
        if ((rc = check_count(h->err, -5, "t", k, t[k], {0, t_max, "0..t_max"})) ||
            (rc = check_count(h->err, -6, "q", k, q[k], {0, t[k], "0..t[k]"}))) return rc;
    if (t_max == 0) {      // no constraint anywhere: nothing to test
        std::fill(s, s + batch, (int64_t)0);
        return 0;
    }
    GN_HIP(hipSetDevice(h->device));
    DeletionScratch D, H;
    if ((rc = place_records(h, D, H, 0, batch, (int64_t)0))) return rc;
    for (int64_t k = 0; k < batch; ++k) H.meta[k] = {(int)t[k], (int)q[k], take_flag(take, k), 0};
    DeletionArgs a = deletion_args(batch, n, t_max, scaling, dlambda, ddiag_scale, dgrad_res, dAt, ldat, strideAt, dcx, dsaved);
    a.meta = D.meta; a.s_out = D.out;
    const bool wave = deletion_wave_form(n, t_max);
    h->form[FORM_DELETION] = wave ? 1 : 0;
    auto launch = [&](hipStream_t st) {
        if (wave) hipLaunchKernelGGL(k_delete_wave, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_delete_general, dim3((unsigned)batch), dim3(256), 0, st, a);
    };
    if ((rc = round_trip(h, D, H, launch, H.out, D.out, H.down_bytes))) return rc;
    std::copy(H.out, H.out + batch, s);
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
        const int64_t hi = s[k] != 0 ? t_max - 1 : t_max;      // a row that comes back needs room
        if ((rc = check_count(h->err, -5, "t", k, t[k], {0, hi, "0..t_max (0..t_max-1 where a row comes back)"})) ||
            (rc = check_count(h->err, -7, "s", k, s[k], {0, t[k] + 1, "0..t[k]+1"}))) return rc;
        any = any || s[k] != 0;
    }
    if (!any) return 0;
    if (!dsaved) { h->err = "dsaved is NULL while some s[k] != 0"; return -12; }
    GN_HIP(hipSetDevice(h->device));
    DeletionScratch D, H;
    if ((rc = place_records(h, D, H, 0, batch, (int64_t)0))) return rc;
    for (int64_t k = 0; k < batch; ++k) H.meta[k] = {(int)t[k], 0, 1, (int)s[k]};
    DeletionArgs a = deletion_args(batch, n, t_max, 0, dlambda, ddiag_scale, nullptr, dAt, ldat, strideAt, dcx, (double*)dsaved);
    a.meta = D.meta;
    const bool wave = deletion_wave_form(n, t_max);
    h->form[FORM_DELETION] = wave ? 1 : 0;
    return round_trip(h, D, H, [&](hipStream_t st) {      // nothing comes down
        if (wave) hipLaunchKernelGGL(k_restore_wave, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_restore_general, dim3((unsigned)batch), dim3(256), 0, st, a);
    });
    GN_CATCH(h)
}

int enlsip_gn_get_deletion_form(enlsip_gn_handle h, int* form) { return get_form(h, FORM_DELETION, form); }

}  // extern "C"
