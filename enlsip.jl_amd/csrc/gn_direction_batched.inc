// The Gauss-Newton direction check of a batch on the caller's device buffers (kernels: gn_kernels_direction_batched.hpp; the
// routines: gn_direction_check.hpp): the norms of search_direction_analys (src/enlsip_functions.jl:1222-1231) and what
// check_gn_direction (:943-1030) reads of lambda, diag_scale and cx.  The call needs and touches nothing resident: the handle lends
// its device, its stream and a scratch for the records (DirectionScratch: the per-problem counts and both lists up; the sums down).
// The method codes are formed on the host from the downloaded sums by dir_decide, the one implementation of the decision.
// Included at the end of enlsip_gn.hip.

namespace {

bool direction_wave_form(int64_t m, int64_t l, int64_t t_max) { return m <= DIR_WAVE_MAX_M && l <= 64 && t_max <= 64; }

}  // namespace

extern "C" {

int enlsip_gn_check_gn_direction(const enlsip_gn_dir_state* s, const enlsip_gn_dir_sums* v, int64_t m, int64_t n,
                                 int64_t* method_code, double* beta) {
    if (!s || !v || !method_code || !beta) return -2;
    long long code;
    dir_decide(*s, *v, m, n, &code, beta);
    *method_code = code;
    return 0;
}

int enlsip_gn_direction_sums(int64_t m, int64_t n, int64_t l, const enlsip_gn_dir_state* s, const int64_t* active,
                             const int64_t* inactive, const double* b, const double* d, const double* lambda,
                             const double* diag_scale, const double* cx_all, int scaling, enlsip_gn_dir_sums* sums,
                             int64_t* status) {
    if (!s || !sums || !status || m < 0 || n < 1 || l < 0 || s->t < 0 || s->t > l || s->l != l || s->q < 0 || s->q > s->t ||
        s->dimA < 0 || s->dimA > s->t || s->dimJ2 < 0 || s->dimJ2 > m || s->prev_t < 0 || s->prev_t > l ||
        s->prev_dimJ2 < -DIR_PREV_MAX || s->prev_dimJ2 > DIR_PREV_MAX)
        return -2;
    if ((m > 0 && !d) || (s->dimA > 0 && !b) || (s->t > s->q && (!lambda || !diag_scale))) return -4;
    if (s->t > 0 && (!active || !cx_all)) return -4;
    if (l - s->t > 0 && (!inactive || !cx_all)) return -4;
    for (int64_t i = 0; i < s->t; ++i)
        if (active[i] < 0 || active[i] > l) return -5;
    for (int64_t i = 0; i < l - s->t; ++i)
        if (inactive[i] < 0 || inactive[i] > l) return -5;
    *status = dir_status(*s, m, n);
    if (*status == 1) return 0;
    dir_sums(*s, {m, l, active, inactive, b, d, lambda, diag_scale, cx_all, scaling != 0}, sums);
    return 0;
}

int enlsip_gn_direction_check_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t l, int64_t t_max,
                                          const enlsip_gn_dir_state* state, const int64_t* active, const int64_t* inactive,
                                          const int64_t* take, int scaling, const double* db, const double* dd,
                                          const double* dlambda, const double* ddiag_scale, const double* dcx_all,
                                          enlsip_gn_dir_sums* sums, int64_t* method_code, double* beta, int64_t* status) {
    if (!h) return -1;
    GN_TRY
    int rc = check_direction(h->err, {batch, m, n, l, t_max}, state, active, inactive, take, sums && method_code && beta && status,
                             dd != nullptr, dcx_all != nullptr, db && dlambda && ddiag_scale);
    if (rc) return rc;
    const bool wave = direction_wave_form(m, l, t_max);
    h->direction_form = wave ? 1 : 0;
    GN_HIP(hipSetDevice(h->device));
    DirectionScratch D, H;
    if ((rc = place_records(h, h->dir_scr, h->h_dir, D, H, 0, batch, 2 * l))) return rc;
    std::vector<int64_t> n_act((size_t)batch), n_ina((size_t)batch);
    for (int64_t k = 0; k < batch; ++k) {      // not taken, or status 1: counts of 0, so that nothing of the problem is read
        const enlsip_gn_dir_state& s = state[k];
        const int tk = take_flag(take, k) && dir_status(s, m, n) != 1;
        const int64_t kp = tk ? std::max<int64_t>(dir_k_prev(s), 0) : 0;
        H.meta[k] = tk ? DirMeta{(int)s.t, (int)s.q, (int)s.dimA, (int)s.dimJ2, (int)kp, 1} : DirMeta{0, 0, 0, 0, 0, 0};
        n_act[k] = tk ? s.t : 0;
        n_ina[k] = tk ? l - s.t : 0;
    }
    pack_rows(H.list, active, n_act.data(), batch, l);
    pack_rows(H.list + batch * l, inactive, n_ina.data(), batch, l);
    hipStream_t st = h->stream;
    GN_HIP(hipMemcpyAsync(D.meta, H.meta, H.up_bytes, hipMemcpyHostToDevice, st));
    DirectionArgs a{};
    a.meta = D.meta; a.act = D.list; a.inact = D.list + batch * l; a.out = D.out;
    a.count = (int)batch; a.m = (int)m; a.l = (int)l; a.t_max = (int)t_max; a.scaling = scaling != 0;
    a.b = db; a.d = dd; a.lambda = dlambda; a.diag_scale = ddiag_scale; a.cx_all = dcx_all;
    if (wave) hipLaunchKernelGGL(k_dir_wave, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_dir_general, dim3((unsigned)batch), dim3(256), 0, st, a);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(H.out, D.out, H.down_bytes, hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));
    for (int64_t k = 0; k < batch; ++k) {
        if (!take_flag(take, k)) continue;
        status[k] = dir_status(state[k], m, n);
        if (status[k] == 1) continue;          // the reference throws at :1231: no sums, no code
        sums[k] = H.out[k];
        long long code;
        dir_decide(state[k], sums[k], m, n, &code, &beta[k]);
        method_code[k] = code;
    }
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_get_direction_form(enlsip_gn_handle h, int* form) {
    GN_GETTER_CHECK(h, form)
    *form = h->direction_form;
    return 0;
}

}  // extern "C"
