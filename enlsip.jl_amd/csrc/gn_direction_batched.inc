// The Gauss-Newton direction check of a batch on the caller's device buffers (kernels: gn_kernels_direction_batched.hpp; the
// routines: gn_direction_check.hpp): the norms of search_direction_analys (src/enlsip_functions.jl:1222-1231) and what
// check_gn_direction (:943-1030) reads of lambda, diag_scale and cx.  The call needs and touches nothing resident: the handle lends
// its device, its stream and its record scratch, in which the call places its records (DirectionScratch: the per-problem counts and both lists up; the sums down).
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
    h->form[FORM_DIRECTION] = wave ? 1 : 0;
    GN_HIP(hipSetDevice(h->device));
    DirectionScratch D, H;
    if ((rc = place_records(h, D, H, 0, batch, 2 * l))) return rc;
    for (int64_t k = 0; k < batch; ++k) {      // not taken, or status 1: counts of 0, so that nothing of the problem is read
        const enlsip_gn_dir_state& s = state[k];
        const int tk = take_flag(take, k) && dir_status(s, m, n) != 1;
        const int64_t kp = tk ? std::max<int64_t>(dir_k_prev(s), 0) : 0;
        H.meta[k] = tk ? DirMeta{(int)s.t, (int)s.q, (int)s.dimA, (int)s.dimJ2, (int)kp, 1} : DirMeta{0, 0, 0, 0, 0, 0};
        pack_working_sets(H.list, batch, l, k, active, inactive, tk ? s.t : -1);
    }
    const WorkingSets<int> Dw(D.list, batch, l);
    DirectionArgs a{};
    a.meta = D.meta; a.act = Dw.act; a.inact = Dw.inact; a.out = D.out;
    a.count = (int)batch; a.m = (int)m; a.l = (int)l; a.t_max = (int)t_max; a.scaling = scaling != 0;
    a.b = db; a.d = dd; a.lambda = dlambda; a.diag_scale = ddiag_scale; a.cx_all = dcx_all;
    auto launch = [&](hipStream_t st) {
        if (wave) hipLaunchKernelGGL(k_dir_wave, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_dir_general, dim3((unsigned)batch), dim3(256), 0, st, a);
    };
    if ((rc = round_trip(h, D, H, launch, H.out, D.out, H.down_bytes))) return rc;
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

int enlsip_gn_get_direction_form(enlsip_gn_handle h, int* form) { return get_form(h, FORM_DIRECTION, form); }

}  // extern "C"
