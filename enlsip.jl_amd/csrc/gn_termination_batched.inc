// The termination test of a batch on the caller's device buffers (kernels: gn_kernels_termination_batched.hpp; the routines:
// gn_termination.hpp): what stands between new_point! and evaluate_violated_constraints in src/enlsip_functions.jl:2828-2839.  The
// call needs and touches nothing resident: the handle lends its device, its stream and its record scratch, in which the call places its records
// (TerminationScratch: the per-problem counts, psi0 and both lists up; the sums down; the partial sums of rx.rx stay on the device).
// The exit codes are formed on the host from the downloaded sums by term_decide, the one implementation of the decision.
// Included at the end of enlsip_gn.hip.

namespace {

bool termination_wave_form(int64_t n, int64_t l) { return n <= 64 && l <= 64; }

}  // namespace

extern "C" {

int enlsip_gn_minmax_lagrangian_mult(int64_t q, int64_t t, const double* lambda, const double* diag_scale, int scaling,
                                     double* sigma_min, double* lambda_abs_max) {
    if (!sigma_min || !lambda_abs_max || q < 0 || t < 0) return -2;
    if (t > q && (!lambda || !diag_scale)) return -4;
    term_minmax(q, t, lambda, diag_scale, scaling != 0, sigma_min, lambda_abs_max);
    return 0;
}

int enlsip_gn_check_termination_criteria(const enlsip_gn_term_state* s, const enlsip_gn_term_sums* v, const enlsip_gn_term_tol* tol,
                                         int64_t* exit_code) {
    if (!s || !v || !tol || !exit_code) return -2;
    *exit_code = term_decide(*s, *v, *tol);
    return 0;
}

int enlsip_gn_termination_sums(int64_t m, int64_t n, int64_t l, int64_t t, int64_t q, int64_t dimJ2, double psi0,
                               const int64_t* active, const int64_t* inactive, const double* J, int64_t ldj, const double* rx,
                               const double* cx_all, const double* x, const double* x_prev, const double* p, const double* d_gn,
                               const double* lambda, const double* cx_active, const double* diag_scale, const double* At,
                               int64_t ldat, const double* w, int scaling, const double* grad_in, const double* rx_sum_in,
                               double* grad_out, enlsip_gn_term_sums* sums) {
    if (!sums || m < 0 || l < 0 || n < 1 || t < 0 || t > l || q < 0 || q > t || dimJ2 < 0 || dimJ2 > n || ldj < m || ldat < n)
        return -2;
    if (!x || !x_prev || !p || (dimJ2 > 0 && !d_gn)) return -4;
    if (m > 0 && ((!grad_in && !J) || ((!grad_in || !rx_sum_in) && !rx))) return -4;
    if (t > 0 && (!active || !lambda || !cx_active || !diag_scale || !At || !w || !cx_all)) return -4;
    if (l - t > 0 && (!inactive || !cx_all)) return -4;
    for (int64_t i = 0; i < t; ++i)
        if (active[i] < 0 || active[i] > l) return -5;
    for (int64_t i = 0; i < l - t; ++i)
        if (inactive[i] < 0 || inactive[i] > l) return -5;
    try {
        std::vector<double> scratch((size_t)n);
        term_sums({m, n, l, t, q, dimJ2, psi0, active, inactive, J, ldj, rx, cx_all, x, x_prev, p, d_gn, lambda, cx_active, diag_scale,
                   At, ldat, w, scaling != 0, grad_in, rx_sum_in, grad_out},
                  scratch.data(), sums);
    } catch (...) {
        return 998;
    }
    return 0;
}

int enlsip_gn_termination_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t l, int64_t t_max,
                                      const enlsip_gn_term_state* state, const enlsip_gn_term_tol* tol, const int64_t* active,
                                      const int64_t* inactive, const int64_t* take, int scaling, const double* dJ, int64_t ldj,
                                      int64_t strideJ, const double* drx, const double* dcx_all, const double* dx,
                                      const double* dx_prev, const double* dp, const double* dd_gn, const double* dlambda,
                                      const double* dcx_active, const double* ddiag_scale, const double* dAt, int64_t ldat,
                                      int64_t strideAt, const double* dw, double* dgrad, enlsip_gn_term_sums* sums,
                                      int64_t* exit_code) {
    if (!h) return -1;
    GN_TRY
    int rc = check_termination(h->err, {batch, m, n, l, t_max, ldj, strideJ, ldat, strideAt}, state, active, inactive, take,
                               tol && sums && exit_code, dJ && drx, dcx_all && dw, dlambda && dcx_active && ddiag_scale && dAt,
                               dx && dx_prev && dp && dd_gn && dgrad);
    if (rc) return rc;
    const bool wave = termination_wave_form(n, l);
    const int64_t col_blocks = (n + 3) / 4;
    const int64_t nblk = m > 0 ? sum_blocks(m) : 0;
    if (!wave && !grid_fits(batch, std::max(col_blocks, nblk))) {
        h->err = "batch * max(ceil(n / 4), partial-sum workgroups) exceeds the grid";
        return -2;
    }
    h->form[FORM_TERMINATION] = wave ? 1 : 0;
    GN_HIP(hipSetDevice(h->device));
    TerminationScratch D, H;      // the partial sums: the general form's only
    if ((rc = place_records(h, D, H, wave ? 0 : nblk, batch, 2 * l))) return rc;
    for (int64_t k = 0; k < batch; ++k) {      // a problem that is not taken: counts of 0, so that nothing of its lists is read
        const int tk = take_flag(take, k);
        const enlsip_gn_term_state& s = state[k];
        H.meta[k] = tk ? TermMeta{s.psi0, (int)s.t, (int)s.q, (int)s.dimJ2, 1} : TermMeta{0.0, 0, 0, 0, 0};
        pack_working_sets(H.list, batch, l, k, active, inactive, tk ? s.t : -1);
    }
    const WorkingSets<int> Dw(D.list, batch, l);
    TerminationArgs a{};
    a.meta = D.meta; a.act = Dw.act; a.inact = Dw.inact; a.out = D.out; a.part = D.part;
    a.count = (int)batch; a.m = (int)m; a.n = (int)n; a.l = (int)l; a.t_max = (int)t_max; a.scaling = scaling != 0;
    a.nblk = (int)nblk; a.col_blocks = (int)col_blocks;
    a.J = dJ; a.ldj = ldj; a.strideJ = strideJ; a.rx = drx; a.cx_all = dcx_all; a.x = dx; a.x_prev = dx_prev; a.p = dp; a.d_gn = dd_gn;
    a.lambda = dlambda; a.cx_active = dcx_active; a.diag_scale = ddiag_scale; a.At = dAt; a.ldat = ldat; a.strideAt = strideAt;
    a.w = dw; a.grad = dgrad;
    auto launch = [&](hipStream_t st) {
        if (wave) {
            hipLaunchKernelGGL(k_term_wave, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
        } else {
            hipLaunchKernelGGL(k_term_grad, dim3((unsigned)(batch * col_blocks)), dim3(256), 0, st, a);
            if (m > 0) hipLaunchKernelGGL(k_term_rx_part, dim3((unsigned)(batch * nblk)), dim3(256), 0, st, a);
            hipLaunchKernelGGL(k_term_short, dim3((unsigned)batch), dim3(256), 0, st, a);
        }
    };
    if ((rc = round_trip(h, D, H, launch, H.out, D.out, H.down_bytes))) return rc;
    for (int64_t k = 0; k < batch; ++k) {
        if (!H.meta[k].take) continue;
        sums[k] = H.out[k];
        exit_code[k] = term_decide(state[k], sums[k], *tol);
    }
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_get_termination_form(enlsip_gn_handle h, int* form) { return get_form(h, FORM_TERMINATION, form); }

}  // extern "C"
