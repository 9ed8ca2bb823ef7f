// The working-set additions of a batch and the rebuild of its active constraints on the caller's device buffers (kernels:
// gn_kernels_addition_batched.hpp; the routines: gn_violated_constraints.hpp): evaluate_violated_constraints
// (src/enlsip_functions.jl:608-650), active_C.cx / active_C.A of :2854-2855 and evaluate_scaling! (src/structures.jl:160-178).  The
// call needs and touches nothing resident: the handle lends its device, its stream and its record scratch, in which the call places its records
// (AdditionScratch: t, q, take, index_alpha_upp and both lists up; the lists, t, added and status down).  Included at the end of
// enlsip_gn.hip.

namespace {

bool addition_wave_form(int64_t n, int64_t l) { return n <= 64 && l <= 64; }

}  // namespace

extern "C" {

int enlsip_gn_evaluate_violated_constraints(int64_t l, int64_t n, int64_t q, int64_t* t, int64_t* active, int64_t* inactive,
                                            const double* cx, int64_t index_alpha_upp, int64_t* added, int64_t* status) {
    if (!t || !added || !status || l < 0 || n < 0 || q < 0 || q > *t || *t > l) return -2;
    if (l > 0 && (!active || !inactive || !cx)) return -4;
    if (index_alpha_upp < 0 || index_alpha_upp > l) return -5;
    for (int64_t i = 0; i < l; ++i)
        if (active[i] < 0 || active[i] > l || inactive[i] < 0 || inactive[i] > l) return -5;
    long long tt = *t;
    int add = 0;
    *status = addition_walk<int64_t>(l, n, q, &tt, active, inactive, cx, index_alpha_upp, &add);
    *t = tt;
    *added = add;
    return 0;
}

int enlsip_gn_gather_active_constraints(int64_t l, int64_t n, int64_t t, const int64_t* active, const double* A, int64_t lda,
                                        const double* cx, int scaling, double* At, int64_t ldat, double* cx_active,
                                        double* diag_scale) {
    if (l < 0 || n < 1 || t < 0 || t > l || lda < l || ldat < n) return -2;
    if (t > 0 && (!active || !A || !cx || !At || !cx_active || !diag_scale)) return -4;
    for (int64_t c = 0; c < t; ++c)
        if (active[c] < 0 || active[c] > l) return -5;
    gather_active<int64_t>(n, t, active, A, lda, cx, scaling != 0, At, ldat, cx_active, diag_scale);
    return 0;
}

int enlsip_gn_add_constraints_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t n, int64_t l, int64_t t_max, const int64_t* q,
                                          int64_t* t, int64_t* active, int64_t* inactive, const int64_t* index_alpha_upp,
                                          const int64_t* take, int scaling, const double* dA, int64_t lda, int64_t strideA,
                                          const double* dcx_all, double* dAt, int64_t ldat, int64_t strideAt, double* dcx,
                                          double* ddiag_scale, int64_t* added, int64_t* status) {
    if (!h) return -1;
    GN_TRY
    int rc = check_addition(h->err, {batch, n, l, t_max, lda, strideA, ldat, strideAt}, q, t, active, inactive, index_alpha_upp, take,
                            added && status, dA && dcx_all, dAt && dcx && ddiag_scale);
    if (rc) return rc;
    const bool wave = addition_wave_form(n, l);
    const int64_t tiles = (t_max + 63) / 64;
    if (!wave && !grid_fits(batch, tiles)) { h->err = "batch * ceil(t_max / 64) exceeds the grid"; return -2; }
    h->form[FORM_ADDITION] = wave ? 1 : 0;
    std::fill(added, added + batch, (int64_t)0);
    std::fill(status, status + batch, (int64_t)0);
    if (l == 0 || t_max == 0) return 0;      // no slot to build and, by the check of t_max, no walk that could add
    GN_HIP(hipSetDevice(h->device));
    AdditionScratch D, H;
    if ((rc = place_records(h, D, H, 0, batch, 2 * l))) return rc;
    const WorkingSets<int> Dw(D.list, batch, l), Hw(H.list, batch, l);
    for (int64_t k = 0; k < batch; ++k) {      // a problem that is not taken: counts of 0, so that nothing of its lists is read
        const int tk = addition_take(take, k);
        H.meta[k] = {tk ? (int)t[k] : 0, tk ? (int)q[k] : 0, tk, tk && index_alpha_upp ? (int)index_alpha_upp[k] : 0};
        pack_working_sets(H.list, batch, l, k, active, inactive, tk ? t[k] : -1);
    }
    AdditionArgs a{};
    a.meta = D.meta; a.act = Dw.act; a.inact = Dw.inact; a.out = D.out;
    a.count = (int)batch; a.n = (int)n; a.l = (int)l; a.t_max = (int)t_max; a.scaling = scaling != 0; a.tiles = (int)tiles;
    a.A = dA; a.lda = lda; a.strideA = strideA; a.cx_all = dcx_all;
    a.At = dAt; a.ldat = ldat; a.strideAt = strideAt; a.cx = dcx; a.diag_scale = ddiag_scale;
    auto launch = [&](hipStream_t st) {
        if (wave) {
            hipLaunchKernelGGL(k_add_wave, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
        } else {
            hipLaunchKernelGGL(k_add_walk, dim3((unsigned)batch), dim3(256), 0, st, a);
            hipLaunchKernelGGL(k_add_gather, dim3((unsigned)(batch * tiles)), dim3(256), 0, st, a);
        }
    };
    if ((rc = round_trip(h, D, H, launch, H.list, D.list, addition_down_bytes(H, batch)))) return rc;
    for (int64_t k = 0; k < batch; ++k) {
        if (H.meta[k].take != 1) continue;      // only a walk changes the host records
        t[k] = H.out[k].t;
        added[k] = H.out[k].added;
        status[k] = H.out[k].status;
        for (int64_t i = 0; i < l; ++i) {
            active[k * l + i] = Hw.act[k * l + i];
            inactive[k * l + i] = Hw.inact[k * l + i];
        }
    }
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_get_addition_form(enlsip_gn_handle h, int* form) { return get_form(h, FORM_ADDITION, form); }

}  // extern "C"
