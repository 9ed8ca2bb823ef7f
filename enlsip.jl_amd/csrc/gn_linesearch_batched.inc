// The line-search set-up of a batch on the caller's device buffers (kernels: gn_kernels_linesearch_batched.hpp; the bound:
// gn_steplength_bound.hpp): Ap = A * p of src/enlsip_functions.jl:2227, upper_bound_steplength (:2149-2178) and the three sums of
// :1561-1584 / :2269.  The call needs and touches nothing resident: the handle lends its device, its stream and its record scratch,
// in which the call places the host records, the partial sums and the five scalars per problem (LinesearchScratch).  Included at the end of enlsip_gn.hip.

namespace {

bool linesearch_wave_form(int64_t n, int64_t l) { return n <= 64 && l <= 64; }

}  // namespace

extern "C" {

int enlsip_gn_upper_bound_steplength(int64_t l, int64_t n_inactive, const int64_t* inactive, int64_t index_del, const double* cx,
                                     const double* Ap, double* alpha_upp, int64_t* index_alpha_upp) {
    if (!alpha_upp || !index_alpha_upp || l < 0 || n_inactive < 0 || n_inactive > l) return -2;
    if (n_inactive > 0 && (!inactive || !cx || !Ap)) return -4;
    for (int64_t i = 0; i < n_inactive; ++i)
        if (inactive[i] < 0 || inactive[i] > l) return -5;
    steplength_bound(n_inactive, inactive, index_del, cx, Ap, alpha_upp, index_alpha_upp);
    return 0;
}

int enlsip_gn_linesearch_setup_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t l, const double* dp,
                                           const double* dA, int64_t lda, int64_t strideA, const double* dcx,
                                           const int64_t* inactive, const int64_t* n_inactive, const int64_t* index_del,
                                           const double* dJp, const double* drx, double* dAp, double* alpha_upp,
                                           int64_t* index_alpha_upp, double* sums) {
    if (!h) return -1;
    GN_TRY
    int rc;
    if ((rc = check_batch(h->err, batch))) return rc;
    const int have = (dJp != nullptr) + (drx != nullptr) + (sums != nullptr);
    const bool want_sums = have == 3;
    if (n < 1 || n > LS_MAX_N) { h->err = "n must be in 1..1024 in this build"; return -3; }
    if ((rc = check_l(h->err, l))) return rc;
    if (want_sums && (m < 1 || m > 0x7fffffff)) { h->err = "m must be in 1..2^31-1 when the sums are asked for"; return -3; }
    if (have != 0 && have != 3) { h->err = "dJp, drx and sums go together: all three or none"; return -4; }
    if (!n_inactive || !alpha_upp || !index_alpha_upp) {
        h->err = "n_inactive, alpha_upp and index_alpha_upp are host arrays of batch entries";
        return -4;
    }
    if (l > 0 && (!dp || !dA || !dcx || !inactive || !dAp)) {
        h->err = "dp, dA, dcx, inactive and dAp are required when l > 0";
        return -4;
    }
    for (int64_t k = 0; k < batch; ++k)      // every count before any list: a bad n_inactive wins over a bad index_del
        if ((rc = check_count(h->err, -5, "n_inactive", k, n_inactive[k], {0, l, "0..l"}))) return rc;
    for (int64_t k = 0; k < batch; ++k)      // entries from 0: the bound skips a 0 (gn_steplength_bound.hpp)
        if ((index_del && (rc = check_count(h->err, -6, "index_del", k, index_del[k], {0, l, "0..l"}))) ||
            (rc = check_list(h->err, -6, "inactive", k, inactive + k * l, n_inactive[k], {0, l, "0..l"}))) return rc;
    if (l > 0 && lda < l) { h->err = "lda < l"; return -9; }
    if (l > 0 && strideA < lda * n) { h->err = "strideA < lda * n"; return -10; }
    const bool wave = linesearch_wave_form(n, l);
    const int64_t row_blocks = (l + 255) / 256;
    const int64_t nblk = want_sums ? sum_blocks(m) : 0;
    if (!wave && !grid_fits(batch, std::max(row_blocks, nblk))) {
        h->err = "batch * max(ceil(l / 256), partial-sum workgroups) exceeds the grid";
        return -2;
    }
    h->form[FORM_LINESEARCH] = wave ? 1 : 0;
    if (l == 0 && !want_sums) {      // no constraint anywhere and no sums: nothing to launch
        std::fill(alpha_upp, alpha_upp + batch, GN_STEPLENGTH_CAP);
        std::fill(index_alpha_upp, index_alpha_upp + batch, (int64_t)0);
        return 0;
    }
    GN_HIP(hipSetDevice(h->device));
    LinesearchScratch D, H;      // the partial sums: the general form's only
    if ((rc = place_records(h, D, H, wave ? 0 : 3 * nblk, batch, l))) return rc;
    for (int64_t k = 0; k < batch; ++k) H.meta[k] = {(int)n_inactive[k], index_del ? (int)index_del[k] : 0};
    pack_rows(H.list, inactive, n_inactive, batch, l);
    LinesearchArgs a{};
    a.meta = D.meta; a.list = D.list; a.out = D.out; a.part = D.part;
    a.count = (int)batch; a.n = (int)n; a.l = (int)l; a.m = want_sums ? (int)m : 0;
    a.row_blocks = (int)row_blocks; a.nblk = (int)nblk;
    a.p = dp; a.A = dA; a.lda = lda; a.strideA = strideA; a.cx = dcx; a.Jp = dJp; a.rx = drx; a.Ap = dAp;
    auto launch = [&](hipStream_t st) {
        if (wave) {
            hipLaunchKernelGGL(k_ls_wave, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
        } else {
            if (l > 0) hipLaunchKernelGGL(k_ls_product, dim3((unsigned)(batch * row_blocks)), dim3(256), 0, st, a);
            if (want_sums) hipLaunchKernelGGL(k_ls_sums_part, dim3((unsigned)(batch * nblk)), dim3(256), 0, st, a);
            hipLaunchKernelGGL(k_ls_bound, dim3((unsigned)batch), dim3(256), 0, st, a);
        }
    };
    if ((rc = round_trip(h, D, H, launch, H.out, D.out, H.down_bytes))) return rc;
    for (int64_t k = 0; k < batch; ++k) {
        alpha_upp[k] = H.out[k].alpha_upp;
        index_alpha_upp[k] = H.out[k].index_alpha_upp;
        if (want_sums) for (int q = 0; q < 3; ++q) sums[3 * k + q] = H.out[k].sums[q];
    }
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_get_linesearch_form(enlsip_gn_handle h, int* form) { return get_form(h, FORM_LINESEARCH, form); }

}  // extern "C"
