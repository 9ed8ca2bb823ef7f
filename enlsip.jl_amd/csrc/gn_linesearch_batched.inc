// The line-search set-up of a batch on the caller's device buffers (kernels: gn_kernels_linesearch_batched.hpp; the bound:
// gn_steplength_bound.hpp): Ap = A * p of src/enlsip_functions.jl:2227, upper_bound_steplength (:2149-2178) and the three sums of
// :1561-1584 / :2269.  The call needs and touches nothing resident: the handle lends its device, its stream and a scratch for the
// host records, the partial sums and the five scalars per problem.  Included at the end of enlsip_gn.hip.

namespace {

// one call's records: up goes [meta | list] in one copy, down comes out in one copy; part stays on the device
struct LinesearchScratch {
    LsMeta* meta = nullptr;
    int* list = nullptr;
    LsOut* out = nullptr;
    double* part = nullptr;
    // part_per_problem: 3 * nblk on the device in the general form, 0 otherwise (the pinned side has none)
    void carve(Carver& c, int64_t batch, int64_t l, int64_t part_per_problem) {
        c.take(meta, "meta", (size_t)batch);
        c.take(list, "list", (size_t)batch * (size_t)l);
        c.take(out, "out", (size_t)batch, 8);
        c.take(part, "part", (size_t)batch * (size_t)part_per_problem);
    }
    size_t up_bytes(int64_t batch, int64_t l) const { return (size_t)batch * sizeof(LsMeta) + (size_t)batch * (size_t)l * sizeof(int); }
};

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
    if (batch < 1 || batch > 0x7fffffff) { h->err = "batch must be in 1..2^31-1"; return -2; }
    const int have = (dJp != nullptr) + (drx != nullptr) + (sums != nullptr);
    const bool want_sums = have == 3;
    if (n < 1 || n > LS_MAX_N) { h->err = "n must be in 1..1024 in this build"; return -3; }
    if (l < 0 || l > (1LL << 27)) { h->err = "l must be in 0..2^27"; return -3; }
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
    for (int64_t k = 0; k < batch; ++k)
        if (n_inactive[k] < 0 || n_inactive[k] > l) { h->err = "n_inactive[" + std::to_string(k) + "] outside 0..l"; return -5; }
    for (int64_t k = 0; k < batch; ++k) {
        if (index_del && (index_del[k] < 0 || index_del[k] > l)) {
            h->err = "index_del[" + std::to_string(k) + "] outside 0..l";
            return -6;
        }
        const int64_t* row = inactive + k * l;
        for (int64_t i = 0; i < n_inactive[k]; ++i)
            if (row[i] < 0 || row[i] > l) {
                h->err = "inactive[" + std::to_string(k) + "][" + std::to_string(i) + "] outside 0..l";
                return -6;
            }
    }
    if (l > 0 && lda < l) { h->err = "lda < l"; return -9; }
    if (l > 0 && strideA < lda * n) { h->err = "strideA < lda * n"; return -10; }
    const bool wave = linesearch_wave_form(n, l);
    const int64_t row_blocks = (l + 255) / 256;
    const int64_t nblk = want_sums ? std::min<int64_t>(LS_MAX_NBLK, (m + LS_SUM_ROWS - 1) / LS_SUM_ROWS) : 0;
    if (!wave && batch * std::max<int64_t>(std::max(row_blocks, nblk), 1) > 0x7fffffff) {
        h->err = "batch * max(ceil(l / 256), partial-sum workgroups) exceeds the grid";
        return -2;
    }
    h->linesearch_form = wave ? 1 : 0;
    if (l == 0 && !want_sums) {      // no constraint anywhere and no sums: nothing to launch
        std::fill(alpha_upp, alpha_upp + batch, GN_STEPLENGTH_CAP);
        std::fill(index_alpha_upp, index_alpha_upp + batch, (int64_t)0);
        return 0;
    }
    GN_HIP(hipSetDevice(h->device));
    LinesearchScratch D, H;
    int rc = place_dev(h, h->ls_scr, D, batch, l, wave ? (int64_t)0 : 3 * nblk);
    if (rc) return rc;
    rc = place_pinned(h, h->h_ls, H, batch, l, (int64_t)0);
    if (rc) return rc;
    for (int64_t k = 0; k < batch; ++k) {
        H.meta[k] = {(int)n_inactive[k], index_del ? (int)index_del[k] : 0};
        const int64_t* row = inactive + k * l;
        int* dst = H.list + k * l;
        const int64_t ni = n_inactive[k];
        for (int64_t i = 0; i < ni; ++i) dst[i] = (int)row[i];
        for (int64_t i = ni; i < l; ++i) dst[i] = 0;
    }
    hipStream_t st = h->stream;
    // meta and list are adjacent in both layouts (int-aligned records): one copy
    GN_HIP(hipMemcpyAsync(D.meta, H.meta, H.up_bytes(batch, l), hipMemcpyHostToDevice, st));
    LinesearchArgs a{};
    a.meta = D.meta; a.list = D.list; a.out = D.out; a.part = D.part;
    a.count = (int)batch; a.n = (int)n; a.l = (int)l; a.m = want_sums ? (int)m : 0;
    a.row_blocks = (int)row_blocks; a.nblk = (int)nblk;
    a.p = dp; a.A = dA; a.lda = lda; a.strideA = strideA; a.cx = dcx; a.Jp = dJp; a.rx = drx; a.Ap = dAp;
    if (wave) {
        hipLaunchKernelGGL(k_ls_wave, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, a);
    } else {
        if (l > 0) hipLaunchKernelGGL(k_ls_product, dim3((unsigned)(batch * row_blocks)), dim3(256), 0, st, a);
        if (want_sums) hipLaunchKernelGGL(k_ls_sums_part, dim3((unsigned)(batch * nblk)), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_ls_bound, dim3((unsigned)batch), dim3(256), 0, st, a);
    }
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(H.out, D.out, (size_t)batch * sizeof(LsOut), hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));
    for (int64_t k = 0; k < batch; ++k) {
        alpha_upp[k] = H.out[k].alpha_upp;
        index_alpha_upp[k] = H.out[k].index_alpha_upp;
        if (want_sums) for (int q = 0; q < 3; ++q) sums[3 * k + q] = H.out[k].sums[q];
    }
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_get_linesearch_form(enlsip_gn_handle h, int* form) {
    GN_GETTER_CHECK(h, form)
    *form = h->linesearch_form;
    return 0;
}

}  // extern "C"
