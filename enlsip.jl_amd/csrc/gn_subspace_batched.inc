// One-call subspace minimisation over a contiguous range of the resident batch (kernels: gn_kernels_subspace_batched.hpp; the
// choice: gn_subspace_choice.hpp): lines :1251-1253 of search_direction_analys with choose_subspace_dimensions
// (src/enlsip_functions.jl:1118-1176) between the stages of the batched re-solve.  Its own kernels are the head, which chooses dimA,
// and the choice of dimJ2; everything else is gn_resolve_batched.inc's: resolve_d_stages after the head, the whole resolve_stages
// where dimA was raised, resolve_tail_launch, bind_outputs, write_alone_slot and the host-buffer form staged_outputs_call.
// The range and its half-segments are the shared ones of gn_accessors.inc.  Included at the end of enlsip_gn.hip.

namespace {

// the largest previous dimension a 32-bit request can carry; anything beyond is out of every range anyway
long long ss_clamp(long long v) { return std::max<long long>(std::min<long long>(v, 1ll << 30), -(1ll << 30)); }

// Enqueues the call for one segment on its handle's stream: ONE copy of the requests and the previous iterates, then a number of
// launches that depends on the CAQR plan alone.  dims: the requests of the segment's slots (host: code -1 / 0 and a status found
// on the host); prev: theirs.  pack: the host image of the copy, alive until the stream is synchronised.
int subspace_launch(enlsip_gn_handle hh, const ResidentSeg& sg, const ResolveDims* dims, const enlsip_gn_subspace_prev* prev,
                    const ResolveIO& io, bool small, std::vector<char>& pack) {
    enlsip_gn_handle h = hh;       // GN_HIP reports on `h`
    const Plan& P = hh->plan;
    const long long k0 = sg.k0, j0 = sg.j0, cnt = sg.cnt;
    const size_t db = (size_t)cnt * sizeof(ResolveDims), pb = (size_t)cnt * sizeof(enlsip_gn_subspace_prev);
    int rc = grow(hh, hh->ssb_req, 2 * db + pb);
    if (rc) return rc;
    rc = grow_pinned(hh, hh->h_ssb, db);
    if (rc) return rc;
    hipStream_t s = hh->stream;
    ResolveDims* d1 = (ResolveDims*)hh->ssb_req.p;
    enlsip_gn_subspace_prev* dprev = (enlsip_gn_subspace_prev*)((char*)d1 + db);
    ResolveDims* d2 = (ResolveDims*)((char*)dprev + pb);
    pack.resize(db + pb);
    std::memcpy(pack.data(), dims, db);
    std::memcpy(pack.data() + db, prev, pb);
    GN_HIP(hipMemcpyAsync(d1, pack.data(), db + pb, hipMemcpyHostToDevice, s));

    ResolveBatchArgs a = resolve_args(hh, k0, cnt);
    a.dims = d1;
    bind_outputs(a, io, j0, P);
    SubspaceArgs c{};
    c.dims = d1; c.dims2 = d2; c.prev = dprev;
    c.nc = (int)rup(std::max<long long>(std::min(P.n, P.t), 1), 8);
    c.nr = (int)rup(std::max<long long>(std::min(P.m, P.n), 1), 8);
    const size_t lds_h = subspace_head_lds_bytes(a.nv, a.blkd, c.nc), lds_j = subspace_dimj2_lds_bytes(c.nr);
    // n, t <= 1024 in this build: at most 74 KB for the head (above 64 KB: the opt-in of GN_LAUNCH_BIG) and 33 KB for the dimJ2 kernel
    const int kpmax = resolve_kpmax(hh, k0, cnt, dims);
    // the max with the previous dimA (:1171-1174) can raise dimA after d was formed: b, p1 and d are then computed again with the
    // final dimA, as sub_search_direction (:1253) does.  Whether any slot can need that is known here: dimA >= 1 where rankA > 0.
    bool again = false;
    for (long long jj = 0; jj < cnt; ++jj) {
        const ResolveDims& d = dims[jj];
        if (d.code == 0 || d.status != 0) continue;
        const enlsip_gn_subspace_prev& pv = prev[jj];
        again = again || (choice_keeps_previous(pv.previous_alpha, pv.restart != 0) && hh->h_state[k0 + jj].rankA > 0 && pv.previous_dimA >= 2);
    }
    const unsigned cn = (unsigned)cnt;
    if (kpmax >= 0) {
        if (small) hipLaunchKernelGGL(k_subspace_head<64>, dim3(cn), dim3(64), lds_h, s, a, c);
        else GN_LAUNCH_BIG(k_subspace_head<256>, dim3(cn), dim3(256), lds_h, s, a, c);
        rc = resolve_d_stages(hh, a, k0, cnt, kpmax, nullptr);
        if (rc) return rc;
    }
    if (small) hipLaunchKernelGGL(k_subspace_dimj2<64>, dim3(cn), dim3(64), lds_j, s, a, c);
    else hipLaunchKernelGGL(k_subspace_dimj2<256>, dim3(cn), dim3(256), lds_j, s, a, c);
    // closing pass on the requests the choice wrote: the stages before the tail only where dimA was raised, then the tail
    a.dims = d2;
    if (again && kpmax >= 0) {
        rc = resolve_stages(hh, a, k0, cnt, kpmax, small, false, nullptr);
        if (rc) return rc;
    }
    resolve_tail_launch(hh, a, cnt, small);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(hh->h_ssb.p, d2, db, hipMemcpyDeviceToHost, s));
    GN_HIP(hipMemcpyAsync(hh->h_state + k0, hh->state + k0, (size_t)cnt * sizeof(ProbState), hipMemcpyDeviceToHost, s));
    return 0;
}

// choose_subspace_dimensions on HOST data of one problem answered on its own (a rescue handle), through enlsip_gn_resolve in the
// way a held request is answered there: b with any dimA, d with the chosen dimA, then the re-solve with the final pair.  Each of
// the up to three calls is a full per-problem re-solve (the rescue route synchronises more, as for every batched consumer), and a
// status found after the first of them leaves the rescue handle's b, p1 and state record at the dimA of that call, as a status
// found by k_subspace_dimj2 does on the batched path; the caller's output slots are not written for status 5.  The norms of d are
// scaled sums (its entries are far from 1 on this route); b comes from A and cx, which the rescue does not scale.
int subspace_alone(enlsip_gn_handle h, int64_t prob, const AloneAt& at, const Plan& P, const enlsip_gn_subspace_prev& pv, double* hp,
                   double* hb, double* hd, int* status, bool* wrote_p) {
    const ProbState st = at.hh->h_state[at.k];
    const int tk = prob_t(at.hh, at.k);
    const long long m = P.m, n = P.n;
    const bool restart = pv.restart != 0;
    *status = 0;
    *wrote_p = false;
    std::vector<double> dg((size_t)std::max<long long>({std::min(m, n), (long long)tk, 1})), tau(dg.size()), rho(dg.size());
    long long dimA = 0, dimJ2 = 0, prevA = 0;
    int rc = 0;
    if (st.rankA > 0) {
        prevA = pv.previous_dimA;
        if (prevA > tk) { *status = CHOICE_OUT_OF_BOUNDS; return 0; }
        rc = enlsip_gn_resolve(h, prob, st.rankA, 0, -1, nullptr, hb, nullptr);
        if (rc) return rc;
        rc = enlsip_gn_get_diagR(h, ENLSIP_GN_FACTOR_L11, prob, dg.data());
        if (rc) return rc;
        double s_all = 0.0, s_prev = 0.0;
        for (int i = 0; i < tk; ++i) { s_all += hb[i] * hb[i]; if (i < prevA) s_prev += hb[i] * hb[i]; }
        rc = choice_determine_solving_dim(prevA, st.rankA, std::sqrt(s_all), pv.constraint_progress, std::sqrt(s_prev), dg.data(), 1, hb,
                                          pv.previous_alpha, restart, tau.data(), rho.data(), &dimA, nullptr);
        if (rc) { *status = rc; return 0; }
    }
    rc = enlsip_gn_resolve(h, prob, dimA, 0, -1, nullptr, hb, hd);
    if (rc) return rc;
    const long long prevJ = pv.previous_dimJ2;
    if (prevJ > m) { *status = CHOICE_OUT_OF_BOUNDS; return 0; }
    if (st.rankJ2 > 0) {
        rc = enlsip_gn_get_diagR(h, ENLSIP_GN_FACTOR_J2, prob, dg.data());
        if (rc) return rc;
    }
    // norms by a scaled sum: the entries of a rescued problem are far from 1
    double mx = 0.0;
    for (long long i = 0; i < m; ++i) mx = std::max(mx, std::fabs(hd[i]));
    double s_all = 0.0, s_prev = 0.0;
    if (mx > 0.0 && mx <= 1.7976931348623157e308)
        for (long long i = 0; i < m; ++i) { const double v = hd[i] / mx; s_all += v * v; if (i < prevJ) s_prev += v * v; }
    rc = choice_determine_solving_dim(prevJ, st.rankJ2, mx * std::sqrt(s_all), pv.residual_progress, mx * std::sqrt(s_prev), dg.data(), 1, hd,
                                      pv.previous_alpha, restart, tau.data(), rho.data(), &dimJ2, nullptr);
    if (rc) { *status = rc; return 0; }
    if (choice_keeps_previous(pv.previous_alpha, restart)) {
        dimA = std::max(dimA, prevA);
        dimJ2 = std::max(dimJ2, prevJ);
    }
    if (dimA < 0 || dimA > std::min<long long>(n, tk)) { *status = RS_DIMA; return 0; }
    if (dimJ2 < 0 || dimJ2 > st.kp) { *status = RS_DIMJ2; return 0; }
    rc = enlsip_gn_resolve(h, prob, dimA, dimJ2, -1, hp, hb, hd);
    if (rc) return rc;
    *wrote_p = true;
    return 0;
}

int subspace_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const int64_t* take, const enlsip_gn_subspace_prev* prev,
                 const ResolveIO& io) {
    if (!h) return -1;
    ResidentRange r;
    int rc = resident_range(h, prob0, count, r);
    if (rc) return rc;
    if (!prev) { h->err = "prev is a host array of count entries"; return -4; }
    for (const ResidentSeg& sg : r.seg) {
        rc = needs_jacobian_side(h, sg.hh);
        if (rc) return rc;
    }
    const Plan& P = r.plan();
    // requests: code -1 for the taken problems; what is certain to index out of bounds in the reference is flagged here, before
    // any launch, from the host mirror of the state records.  The 32-bit device records carry the previous dimensions clamped.
    std::vector<ResolveDims> dims((size_t)count, ResolveDims{0, 0, 0, 0});
    std::vector<enlsip_gn_subspace_prev> pvs(prev, prev + count);
    for (const ResidentSeg& sg : r.seg) {
        enlsip_gn_handle hh = sg.hh;
        if (hh->held.size() < (size_t)hh->plan.batch) hh->held.resize((size_t)hh->plan.batch);
        for (long long jj = 0; jj < sg.cnt; ++jj) {
            const long long j = sg.j0 + jj, k = sg.k0 + jj;
            if (!r.alone.empty() && r.alone[(size_t)j].hh) continue;       // left at code 0 here
            if (take && take[j] == 0) continue;
            const ProbState& st = hh->h_state[k];
            const int tk = prob_t(hh, k);
            enlsip_gn_subspace_prev& pv = pvs[(size_t)j];
            pv.previous_dimA = ss_clamp(pv.previous_dimA);
            pv.previous_dimJ2 = ss_clamp(pv.previous_dimJ2);
            ResolveDims d{0, RESOLVE_HOLD, -1, 0};
            const bool restart = pv.restart != 0;
            if (st.rankA > 0 && (pv.previous_dimA > tk || choice_certainly_out_of_bounds(pv.previous_dimA, st.rankA, pv.previous_alpha, restart)))
                d.status = CHOICE_OUT_OF_BOUNDS;
            if (pv.previous_dimJ2 > P.m || choice_certainly_out_of_bounds(pv.previous_dimJ2, st.rankJ2, pv.previous_alpha, restart))
                d.status = CHOICE_OUT_OF_BOUNDS;
            dims[(size_t)j] = d;
        }
    }
    GN_HIP(hipSetDevice(h->device));
    const bool small = resolve_small(P);
    h->form[FORM_SUBSPACE] = small ? 1 : 0;
    std::vector<std::vector<char>> packs(r.seg.size());      // one per segment, alive until the streams are synchronised
    rc = for_each_segment(h, r, [&](const ResidentSeg& sg) {
        return subspace_launch(sg.hh, sg, dims.data() + sg.j0, pvs.data() + sg.j0, io, small, packs[(size_t)(&sg - r.seg.data())]);
    });
    if (rc) return rc;
    bool flagged = false;
    for (const ResidentSeg& sg : r.seg) {
        GN_HIP(hipStreamSynchronize(sg.hh->stream));
        const ResolveDims* res = (const ResolveDims*)sg.hh->h_ssb.p;
        for (long long jj = 0; jj < sg.cnt; ++jj) {
            if (dims[(size_t)(sg.j0 + jj)].code == 0) continue;
            flagged = flagged || res[jj].status != 0;
            // b, p1 and the vector buffer of a problem that got past the choice of dimA were rewritten: a held result is gone.  One
            // flagged before that (on the host, or by the head) comes back with dimA = HOLD in its record: nothing of it was touched
            if (!(res[jj].status != 0 && res[jj].dimA == RESOLVE_HOLD)) sg.hh->held[(size_t)(sg.k0 + jj)] = {};
        }
    }
    // problems answered on their own (rescue handles): the HOST instantiation of the same choice around enlsip_gn_resolve
    if (!r.slots.empty()) {
        std::vector<double> hp((size_t)P.n), hb((size_t)std::max<long long>(P.t, 1)), hd_((size_t)P.m);
        for (long long j : r.slots) {
            if (take && take[j] == 0) continue;
            const AloneAt at = r.alone[(size_t)j];
            std::fill(hb.begin(), hb.end(), 0.0);
            int st = 0;
            bool wrote_p = false;
            rc = subspace_alone(h, prob0 + j, at, P, prev[j], hp.data(), hb.data(), hd_.data(), &st, &wrote_p);
            if (rc) return rc;
            const enlsip_gn_info inf = info_of(at.hh->h_state[at.k]);
            if (st == CHOICE_OUT_OF_BOUNDS) rc = write_alone_slot(h, io, j, P, nullptr, nullptr, nullptr, nullptr, st);
            else rc = write_alone_slot(h, io, j, P, wrote_p ? hp.data() : nullptr, hb.data(), hd_.data(), wrote_p ? &inf : nullptr, st);
            if (rc) return rc;
            flagged = flagged || st != 0;
        }
    }
    return flagged ? 1 : 0;
}

}  // namespace

extern "C" {

int enlsip_gn_determine_solving_dim(int64_t previous_dimR, int64_t rankR, double predicted_linear_progress, double obj_progress,
                                    double prelin_previous_dim, const double* diagR, const double* y, double previous_alpha,
                                    int64_t restart, int64_t* newdim) {
    if (!newdim || rankR < 0) return -2;
    if (rankR > 0 && (!diagR || !y)) return -4;
    try {
        std::vector<double> ws((size_t)(2 * rankR + 1));
        long long nd = 0;
        const int rc = choice_determine_solving_dim(previous_dimR, rankR, predicted_linear_progress, obj_progress, prelin_previous_dim, diagR,
                                                    1, y, previous_alpha, restart != 0, ws.data(), ws.data() + rankR, &nd, nullptr);
        if (rc == 0) *newdim = nd;
        return rc;
    } catch (...) {
        return -10;
    }
}

int enlsip_gn_subspace_direction_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const int64_t* take,
                                             const enlsip_gn_subspace_prev* prev, double* dp, double* db, double* dd,
                                             enlsip_gn_info* dinfo, int* dstatus) {
    if (!h) return -1;
    GN_TRY
    return subspace_dev(h, prob0, count, take, prev, {dp, db, dd, dinfo, dstatus});
    GN_CATCH(h)
}

int enlsip_gn_subspace_direction_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const int64_t* take,
                                         const enlsip_gn_subspace_prev* prev, double* p, double* b, double* d, enlsip_gn_info* info,
                                         int* status) {
    if (!h) return -1;
    GN_TRY
    ResidentRange r;
    const int rc = resident_range(h, prob0, count, r);
    if (rc) return rc;
    if (!prev) { h->err = "prev is a host array of count entries"; return -4; }
    return staged_outputs_call(h, h->ssb_io, count, r.plan(), {p, b, d, info, status},
                               [&](const ResolveIO& io) { return subspace_dev(h, prob0, count, take, prev, io); });
    GN_CATCH(h)
}

int enlsip_gn_get_subspace_form(enlsip_gn_handle h, int* form) { return get_form(h, FORM_SUBSPACE, form); }

}  // extern "C"
