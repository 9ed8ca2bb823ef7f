// Batched Newton direction over a contiguous range of the resident batch (kernels: gn_kernels_newton_batched.hpp): what
// newton_search_direction does per problem at src/enlsip_functions.jl:371-421 after its Hessian sums, in a number of launches and
// synchronisations that does not depend on the size of the range.  The range and the driver of its half-segments are the shared
// ones of gn_accessors.inc (resident_range, for_each_segment); the b / p1 / d stages are the batched re-solve's (resolve_stages,
// gn_resolve_batched.inc).  Included at the end of enlsip_gn.hip, after gn_newton.inc.

namespace {

struct NewtonIO {        // device buffers, slot 0 = problem prob0
    const double* Gamma; long long ldg, strideG;
    double* p;
    int* status;         // may be null
};

enum { NW_SKIP = 0, NW_TAKE = 1, NW_RANKDEF = 2 };

// Enqueues the step of one segment on its handle's stream: one copy of the requests, one copy of the state records, the
// b / p1 / d stages of the batched re-solve with the DEFAULT dimensions (dimA = rankA) into the call's own vec, then 4 launches.
// req: the requests of the segment's slots (host).  pack: host image of the request copy, owned by the caller so that it outlives
// the copy.  The segment's "some slot flagged" word lands in the handle's pinned h_nwflag.
int newton_launch(enlsip_gn_handle hh, const ResidentSeg& sg, const int* req, const NewtonIO& io, bool small, bool prof, std::vector<int>& pack) {
    enlsip_gn_handle h = hh;       // GN_HIP reports on `h`
    const Plan& P = hh->plan;
    const long long k0 = sg.k0, j0 = sg.j0, cnt = sg.cnt;
    const int n = (int)P.n;
    const size_t nn = (size_t)n * n;
    // workspace: X nn | E nn | rhs n per slot, vec sVec per slot, state records, status, then ONE block that one copy of `pack` fills:
    // the requests' ResolveDims | req | flag
    struct { double *X = nullptr, *E = nullptr, *rhs = nullptr, *vec = nullptr; ProbState* st = nullptr; int *status = nullptr, *pack = nullptr;
             void carve(Carver& c, size_t cnt, size_t nn, size_t n, size_t sVec) {
                 c.take(X, "X", cnt * nn); c.take(E, "E", cnt * nn); c.take(rhs, "rhs", cnt * n); c.take(vec, "vec", cnt * sVec);
                 c.take(st, "state", cnt, 8); c.take(status, "status", cnt); c.take(pack, "pack", cnt * 5 + 1, 8);
             } } N;
    static_assert(sizeof(ResolveDims) == 4 * sizeof(int), "pack: four words of dimensions, one request per slot, one flag");
    int rc = place_dev(hh, hh->nwb_ws, N, (size_t)cnt, nn, (size_t)n, (size_t)P.sVec);
    if (rc) return rc;
    rc = grow_pinned(hh, hh->h_nwflag, sizeof(int));
    if (rc) return rc;
    double *dX = N.X, *dE = N.E, *drhs = N.rhs, *dvec = N.vec;
    ProbState* dst = N.st;
    int* dstatus = N.status;
    ResolveDims* ddims = (ResolveDims*)N.pack;
    int* dreq = N.pack + 4 * cnt;
    int* dflag = dreq + cnt;
    hipStream_t s = hh->stream;

    // requests: the re-solve's record with the default dimensions for the slots that take the step
    pack.assign((size_t)cnt * 5 + 1, 0);
    ResolveDims* hd = (ResolveDims*)pack.data();
    for (long long jj = 0; jj < cnt; ++jj) {
        pack[(size_t)cnt * 4 + jj] = req[jj];
        if (req[jj] != NW_TAKE) continue;
        const ProbState& st = hh->h_state[k0 + jj];
        hd[jj] = {st.rankA, RESOLVE_HOLD, st.rankA == prob_t(hh, k0 + jj) ? 1 : -1, 0};
    }
    const int kpmax = resolve_kpmax(hh, k0, cnt, hd);
    GN_HIP(hipMemcpyAsync(ddims, pack.data(), pack.size() * sizeof(int), hipMemcpyHostToDevice, s));
    GN_HIP(hipMemcpyAsync(dst, hh->state + k0, (size_t)cnt * sizeof(ProbState), hipMemcpyDeviceToDevice, s));
    const unsigned cn = (unsigned)cnt;
    const bool timed = prof;
    if (timed) {
        for (hipEvent_t& e : hh->nwb_ev)
            if (!e) GN_HIP(hipEventCreate(&e));
        GN_HIP(hipEventRecord(hh->nwb_ev[0], s));
    }
    hh->nwb_timed = timed;
    // b, p1 (resident, as the per-problem entry point leaves them) and d = F_J2.Q' d_temp (the call's own vec); the state
    // records the head stage writes are the copy's, so the resident ones stay what they were (the per-problem call restores them)
    ResolveBatchArgs ra = resolve_args(hh, k0, cnt);
    ra.dims = ddims;
    ra.state = dst;
    ra.vec = dvec;
    rc = resolve_stages(hh, ra, k0, cnt, kpmax, resolve_small(P), false, nullptr);
    if (rc) return rc;
    if (timed) GN_HIP(hipEventRecord(hh->nwb_ev[1], s));
    NewtonBatchArgs a{};
    a.n = n; a.t = (int)P.t; a.kA = P.kA; a.ldr = P.ldr;
    a.req = dreq;
    a.tk = hh->h_tk.empty() ? nullptr : (const int*)hh->tkbuf.p + k0;
    a.state = hh->state + k0;
    a.FA = hh->FA + k0 * P.sFA; a.sFA = P.sFA; a.tauA = hh->tauA + k0 * P.sTauA; a.sTauA = P.sTauA;
    a.jpvtL = hh->jpvtL + k0 * P.sJL; a.sJL = P.sJL;
    a.p1 = hh->p1 + k0 * P.sP1; a.sP1 = P.sP1;
    a.vec = dvec; a.sVec = P.sVec;
    a.Rt = hh->Rt + k0 * P.sRt; a.sRt = P.sRt; a.jpvtJ = hh->jpvtJ + k0 * P.sJJ; a.sJJ = P.sJJ;
    a.Gamma = io.Gamma + j0 * io.strideG; a.ldg = io.ldg; a.strideG = io.strideG;
    a.X = dX; a.sX = (long long)nn; a.E = dE; a.rhs = drhs;
    a.p_out = io.p + j0 * n;
    a.status_out = io.status ? io.status + j0 : dstatus;
    a.flag = dflag;
    const unsigned nvb = (unsigned)((n + NWB_VEC - 1) / NWB_VEC), nt = (unsigned)((n + 15) / 16);
    const size_t slds = newton_side_lds(n);
    if (kpmax >= 0) {
        GN_LAUNCH_BIG(k_newton_side<false>, dim3(nvb, cn), dim3(256), slds, s, a);
        GN_LAUNCH_BIG(k_newton_side<true>, dim3(nvb, cn), dim3(256), slds, s, a);
    }
    if (timed) GN_HIP(hipEventRecord(hh->nwb_ev[2], s));
    if (kpmax >= 0) hipLaunchKernelGGL(k_newton_w22, dim3(nt * nt + (unsigned)((n + 63) / 64), cn), dim3(64), 0, s, a);
    if (timed) GN_HIP(hipEventRecord(hh->nwb_ev[3], s));
    if (small) hipLaunchKernelGGL(k_newton_chol_batched<64>, dim3(cn), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(k_newton_chol_batched<256>, dim3(cn), dim3(256), 0, s, a);
    if (timed) GN_HIP(hipEventRecord(hh->nwb_ev[4], s));
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(hh->h_nwflag.p, dflag, sizeof(int), hipMemcpyDeviceToHost, s));
    return 0;
}

int newton_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const NewtonIO& io, const int64_t* take) {
    if (!h) return -1;
    ResidentRange r;
    int rc = resident_range(h, prob0, count, r);
    if (rc) return rc;
    for (const ResidentSeg& sg : r.seg) {
        rc = needs_jacobian_side(h, sg.hh);
        if (rc) return rc;
    }
    const Plan& P = r.plan();
    if (!io.Gamma) { h->err = "Gamma is NULL"; return -4; }
    if (!io.p) { h->err = "p is NULL"; return -4; }
    if (io.ldg < P.n) { h->err = "ldg < n"; return -5; }
    if (io.strideG < io.ldg * P.n) { h->err = "strideG < ldg * n"; return -5; }
    for (const ResidentSeg& sg : r.seg)
        if (P.t > 0 && sg.hh->cdist.valid) { h->err = "newton direction after the distributed constraint stage is not supported"; return -7; }
    // per-problem validation (enlsip_gn_newton_direction's) on the host mirror of the state records
    std::vector<int> req((size_t)count, NW_SKIP);
    for (const ResidentSeg& sg : r.seg)
        for (long long jj = 0; jj < sg.cnt; ++jj) {
            const long long j = sg.j0 + jj, k = sg.k0 + jj;
            if (!r.alone.empty() && r.alone[(size_t)j].hh) continue;       // answered on its own below
            if (take && take[j] == 0) continue;
            const int tk = prob_t(sg.hh, k);
            req[(size_t)j] = (tk != sg.hh->h_state[k].rankA && tk < P.n) ? NW_RANKDEF : NW_TAKE;
        }
    GN_HIP(hipSetDevice(h->device));
    const bool small = P.n <= 64;
    h->form[FORM_NEWTON] = small ? 1 : 0;
    std::vector<std::vector<int>> packs(r.seg.size());      // one per segment, alive until the streams are synchronised
    rc = for_each_segment(h, r, [&](const ResidentSeg& sg) {
        return newton_launch(sg.hh, sg, req.data() + sg.j0, io, small, h->profiling, packs[(size_t)(&sg - r.seg.data())]);
    });
    if (rc) return rc;
    bool flagged = false;
    for (float& ms : h->newton_ms) ms = 0.f;
    for (const ResidentSeg& sg : r.seg) {
        GN_HIP(hipStreamSynchronize(sg.hh->stream));
        flagged = flagged || *(const int*)sg.hh->h_nwflag.p != 0;
        if (sg.hh->nwb_timed)
            for (int e = 0; e < 4; ++e) {
                float ms = 0.f;
                GN_HIP(hipEventElapsedTime(&ms, sg.hh->nwb_ev[e], sg.hh->nwb_ev[e + 1]));
                h->newton_ms[e] += ms;
            }
        // the resident p1 is the default one again: a result held for dimA = HOLD is gone
        for (long long jj = 0; jj < sg.cnt; ++jj)
            if (req[(size_t)(sg.j0 + jj)] == NW_TAKE && sg.hh->held.size() > (size_t)(sg.k0 + jj)) sg.hh->held[(size_t)(sg.k0 + jj)] = {};
    }
    // problems answered on their own (rescue handles): enlsip_gn_newton_direction
    if (!r.slots.empty()) {
        std::vector<double> hG((size_t)P.n * P.n), hp((size_t)P.n);
        for (long long j : r.slots) {
            if (take && take[j] == 0) continue;
            GN_HIP(hipMemcpy2D(hG.data(), (size_t)P.n * 8, io.Gamma + j * io.strideG, (size_t)io.ldg * 8, (size_t)P.n * 8, (size_t)P.n,
                               hipMemcpyDeviceToHost));
            int64_t bad = 0;
            int st = 0;
            rc = enlsip_gn_newton_direction(h, prob0 + j, hG.data(), P.n, hp.data(), &bad);
            if (rc == -7) st = NW_RANKDEF;
            else if (rc) return rc;
            else st = bad ? 1 : 0;
            if (st != NW_RANKDEF) GN_HIP(hipMemcpy(io.p + j * P.n, hp.data(), (size_t)P.n * 8, hipMemcpyHostToDevice));
            if (io.status) GN_HIP(hipMemcpy(io.status + j, &st, sizeof(int), hipMemcpyHostToDevice));
            flagged = flagged || st != 0;
        }
    }
    return flagged ? 1 : 0;
}

}  // namespace

extern "C" {

int enlsip_gn_newton_direction_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* dGamma, int64_t ldg,
                                           int64_t strideG, const int64_t* take, double* dp, int* dstatus) {
    if (!h) return -1;
    GN_TRY
    return newton_dev(h, prob0, count, {dGamma, ldg, strideG, dp, dstatus}, take);
    GN_CATCH(h)
}

int enlsip_gn_newton_direction_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* Gamma, int64_t ldg,
                                       int64_t strideG, const int64_t* take, double* p, int* status) {
    if (!h) return -1;
    GN_TRY
    ResidentRange r;
    int rc = resident_range(h, prob0, count, r);
    if (rc) return rc;
    const Plan& P = r.plan();
    if (r.seg[0].hh->constraints_only) { h->err = GN_ERR_CONSTRAINTS_ONLY; return -1; }
    if (!Gamma) { h->err = "Gamma is NULL"; return -4; }
    if (!p) { h->err = "p is NULL"; return -4; }
    if (ldg < P.n) { h->err = "ldg < n"; return -5; }
    if (strideG < ldg * P.n) { h->err = "strideG < ldg * n"; return -5; }
    const size_t c = (size_t)count;
    // staged through a buffer of its own, one copy each way; the caller's p and status go in first so that the slots the call
    // leaves alone come back as they were
    Staged a[3] = {{(void*)Gamma, ((c - 1) * (size_t)strideG + (size_t)ldg * P.n) * 8, true, false}, {p, c * P.n * 8, true, true},
                   {status, c * sizeof(int), true, true}};
    rc = stage_in(h, h->nwb_io, a, 3);
    if (rc) return rc;
    rc = newton_dev(h, prob0, count, {(double*)a[0].dev, ldg, strideG, (double*)a[1].dev, (int*)a[2].dev}, take);
    if (rc < 0 || rc > 1) return rc;
    const int rc2 = stage_out(h, a, 3);
    return rc2 ? rc2 : rc;
    GN_CATCH(h)
}

int enlsip_gn_get_newton_form(enlsip_gn_handle h, int* form) { return get_form(h, FORM_NEWTON, form); }

int enlsip_gn_get_newton_stage_ms(enlsip_gn_handle h, float* ms) {
    GN_GETTER_CHECK(h, ms)
    for (int e = 0; e < 4; ++e) ms[e] = h->newton_ms[e];
    return 0;
}

}  // extern "C"
