// Batched subspace re-solve over a contiguous range of the resident batch (kernels: gn_kernels_resolve_batched.hpp): what
// search_direction_analys does per problem at src/enlsip_functions.jl:1249-1253 — b = F_L11.Q' (-cx[F_A.p]), the d of
// choose_subspace_dimensions (:1118-1176, :1156-1163) and sub_search_direction (:116-153) — in a number of launches and
// synchronisations that does not depend on the size of the range.  The range and the driver of its half-segments are the shared
// ones of gn_accessors.inc (resident_range, for_each_segment).  What the calls that answer with p / b / d / info / status share is
// here: resolve_stages (head, then resolve_d_stages; the batched Newton direction enqueues it too), resolve_tail_launch,
// bind_outputs, write_alone_slot and the host-buffer form, staged_outputs_call.  Included at the end of enlsip_gn.hip.

namespace {

struct ResolveIO {       // device buffers, slot 0 = problem prob0; any may be null
    double *p, *b, *d;
    enlsip_gn_info* info;
    int* status;
};

enum { RS_DIMA = 1, RS_DIMJ2 = 2, RS_NO_HOLD = 3, RS_CODE = 4 };

ResolveBatchArgs resolve_args(enlsip_gn_handle hh, long long k0, long long cnt) {
    const Plan& P = hh->plan;
    const BatchOperands in = hh->last.slice(k0, cnt);
    ResolveBatchArgs a{};
    a.m = (int)P.m; a.n = (int)P.n; a.t = (int)P.t; a.kA = P.kA; a.ldw = P.ldw; a.ldr = P.ldr;
    a.nv = (int)rup(std::max<long long>({P.n, P.t, 1}), 8);
    a.blkd = 65 * (int)std::min<long long>(64, std::max<long long>({P.n, P.t, 1}));
    a.tk = hh->h_tk.empty() ? nullptr : (const int*)hh->tkbuf.p + k0;
    a.state = hh->state + k0;
    a.cx = in.cx; a.scx = in.t; a.rx = in.rx;
    a.FA = hh->FA + k0 * P.sFA; a.sFA = P.sFA; a.tauA = hh->tauA + k0 * P.sTauA; a.sTauA = P.sTauA;
    a.jpvtA = hh->jpvtA + k0 * P.sJA; a.sJA = P.sJA;
    a.FL = hh->FL + k0 * P.sFL; a.sFL = P.sFL; a.tauL = hh->tauL + k0 * P.sTauL; a.sTauL = P.sTauL;
    a.jpvtL = hh->jpvtL + k0 * P.sJL; a.sJL = P.sJL;
    a.qb = hh->cdist.valid ? hh->cdist.qb + k0 * hh->cdist.sQb : nullptr; a.sQb = hh->cdist.sQb;
    a.p1 = hh->p1 + k0 * P.sP1; a.sP1 = P.sP1; a.bvec = hh->bvec + k0 * P.sB; a.sB = P.sB;
    a.W = hh->W + k0 * P.sW; a.sW = P.sW; a.vec = hh->vec + k0 * P.sVec; a.sVec = P.sVec;
    a.Rt = hh->Rt + k0 * P.sRt; a.sRt = P.sRt; a.tauJ = hh->tauJ + k0 * P.sTauJ; a.sTauJ = P.sTauJ;
    a.jpvtJ = hh->jpvtJ + k0 * P.sJJ; a.sJJ = P.sJJ;
    return a;
}

bool resolve_small(const Plan& P) { return P.n <= 64 && P.t <= 64; }      // head and tail in their one-wave form

// the largest kp among the requests (host) that run the stages before the tail (not skipped, flagged or held); -1: none does
int resolve_kpmax(enlsip_gn_handle hh, long long k0, long long cnt, const ResolveDims* dims) {
    int kpmax = -1;
    for (long long jj = 0; jj < cnt; ++jj) {
        const ResolveDims& d = dims[jj];
        if (d.code == 0 || d.status != 0 || d.dimA == RESOLVE_HOLD) continue;
        kpmax = std::max(kpmax, hh->h_state[k0 + jj].kp);
    }
    return kpmax;
}

// Enqueues on hh's stream the d stages for problems k0 .. k0+cnt-1 of hh, after a head that left p1: d_temp, and
// d = F_J2.Q' d_temp as Q0' (one launch per (panel, level) of the CAQR plan) then Qt', into a.vec.  a.dims: the requests on the
// device; kpmax >= 0: theirs.  q0_ev: null, or two events recorded around the Q0' launches.
int resolve_d_stages(enlsip_gn_handle hh, const ResolveBatchArgs& a, long long k0, long long cnt, int kpmax, hipEvent_t* q0_ev) {
    enlsip_gn_handle h = hh;       // GN_HIP reports on `h`
    const Plan& P = hh->plan;
    hipStream_t s = hh->stream;
    const unsigned cn = (unsigned)cnt;
    hipLaunchKernelGGL(k_dtemp_batched, dim3((unsigned)(P.ldw + 255) / 256, cn), dim3(256), 0, s, a);
    const int npan = (kpmax + PB - 1) / PB;
    if (q0_ev) {
        for (int e = 0; e < 2; ++e)
            if (!q0_ev[e]) GN_HIP(hipEventCreate(&q0_ev[e]));
        GN_HIP(hipEventRecord(q0_ev[0], s));
    }
    for (int k = 0; k < npan; ++k)
        for (const LevelPlan& L : P.panels[k].levels) {
            CaqrArgs ca = caqr_args(hh, k, L);
            ca.ext_cols = 1; ca.C = a.vec - k0 * P.sVec; ca.sC = P.sVec; ca.prob0 = (int)k0;      // C: indexed from hh's problem 0
            if (P.F == 16) hipLaunchKernelGGL(k_caqr_vec_batched<4>, dim3(L.groups, cn), dim3(256), 0, s, ca, a.dims);
            else hipLaunchKernelGGL(k_caqr_vec_batched<2>, dim3(L.groups, cn), dim3(128), 0, s, ca, a.dims);
        }
    if (q0_ev) GN_HIP(hipEventRecord(q0_ev[1], s));
    if (kpmax > 0) hipLaunchKernelGGL(k_vec_reflectors_batched, dim3(cn), dim3(64), 0, s, a);
    return 0;
}

// Enqueues on hh's stream the stages before the tail: b and p1 (head), then the d stages.  kpmax < 0: no request runs them.
// b_only: b and p1 are all there is to compute (q0_ev is null then).
int resolve_stages(enlsip_gn_handle hh, const ResolveBatchArgs& a, long long k0, long long cnt, int kpmax, bool small, bool b_only,
                   hipEvent_t* q0_ev) {
    if (kpmax < 0) return 0;
    const size_t lds = resolve_lds_bytes(a.nv, a.blkd);
    const unsigned cn = (unsigned)cnt;
    if (small) hipLaunchKernelGGL(k_resolve_head<64>, dim3(cn), dim3(64), lds, hh->stream, a);
    else hipLaunchKernelGGL(k_resolve_head<256>, dim3(cn), dim3(256), lds, hh->stream, a);
    return b_only ? 0 : resolve_d_stages(hh, a, k0, cnt, kpmax, q0_ev);
}

// the tail (triangular solve with dimJ2, p, the outputs) in the form that goes with the shape
void resolve_tail_launch(enlsip_gn_handle hh, const ResolveBatchArgs& a, long long cnt, bool small) {
    const size_t lds = resolve_lds_bytes(a.nv, a.blkd);
    const unsigned cn = (unsigned)cnt;
    if (small) hipLaunchKernelGGL((k_resolve_tail<1, 64>), dim3(cn), dim3(64), lds, hh->stream, a);
    else if (hh->plan.n <= 512) hipLaunchKernelGGL((k_resolve_tail<8, 256>), dim3(cn), dim3(256), lds, hh->stream, a);
    else hipLaunchKernelGGL((k_resolve_tail<0, 256>), dim3(cn), dim3(256), lds, hh->stream, a);
}

// the caller's output buffers as a segment whose first problem is slot j0 writes them
void bind_outputs(ResolveBatchArgs& a, const ResolveIO& io, long long j0, const Plan& P) {
    a.p_out = io.p ? io.p + j0 * P.n : nullptr;
    a.b_out = (io.b && P.t > 0) ? io.b + j0 * P.t : nullptr;
    a.d_out = io.d ? io.d + j0 * P.m : nullptr;
    a.info_out = io.info ? io.info + j0 : nullptr;
    a.status_out = io.status ? io.status + j0 : nullptr;
}

// Writes what the per-problem entry point answered for slot j (a problem on a rescue handle) into the caller's device buffers;
// p, b, d, info: host, null for what this answer does not write.
int write_alone_slot(enlsip_gn_handle h, const ResolveIO& io, long long j, const Plan& P, const double* p, const double* b,
                     const double* d, const enlsip_gn_info* info, int status) {
    if (io.p && p) GN_HIP(hipMemcpy(io.p + j * P.n, p, (size_t)P.n * 8, hipMemcpyHostToDevice));
    if (io.b && b && P.t > 0) GN_HIP(hipMemcpy(io.b + j * P.t, b, (size_t)P.t * 8, hipMemcpyHostToDevice));
    if (io.d && d) GN_HIP(hipMemcpy(io.d + j * P.m, d, (size_t)P.m * 8, hipMemcpyHostToDevice));
    if (io.info && info) GN_HIP(hipMemcpy(io.info + j, info, sizeof(*info), hipMemcpyHostToDevice));
    if (io.status) GN_HIP(hipMemcpy(io.status + j, &status, sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

// The host-buffer form of a call with these five outputs: `host` staged through buf, dev(io) on the staged copies, the outputs
// copied back unless dev failed.  The caller's arrays go in first so that the slots the call leaves alone come back as they were.
template <class Dev>
int staged_outputs_call(enlsip_gn_handle h, DevBuf& buf, int64_t count, const Plan& P, const ResolveIO& host, Dev&& dev) {
    const size_t c = (size_t)count;
    Staged a[5] = {{host.p, c * P.n * 8, true, true}, {host.b, c * P.t * 8, true, true}, {host.d, c * P.m * 8, true, true},
                   {host.info, c * sizeof(enlsip_gn_info), true, true}, {host.status, c * sizeof(int), true, true}};
    int rc = stage_in(h, buf, a, 5);
    if (rc) return rc;
    rc = dev(ResolveIO{(double*)a[0].dev, (double*)a[1].dev, (double*)a[2].dev, (enlsip_gn_info*)a[3].dev, (int*)a[4].dev});
    if (rc < 0 || rc > 1) return rc;
    const int rc2 = stage_out(h, a, 5);
    return rc2 ? rc2 : rc;
}

// Enqueues the re-solve of one segment on its handle's stream: one copy of the requests, then 4 launches plus one per
// (panel, level) of the CAQR plan, whatever the segment's size.  dims: the requests of the segment's slots (host).
int resolve_launch(enlsip_gn_handle hh, const ResidentSeg& sg, const ResolveDims* dims, const ResolveIO& io, bool small, bool b_only, bool prof) {
    enlsip_gn_handle h = hh;       // GN_HIP reports on `h`
    const Plan& P = hh->plan;
    const long long k0 = sg.k0, j0 = sg.j0, cnt = sg.cnt;
    int rc = grow(hh, hh->rsb_dims, (size_t)cnt * sizeof(ResolveDims));
    if (rc) return rc;
    hipStream_t s = hh->stream;
    ResolveDims* ddims = (ResolveDims*)hh->rsb_dims.p;
    GN_HIP(hipMemcpyAsync(ddims, dims, (size_t)cnt * sizeof(ResolveDims), hipMemcpyHostToDevice, s));
    ResolveBatchArgs a = resolve_args(hh, k0, cnt);
    a.dims = ddims;
    bind_outputs(a, io, j0, P);
    // the stages before the tail run for the slots that do not start from a held result; b_only: every request of the call stops at
    // HOLD and no d is asked for.  Profiling on: HIP events around the Q0' launches, if there are any (enlsip_gn_get_resolve_q0_ms)
    const int kpmax = resolve_kpmax(hh, k0, cnt, dims);
    hh->rsb_timed = prof && !b_only && kpmax > 0;
    rc = resolve_stages(hh, a, k0, cnt, kpmax, small, b_only, hh->rsb_timed ? hh->rsb_ev : nullptr);
    if (rc) return rc;
    resolve_tail_launch(hh, a, cnt, small);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(hh->h_state + k0, hh->state + k0, (size_t)cnt * sizeof(ProbState), hipMemcpyDeviceToHost, s));
    return 0;
}

int resolve_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const int64_t* dimA, const int64_t* dimJ2, const int64_t* code,
                const ResolveIO& io) {
    if (!h) return -1;
    ResidentRange r;
    int rc = resident_range(h, prob0, count, r);
    if (rc) return rc;
    if (!dimA || !dimJ2 || !code) { h->err = "dimA, dimJ2 and code are host arrays of count entries"; return -4; }
    for (const ResidentSeg& sg : r.seg) {
        rc = needs_jacobian_side(h, sg.hh);
        if (rc) return rc;
    }
    const Plan& P = r.plan();
    // per-problem validation (enlsip_gn_resolve's) on the host mirror of the state records
    std::vector<ResolveDims> dims((size_t)count, ResolveDims{0, 0, 0, 0});
    bool flagged = false;
    for (const ResidentSeg& sg : r.seg) {
        enlsip_gn_handle hh = sg.hh;
        if (hh->held.size() < (size_t)hh->plan.batch) hh->held.resize((size_t)hh->plan.batch);
        for (long long jj = 0; jj < sg.cnt; ++jj) {
            const long long j = sg.j0 + jj, k = sg.k0 + jj;
            if (!r.alone.empty() && r.alone[(size_t)j].hh) continue;       // left at code 0 here
            if (code[j] == 0) continue;
            const ProbState& st = hh->h_state[k];
            const int tk = prob_t(hh, k);
            ResolveDims d{(int)dimA[j], (int)dimJ2[j], (int)code[j], 0};
            if (code[j] != 1 && code[j] != -1) d.status = RS_CODE;
            else if (dimA[j] == ENLSIP_GN_DIM_HOLD) {
                const auto& hd = hh->held[(size_t)k];
                if (hd.code == 0) d.status = RS_NO_HOLD;
                d.code = hd.code ? hd.code : d.code;
            } else if (dimA[j] < 0 || dimA[j] > std::min<long long>(P.n, tk)) d.status = RS_DIMA;
            else if (code[j] == 1 && st.rankA != tk) d.status = RS_CODE;
            if (!d.status && dimJ2[j] != ENLSIP_GN_DIM_HOLD && (dimJ2[j] < 0 || dimJ2[j] > st.kp)) d.status = RS_DIMJ2;
            flagged = flagged || d.status != 0;
            dims[(size_t)j] = d;
        }
    }
    GN_HIP(hipSetDevice(h->device));
    const bool small = resolve_small(P);
    h->form[FORM_RESOLVE] = small ? 1 : 0;
    // the first call of the reference's flow asks for b alone (:1251): no d pointer and every request held — F_J2.Q' is not applied
    bool b_only = io.d == nullptr;
    for (const ResolveDims& d : dims)
        if (d.code != 0 && d.status == 0 && d.dimJ2 != RESOLVE_HOLD) b_only = false;
    rc = for_each_segment(h, r, [&](const ResidentSeg& sg) {
        return resolve_launch(sg.hh, sg, dims.data() + sg.j0, io, small, b_only, h->profiling);
    });
    if (rc) return rc;
    h->resolve_q0_ms = 0.f;
    for (const ResidentSeg& sg : r.seg) {
        GN_HIP(hipStreamSynchronize(sg.hh->stream));
        if (sg.hh->rsb_timed) {       // the halves fill the device one after the other: their Q0' times add up
            float ms = 0.f;
            GN_HIP(hipEventElapsedTime(&ms, sg.hh->rsb_ev[0], sg.hh->rsb_ev[1]));
            h->resolve_q0_ms += ms;
        }
        for (long long jj = 0; jj < sg.cnt; ++jj) {      // which problems now hold p1 and Q3' d_temp for a later dimA = HOLD call
            const ResolveDims& d = dims[(size_t)(sg.j0 + jj)];
            if (d.code == 0 || d.status != 0 || d.dimA == RESOLVE_HOLD) continue;
            auto& hd = sg.hh->held[(size_t)(sg.k0 + jj)];
            if (d.dimJ2 == RESOLVE_HOLD && !b_only) hd = {d.code, d.dimA};
            else hd = {};
        }
    }
    // problems answered on their own (rescue handles): enlsip_gn_resolve; a held call is the re-solve with dimJ2 = 0, whose b and d
    // are the held ones, and dimA = HOLD repeats the held dimA
    if (!r.slots.empty()) {
        std::vector<double> hp((size_t)P.n), hb((size_t)std::max<long long>(P.t, 1)), hd_((size_t)P.m);
        for (long long j : r.slots) {
            if (code[j] == 0) continue;
            const AloneAt at = r.alone[(size_t)j];
            if (at.hh->held.size() <= (size_t)at.k) at.hh->held.resize((size_t)at.k + 1);
            const auto was = at.hh->held[(size_t)at.k];
            long long dA = dimA[j], dJ = dimJ2[j], c = code[j];
            int st = 0;
            if (dA == ENLSIP_GN_DIM_HOLD) {
                if (was.code == 0) st = RS_NO_HOLD;
                dA = was.dimA; c = was.code;
            }
            const bool hold2 = dJ == ENLSIP_GN_DIM_HOLD;
            if (!st) {
                std::fill(hb.begin(), hb.end(), 0.0);
                rc = enlsip_gn_resolve(h, prob0 + j, dA, hold2 ? 0 : dJ, c, hp.data(), hb.data(), hd_.data());
                if (rc == -3) st = RS_DIMA;
                else if (rc == -4) st = RS_DIMJ2;
                else if (rc == -5) st = RS_CODE;
                else if (rc) return rc;
            }
            const enlsip_gn_info inf = info_of(at.hh->h_state[at.k]);
            if (st) rc = write_alone_slot(h, io, j, P, nullptr, nullptr, nullptr, nullptr, st);
            else rc = write_alone_slot(h, io, j, P, hold2 ? nullptr : hp.data(), hb.data(), hd_.data(), &inf, 0);
            if (rc) return rc;
            if (!st) {
                if (hold2 && dimA[j] != ENLSIP_GN_DIM_HOLD && !b_only) at.hh->held[(size_t)at.k] = {(int)c, (int)dA};
                else if (dimA[j] == ENLSIP_GN_DIM_HOLD) at.hh->held[(size_t)at.k] = was;
            }
            flagged = flagged || st != 0;
        }
    }
    return flagged ? 1 : 0;
}

}  // namespace

extern "C" {

int enlsip_gn_resolve_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const int64_t* dimA, const int64_t* dimJ2,
                                  const int64_t* code, double* dp, double* db, double* dd, enlsip_gn_info* dinfo, int* dstatus) {
    if (!h) return -1;
    GN_TRY
    return resolve_dev(h, prob0, count, dimA, dimJ2, code, {dp, db, dd, dinfo, dstatus});
    GN_CATCH(h)
}

int enlsip_gn_resolve_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const int64_t* dimA, const int64_t* dimJ2,
                              const int64_t* code, double* p, double* b, double* d, enlsip_gn_info* info, int* status) {
    if (!h) return -1;
    GN_TRY
    ResidentRange r;
    const int rc = resident_range(h, prob0, count, r);
    if (rc) return rc;
    return staged_outputs_call(h, h->rsb_io, count, r.plan(), {p, b, d, info, status},
                               [&](const ResolveIO& io) { return resolve_dev(h, prob0, count, dimA, dimJ2, code, io); });
    GN_CATCH(h)
}

int enlsip_gn_get_diagR_batched(enlsip_gn_handle h, int which, int64_t prob0, int64_t count, double* diag, int64_t stride) {
    if (!h) return -1;
    GN_TRY
    ResidentRange r;
    int rc = resident_range(h, prob0, count, r);
    if (rc) return rc;
    if (which != ENLSIP_GN_FACTOR_A && which != ENLSIP_GN_FACTOR_L11 && which != ENLSIP_GN_FACTOR_J2) { h->err = "bad factor selector"; return -2; }
    if (!diag) { h->err = "diag is NULL"; return -5; }
    const Plan& P = r.plan();
    long long need = which == ENLSIP_GN_FACTOR_J2 ? 0 : std::min(P.n, P.t);
    if (which == ENLSIP_GN_FACTOR_J2)
        for (const ResidentSeg& sg : r.seg) {
            rc = needs_jacobian_side(h, sg.hh);
            if (rc) return rc;
            for (long long k = sg.k0; k < sg.k0 + sg.cnt; ++k) need = std::max<long long>(need, sg.hh->h_state[k].kp);
        }
    if (stride < need || stride < 1) { h->err = "stride is smaller than the longest diagonal of the range"; return -6; }
    GN_HIP(hipSetDevice(h->device));
    for (const ResidentSeg& sg : r.seg) {
        enlsip_gn_handle hh = sg.hh;
        rc = grow(hh, hh->rsb_io, (size_t)sg.cnt * stride * 8);
        if (rc) { h->err = hh->err; return rc; }
        const ResolveBatchArgs a = resolve_args(hh, sg.k0, sg.cnt);
        hipLaunchKernelGGL(k_diag_gather, dim3((unsigned)sg.cnt), dim3(64), 0, hh->stream, a, which, (double*)hh->rsb_io.p, (long long)stride);
        GN_HIP(hipGetLastError());
        GN_HIP(hipMemcpyAsync(diag + sg.j0 * stride, hh->rsb_io.p, (size_t)sg.cnt * stride * 8, hipMemcpyDeviceToHost, hh->stream));
    }
    for (const ResidentSeg& sg : r.seg) GN_HIP(hipStreamSynchronize(sg.hh->stream));
    for (long long j : r.slots) {      // answered on their own
        std::fill(diag + j * stride, diag + (j + 1) * stride, 0.0);
        int64_t r = 0, c = 0;
        rc = enlsip_gn_factor_shape(h, which, prob0 + j, &r, &c);
        if (rc) return rc;
        if (std::min(r, c) > stride) { h->err = "stride is smaller than the longest diagonal of the range"; return -6; }
        rc = enlsip_gn_get_diagR(h, which, prob0 + j, diag + j * stride);
        if (rc) return rc;
    }
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_get_resolve_q0_ms(enlsip_gn_handle h, float* ms) {
    GN_GETTER_CHECK(h, ms)
    *ms = h->resolve_q0_ms;
    return 0;
}

int enlsip_gn_get_resolve_form(enlsip_gn_handle h, int* form) { return get_form(h, FORM_RESOLVE, form); }

}  // extern "C"
