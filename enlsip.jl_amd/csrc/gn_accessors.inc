// Accessors on the resident factors (QRPivoted .R / .p / .Q' / .Q, J*F_A.Q) and the re-solve entry, and what the batched calls
// over a range of the resident batch share: resident_range, for_each_segment, needs_jacobian_side, stage_in / stage_out.  Included at
// the end of enlsip_gn.hip.

#define GN_ERR_CONSTRAINTS_ONLY "only F_A / F_L11 are resident (enlsip_gn_factor_constraints)"

namespace {

// the part of a range of the caller's batch that one handle holds: its problems k0 .. k0+cnt-1 in the caller's slots j0 .. j0+cnt-1
struct ResidentSeg {
    enlsip_gn_handle hh;
    long long k0, j0, cnt;
    bool alone;       // answered on its own: a problem on a rescue handle, or the one problem of a handle rescaled in place
};

// Maps problems prob0 .. prob0+count-1 of the caller's batch to the handles that hold them, calling each(seg) in slot order:
// only the last chunk of a batch above the launch limit is resident (solve_chunked); the problems from h->split on live on the
// pipeline child (solve_launchable); a rescued problem lives on a one-problem rescue handle of its half (gn_rescale.hpp).  Every
// half gives one segment over its part of the range, followed by an `alone` segment for each of its problems answered on its own.
// one: a single problem (need_factors): errors past the pipeline split are reported on the half that holds it.
template <class Each>
int map_resident(enlsip_gn_handle h, int64_t prob0, int64_t count, bool one, Each&& each) {
    if (count < 1) { h->err = "count must be >= 1"; return -2; }
    long long p = prob0;
    if (h->chunk0 > 0) {
        if (p < h->chunk0) { h->err = "problem belongs to an earlier chunk of a batch above the launch limit: its factors are no longer resident"; return -3; }
        p -= h->chunk0;
    }
    const enlsip_gn_handle c = h->split > 0 ? h->child : nullptr;
    const long long b0 = c ? h->split : h->plan.batch;
    const long long total = c ? b0 + c->plan.batch : b0;
    const enlsip_gn_handle rh = (one && c && p >= b0) ? c : h;
    if (!h->factors_valid || (c && !c->factors_valid)) { rh->err = "no resident factors: call a solve first"; return -1; }
    if (p < 0 || count > total || p > total - count) {
        rh->err = one ? "problem index out of range" : "problem range out of range: prob0 .. prob0+count-1 must lie in the resident batch";
        return -3;
    }
    const long long e = p + count;
    const struct { enlsip_gn_handle hh; long long lo, hi; } halves[2] = {{h, 0, b0}, {c, b0, total}};
    for (const auto& hf : halves) {
        const long long lo = std::max(p, hf.lo), hi = std::min(e, hf.hi);
        if (lo >= hi) continue;
        const ResidentSeg sg = {hf.hh, lo - hf.lo, lo - p, hi - lo, false};
        each(sg);
        if (hf.hh->sc_eJ || hf.hh->sc_eA) each(ResidentSeg{hf.hh, sg.k0, sg.j0, sg.cnt, true});
        for (size_t j = 0; j < hf.hh->rescue_prob.size(); ++j) {
            const long long k = hf.hh->rescue_prob[j];
            if (k < sg.k0 || k >= sg.k0 + sg.cnt) continue;
            const enlsip_gn_handle r = hf.hh->rescue[j];
            if (!r->factors_valid) { r->err = "no resident factors: call a solve first"; return -1; }
            each(ResidentSeg{r, 0, sg.j0 + k - sg.k0, 1, true});
        }
    }
    return 0;
}

// routes (h, prob) to the handle that holds the problem and its index there (the last segment of its map)
int need_factors(enlsip_gn_handle& h, int64_t& prob) {
    if (!h) return -1;
    ResidentSeg at{};
    const int rc = map_resident(h, prob, 1, true, [&](const ResidentSeg& sg) { at = sg; });
    if (rc) return rc;
    h = at.hh;
    prob = at.k0;
    return 0;
}

struct AloneAt { enlsip_gn_handle hh = nullptr; long long k = 0; };      // where a slot answered on its own lives

// The range prob0 .. prob0+count-1 of the caller's batch as a batched call sees it.
struct ResidentRange {
    std::vector<ResidentSeg> seg;       // the half-segments, slot order: they get the batched launches
    std::vector<long long> slots;       // the slots answered on their own, by the per-problem entry point
    std::vector<AloneAt> alone;         // empty, or count entries: where each such slot lives (hh null: not on its own)
    const Plan& plan() const { return seg[0].hh->plan; }      // of the half that holds prob0
};
int resident_range(enlsip_gn_handle h, int64_t prob0, int64_t count, ResidentRange& r) {
    return map_resident(h, prob0, count, false, [&](const ResidentSeg& sg) {
        if (!sg.alone) { r.seg.push_back(sg); return; }
        if (r.alone.empty()) r.alone.resize((size_t)count);
        for (long long j = sg.j0; j < sg.j0 + sg.cnt; ++j) {
            r.slots.push_back(j);
            r.alone[(size_t)j] = {sg.hh, sg.k0 + (j - sg.j0)};
        }
    });
}

// launch(sg) for every half-segment of the range, enqueued on its own handle's stream.  A segment on another handle than h (the
// second pipeline half) is ordered after what the caller enqueued on h's stream, and its error text is reported on h.
template <class Launch>
int for_each_segment(enlsip_gn_handle h, const ResidentRange& r, Launch&& launch) {
    for (const ResidentSeg& sg : r.seg) {
        int rc = sg.hh != h ? fork_after(h, sg.hh->stream) : 0;
        if (rc) return rc;
        rc = launch(sg);
        if (rc && sg.hh != h) h->err = sg.hh->err;
        if (rc) return rc;
    }
    return 0;
}

// what a handle of the range must hold for the calls that work on the Jacobian side (re-solve, Newton direction, diag of F_J2)
int needs_jacobian_side(enlsip_gn_handle h, enlsip_gn_handle hh) {
    if (hh->constraints_only) { h->err = GN_ERR_CONSTRAINTS_ONLY; return -1; }
    if (!hh->last.rx || (hh->plan.t > 0 && !hh->last.cx)) { h->err = "rx / cx of the last solve are not available"; return -1; }
    return 0;
}

// One array of a host-buffer form, staged through a device buffer of the call's own.  A NULL array stays NULL on the device; one of
// zero bytes (t_max = 0) does not.
struct Staged { void* host; size_t bytes; bool in, out; void* dev; };

// Carves the arrays in order from buf (64 bytes of slack) and copies in those marked `in`: a call's outputs too, so that the
// slots it leaves alone come back as they were.
int stage_in(enlsip_gn_handle h, DevBuf& buf, Staged* a, int na) {
    GN_HIP(hipSetDevice(h->device));
    size_t tot = 64;
    for (int i = 0; i < na; ++i) tot += a[i].host ? (size_t)rup((long long)a[i].bytes, 8) : 0;
    int rc = grow(h, buf, tot);
    if (rc) return rc;
    char* at = (char*)buf.p;
    for (int i = 0; i < na; ++i) {
        if (!a[i].host) continue;
        a[i].dev = at;
        at += rup((long long)a[i].bytes, 8);
        if (a[i].in && a[i].bytes) GN_HIP(hipMemcpyAsync(a[i].dev, a[i].host, a[i].bytes, hipMemcpyHostToDevice, h->stream));
    }
    return 0;
}

// copies back those marked `out` and synchronises
int stage_out(enlsip_gn_handle h, const Staged* a, int na) {
    for (int i = 0; i < na; ++i)
        if (a[i].dev && a[i].out && a[i].bytes) GN_HIP(hipMemcpyAsync(a[i].host, a[i].dev, a[i].bytes, hipMemcpyDeviceToHost, h->stream));
    GN_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

// the NULL checks of the getters of what a batched call recorded on the handle
#define GN_GETTER_CHECK(h, out) if (!(h)) return -1; if (!(out)) { (h)->err = #out " is NULL"; return -2; }

// the ten enlsip_gn_get_*_form getters
int get_form(enlsip_gn_handle h, Form which, int* form) {
    GN_GETTER_CHECK(h, form)
    *form = h->form[which];
    return 0;
}

// the constraint count of problem `prob` of the resident batch: its own t after a ragged solve, the batch's t otherwise
int prob_t(enlsip_gn_handle h, int64_t prob) {
    return h->h_tk.empty() ? (int)h->plan.t : h->h_tk[(size_t)prob];
}

struct FactorView {
    const double* F; int ld; int rows, cols, k; const double* tau; const long long* jpvt;
};

// F_A, F_L11: compact LAPACK factors; F_J2: the pivoted factors of R0 (rows = kp) — its Q part
// is only the small Qt, the big Q0 lives in the CAQR storage.
int view(enlsip_gn_handle h, int which, int64_t prob, FactorView& v) {
    const Plan& P = h->plan;
    const ProbState& st = h->h_state[prob];
    const int t = prob_t(h, prob), kA = (int)std::min<long long>(P.n, t);     // F_L11 of a ragged batch has ld t (its own)
    switch (which) {
        case ENLSIP_GN_FACTOR_A:
            v = {h->FA + prob * P.sFA, (int)P.n, (int)P.n, t, kA, h->tauA + prob * P.sTauA,
                 h->jpvtA + prob * P.sJA};
            return 0;
        case ENLSIP_GN_FACTOR_L11:
            v = {h->FL + prob * P.sFL, t, t, kA, std::min(t, kA),
                 h->tauL + prob * P.sTauL, h->jpvtL + prob * P.sJL};
            return 0;
        case ENLSIP_GN_FACTOR_J2:
            if (h->constraints_only) { h->err = GN_ERR_CONSTRAINTS_ONLY; return -1; }
            v = {h->Rt + prob * P.sRt, P.ldr, st.kp, st.n2, st.kp, h->tauJ + prob * P.sTauJ, h->jpvtJ + prob * P.sJJ};
            return 0;
        default:
            h->err = "bad factor selector";
            return -2;
    }
}

}  // namespace

extern "C" {

int enlsip_gn_factor_shape(enlsip_gn_handle h, int which, int64_t prob, int64_t* rows, int64_t* cols) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    FactorView v;
    rc = view(h, which, prob, v);
    if (rc) return rc;
    if (rows) *rows = v.k;       // rows of F.R
    if (cols) *cols = v.cols;
    return 0;
}

int enlsip_gn_get_R(enlsip_gn_handle h, int which, int64_t prob, double* R, int64_t ldr) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    FactorView v;
    rc = view(h, which, prob, v);
    if (rc) return rc;
    if (!R) return -4;
    if (ldr < v.k) return -5;
    GN_HIP(hipSetDevice(h->device));
    if (v.k == 0 || v.cols == 0) return 0;
    GN_HIP(hipMemcpy2DAsync(R, (size_t)ldr * 8, v.F, (size_t)v.ld * 8, (size_t)v.k * 8, (size_t)v.cols,
                            hipMemcpyDeviceToHost, h->stream));
    GN_HIP(hipStreamSynchronize(h->stream));
    for (int c = 0; c < v.cols; ++c)
        for (int r = c + 1; r < v.k; ++r) R[r + (size_t)c * ldr] = 0.0;   // triu
    return 0;
}

int enlsip_gn_get_diagR(enlsip_gn_handle h, int which, int64_t prob, double* diag) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    FactorView v;
    rc = view(h, which, prob, v);
    if (rc) return rc;
    if (!diag) return -4;
    GN_HIP(hipSetDevice(h->device));
    const int kd = std::min(v.k, v.cols);
    if (kd == 0) return 0;
    GN_HIP(hipMemcpy2DAsync(diag, 8, v.F, (size_t)(v.ld + 1) * 8, 8, (size_t)kd, hipMemcpyDeviceToHost, h->stream));
    GN_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int enlsip_gn_get_jpvt(enlsip_gn_handle h, int which, int64_t prob, int64_t* jpvt) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    FactorView v;
    rc = view(h, which, prob, v);
    if (rc) return rc;
    if (!jpvt) return -4;
    GN_HIP(hipSetDevice(h->device));
    if (v.cols == 0) return 0;
    GN_HIP(hipMemcpyAsync(jpvt, v.jpvt, (size_t)v.cols * 8, hipMemcpyDeviceToHost, h->stream));
    GN_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

// direction: trans = 1 -> Q' v, 0 -> Q v
static int apply_q_common(enlsip_gn_handle h, int which, int64_t prob, double* vhost, int trans) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    FactorView v;
    rc = view(h, which, prob, v);
    if (rc) return rc;
    if (!vhost) return -4;
    GN_HIP(hipSetDevice(h->device));
    const Plan& P = h->plan;
    hipStream_t s = h->stream;
    double* dv = h->vec + prob * P.sVec;         // ldw doubles (+ ldw staging)
    double* stage = dv + P.ldw;
    if (which != ENLSIP_GN_FACTOR_J2) {
        const int len = v.rows;
        if (len == 0) return 0;
        // vec buffer has 2*ldw doubles; lengths here are n or t (<= 1024): use the scratch buffer when larger
        rc = grow(h, h->scratch, (size_t)std::max(len, 1) * 8);
        if (rc) return rc;
        double* x = (double*)h->scratch.p;
        GN_HIP(hipMemcpyAsync(x, vhost, (size_t)len * 8, hipMemcpyHostToDevice, s));
        if (v.k > 0) {
            if (trans) hipLaunchKernelGGL(k_vec_reflectors<true>, dim3(1), dim3(64), 0, s, v.F, v.ld, v.tau, v.k, len, x);
            else hipLaunchKernelGGL(k_vec_reflectors<false>, dim3(1), dim3(64), 0, s, v.F, v.ld, v.tau, v.k, len, x);
        }
        GN_HIP(hipMemcpyAsync(vhost, x, (size_t)len * 8, hipMemcpyDeviceToHost, s));
        GN_HIP(hipStreamSynchronize(s));
        return 0;
    }
    // F_J2.Q = Q0 * diag(Qt, I): Q' v = [Qt' (Q0' v)[1:kp] ; (Q0' v)[kp+1:m]]
    const ProbState& st = h->h_state[prob];
    const int m = (int)P.m, kp = st.kp;
    const int npan = (kp + PB - 1) / PB;
    if ((size_t)prob < h->held.size()) h->held[(size_t)prob] = {};      // the vector buffer of a held batched re-solve is overwritten
    GN_HIP(hipMemcpyAsync(stage, vhost, (size_t)m * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pad_copy, dim3((P.ldw + 255) / 256), dim3(256), 0, s, stage, m, P.ldw, dv);
    if (trans) {
        caqr_apply_ext(h, dv, (int)prob, npan, false);
        if (kp > 0) hipLaunchKernelGGL(k_vec_reflectors<true>, dim3(1), dim3(64), 0, s, v.F, v.ld, v.tau, kp, kp, dv);
    } else {
        if (kp > 0) hipLaunchKernelGGL(k_vec_reflectors<false>, dim3(1), dim3(64), 0, s, v.F, v.ld, v.tau, kp, kp, dv);
        caqr_apply_ext(h, dv, (int)prob, npan, true);
    }
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(vhost, dv, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    return 0;
}

int enlsip_gn_apply_qt(enlsip_gn_handle h, int which, int64_t prob, double* v) {
    return apply_q_common(h, which, prob, v, 1);
}
int enlsip_gn_apply_q(enlsip_gn_handle h, int which, int64_t prob, double* v) {
    return apply_q_common(h, which, prob, v, 0);
}

int enlsip_gn_get_JQ1(enlsip_gn_handle h, int64_t prob, double* out, int64_t ld) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    if (!out) return -3;
    const Plan& P = h->plan;
    if (ld < P.m) return -4;
    if (!h->last.J) { h->err = "J of the last solve is not available"; return -1; }
    GN_HIP(hipSetDevice(h->device));
    rc = grow(h, h->scratch, (size_t)P.ldw * (P.n + 1) * 8);
    if (rc) return rc;
    JQ1Args qa = jq1_args(h, h->last.J, h->last.ldj, h->last.strideJ, h->last.rx);
    qa.W = (double*)h->scratch.p; qa.sW = 0; qa.prob0 = (int)prob;
    launch_jq1(qa, 1, h->stream);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpy2DAsync(out, (size_t)ld * 8, h->scratch.p, (size_t)P.ldw * 8, (size_t)P.m * 8, (size_t)P.n,
                            hipMemcpyDeviceToHost, h->stream));
    GN_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int enlsip_gn_resolve(enlsip_gn_handle h, int64_t prob, int64_t dimA, int64_t dimJ2, int64_t code, double* p,
                      double* b, double* d) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    if (code != 1 && code != -1) { h->err = "code must be 1 or -1"; return -5; }
    if (h->constraints_only) { h->err = GN_ERR_CONSTRAINTS_ONLY; return -1; }
    const Plan& P = h->plan;
    const ProbState st0 = h->h_state[prob];
    const int tk = prob_t(h, prob);       // the problem's own t (ragged batch); the stage below runs with the batch's t_max
    if (dimA < 0 || dimA > std::min<long long>(P.n, tk)) { h->err = "dimA out of range"; return -3; }
    if (dimJ2 < 0 || dimJ2 > st0.kp) { h->err = "dimJ2 out of range"; return -4; }
    if (code == 1 && st0.rankA != tk) { h->err = "code 1 requires rankA == t"; return -5; }
    GN_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int m = (int)P.m, n = (int)P.n, t = (int)P.t;
    if ((size_t)prob < h->held.size()) h->held[(size_t)prob] = {};      // p1 and the vector buffer of a held batched re-solve are overwritten
    // (1) b, p1 with the requested dimA / code: the constraint stage of this one problem again, through the SAME kernels that
    //     produced its factors (register / LDS / wave forms rewrite them bit for bit; the distributed form of many constraints
    //     keeps its factors and redoes only b and p1).  The kernels reset rankJ2 / dimJ2 / status in the state record:
    //     restored below.
    if (h->cdist.valid) {
        ConstraintArgs ca{};
        ca.n = n; ca.t = t; ca.kA = P.kA; ca.m = m; ca.eps_rank = h->eps_rank;
        ca.dimA_override = (int)dimA; ca.code_override = (int)code; ca.prob0 = (int)prob;
        ca.At = h->last.At; ca.ldat = h->last.ldat; ca.strideAt = h->last.strideAt; ca.cx = h->last.cx; ca.stride_cx = t;
        ca.FA = h->FA; ca.sFA = P.sFA; ca.tauA = h->tauA; ca.sTauA = P.sTauA; ca.jpvtA = h->jpvtA; ca.sJA = P.sJA;
        ca.FL = h->FL; ca.sFL = P.sFL; ca.tauL = h->tauL; ca.sTauL = P.sTauL; ca.jpvtL = h->jpvtL; ca.sJL = P.sJL;
        ca.TA = h->TA; ca.sTA = P.sTA; ca.p1 = h->p1; ca.sP1 = P.sP1; ca.bvec = h->bvec; ca.sB = P.sB;
        ca.state = h->state;
        ca.fa_done = 1; ca.fl_done = 1; ca.need_T = 0;
        ca.Lmat = h->cdist.L; ca.ldL = h->cdist.ldL; ca.sL = h->cdist.sL; ca.qb = h->cdist.qb; ca.sQb = h->cdist.sQb;
        launch_constraint((int)std::max<long long>(n, t), 1, s, ca, h->h_tk.empty() ? nullptr : (const int*)h->tkbuf.p);
    } else {
        rc = run_constraint_stage(h, 1, m, n, t, h->last.At, h->last.ldat, h->last.strideAt, h->last.cx, h->eps_rank, dimA, (int)prob,
                                  (int)code);
        if (rc) return rc;
    }
    // (2) d_temp = -J1 p1 - rx into the vector buffer, (3) Q0' d, (4) Qt' on the leading kp entries
    double* dv = h->vec + prob * P.sVec;
    hipLaunchKernelGGL(k_dtemp, dim3((P.ldw + 255) / 256), dim3(256), 0, s, h->W + prob * P.sW, P.ldw, m,
                       st0.rankA, h->p1 + prob * P.sP1, h->last.slice(prob, 1).rx, dv);
    const int kp = st0.kp, npan = (kp + PB - 1) / PB;
    caqr_apply_ext(h, dv, (int)prob, npan, false);
    if (kp > 0)
        hipLaunchKernelGGL(k_vec_reflectors<true>, dim3(1), dim3(64), 0, s, h->Rt + prob * P.sRt, P.ldr,
                           h->tauJ + prob * P.sTauJ, kp, kp, dv);
    // restore rankJ2 (constraint kernel zeroed it) before the solve kernel reads the state
    ProbState fix = st0;
    fix.code = (int)code; fix.dimA = (int)dimA;
    GN_HIP(hipMemcpyAsync(h->state + prob, &fix, sizeof(ProbState), hipMemcpyHostToDevice, s));
    GN_HIP(hipStreamSynchronize(s));
    // (5) triangular solve with dimJ2, scatter, p = Q1 [p1; p2]
    StageOut out;
    rc = place_dev(h, h->out_stage, out, 1LL, (long long)m, (long long)n, (long long)t);
    if (rc) return rc;
    double *dp = out.p, *db = out.b, *dd = out.d;
    FinalArgs fa{};
    fa.m = m; fa.n = n; fa.t = t; fa.kA = P.kA; fa.ldw = P.ldw; fa.ldr = P.ldr; fa.eps_rank = h->eps_rank;
    fa.dimJ2_override = (int)dimJ2; fa.refactor = 0; fa.prob0 = (int)prob; fa.dsrc = dv;
    fa.W = h->W; fa.sW = P.sW; fa.Rt = h->Rt; fa.sRt = P.sRt; fa.tauJ = h->tauJ; fa.sTauJ = P.sTauJ;
    fa.jpvtJ = h->jpvtJ; fa.sJJ = P.sJJ; fa.FA = h->FA; fa.sFA = P.sFA; fa.tauA = h->tauA; fa.sTauA = P.sTauA;
    fa.p1 = h->p1; fa.sP1 = P.sP1; fa.bvec = h->bvec; fa.sB = P.sB; fa.zsave = nullptr; fa.sZ = 0;
    // outputs are indexed with the true problem index inside the kernel: offset the bases back
    fa.p_out = dp - prob * (long long)n; fa.sPo = n;
    fa.b_out = db - prob * (long long)t; fa.sBo = t;
    fa.d_out = dd - prob * (long long)m; fa.sDo = m;
    fa.state = h->state;
    launch_pivot((int)std::min<long long>(m, n), 1, s, fa);
    GN_HIP(hipGetLastError());
    if (p) GN_HIP(hipMemcpyAsync(p, dp, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (b && tk > 0) GN_HIP(hipMemcpyAsync(b, db, (size_t)tk * 8, hipMemcpyDeviceToHost, s));
    if (d) GN_HIP(hipMemcpyAsync(d, dd, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipMemcpyAsync(h->h_state + prob, h->state + prob, sizeof(ProbState), hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
