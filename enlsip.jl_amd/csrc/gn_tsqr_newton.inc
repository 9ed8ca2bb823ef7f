// Newton direction on a row-sharded J: newton_search_direction (src/enlsip_functions.jl:348-423) after its Hessian sums, on what
// the combine stage of a sharded solve leaves resident on every rank (tsqr_combine_core, gn_tsqr.inc) — F_A, tauA, F_L11.p, p1 and
// the state record on the handle; R, Pi and the carried d = F_J2.Q' d_stack of the stacked problem on its sub-handle.  The stages
// E, sW22 and the right-hand side are the batched call's kernels (gn_kernels_newton_batched.hpp) with count = 1; the factorisation
// is either that call's one-workgroup kernel or the device-wide one (gn_kernels_newton_wide.hpp).  No shard is read and nothing is
// exchanged.  Included at the end of enlsip_gn.hip, after gn_newton_batched.inc.

namespace {

// Smallest n2 from which the default takes the device-wide factorisation: the smallest swept n2 from which its slowest run beat the
// one-workgroup form's fastest (tests/probes/tsqr_newton_probe.py; table in DESIGN.md section 7, "Newton direction on the shards").
// 64 is the smallest size the sweep has: below it nothing is measured and the one-workgroup form stays.
constexpr int TSQR_NEWTON_WIDE_MIN_N2 = 64;

struct TsqrNewtonWs {
    double *X = nullptr, *E = nullptr, *rhs = nullptr, *D = nullptr;
    ProbState* st = nullptr;
    int *status = nullptr, *pack = nullptr;      // pack: req | flag, one copy fills both
    void carve(Carver& c, size_t nn, size_t n) {
        c.take(X, "X", nn); c.take(E, "E", nn); c.take(rhs, "rhs", n); c.take(D, "L11", (size_t)NWB_NB * NWB_NB);
        c.take(st, "state", 1, 8); c.take(status, "status", 1); c.take(pack, "pack", 2, 8);
    }
};

// everything the call refuses, before any launch and with nothing written
int tsqr_newton_check(enlsip_gn_handle h, const double* Gamma, int64_t ldg, const double* p) {
    if (!Gamma) { h->err = "Gamma is NULL"; return -3; }
    if (!p) { h->err = "p is NULL"; return -5; }
    if (h->tsqr_stage != 2 || !h->have_plan) {
        h->err = "no sharded solve is resident: the handle's last successful solve must be enlsip_gn_solve_tsqr (or a tsqr combine "
                 "after its local stage)";
        return -7;
    }
    if (ldg < h->plan.n) { h->err = "ldg < n"; return -4; }       // n is the resident sharded solve's: known only from here on
    if (h->tsqr_e != 0 || h->tsqr_E != 0 || h->sc_eJ != 0 || h->sc_eA != 0) {
        h->err = "the last sharded solve was rescaled (enlsip_gn_tsqr_get_scale): the resident factors may be those of a scaled "
                 "copy, and this call is outside the magnitude contract";
        return -15;
    }
    const Plan& P = h->plan;
    const ProbState& st = h->h_state[0];
    if ((int)P.t != st.rankA && P.t < P.n) {
        h->err = "rank-deficient working set with t < n: newton_search_direction indexes E[F_L11.p, F_L11.p] (t x t) up to row n — out "
                 "of bounds in the reference too";
        return -8;
    }
    if (st.n2 > 0 && (!h->sub || !h->sub->have_plan || h->sub->plan.n != st.n2)) {
        h->err = "the stacked problem of the combine stage is not resident on the sub-handle";
        return -7;
    }
    return 0;
}

// dGamma, dp, dstatus: device.  Enqueues on the handle's stream; the caller synchronises.
int tsqr_newton_enqueue(enlsip_gn_handle h, const double* dGamma, int64_t ldg, double* dp, int* dstatus) {
    const Plan& P = h->plan;
    const int n = (int)P.n;
    const ProbState hs = h->h_state[0];
    const int n2 = hs.n2;
    GN_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    // n2 == 0 factors nothing: it never reports the device-wide form
    const bool wide = n2 > 0 && h->newton_wide && (h->newton_wide_forced || n2 >= TSQR_NEWTON_WIDE_MIN_N2);
    h->form[FORM_NEWTON] = wide ? 2 : (n <= 64 ? 1 : 0);
    for (float& ms : h->newton_ms) ms = 0.f;
    h->nwb_timed = false;
    TsqrNewtonWs N;
    int rc = place_dev(h, h->tnw_ws, N, (size_t)n * n, (size_t)n);
    if (rc) return rc;
    int* dst_status = dstatus ? dstatus : N.status;
    if (n2 == 0) {        // :379-381: p1 as it is
        GN_HIP(hipMemcpyAsync(dp, h->p1, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
        GN_HIP(hipMemsetAsync(dst_status, 0, sizeof(int), s));
        return 0;
    }
    enlsip_gn_handle sub = h->sub;
    const Plan& S = sub->plan;
    // one state record for the kernels: rankA, n2, code, dimA are the handle's, kp, rankJ2, dimJ2 the stacked problem's
    const ProbState ss = sub->h_state[0];
    ProbState merged = hs;
    merged.kp = ss.kp; merged.rankJ2 = ss.rankJ2; merged.dimJ2 = ss.dimJ2; merged.status = hs.status | ss.status;
    const int pack[2] = {NW_TAKE, 0};
    const bool timed = h->profiling;
    if (timed) {
        for (hipEvent_t& e : h->nwb_ev)
            if (!e) GN_HIP(hipEventCreate(&e));
        GN_HIP(hipEventRecord(h->nwb_ev[0], s));
    }
    GN_HIP(hipMemcpyAsync(N.st, &merged, sizeof merged, hipMemcpyHostToDevice, s));
    GN_HIP(hipMemcpyAsync(N.pack, pack, sizeof pack, hipMemcpyHostToDevice, s));
    if (timed) GN_HIP(hipEventRecord(h->nwb_ev[1], s));
    NewtonBatchArgs a{};
    a.n = n; a.t = (int)P.t; a.kA = P.kA; a.ldr = S.ldr;
    a.req = N.pack; a.tk = nullptr; a.state = N.st;
    a.FA = h->FA; a.sFA = P.sFA; a.tauA = h->tauA; a.sTauA = P.sTauA;
    a.jpvtL = h->jpvtL; a.sJL = P.sJL; a.p1 = h->p1; a.sP1 = P.sP1;
    a.Rt = sub->Rt; a.sRt = S.sRt; a.jpvtJ = sub->jpvtJ; a.sJJ = S.sJJ;
    a.vec = sub->Rt + (size_t)n2 * S.ldr; a.sVec = S.sVec;      // the right-hand side carried beside R: (F_J2.Q' d_stack)[1:kp]
    a.Gamma = dGamma; a.ldg = ldg; a.strideG = ldg * n;
    a.X = N.X; a.sX = (long long)n * n; a.E = N.E; a.rhs = N.rhs;
    a.p_out = dp; a.status_out = dst_status; a.flag = N.pack + 1;
    const unsigned nvb = (unsigned)((n + NWB_VEC - 1) / NWB_VEC), nt = (unsigned)((n + 15) / 16);
    const size_t slds = newton_side_lds(n);
    GN_LAUNCH_BIG(k_newton_side<false>, dim3(nvb, 1), dim3(256), slds, s, a);
    GN_LAUNCH_BIG(k_newton_side<true>, dim3(nvb, 1), dim3(256), slds, s, a);
    if (timed) GN_HIP(hipEventRecord(h->nwb_ev[2], s));
    hipLaunchKernelGGL(k_newton_w22, dim3(nt * nt + (unsigned)((n + 63) / 64), 1), dim3(64), 0, s, a);
    if (timed) GN_HIP(hipEventRecord(h->nwb_ev[3], s));
    if (!wide) {
        if (n <= 64) hipLaunchKernelGGL(k_newton_chol_batched<64>, dim3(1), dim3(64), 0, s, a);
        else hipLaunchKernelGGL(k_newton_chol_batched<256>, dim3(1), dim3(256), 0, s, a);
    } else {
        const NewtonWideArgs w{n2, N.X, N.D, N.pack + 1};
        for (int j0 = 0; j0 < n2; j0 += NWB_NB) {
            hipLaunchKernelGGL(k_nw_panel, dim3((unsigned)((n2 - j0 + NW_STRIP - 1) / NW_STRIP)), dim3(64), 0, s, w, j0);
            const int rest = n2 - j0 - NWB_NB;
            if (rest > 0) {
                const unsigned nbk = (unsigned)((rest + NW_STRIP - 1) / NW_STRIP);
                hipLaunchKernelGGL(k_nw_syrk, dim3(nbk, nbk), dim3(256), 0, s, w, j0);
            }
        }
        hipLaunchKernelGGL(k_nw_finish, dim3(1), dim3(256), 0, s, a);
    }
    if (timed) GN_HIP(hipEventRecord(h->nwb_ev[4], s));
    GN_HIP(hipGetLastError());
    h->nwb_timed = timed;
    return 0;
}

int tsqr_newton_times(enlsip_gn_handle h) {
    if (!h->nwb_timed) return 0;
    for (int e = 0; e < 4; ++e) GN_HIP(hipEventElapsedTime(&h->newton_ms[e], h->nwb_ev[e], h->nwb_ev[e + 1]));
    return 0;
}

}  // namespace

extern "C" {

int enlsip_gn_tsqr_newton_direction_dev(enlsip_gn_handle h, const double* dGamma, int64_t ldg, double* dp, int* dstatus) {
    if (!h) return -1;
    GN_TRY
    int rc = tsqr_newton_check(h, dGamma, ldg, dp);
    if (rc) return rc;
    rc = tsqr_newton_enqueue(h, dGamma, ldg, dp, dstatus);
    if (rc) return rc;
    GN_HIP(hipStreamSynchronize(h->stream));
    return tsqr_newton_times(h);
    GN_CATCH(h)
}

int enlsip_gn_tsqr_newton_direction(enlsip_gn_handle h, const double* Gamma, int64_t ldg, double* p, int64_t* not_posdef) {
    if (!h) return -1;
    GN_TRY
    int rc = tsqr_newton_check(h, Gamma, ldg, p);
    if (rc) return rc;
    const size_t n = (size_t)h->plan.n;
    int status = 0;
    // staged through a buffer of the call, one copy each way
    Staged a[3] = {{(void*)Gamma, ((n - 1) * (size_t)ldg + n) * 8, true, false}, {p, n * 8, false, true}, {&status, sizeof(int), false, true}};
    rc = stage_in(h, h->tnw_io, a, 3);
    if (rc) return rc;
    rc = tsqr_newton_enqueue(h, (const double*)a[0].dev, ldg, (double*)a[1].dev, (int*)a[2].dev);
    if (rc) return rc;
    rc = stage_out(h, a, 3);
    if (rc) return rc;
    if (not_posdef) *not_posdef = status ? 1 : 0;
    return tsqr_newton_times(h);
    GN_CATCH(h)
}

}  // extern "C"
