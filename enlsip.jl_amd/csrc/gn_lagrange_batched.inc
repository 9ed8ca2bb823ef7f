// Batched consumers of a solve: gradient, J p / A p and the two multiplier estimates over a contiguous range of the resident batch
// (kernels: gn_kernels_lagrange_batched.hpp).  The range and the driver of its half-segments are the shared ones of
// gn_accessors.inc (resident_range, for_each_segment).  Included at the end of enlsip_gn.hip, after gn_lagrange.inc.

namespace {

enum { CONS_GRADIENT = 0, CONS_JTIMES = 1, CONS_FIRST = 2, CONS_SECOND = 3 };

// device buffers of one call; slot 0 = problem prob0 of the caller's batch
struct ConsumerIO {
    const double* in;       // grad_fx (first estimate, may be null), p (jacobian_times), p_gn (second estimate)
    const double* diag;     // diag_scale (estimates), may be null
    double eps_rank;
    double* out0;           // grad / Jp / lambda
    double* out1;           // Ap / grad_res
    int* status;            // estimates, may be null
};

// what every handle of the range must hold for the consumer (the per-problem entry points' checks)
int consumer_needs(enlsip_gn_handle h, enlsip_gn_handle hh, int kind, const ConsumerIO& io) {
    const char* no_j = "J / rx of the last solve are not available";
    switch (kind) {
        case CONS_GRADIENT:
            if (!hh->last.J || !hh->last.rx) { h->err = no_j; return -1; }
            return 0;
        case CONS_JTIMES:
            if (!hh->last.J) { h->err = "J of the last solve is not available"; return -1; }
            if (io.out1 && hh->plan.t > 0 && !hh->last.At) { h->err = "A' of the last solve is not available"; return -1; }
            return 0;
        case CONS_FIRST:
            if (hh->constraints_only && !io.in) {
                h->err = GN_ERR_CONSTRAINTS_ONLY ": pass grad_fx; no second estimate";
                return -1;
            }
            if (hh->plan.t > 0 && !hh->last.cx) { h->err = "cx of the last solve is not available"; return -1; }
            if (!io.in && (!hh->last.J || !hh->last.rx)) { h->err = no_j; return -1; }
            return 0;
        default:
            if (hh->constraints_only) {
                h->err = GN_ERR_CONSTRAINTS_ONLY ": pass grad_fx; no second estimate";
                return -1;
            }
            if (!hh->last.J || !hh->last.rx) { h->err = no_j; return -1; }
            return 0;
    }
}

// temporaries of a segment in lagb_scr: flag word | status (when the caller passes none) | grad (first, no grad_fx) | rx + J p (m) |
// J1'(.) (t_max)
struct LagbScratch {
    int *flag = nullptr, *status = nullptr;
    double *g = nullptr, *y = nullptr, *bv = nullptr;
    void carve(Carver& c, long long cnt, long long m, long long n, long long tmax) {
        c.take(flag, "flag", 1, 256); c.take(status, "status", (size_t)cnt, 256);
        c.take(g, "grad", (size_t)(cnt * n), 256); c.take(y, "rx + J p", (size_t)(cnt * m)); c.take(bv, "J1'(.)", (size_t)(cnt * std::max(tmax, 1LL)));
    }
};

// Enqueues the consumer for one segment on its handle's stream: at most three launches whatever the segment's size.
int consumer_launch(enlsip_gn_handle hh, int kind, const ResidentSeg& sg, const ConsumerIO& io, bool small) {
    enlsip_gn_handle h = hh;       // GN_HIP reports on `h`
    const Plan& P = hh->plan;
    const long long m = P.m, n = P.n, tmax = P.t, k0 = sg.k0, j0 = sg.j0, cnt = sg.cnt;
    const int* tk = hh->h_tk.empty() ? nullptr : (const int*)hh->tkbuf.p + k0;
    const BatchOperands in = hh->last.slice(k0, cnt);
    const bool est = kind == CONS_FIRST || kind == CONS_SECOND;
    LagbScratch scr;
    int rc = place_dev(hh, hh->lagb_scr, scr, cnt, m, n, tmax);
    if (rc) return rc;
    if (est) {
        rc = grow_pinned(hh, hh->h_lagflag, sizeof(int));
        if (rc) return rc;
    }
    hipStream_t s = hh->stream;
    const unsigned cn = (unsigned)cnt;
    auto jt = [&](const double* x, long long sx, double* y) {          // J' x
        hipLaunchKernelGGL(k_gemv_t_batched, dim3((unsigned)(n + 3) / 4, cn), dim3(256), 0, s, in.J, in.ldj, in.strideJ, (int)m, (int)n,
                           (const int*)nullptr, x, sx, y, n);
    };
    switch (kind) {
        case CONS_GRADIENT:
            jt(in.rx, m, io.out0 + j0 * n);
            break;
        case CONS_JTIMES:
            if (io.out0)
                hipLaunchKernelGGL(k_gemv_n_add_batched, dim3((unsigned)(m + 255) / 256, cn), dim3(256), 0, s, in.J, in.ldj, in.strideJ,
                                   (int)m, (int)n, io.in + j0 * n, n, (const double*)nullptr, 0LL, io.out0 + j0 * m, m);
            if (io.out1 && tmax > 0)     // (A p)[i] = sum_r At[r + i * ldat] p[r]: A' is stored n x t; slots past t_k are 0
                hipLaunchKernelGGL(k_gemv_t_batched, dim3((unsigned)(tmax + 3) / 4, cn), dim3(256), 0, s, in.At, in.ldat, in.strideAt,
                                   (int)n, (int)tmax, tk, io.in + j0 * n, n, io.out1 + j0 * tmax, tmax);
            break;
        default: {
            LagrangeBatchArgs a{};
            a.mode = kind == CONS_FIRST ? 1 : 2;
            a.count = (int)cnt; a.n = (int)n; a.t_max = (int)tmax; a.tk = tk; a.state = hh->state + k0;
            a.FA = hh->FA + k0 * P.sFA; a.sFA = P.sFA; a.tauA = hh->tauA + k0 * P.sTauA; a.sTauA = P.sTauA;
            a.jpvtA = hh->jpvtA + k0 * P.sJA; a.sJA = P.sJA;
            a.cx = in.cx; a.scx = in.t;
            a.diag_scale = io.diag ? io.diag + j0 * tmax : nullptr;
            a.eps_rank = io.eps_rank;
            a.lambda = io.out0 + j0 * tmax;
            a.grad_res = (kind == CONS_FIRST && io.out1) ? io.out1 + j0 : nullptr;
            a.status = io.status ? io.status + j0 : scr.status;
            a.flag = scr.flag;
            GN_HIP(hipMemsetAsync(scr.flag, 0, sizeof(int), s));
            if (kind == CONS_FIRST) {
                if (io.in) {
                    a.vec = io.in + j0 * n;
                } else {       // gradient from the resident J, rx
                    double* g = scr.g;
                    jt(in.rx, m, g);
                    a.vec = g;
                }
                a.svec = n;
            } else {
                double *y = scr.y, *bv = scr.bv;
                hipLaunchKernelGGL(k_gemv_n_add_batched, dim3((unsigned)(m + 255) / 256, cn), dim3(256), 0, s, in.J, in.ldj, in.strideJ,
                                   (int)m, (int)n, io.in + j0 * n, n, in.rx, m, y, m);       // rx + J p
                if (tmax > 0)
                    hipLaunchKernelGGL(k_gemv_t_batched, dim3((unsigned)(tmax + 3) / 4, cn), dim3(256), 0, s, (const double*)hh->W + k0 * P.sW,
                                       (long long)P.ldw, P.sW, (int)m, (int)tmax, tk, (const double*)y, m, bv, tmax);   // J1' (.)
                a.vec = bv;
                a.svec = tmax;
            }
            if (small)
                hipLaunchKernelGGL(k_lagrange_wave, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, s, a);
            else
                hipLaunchKernelGGL(k_lagrange_batched, dim3(cn), dim3(256), 0, s, a);
            GN_HIP(hipMemcpyAsync(hh->h_lagflag.p, scr.flag, sizeof(int), hipMemcpyDeviceToHost, s));
        }
    }
    GN_HIP(hipGetLastError());
    return 0;
}

// rc of a per-problem estimate -> the batched status (0, 1 singular, 2 rank beyond the solve's); other codes are errors
int per_problem_status(int rc, int& st) {
    st = rc == 0 ? 0 : rc == 1 ? 1 : rc == -7 ? 2 : -1;
    return st < 0 ? rc : 0;
}

// Problems of the range that live on a rescue handle (or on a handle whose one problem was rescaled in place) are answered by the
// per-problem entry point; their slots are overwritten with its results.  Returns the status OR of the whole range in *flagged.
int consumer_per_problem(enlsip_gn_handle h, int kind, int64_t prob0, int64_t count, const ResidentRange& r, const ConsumerIO& io,
                         bool& flagged) {
    const Plan& P = r.plan();
    const long long m = P.m, n = P.n, tmax = P.t;
    hipStream_t s = h->stream;
    std::vector<double> in((size_t)n), dg((size_t)std::max(tmax, 1LL)), o0((size_t)std::max({m, n, tmax, 1LL})),
        o1((size_t)std::max(tmax, 1LL));
    std::vector<int> st_all;
    const bool est = kind == CONS_FIRST || kind == CONS_SECOND;
    if (est) {      // statuses of the batched launch: the rescued slots' entries are replaced below
        st_all.assign((size_t)count, 0);
        for (const ResidentSeg& sg : r.seg) {
            LagbScratch scr;      // the segment's launch grew it: placed again
            const int rc = place_dev(sg.hh, sg.hh->lagb_scr, scr, sg.cnt, m, n, tmax);
            if (rc) return rc;
            const int* src = io.status ? io.status + sg.j0 : scr.status;
            GN_HIP(hipMemcpy(st_all.data() + sg.j0, src, (size_t)sg.cnt * sizeof(int), hipMemcpyDeviceToHost));
        }
    }
    for (long long j : r.slots) {
        const int64_t gp = prob0 + j;
        if (io.in) GN_HIP(hipMemcpy(in.data(), io.in + j * n, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (io.diag && tmax > 0) GN_HIP(hipMemcpy(dg.data(), io.diag + j * tmax, (size_t)tmax * 8, hipMemcpyDeviceToHost));
        std::fill(o0.begin(), o0.end(), 0.0);
        std::fill(o1.begin(), o1.end(), 0.0);
        int rc = 0, st = 0;
        switch (kind) {
            case CONS_GRADIENT:
                rc = enlsip_gn_gradient(h, gp, o0.data());
                if (rc) return rc;
                GN_HIP(hipMemcpyAsync(io.out0 + j * n, o0.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
                break;
            case CONS_JTIMES:
                rc = enlsip_gn_jacobian_times(h, gp, in.data(), io.out0 ? o0.data() : nullptr, io.out1 ? o1.data() : nullptr);
                if (rc) return rc;
                if (io.out0) GN_HIP(hipMemcpyAsync(io.out0 + j * m, o0.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
                if (io.out1 && tmax > 0) GN_HIP(hipMemcpyAsync(io.out1 + j * tmax, o1.data(), (size_t)tmax * 8, hipMemcpyHostToDevice, s));
                break;
            default: {
                double gres = 0.0;
                rc = kind == CONS_FIRST
                         ? enlsip_gn_first_lagrange(h, gp, io.in ? in.data() : nullptr, io.diag ? dg.data() : nullptr, io.eps_rank,
                                                    o0.data(), &gres)
                         : enlsip_gn_second_lagrange(h, gp, in.data(), io.diag ? dg.data() : nullptr, io.eps_rank, o0.data());
                rc = per_problem_status(rc, st);
                if (rc) return rc;
                st_all[(size_t)j] = st;
                if (tmax > 0) GN_HIP(hipMemcpyAsync(io.out0 + j * tmax, o0.data(), (size_t)tmax * 8, hipMemcpyHostToDevice, s));
                if (kind == CONS_FIRST && io.out1) GN_HIP(hipMemcpyAsync(io.out1 + j, &gres, 8, hipMemcpyHostToDevice, s));
                if (io.status) GN_HIP(hipMemcpyAsync(io.status + j, &st, sizeof(int), hipMemcpyHostToDevice, s));
                GN_HIP(hipStreamSynchronize(s));       // gres / st live on this frame
            }
        }
    }
    GN_HIP(hipStreamSynchronize(s));
    flagged = false;
    for (int v : st_all) flagged = flagged || v != 0;
    return 0;
}

// The batched consumer on device buffers: validation, launches on the halves that own the range, one synchronisation per half,
// then the per-problem route for rescued problems.  0, 1 (some estimate flagged) or a negative argument / state error.
int consumer_dev(enlsip_gn_handle h, int kind, int64_t prob0, int64_t count, const ConsumerIO& io) {
    if (!h) return -1;
    // the halves that hold the range get the batched launches; the slots answered on their own, the per-problem entry point
    ResidentRange r;
    int rc = resident_range(h, prob0, count, r);
    if (rc) return rc;
    const Plan& P = r.plan();
    const bool est = kind == CONS_FIRST || kind == CONS_SECOND;
    switch (kind) {
        case CONS_GRADIENT: if (!io.out0) { h->err = "dgrad is NULL"; return -4; } break;
        case CONS_JTIMES:
            if (!io.in) { h->err = "dp is NULL"; return -4; }
            if (!io.out0 && !io.out1) { h->err = "dJp and dAp are both NULL"; return -4; }
            break;
        case CONS_FIRST: if (!io.out0 && P.t > 0) { h->err = "dlambda is NULL"; return -4; } break;
        default:
            if (!io.in) { h->err = "dp_gn is NULL"; return -4; }
            if (!io.out0 && P.t > 0) { h->err = "dlambda is NULL"; return -4; }
    }
    for (const ResidentSeg& sg : r.seg) {
        rc = consumer_needs(h, sg.hh, kind, io);
        if (rc) return rc;
    }
    GN_HIP(hipSetDevice(h->device));
    const bool small = h->lagrange_small && P.n <= 64 && P.t <= 64;
    if (est) h->form[FORM_CONSUMER] = small ? 1 : 0;
    rc = for_each_segment(h, r, [&](const ResidentSeg& sg) { return consumer_launch(sg.hh, kind, sg, io, small); });
    if (rc) return rc;
    bool flagged = false;
    for (const ResidentSeg& sg : r.seg) {
        GN_HIP(hipStreamSynchronize(sg.hh->stream));
        if (est) flagged = flagged || *(const int*)sg.hh->h_lagflag.p != 0;
    }
    if (!r.slots.empty()) {
        rc = consumer_per_problem(h, kind, prob0, count, r, io, flagged);
        if (rc) return rc;
    }
    return flagged ? 1 : 0;
}

// The host-buffer forms: inputs staged into lagb_io (never in_stage, which the resident J / rx of a host solve live in), the
// device form, outputs copied back.
int consumer_host(enlsip_gn_handle h, int kind, int64_t prob0, int64_t count, const double* in, const double* diag, double eps_rank,
                  double* out0, double* out1, int* status) {
    if (!h) return -1;
    ResidentRange r;
    int rc = resident_range(h, prob0, count, r);
    if (rc) return rc;
    const Plan& P = r.plan();
    const long long m = P.m, n = P.n, tmax = P.t;
    const bool est = kind == CONS_FIRST || kind == CONS_SECOND;
    const size_t c = (size_t)count, dbl = c * 8;
    const size_t b_o0 = dbl * (kind == CONS_GRADIENT ? n : kind == CONS_JTIMES ? m : tmax), b_o1 = dbl * (kind == CONS_JTIMES ? tmax : 1);
    // a NULL pointer keeps its meaning; an output of zero entries (t_max = 0) still passes the NULL checks
    Staged a[5] = {{(void*)in, dbl * n, true, false}, {est ? (void*)diag : nullptr, dbl * tmax, true, false}, {out0, b_o0, false, true},
                   {(kind == CONS_JTIMES || kind == CONS_FIRST) ? out1 : nullptr, b_o1, false, true},
                   {est ? status : nullptr, c * sizeof(int), false, true}};
    rc = stage_in(h, h->lagb_io, a, 5);
    if (rc) return rc;
    const ConsumerIO io{(double*)a[0].dev, (double*)a[1].dev, eps_rank, (double*)a[2].dev, (double*)a[3].dev, (int*)a[4].dev};
    rc = consumer_dev(h, kind, prob0, count, io);
    if (rc < 0) return rc;
    const int rc2 = stage_out(h, a, 5);
    return rc2 ? rc2 : rc;
}

}  // namespace

extern "C" {

int enlsip_gn_gradient_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, double* dgrad) {
    if (!h) return -1;
    GN_TRY
    return consumer_dev(h, CONS_GRADIENT, prob0, count, {nullptr, nullptr, 0.0, dgrad, nullptr, nullptr});
    GN_CATCH(h)
}

int enlsip_gn_jacobian_times_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* dp, double* dJp,
                                         double* dAp) {
    if (!h) return -1;
    GN_TRY
    return consumer_dev(h, CONS_JTIMES, prob0, count, {dp, nullptr, 0.0, dJp, dAp, nullptr});
    GN_CATCH(h)
}

int enlsip_gn_first_lagrange_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* dgrad_fx,
                                         const double* ddiag_scale, double eps_rank, double* dlambda, double* dgrad_res,
                                         int* dstatus) {
    if (!h) return -1;
    GN_TRY
    return consumer_dev(h, CONS_FIRST, prob0, count, {dgrad_fx, ddiag_scale, eps_rank, dlambda, dgrad_res, dstatus});
    GN_CATCH(h)
}

int enlsip_gn_second_lagrange_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* dp_gn,
                                          const double* ddiag_scale, double eps_rank, double* dlambda, int* dstatus) {
    if (!h) return -1;
    GN_TRY
    return consumer_dev(h, CONS_SECOND, prob0, count, {dp_gn, ddiag_scale, eps_rank, dlambda, nullptr, dstatus});
    GN_CATCH(h)
}

int enlsip_gn_gradient_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, double* grad) {
    if (!h) return -1;
    GN_TRY
    if (!grad) { h->err = "grad is NULL"; return -4; }
    return consumer_host(h, CONS_GRADIENT, prob0, count, nullptr, nullptr, 0.0, grad, nullptr, nullptr);
    GN_CATCH(h)
}

int enlsip_gn_jacobian_times_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* p, double* Jp, double* Ap) {
    if (!h) return -1;
    GN_TRY
    if (!p) { h->err = "p is NULL"; return -4; }
    if (!Jp && !Ap) { h->err = "Jp and Ap are both NULL"; return -4; }
    return consumer_host(h, CONS_JTIMES, prob0, count, p, nullptr, 0.0, Jp, Ap, nullptr);
    GN_CATCH(h)
}

int enlsip_gn_first_lagrange_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* grad_fx,
                                     const double* diag_scale, double eps_rank, double* lambda, double* grad_res, int* status) {
    if (!h) return -1;
    GN_TRY
    return consumer_host(h, CONS_FIRST, prob0, count, grad_fx, diag_scale, eps_rank, lambda, grad_res, status);
    GN_CATCH(h)
}

int enlsip_gn_second_lagrange_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* p_gn,
                                      const double* diag_scale, double eps_rank, double* lambda, int* status) {
    if (!h) return -1;
    GN_TRY
    if (!p_gn) { h->err = "p_gn is NULL"; return -4; }
    return consumer_host(h, CONS_SECOND, prob0, count, p_gn, diag_scale, eps_rank, lambda, nullptr, status);
    GN_CATCH(h)
}

int enlsip_gn_get_consumer_form(enlsip_gn_handle h, int* form) { return get_form(h, FORM_CONSUMER, form); }

}  // extern "C"
