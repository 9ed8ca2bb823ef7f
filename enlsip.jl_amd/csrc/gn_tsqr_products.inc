// Consumers around the subproblem on a row-sharded J (config C4): J' (rx + J p), J p, the three sums of the line search and the
// two multiplier estimates, across the shards of the handle's last enlsip_gn_solve_tsqr.  Kernels: gn_kernels_tsqr_products.hpp.
// One message per rank ([header | g_g (n) | three sums], tp_msg_len(n) doubles), ONE exchange step (tsqr_exchange_step, the one
// enlsip_gn_solve_tsqr uses), and a combine that adds the messages in rank order on every rank: every rank holds the same bits.
// The replicated stage (F_A.Q' on an n-vector, the triangular solves) is k_lagrange on the resident F_A.
// Included by enlsip_gn.hip after gn_tsqr.inc and gn_lagrange.inc.

namespace {

struct TsqrProductsScratch {
    double *p = nullptr, *Jp = nullptr, *partial = nullptr, *send = nullptr, *recv = nullptr, *out = nullptr, *b = nullptr, *Ap = nullptr;
    void carve(Carver& c, long long m, long long n, long long nchunks, long long len, long long G) {
        c.take(p, "p", (size_t)n, 16); c.take(Jp, "J p", (size_t)std::max<long long>(m, 1), 16);
        c.take(partial, "chunk partials", (size_t)std::max<long long>(nchunks, 1) * (size_t)(n + TP_SUMS), 16);
        c.take(send, "send", (size_t)len, 16); c.take(recv, "recv", (size_t)(G * len), 16);
        c.take(out, "combined", (size_t)(n + TP_SUMS + 1), 16); c.take(b, "Q' g", (size_t)n, 16); c.take(Ap, "A p", 1024, 16);
    }
};

long long tp_chunks(long long m) { return (m + TP_CH - 1) / TP_CH; }

// the shard's message into dmsg, on the handle's stream: dp (device, n) or NULL; Jp_out (device, m) receives J p when dp is given
void tp_enqueue_local(enlsip_gn_handle h, long long m, long long n, const double* dJ, long long ldj, const double* drx, const double* dp,
                      double* Jp_out, double* partial, double* dmsg, double rank_tag, double ranks) {
    hipStream_t s = h->stream;
    const long long nch = tp_chunks(m);
    if (m > 0) {
        if (dp) hipLaunchKernelGGL(k_tp_rows, dim3((unsigned)((m + 63) / 64)), dim3(256), 0, s, dJ, ldj, (int)m, (int)n, dp, Jp_out);
        hipLaunchKernelGGL(k_tp_cols, dim3((unsigned)nch, (unsigned)((n + TP_CPG - 1) / TP_CPG) + 1), dim3(256), 0, s, dJ, ldj, (int)m,
                           (int)n, drx, dp ? (const double*)Jp_out : (const double*)nullptr, partial);
    }
    hipLaunchKernelGGL(k_tp_reduce, dim3((unsigned)((n + TP_SUMS + 255) / 256)), dim3(256), 0, s, (const double*)partial, nch, (int)n, dmsg,
                       rank_tag, ranks);
}

void tp_enqueue_combine(enlsip_gn_handle h, long long G, long long n, const double* dmsgs, double* out) {
    hipLaunchKernelGGL(k_tp_combine, dim3((unsigned)((n + TP_SUMS + 255) / 256)), dim3(256), 0, h->stream, dmsgs, tp_msg_len(n), (int)G,
                       (int)n, out);
}

int tp_bad_headers(enlsip_gn_handle h, double bad) {
    if (bad == 0.0) return 0;
    h->err = "tsqr_products: a gathered message names another n, another rank count or another slot than the one it arrived in";
    return -13;
}

// -7 / -15 of the collective forms: nothing is launched
int tp_need_shard(enlsip_gn_handle h) {
    if (!h) return -1;
    if (h->tsqr_stage != 2 || !h->have_plan || !h->last.J || !h->last.rx) {
        h->err = "no row shard is resident: the handle's last successful solve must be enlsip_gn_solve_tsqr (or a tsqr combine after "
                 "its local stage)";
        return -7;
    }
    if (h->tsqr_e != 0 || h->tsqr_E != 0 || h->sc_eJ != 0 || h->sc_eA != 0) {
        h->err = "the last sharded solve was rescaled (enlsip_gn_tsqr_get_scale): the resident factors may be those of a scaled "
                 "copy, and these calls are outside the magnitude contract";
        return -15;
    }
    if (h->tsqr_broken || (h->tsqr_ranks > 1 && !h->tsqr_comm && !h->tsqr_xfn)) { h->err = "no communicator on this handle"; return -1; }
    return 0;
}

// local products of the resident shard, the exchange, the combine: X.out = [J'(rx + J p) | three sums | bad headers] on the device,
// enqueued (the callback transport synchronises before it calls out, as in the solve).  p: host (n) or NULL.
int tp_collective(enlsip_gn_handle h, const double* p, double* dJp, TsqrProductsScratch& X) {
    const BatchOperands& in = h->last;
    const long long m = in.m, n = in.n, G = h->tsqr_ranks, len = tp_msg_len(n);
    GN_HIP(hipSetDevice(h->device));
    int rc = place_dev(h, h->tsqr_prod, X, m, n, tp_chunks(m), len, G);
    if (rc) return rc;
    hipStream_t s = h->stream;
    if (p) GN_HIP(hipMemcpyAsync(X.p, p, (size_t)n * 8, hipMemcpyHostToDevice, s));
    tp_enqueue_local(h, m, n, in.J, in.ldj, in.rx, p ? X.p : nullptr, dJp ? dJp : X.Jp, X.partial, X.send, (double)(h->tsqr_rank + 1),
                     (double)G);
    GN_HIP(hipGetLastError());
    rc = tsqr_exchange_step(h, X.send, X.recv, (size_t)len);
    if (rc) return rc;
    tp_enqueue_combine(h, G, n, X.recv, X.out);
    GN_HIP(hipGetLastError());
    return 0;
}

// k_lagrange on the shard's resident F_A (the arithmetic of enlsip_gn_first_lagrange / _second_lagrange).  mode 1: vec = grad (n);
// mode 2: vec = (F_A.Q' J'(rx + J p))[1:t], formed from the whole J: no column of a factored W is read, so there is no -7 here.
void tp_enqueue_lagrange(enlsip_gn_handle h, int mode, const double* dvec, const double* ddiag, double eps_rank, const LagrangeScratch& L) {
    const Plan& P = h->plan;
    LagrangeArgs a{};
    a.mode = mode; a.n = (int)P.n; a.t = (int)P.t; a.kA = P.kA; a.rank_solve = P.kA;
    a.FA = h->FA; a.tauA = h->tauA; a.jpvtA = h->jpvtA;
    a.vec = dvec; a.cx = h->last.cx; a.diag_scale = ddiag; a.eps_rank = eps_rank; a.lambda = L.lambda; a.scal = L.scal;
    hipLaunchKernelGGL(k_lagrange, dim3(1), dim3(256), 0, h->stream, a);
}

}  // namespace

extern "C" {

int64_t enlsip_gn_tsqr_products_msg_len(int64_t n) { return n < 1 ? 0 : (int64_t)tp_msg_len(n); }

int enlsip_gn_tsqr_products_local_dev(enlsip_gn_handle h, int64_t m_loc, int64_t n, const double* dJ, int64_t ldj, const double* drx,
                                      const double* dp, double* dJp, double* dmsg) {
    if (!h) return -1;
    GN_TRY
    if (m_loc < 0 || m_loc > (1LL << 27) - 4096) { h->err = "m_loc out of range (0 .. 2^27 - 4096)"; return -2; }
    if (n < 1 || n > 1024) { h->err = "n must be in 1..1024 in this build"; return -3; }
    if (m_loc > 0 && !dJ) { h->err = "dJ is NULL"; return -4; }
    if (ldj < m_loc) { h->err = "ldj < m_loc"; return -5; }
    if (m_loc > 0 && !drx) { h->err = "drx is NULL"; return -6; }
    if (!dmsg) { h->err = "dmsg is NULL"; return -8; }
    GN_HIP(hipSetDevice(h->device));
    TsqrProductsScratch X;
    int rc = place_dev(h, h->tsqr_prod, X, (long long)m_loc, (long long)n, tp_chunks(m_loc), tp_msg_len(n), 1LL);
    if (rc) return rc;
    // a handle with a communicator states its rank and rank count; one without leaves both open (0) for the caller to fill in
    const bool attached = h->tsqr_comm || h->tsqr_xfn;
    tp_enqueue_local(h, m_loc, n, dJ, ldj, drx, dp, dJp ? dJp : X.Jp, X.partial, dmsg, attached ? (double)(h->tsqr_rank + 1) : 0.0,
                     attached ? (double)h->tsqr_ranks : 0.0);
    GN_HIP(hipGetLastError());
    GN_HIP(hipStreamSynchronize(h->stream));
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_tsqr_products_combine_dev(enlsip_gn_handle h, int64_t G, int64_t n, const double* dmsgs, double* grad, double* sums) {
    if (!h) return -1;
    GN_TRY
    if (G < 1 || G > (1 << 20)) { h->err = "G out of range"; return -2; }
    if (n < 1 || n > 1024) { h->err = "n must be in 1..1024 in this build"; return -3; }
    if (!dmsgs) { h->err = "dmsgs is NULL"; return -4; }
    GN_HIP(hipSetDevice(h->device));
    TsqrProductsScratch X;
    int rc = place_dev(h, h->tsqr_prod, X, 0LL, (long long)n, 0LL, tp_msg_len(n), 1LL);
    if (rc) return rc;
    tp_enqueue_combine(h, G, n, dmsgs, X.out);
    GN_HIP(hipGetLastError());
    std::vector<double> out((size_t)n + TP_SUMS + 1);
    GN_HIP(hipMemcpyAsync(out.data(), X.out, out.size() * 8, hipMemcpyDeviceToHost, h->stream));
    GN_HIP(hipStreamSynchronize(h->stream));
    rc = tp_bad_headers(h, out[(size_t)n + TP_SUMS]);
    if (rc) return rc;
    if (grad) memcpy(grad, out.data(), (size_t)n * 8);
    if (sums) memcpy(sums, out.data() + n, TP_SUMS * 8);
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_tsqr_products(enlsip_gn_handle h, const double* p, double* dJp, double* grad, double* sums, double* Ap) {
    int rc = tp_need_shard(h);
    if (rc) return rc;
    GN_TRY
    const long long n = h->last.n, t = h->last.t;
    if (Ap && !p) { h->err = "Ap needs p"; return -3; }
    if (Ap && t > 0 && !h->last.At) { h->err = "A' of the last solve is not available"; return -1; }
    TsqrProductsScratch X;
    rc = tp_collective(h, p, dJp, X);
    if (rc) return rc;
    hipStream_t s = h->stream;
    if (Ap && t > 0) {      // (A p)[i] = sum_r At[r + i ldat] p[r] on the replicated active rows: no exchange
        hipLaunchKernelGGL(k_gemv_t, dim3(((unsigned)t + 3) / 4), dim3(256), 0, s, h->last.At, h->last.ldat, (int)n, (int)t,
                           (const double*)X.p, X.Ap);
        GN_HIP(hipGetLastError());
    }
    std::vector<double> out((size_t)n + TP_SUMS + 1), ap((size_t)std::max<long long>(t, 1));
    GN_HIP(hipMemcpyAsync(out.data(), X.out, out.size() * 8, hipMemcpyDeviceToHost, s));
    if (Ap && t > 0) GN_HIP(hipMemcpyAsync(ap.data(), X.Ap, (size_t)t * 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    rc = tp_bad_headers(h, out[(size_t)n + TP_SUMS]);
    if (rc) return rc;
    if (grad) memcpy(grad, out.data(), (size_t)n * 8);
    if (sums) memcpy(sums, out.data() + n, TP_SUMS * 8);
    if (Ap && t > 0) memcpy(Ap, ap.data(), (size_t)t * 8);
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_tsqr_first_lagrange(enlsip_gn_handle h, const double* grad_fx, const double* diag_scale, double eps_rank,
                                  double* lambda, double* grad_res) {
    int rc = tp_need_shard(h);
    if (rc) return rc;
    GN_TRY
    const long long n = h->last.n, t = h->last.t;
    if (t > 0 && !lambda) { h->err = "lambda is NULL"; return -6; }
    if (t > 0 && !h->last.cx) { h->err = "cx of the last solve is not available"; return -1; }
    GN_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    TsqrProductsScratch X;
    LagrangeScratch L;
    rc = lagrange_scratch(h, 1, L);
    if (rc) return rc;
    const double* dgrad = L.gp;
    if (grad_fx) {
        GN_HIP(hipMemcpyAsync(L.gp, grad_fx, (size_t)n * 8, hipMemcpyHostToDevice, s));
    } else {      // J' rx over the ranks
        rc = tp_collective(h, nullptr, nullptr, X);
        if (rc) return rc;
        dgrad = X.out;
    }
    std::vector<double> out((size_t)n + TP_SUMS + 1, 0.0), lam((size_t)std::max<long long>(t, 1));
    double scal[2] = {0.0, 0.0};
    if (t > 0) {
        if (diag_scale) GN_HIP(hipMemcpyAsync(L.diag, diag_scale, (size_t)t * 8, hipMemcpyHostToDevice, s));
        tp_enqueue_lagrange(h, 1, dgrad, diag_scale ? L.diag : nullptr, eps_rank, L);
        GN_HIP(hipGetLastError());
        GN_HIP(hipMemcpyAsync(lam.data(), L.lambda, (size_t)t * 8, hipMemcpyDeviceToHost, s));
        GN_HIP(hipMemcpyAsync(scal, L.scal, 16, hipMemcpyDeviceToHost, s));
    }
    if (!grad_fx) GN_HIP(hipMemcpyAsync(out.data(), X.out, out.size() * 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    if (!grad_fx) {
        rc = tp_bad_headers(h, out[(size_t)n + TP_SUMS]);
        if (rc) return rc;
    }
    if (t == 0) {      // no constraints: grad_res = ||grad|| (Q = I, prankA = 0), as enlsip_gn_first_lagrange
        if (grad_res) {
            const double* g = grad_fx ? grad_fx : out.data();
            double q = 0.0;
            for (long long i = 0; i < n; ++i) q += g[i] * g[i];
            *grad_res = std::sqrt(q);
        }
        return 0;
    }
    memcpy(lambda, lam.data(), (size_t)t * 8);
    if (grad_res) *grad_res = scal[0];
    if ((int)scal[1] & 1) { h->err = "singular triangular system in the multiplier estimate"; return 1; }
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_tsqr_second_lagrange(enlsip_gn_handle h, const double* p_gn, const double* diag_scale, double eps_rank,
                                   double* lambda) {
    int rc = tp_need_shard(h);
    if (rc) return rc;
    GN_TRY
    const long long n = h->last.n, t = h->last.t;
    if (!p_gn) { h->err = "p_gn is NULL"; return -3; }
    if (t > 0 && !lambda) { h->err = "lambda is NULL"; return -6; }
    GN_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    TsqrProductsScratch X;
    LagrangeScratch L;
    rc = lagrange_scratch(h, 1, L);
    if (rc) return rc;
    rc = tp_collective(h, p_gn, nullptr, X);      // also with t == 0: the peers are in the exchange
    if (rc) return rc;
    std::vector<double> lam((size_t)std::max<long long>(t, 1));
    double scal[2] = {0.0, 0.0}, bad = 0.0;
    if (t > 0) {
        // b = (F_A.Q' J'(rx + J p_gn))[1:t]
        GN_HIP(hipMemcpyAsync(X.b, X.out, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_tp_qt, dim3(1), dim3(64), 0, s, (const double*)h->FA, (int)n, (const double*)h->tauA, h->plan.kA, X.b);
        if (diag_scale) GN_HIP(hipMemcpyAsync(L.diag, diag_scale, (size_t)t * 8, hipMemcpyHostToDevice, s));
        tp_enqueue_lagrange(h, 2, X.b, diag_scale ? L.diag : nullptr, eps_rank, L);
        GN_HIP(hipGetLastError());
        GN_HIP(hipMemcpyAsync(lam.data(), L.lambda, (size_t)t * 8, hipMemcpyDeviceToHost, s));
        GN_HIP(hipMemcpyAsync(scal, L.scal, 16, hipMemcpyDeviceToHost, s));
    }
    GN_HIP(hipMemcpyAsync(&bad, X.out + n + TP_SUMS, 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    rc = tp_bad_headers(h, bad);
    if (rc) return rc;
    if (t == 0) return 0;
    memcpy(lambda, lam.data(), (size_t)t * 8);
    if ((int)scal[1] & 1) { h->err = "singular triangular system in the multiplier estimate"; return 1; }
    return 0;
    GN_CATCH(h)
}

}  // extern "C"
