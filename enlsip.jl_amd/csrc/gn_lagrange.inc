// Multiplier estimates and gradient on the resident data of the last solve (SURVEY §8f #1).
// Included at the end of enlsip_gn.hip.

namespace {

// device scratch of the per-problem consumers in h->lag: slots of 1024 doubles (n, t <= 1024 in this build), then the residual vector
struct LagrangeScratch {
    double *gp = nullptr, *b = nullptr, *lambda = nullptr, *scal = nullptr, *diag = nullptr, *r = nullptr;
    void carve(Carver& c, long long m) {
        c.take(gp, "grad / p", 1024); c.take(b, "b", 1024); c.take(lambda, "lambda", 1024); c.take(scal, "scalars", 1024);
        c.take(diag, "diag_scale", 1024); c.take(r, "residual", (size_t)std::max<long long>(m, 1));
    }
};
int lagrange_scratch(enlsip_gn_handle h, long long m, LagrangeScratch& L) { return place_dev(h, h->lag, L, m); }

}  // namespace

extern "C" {

int enlsip_gn_gradient(enlsip_gn_handle h, int64_t prob, double* grad) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    if (!grad) return -3;
    if (!h->last.J || !h->last.rx) { h->err = "J / rx of the last solve are not available"; return -1; }
    const Plan& P = h->plan;
    const BatchOperands in = h->last.slice(prob, 1);
    GN_HIP(hipSetDevice(h->device));
    LagrangeScratch L;
    rc = lagrange_scratch(h, P.m, L);
    if (rc) return rc;
    double* d = L.gp;
    hipStream_t s = h->stream;
    hipLaunchKernelGGL(k_gemv_t, dim3(((unsigned)P.n + 3) / 4), dim3(256), 0, s, in.J, in.ldj, (int)P.m, (int)P.n, in.rx, d);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(grad, d, (size_t)P.n * 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    return 0;
}

int enlsip_gn_jacobian_times(enlsip_gn_handle h, int64_t prob, const double* p, double* Jp, double* Ap) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    if (!p) return -3;
    if (!Jp && !Ap) return -4;
    if (!h->last.J) { h->err = "J of the last solve is not available"; return -1; }
    const Plan& P = h->plan;
    const BatchOperands in = h->last.slice(prob, 1);
    const int n = (int)P.n, t = prob_t(h, prob), m = (int)P.m;       // Ap: the problem's own active rows
    GN_HIP(hipSetDevice(h->device));
    LagrangeScratch L;
    rc = lagrange_scratch(h, m, L);
    if (rc) return rc;
    double *dp = L.gp, *dAp = L.b, *dJp = L.r;      // n, t, m
    hipStream_t s = h->stream;
    GN_HIP(hipMemcpyAsync(dp, p, (size_t)n * 8, hipMemcpyHostToDevice, s));
    if (Jp) {
        hipLaunchKernelGGL(k_gemv_n_add, dim3(((unsigned)m + 255) / 256), dim3(256), 0, s, in.J, in.ldj, m, n, dp,
                           (const double*)nullptr, dJp);
        GN_HIP(hipMemcpyAsync(Jp, dJp, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    }
    if (Ap && t > 0) {
        if (!in.At) { h->err = "A' of the last solve is not available"; return -1; }
        // (A p)[i] = sum_r At[r + i * ldat] p[r]: A' is stored n x t
        hipLaunchKernelGGL(k_gemv_t, dim3(((unsigned)t + 3) / 4), dim3(256), 0, s, in.At, in.ldat, n, t, dp, dAp);
        GN_HIP(hipMemcpyAsync(Ap, dAp, (size_t)t * 8, hipMemcpyDeviceToHost, s));
    }
    GN_HIP(hipGetLastError());
    GN_HIP(hipStreamSynchronize(s));
    return 0;
}

// Ap = A p with the FULL constraint Jacobian (l x n, host): the product of the line-search set-up that involves the inactive
// rows too (src/enlsip_functions.jl:2227).  A is staged; no resident factors are needed.
int enlsip_gn_full_constraints_times(enlsip_gn_handle h, int64_t l, int64_t n, const double* A, int64_t lda, const double* p,
                                     double* Ap) {
    if (!h) return -1;
    if (l < 0 || l > (1LL << 27)) { h->err = "l out of range"; return -2; }
    if (n < 1 || n > 1024) { h->err = "n must be in 1..1024 in this build"; return -3; }
    if (l == 0) return 0;
    if (!A) { h->err = "A is NULL"; return -4; }
    if (lda < l) { h->err = "lda < l"; return -5; }
    if (!p) { h->err = "p is NULL"; return -6; }
    if (!Ap) { h->err = "Ap is NULL"; return -7; }
    GN_HIP(hipSetDevice(h->device));
    int rc = grow(h, h->scratch, ((size_t)l * n + (size_t)n + (size_t)l) * 8);
    if (rc) return rc;
    double* dA = (double*)h->scratch.p;
    double* dp = dA + (size_t)l * n;
    double* dy = dp + n;
    hipStream_t s = h->stream;
    GN_HIP(hipMemcpy2DAsync(dA, (size_t)l * 8, A, (size_t)lda * 8, (size_t)l * 8, (size_t)n, hipMemcpyHostToDevice, s));
    GN_HIP(hipMemcpyAsync(dp, p, (size_t)n * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_gemv_n_add, dim3(((unsigned)l + 255) / 256), dim3(256), 0, s, dA, (long long)l, (int)l, (int)n, dp,
                       (const double*)nullptr, dy);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(Ap, dy, (size_t)l * 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    return 0;
}

// out = M * F_A.Q for a host matrix M with the row count of the last solve: `J * F_A.Q` of the reference's consumers
// (src/enlsip_functions.jl:384, :526, :1249) for any such matrix, on the resident reflectors of F_A.
int enlsip_gn_matrix_times_QA(enlsip_gn_handle h, int64_t prob, int64_t rows, const double* M, int64_t ldm, double* out,
                              int64_t ldo) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    const Plan& P = h->plan;
    if (rows != P.m) { h->err = "matrix_times_QA: the matrix must have the row count m of the last solve"; return -3; }
    if (!M) { h->err = "M is NULL"; return -4; }
    if (ldm < rows) { h->err = "ldm < rows"; return -5; }
    if (!out) { h->err = "out is NULL"; return -6; }
    if (ldo < rows) { h->err = "ldo < rows"; return -7; }
    GN_HIP(hipSetDevice(h->device));
    const size_t wsz = (size_t)P.ldw * (P.n + 1), msz = (size_t)P.m * P.n;
    rc = grow(h, h->scratch, (wsz + msz + (size_t)P.m) * 8);
    if (rc) return rc;
    double* W = (double*)h->scratch.p;
    double* dM = W + wsz;
    double* dz = dM + msz;                       // a zero "rx": the kernel also forms -J1 p1 - rx, which nobody reads here
    hipStream_t s = h->stream;
    GN_HIP(hipMemcpy2DAsync(dM, (size_t)P.m * 8, M, (size_t)ldm * 8, (size_t)P.m * 8, (size_t)P.n, hipMemcpyHostToDevice, s));
    GN_HIP(hipMemsetAsync(dz, 0, (size_t)P.m * 8, s));
    JQ1Args qa{};
    qa.m = (int)P.m; qa.n = (int)P.n; qa.kA = P.kA; qa.ldw = P.ldw;
    // the kernel indexes its inputs with the problem index: offset the bases of this one staged matrix back
    qa.J = dM - prob * (long long)msz; qa.ldj = P.m; qa.strideJ = (long long)msz; qa.rx = dz - prob * P.m; qa.stride_rx = P.m;
    qa.FA = h->FA; qa.sFA = P.sFA; qa.TA = h->TA; qa.sTA = P.sTA; qa.p1 = h->p1; qa.sP1 = P.sP1;
    qa.W = W; qa.sW = 0; qa.state = h->state; qa.prob0 = (int)prob;
    launch_jq1(qa, 1, s);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpy2DAsync(out, (size_t)ldo * 8, W, (size_t)P.ldw * 8, (size_t)P.m * 8, (size_t)P.n, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    return 0;
}

static int lagrange_common(enlsip_gn_handle h, int64_t prob, int mode, const double* host_vec, const double* diag_scale,
                           double eps_rank, double* lambda, double* grad_res) {
    const Plan& P = h->plan;
    const int n = (int)P.n, t = prob_t(h, prob), m = (int)P.m;       // lambda: the problem's own t (ragged batch)
    if (!lambda) return -6;
    if (h->constraints_only && (mode == 2 || !host_vec)) {
        h->err = "only F_A / F_L11 are resident (enlsip_gn_factor_constraints): pass grad_fx; no second estimate";
        return -1;
    }
    if (t == 0) {
        if (grad_res && mode == 1) {
            // no constraints: grad_res = ||grad|| (b = Q' grad with Q = I, prankA = 0)
            double s = 0.0;
            if (host_vec) for (int i = 0; i < n; ++i) s += host_vec[i] * host_vec[i];
            *grad_res = std::sqrt(s);
        }
        return 0;
    }
    GN_HIP(hipSetDevice(h->device));
    LagrangeScratch L;
    int rc = lagrange_scratch(h, m, L);
    if (rc) return rc;
    double* d = L.gp;
    hipStream_t s = h->stream;
    LagrangeArgs a{};
    a.mode = mode; a.n = n; a.t = t; a.kA = std::min(n, t); a.rank_solve = h->h_state[prob].rankA;
    a.FA = h->FA + prob * P.sFA; a.tauA = h->tauA + prob * P.sTauA; a.jpvtA = h->jpvtA + prob * P.sJA;
    const BatchOperands in = h->last.slice(prob, 1);
    a.cx = in.cx;
    a.eps_rank = eps_rank; a.lambda = L.lambda; a.scal = L.scal;
    a.diag_scale = nullptr;
    if (diag_scale) {
        GN_HIP(hipMemcpyAsync(L.diag, diag_scale, (size_t)t * 8, hipMemcpyHostToDevice, s));
        a.diag_scale = L.diag;
    }
    if (mode == 1) {
        if (!a.cx) { h->err = "cx of the last solve is not available"; return -1; }
        if (host_vec) {
            GN_HIP(hipMemcpyAsync(d, host_vec, (size_t)n * 8, hipMemcpyHostToDevice, s));
        } else {   // gradient from the resident J, rx
            if (!in.J || !in.rx) { h->err = "J / rx of the last solve are not available"; return -1; }
            hipLaunchKernelGGL(k_gemv_t, dim3(((unsigned)n + 3) / 4), dim3(256), 0, s, in.J, in.ldj, m, n, in.rx, d);
        }
        a.vec = d;
    } else {
        if (!host_vec) return -3;
        if (!in.J || !in.rx) { h->err = "J / rx of the last solve are not available"; return -1; }
        GN_HIP(hipMemcpyAsync(d, host_vec, (size_t)n * 8, hipMemcpyHostToDevice, s));          // p_gn
        hipLaunchKernelGGL(k_gemv_n_add, dim3(((unsigned)m + 255) / 256), dim3(256), 0, s, in.J, in.ldj, m, n, d, in.rx,
                           L.r);   // rx + J p
        hipLaunchKernelGGL(k_gemv_t, dim3(((unsigned)t + 3) / 4), dim3(256), 0, s, h->W + prob * P.sW, (long long)P.ldw, m, t,
                           L.r, L.b);                                                       // J1' (.)
        a.vec = L.b;
    }
    hipLaunchKernelGGL(k_lagrange, dim3(1), dim3(256), 0, s, a);
    GN_HIP(hipGetLastError());
    double scal[2] = {0.0, 0.0};
    GN_HIP(hipMemcpyAsync(lambda, L.lambda, (size_t)t * 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipMemcpyAsync(scal, L.scal, 16, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    if (grad_res && mode == 1) *grad_res = scal[0];
    const int st = (int)scal[1];
    if (st & 2) { h->err = "second estimate: pseudo-rank under eps_rank exceeds the rank the solve used (J1 columns not resident)"; return -7; }
    if (st & 1) { h->err = "singular triangular system in the multiplier estimate"; return 1; }
    return 0;
}

int enlsip_gn_first_lagrange(enlsip_gn_handle h, int64_t prob, const double* grad_fx, const double* diag_scale,
                             double eps_rank, double* lambda, double* grad_res) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    return lagrange_common(h, prob, 1, grad_fx, diag_scale, eps_rank, lambda, grad_res);
}

int enlsip_gn_second_lagrange(enlsip_gn_handle h, int64_t prob, const double* p_gn, const double* diag_scale,
                              double eps_rank, double* lambda) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    return lagrange_common(h, prob, 2, p_gn, diag_scale, eps_rank, lambda, nullptr);
}

}  // extern "C"
