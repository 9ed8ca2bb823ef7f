// enlsip_gn_newton_direction: device part of newton_search_direction (src/enlsip_functions.jl:348-423).  Included at the end of
// enlsip_gn.hip (after gn_tsqr.inc, whose k_tsqr_q1 forms p = F_A.Q [p1; p2]).

extern "C" {

int enlsip_gn_newton_direction(enlsip_gn_handle h, int64_t prob, const double* Gamma, int64_t ldg, double* p, int64_t* not_posdef) {
    int rc = need_factors(h, prob);
    if (rc) return rc;
    GN_TRY
    if (h->constraints_only) { h->err = GN_ERR_CONSTRAINTS_ONLY; return -1; }
    if (!Gamma) { h->err = "Gamma is NULL"; return -3; }
    if (!p) { h->err = "p is NULL"; return -5; }
    if (!h->last.J || !h->last.rx) { h->err = "J / rx of the last solve are not available"; return -1; }
    const Plan& P = h->plan;
    const int m = (int)P.m, n = (int)P.n, t = prob_t(h, prob);      // the problem's own t (ragged batch)
    if (ldg < n) { h->err = "ldg < n"; return -4; }
    const ProbState st0 = h->h_state[prob];
    const int rankA = st0.rankA, n2 = n - rankA;
    // rank-deficient working set (t > rankA, :371-373, :396-399): p1 = F_L11.P[1:rankA, 1:rankA] * dp1 is what the constraint
    // stage leaves in p1 for code -1 ((P w)[i] = w[j] with p[j] = i, the same scatter as :144), and E is re-indexed with F_L11.p
    // on both sides.  F_L11.p has min(n, t) entries and :402-403 then read rows up to n: the reference itself is defined for
    // t >= n only (a BoundsError otherwise), and so is this entry point.
    const bool permute_E = (t != rankA);
    if (permute_E && t < n) {
        h->err = "rank-deficient working set with t < n: newton_search_direction indexes E[F_L11.p, F_L11.p] (t x t) up to row n — out of bounds in the reference too";
        return -7;
    }
    if (not_posdef) *not_posdef = 0;
    GN_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    // b, p1 with the default dimensions (a re-solve may have left truncated ones), state record restored afterwards
    if (t > 0) {
        if (h->cdist.valid) { h->err = "newton direction after the distributed constraint stage is not supported"; return -7; }
        rc = run_constraint_stage(h, 1, m, n, P.t, h->last.At, h->last.ldat, h->last.strideAt, h->last.cx, h->eps_rank, -1, (int)prob, 0);
        if (rc) return rc;
        GN_HIP(hipMemcpyAsync(h->state + prob, &st0, sizeof(ProbState), hipMemcpyHostToDevice, s));
    }
    const double* p1 = h->p1 + prob * P.sP1;
    if (n2 == 0) {      // :374-376: the reference returns p1 as it is
        GN_HIP(hipMemcpyAsync(p, p1, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        GN_HIP(hipStreamSynchronize(s));
        return 0;
    }
    NewtonWs N;
    rc = place_dev(h, h->newton, N, (long long)n, (long long)n2, (long long)rankA);
    if (rc) return rc;
    double *dG = N.G, *dQ = N.Q, *dT1 = N.T1, *dE = N.E, *dW22 = N.W22, *dUt = N.Ut, *dW21 = N.W21, *dg = N.g, *dd = N.d, *dp2 = N.p2,
           *dpo = N.pout;
    int* dflag = N.flag;
    GN_HIP(hipMemcpy2DAsync(dG, (size_t)n * 8, Gamma, (size_t)ldg * 8, (size_t)n * 8, (size_t)n, hipMemcpyHostToDevice, s));
    GN_HIP(hipMemsetAsync(dflag, 0, 16, s));
    // J * F_A.Q into scratch (:384)
    rc = grow(h, h->scratch, (size_t)P.ldw * (P.n + 1) * 8);
    if (rc) return rc;
    double* JQ = (double*)h->scratch.p;
    {
        JQ1Args qa{};
        qa.m = m; qa.n = n; qa.kA = P.kA; qa.ldw = P.ldw;
        qa.J = h->last.J; qa.ldj = h->last.ldj; qa.strideJ = h->last.strideJ; qa.rx = h->last.rx; qa.stride_rx = P.m;
        qa.FA = h->FA; qa.sFA = P.sFA; qa.TA = h->TA; qa.sTA = P.sTA; qa.p1 = h->p1; qa.sP1 = P.sP1;
        qa.W = JQ; qa.sW = 0; qa.state = h->state; qa.prob0 = (int)prob;
        launch_jq1(qa, 1, s);
    }
    const double* J1 = JQ;
    const double* J2 = JQ + (size_t)rankA * P.ldw;
    const double* FA = h->FA + prob * P.sFA;
    const double* tauA = h->tauA + prob * P.sTauA;
    auto g2 = [](int M, int N) { return dim3((unsigned)((M + 15) / 16), (unsigned)((N + 15) / 16)); };
    // E = Q' (Gam Q)
    hipLaunchKernelGGL(k_newton_q1, dim3((unsigned)n), dim3(64), 0, s, FA, n, tauA, P.kA, dQ);
    hipLaunchKernelGGL(k_newton_gemm<false>, g2(n, n), dim3(256), 0, s, n, n, n, dG, (long long)n, dQ, (long long)n, (const double*)nullptr, 0LL, dT1, (long long)n);
    hipLaunchKernelGGL(k_newton_gemm<true>, g2(n, n), dim3(256), 0, s, n, n, n, dQ, (long long)n, dT1, (long long)n, (const double*)nullptr, 0LL, dE, (long long)n);
    if (permute_E) {            // E = E[F_L11.p, F_L11.p]  (:396-399; kA = n entries here)
        hipLaunchKernelGGL(k_newton_perm, dim3((unsigned)n), dim3(256), 0, s, n, dE, h->jpvtL + prob * P.sJL, dT1);
        std::swap(dE, dT1);
    }
    // W22 = E22 + J2' J2 ; W21 = E21 + J2' J1
    hipLaunchKernelGGL(k_newton_gemm<true>, g2(n2, n2), dim3(256), 0, s, n2, n2, m, J2, (long long)P.ldw, J2, (long long)P.ldw,
                       dE + rankA + (size_t)rankA * n, (long long)n, dW22, (long long)n2);
    if (rankA > 0)
        hipLaunchKernelGGL(k_newton_gemm<true>, g2(n2, rankA), dim3(256), 0, s, n2, rankA, m, J2, (long long)P.ldw, J1, (long long)P.ldw,
                           dE + rankA, (long long)n, dW21, (long long)n2);
    // d = -W21 p1 - J2' rx
    hipLaunchKernelGGL(k_gemv_t, dim3(((unsigned)n2 + 3) / 4), dim3(256), 0, s, J2, (long long)P.ldw, m, n2,
                       h->last.slice(prob, 1).rx, dg);
    hipLaunchKernelGGL(k_newton_rhs, dim3(((unsigned)n2 + 255) / 256), dim3(256), 0, s, n2, rankA, dW21, (long long)n2, p1, dg, dd);
    // cholesky(sW22), the two triangular solves, p = Q [p1; p2]
    hipLaunchKernelGGL(k_newton_chol, dim3(1), dim3(1024), 0, s, n2, dW22, (long long)n2, dUt, dflag);
    int hflag[2] = {0, 0};
    GN_HIP(hipMemcpyAsync(hflag, dflag, 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    if (hflag[0]) {     // :417-420: p = zeros, error = true
        for (int i = 0; i < n; ++i) p[i] = 0.0;
        if (not_posdef) *not_posdef = 1;
        return 0;
    }
    hipLaunchKernelGGL(k_newton_solve, dim3(1), dim3(256), 0, s, n2, dW22, (long long)n2, dUt, dd, dp2, dflag);
    hipLaunchKernelGGL(k_tsqr_q1, dim3(1), dim3(64), 0, s, FA, n, tauA, P.kA, p1, h->state + prob, dp2, dpo);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpyAsync(p, dpo, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    return 0;
    GN_CATCH(h)
}

}  // extern "C"
