// The finite-difference Hessian sums of the Newton branch (src/enlsip_functions.jl:243-328) around the caller's evaluations, on
// the host for one problem and for a batch on the caller's device buffers (kernels: gn_kernels_hessian_batched.hpp; the routines:
// gn_hessian_sums.hpp).  The batched calls need and touch nothing resident: the handle lends its device, its stream and its record
// scratch, in which the sums call places its records (HessianScratch: the per-problem counts and slots and the active lists up; nothing comes down).
// eps1 is formed on the host, once per call, and handed to the kernels.  Included at the end of enlsip_gn.hip.

extern "C" {

int enlsip_gn_hessian_points(int64_t n, int64_t pair0, int64_t npairs, const double* x, double* X) {
    std::string err;
    const int rc = check_hessian_points(err, 1, n, pair0, npairs, x != nullptr, X != nullptr);
    if (rc) return rc;
    hess_points(n, pair0, npairs, x, hess_eps1(), X);
    return 0;
}

int enlsip_gn_hessian_sums(int64_t m, int64_t n, int64_t l, int64_t t, int64_t pair0, int64_t npairs, const int64_t* active,
                           const double* x, const double* F, const double* rx, const double* G, const double* lambda,
                           double* Gamma, int64_t ldg) {
    std::string err;
    const int64_t t_max = std::max<int64_t>(t, 0);      // one problem: its own count bounds it, and t < 0 is -5
    const int64_t strideG = n > 0 && ldg > 0 && ldg <= INT64_MAX / n ? ldg * n : INT64_MAX;
    const int rc = check_hessian_sums(err, {1, m, n, l, t_max, pair0, npairs, ldg, strideG}, &t, active, nullptr, x != nullptr,
                                      F != nullptr, rx != nullptr, G != nullptr, lambda != nullptr, Gamma != nullptr);
    if (rc) return rc;
    hess_sums({m, n, l, t, pair0, npairs, active, x, F, rx, G, lambda}, hess_eps1(), Gamma, ldg);
    return 0;
}

int enlsip_gn_hessian_points_batched_dev(enlsip_gn_handle h, int64_t count, int64_t n, int64_t pair0, int64_t npairs,
                                         const double* dx, double* dX) {
    if (!h) return -1;
    GN_TRY
    const int rc = check_hessian_points(h->err, count, n, pair0, npairs, dx != nullptr, dX != nullptr);
    if (rc) return rc;
    GN_HIP(hipSetDevice(h->device));
    HessianPointsArgs a{};
    a.n = (int)n; a.pair0 = pair0; a.npairs = npairs; a.eps1 = hess_eps1(); a.x = dx; a.X = dX;
    const int64_t blocks = (npairs * 4 * n + 255) / 256;
    hipLaunchKernelGGL(k_hessian_points, dim3((unsigned)count, (unsigned)std::min<int64_t>(blocks, HESS_MAX_GRID_Y)), dim3(256), 0,
                       h->stream, a);
    GN_HIP(hipGetLastError());
    GN_HIP(hipStreamSynchronize(h->stream));
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_hessian_sums_batched_dev(enlsip_gn_handle h, int64_t count, int64_t m, int64_t n, int64_t l, int64_t t_max,
                                       int64_t pair0, int64_t npairs, const int64_t* t, const int64_t* active,
                                       const int64_t* slot, const double* dx, const double* dF, const double* drx,
                                       const double* dG, const double* dlambda, double* dGamma, int64_t ldg, int64_t strideG) {
    if (!h) return -1;
    GN_TRY
    int rc = check_hessian_sums(h->err, {count, m, n, l, t_max, pair0, npairs, ldg, strideG}, t, active, slot, dx != nullptr,
                                dF != nullptr, drx != nullptr, dG != nullptr, dlambda != nullptr, dGamma != nullptr);
    if (rc) return rc;
    GN_HIP(hipSetDevice(h->device));
    HessianScratch D, H;
    if ((rc = place_records(h, D, H, 0, count, l))) return rc;
    for (int64_t k = 0; k < count; ++k) {      // slot[k] < 0: a count of 0, so that nothing of the problem is read
        const bool tk = !slot || slot[k] >= 0;
        H.meta[k] = tk ? HessMeta{(int)t[k], (int)(slot ? slot[k] : k)} : HessMeta{0, -1};
        if (active) pack_row(H.list, active, k, tk ? t[k] : 0, l);      // the active half of a working-set list
    }
    if (!active) std::fill(H.list, H.list + count * l, 0);             // no active array (every count is 0): zeros
    HessianSumsArgs a{};
    a.meta = D.meta; a.act = D.list;
    a.m = (int)m; a.n = (int)n; a.l = (int)l; a.t_max = (int)t_max; a.pair0 = pair0; a.npairs = npairs; a.eps1 = hess_eps1();
    a.x = dx; a.F = dF; a.rx = drx; a.G = dG; a.lambda = dlambda; a.Gamma = dGamma; a.ldg = ldg; a.strideG = strideG;
    const int64_t blocks = (npairs + HESS_PAIRS_PER_WG - 1) / HESS_PAIRS_PER_WG;
    return round_trip(h, D, H, [&](hipStream_t st) {      // nothing comes down
        hipLaunchKernelGGL(k_hessian_sums, dim3((unsigned)count, (unsigned)std::min<int64_t>(blocks, HESS_MAX_GRID_Y)), dim3(256), 0, st, a);
    });
    GN_CATCH(h)
}

}  // extern "C"
