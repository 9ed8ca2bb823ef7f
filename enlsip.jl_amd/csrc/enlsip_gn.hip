// libenlsip_gn.so — C ABI (include/enlsip_gn.h) over the gfx950 kernels.
// One handle = one stream + one lazily grown device workspace.  No exceptions cross the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <thread>

#include "gn_context.hpp"
#include "gn_kernels_caqr.hpp"
#include "gn_kernels_constraint.hpp"
#include "gn_kernels_geqp3_reg.hpp"
#include "gn_kernels_final.hpp"
#include "gn_kernels_q1.hpp"
#include "gn_kernels_q1_mfma.hpp"
#include "gn_kernels_q1_v2.hpp"
#include "gn_kernels_q1_rows.hpp"
#include "gn_kernels_final_small.hpp"
#include "gn_kernels_small_fused.hpp"
#include "gn_kernels_constraint_small.hpp"
#include "gn_kernels_constraint_dist.hpp"
#include "gn_kernels_update_v4.hpp"
#include "gn_kernels_misc.hpp"
#include "gn_kernels_lagrange.hpp"
#include "gn_kernels_lagrange_batched.hpp"
#include "gn_kernels_tsqr_products.hpp"
#include "gn_kernels_resolve_batched.hpp"
#include "gn_kernels_subspace_batched.hpp"
#include "gn_kernels_deletion_batched.hpp"
#include "gn_kernels_linesearch_batched.hpp"
#include "gn_kernels_penalty_batched.hpp"
#include "gn_kernels_linesearch_fit_batched.hpp"
#include "gn_kernels_addition_batched.hpp"
#include "gn_kernels_termination_batched.hpp"
#include "gn_kernels_direction_batched.hpp"
#include "gn_kernels_hessian_batched.hpp"
#include "gn_linesearch_fit.hpp"
#include "gn_kernels_newton.hpp"
#include "gn_kernels_newton_batched.hpp"
#include "gn_kernels_newton_wide.hpp"
#include "gn_kernels_qrcp_dist.hpp"
#include "gn_kernels_qrcp_block.hpp"
#include "gn_kernels_qrcp_block_reg.hpp"
#include "gn_rescale.hpp"

using namespace gn;

#define GN_HIP(call)                                                                   \
    do {                                                                               \
        hipError_t e__ = (call);                                                       \
        if (e__ != hipSuccess) {                                                       \
            char buf__[512];                                                           \
            snprintf(buf__, sizeof buf__, "%s:%d %s -> %s", __FILE__, __LINE__, #call, \
                     hipGetErrorString(e__));                                          \
            h->err = buf__;                                                            \
            return (int)e__ > 0 ? (int)e__ : 999;                                      \
        }                                                                              \
    } while (0)

// No exception crosses the ABI: entry points that allocate on the host (std::vector, std::string, std::thread) run inside
// GN_TRY ... GN_CATCH(h), which turns an exception into an error code and a message.
#define GN_TRY try {
#define GN_CATCH(h)                                                                    \
    }                                                                                  \
    catch (const std::bad_alloc&) {                                                    \
        try { (h)->err = "out of host memory"; } catch (...) {}                        \
        return 998;                                                                    \
    }                                                                                  \
    catch (const std::exception& e__) {                                                \
        try { (h)->err = std::string("host exception: ") + e__.what(); } catch (...) {}\
        return 997;                                                                    \
    }                                                                                  \
    catch (...) {                                                                      \
        return 997;                                                                    \
    }

#define GN_TRACE(h, ...)                                              \
    do {                                                              \
        if ((h)->trace) {                                             \
            (void)hipStreamSynchronize((h)->stream);                  \
            fprintf(stderr, "[enlsip_gn] " __VA_ARGS__);              \
            fputc('\n', stderr);                                      \
            fflush(stderr);                                           \
        }                                                             \
    } while (0)

static int grow(enlsip_gn_handle h, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes) return 0;
    if (b.p) GN_HIP(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    GN_HIP(hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return 0;
}

// The same for a call's pinned scratch: grown, never shrunk, the old block freed first.  A stream that was handed the old block
// must have been synchronised before this is called: every caller synchronises its streams before it returns, so growing at the
// start of a call is safe.
static int grow_pinned(enlsip_gn_handle h, PinnedBuf& b, size_t bytes) {
    if (b.cap >= bytes) return 0;
    if (b.p) (void)hipHostFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    GN_HIP(hipHostMalloc(&b.p, bytes, hipHostMallocDefault));
    b.cap = bytes;
    return 0;
}

// A layout (gn_layout.hpp, gn_plan.hpp) in a device buffer / in a call's pinned scratch: measure, grow, place.
template <class Layout, class... Shape>
static int place_dev(enlsip_gn_handle h, DevBuf& b, Layout& L, const Shape&... shape) {
    return place(L, [&](size_t bytes, void** base) { const int rc = grow(h, b, bytes); *base = b.p; return rc; }, shape...);
}
template <class Layout, class... Shape>
static int place_pinned(enlsip_gn_handle h, PinnedBuf& b, Layout& L, const Shape&... shape) {
    return place(L, [&](size_t bytes, void** base) { const int rc = grow_pinned(h, b, bytes); *base = b.p; return rc; }, shape...);
}
// The records of a call on the caller's buffers (gn_batch_records.hpp): the same layout in the handle's record scratch on the
// device and in pinned memory, there without the partial sums (`part` per problem), which stay on the device.
template <class Layout, class... Shape>
static int place_records(enlsip_gn_handle h, Layout& D, Layout& H, int64_t part, const Shape&... shape) {
    const int rc = place_dev(h, h->rec_scr, D, shape..., part);
    return rc ? rc : place_pinned(h, h->h_rec, H, shape..., (int64_t)0);
}
// The round trip of such a call on h->stream: the uploaded arrays (they start at `meta` on both sides) in one copy, the call's
// launches, `down_bytes` from `d_down` to `h_down` in one copy down (the same array of D and of H; none: nothing comes down), and
// the synchronisation that frees the record scratch for the next call.  Errors as GN_HIP reports them.
template <class Layout, class Launch>
static int round_trip(enlsip_gn_handle h, const Layout& D, const Layout& H, Launch&& launch, void* h_down = nullptr,
                      const void* d_down = nullptr, size_t down_bytes = 0) {
    hipStream_t st = h->stream;
    GN_HIP(hipMemcpyAsync(D.meta, H.meta, H.up_bytes, hipMemcpyHostToDevice, st));
    launch(st);
    GN_HIP(hipGetLastError());
    if (h_down) GN_HIP(hipMemcpyAsync(h_down, d_down, down_bytes, hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));
    return 0;
}
static_assert(PLAN_PB == PB && PLAN_KBLK == KBLK && PLAN_QD_CPW == QD_CPW && PLAN_QDCAND_BYTES == sizeof(QdCand) &&
              PLAN_SBINFO_BYTES == sizeof(SbInfo), "gn_plan.hpp sizes the workspaces with the kernels' constants");
// the pair rule lives in plan_geometry; the dispatch tests read its threshold from this file, so it is pinned here
static_assert(PLAN_PAIR_MIN_WGS == 8192, "panel pairs from far_wgs >= 8192 on (plan_geometry)");

// ---------------------------------------------------------------------------------------------
// plan: geometry (gn_plan.hpp) + placed workspace for (batch, m, n, t)
// ---------------------------------------------------------------------------------------------
static int make_plan(enlsip_gn_handle h, long long batch, long long m, long long n, long long t) {
    Plan& P = h->plan;
    if (h->have_plan && P.batch == batch && P.m == m && P.n == n && P.t == t) return 0;
    P = plan_geometry(batch, m, n, t, h->tile_rows, (h->flags & ENLSIP_GN_UPDATE_REFLECTORS) != 0, h->pair_enabled, h->pair_forced);
    int rc = place_dev(h, h->ws, static_cast<WsLayout&>(*h), P);
    if (rc) return rc;
    if (h->h_state_cap < (size_t)batch) {
        if (h->h_state) GN_HIP(hipHostFree(h->h_state));
        h->h_state = nullptr;
        GN_HIP(hipHostMalloc((void**)&h->h_state, (size_t)batch * sizeof(ProbState), hipHostMallocDefault));
        if (h->h_sbinfo) GN_HIP(hipHostFree(h->h_sbinfo));
        h->h_sbinfo = nullptr;
        GN_HIP(hipHostMalloc(&h->h_sbinfo, (size_t)batch * sizeof(SbInfo), hipHostMallocDefault));
        h->h_state_cap = (size_t)batch;
    }
    h->have_plan = true;
    h->factors_valid = false;
    h->tsqr_stage = 0;
    return 0;
}

// Problems per launch: the batch index is a grid y / z dimension (limit 65535).  Larger batches are cut into
// consecutive chunks by solve_chunked; the limit is kept a power of two so that C5's 65536 problems are two even chunks.
constexpr long long GN_MAX_LAUNCH_BATCH = 32768;

static int check_limits(enlsip_gn_handle h, long long batch, long long m, long long n, long long t) {
    if (batch < 1) { h->err = "batch must be >= 1"; return -2; }
    if (batch > (1LL << 31) - 1) { h->err = "batch must be < 2^31"; return -2; }
    if (m < 1 || m > (1LL << 27) - 4096) { h->err = "m out of range (1 .. 2^27 - 4096: 32-bit lane offsets in the update kernels)"; return -3; }
    if (n < 1 || n > 1024) { h->err = "n must be in 1..1024 in this build"; return -4; }
    if (t < 0 || t > 1024) { h->err = "t must be in 0..1024 in this build"; return -5; }
    return 0;
}

// kernels that declare more than 64 KB of dynamic LDS need the opt-in attribute
template <class KernelT>
static void big_lds(KernelT k, size_t bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
#define GN_LAUNCH_BIG(kern, grid, block, lds, stream, ...) \
    do {                                                     \
        big_lds(kern, lds);                                  \
        hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__); \
    } while (0)

// dispatch helpers over the rows-per-lane instantiations of the single-workgroup kernels
// Problems with at most 64 rows run with 256 or 512 threads and an LDS carve sized to the problem, so that batches of
// small problems (C3, C5) keep several workgroups resident per CU; larger ones use 1024 threads.
// tk: each problem's own t of a ragged batch (device), NULL for a uniform batch
static void launch_constraint(int rows, int batch, hipStream_t s, ConstraintArgs a, const int* tk = nullptr) {
    if (launch_constraint_small(batch, s, a, tk)) return;
    constraint_carve(a.n, a.t, a.fa_done, a.nv, a.blkd, a.gld, a.matd, a.need_T, a.fl_done);
    const size_t lds = constraint_lds_bytes(a.nv, a.blkd, a.gld, a.matd);
    if (!a.fa_done && (size_t)a.n * a.t > (size_t)CMAT_DOUBLES) GN_ROUTE(ENLSIP_GN_ROUTE_CONSTRAINT_GLOBAL);
    GN_ROUTE(rows <= 32 ? ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R1_256 : rows <= 64 ? ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R1_512 :
             rows <= 128 ? ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R2 : rows <= 256 ? ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R4 :
             rows <= 512 ? ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R8 : ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R16);
    if (tk) {       // ragged batch: the same instantiations reading each problem's own t (gn_kernels_constraint.hpp)
        auto launch_ragged = [&](void (*k)(ConstraintArgs, const int*), int nth) {
            big_lds(k, lds);
            hipLaunchKernelGGL(k, dim3(batch), dim3(nth), lds, s, a, tk);
        };
        if (rows <= 32) launch_ragged(k_constraint_ragged<1, 8, 256>, 256);
        else if (rows <= 64) launch_ragged(k_constraint_ragged<1, 8, 512>, 512);
        else if (rows <= 128) launch_ragged(k_constraint_ragged<2, 8, 1024>, 1024);
        else if (rows <= 256) launch_ragged(k_constraint_ragged<4, 8, 1024>, 1024);
        else if (rows <= 512) launch_ragged(k_constraint_ragged<8, 4, 1024>, 1024);
        else launch_ragged(k_constraint_ragged<16, 2, 1024>, 1024);
        return;
    }
    if (rows <= 32) GN_LAUNCH_BIG((k_constraint<1, 8, 256>), dim3(batch), dim3(256), lds, s, a);
    else if (rows <= 64) GN_LAUNCH_BIG((k_constraint<1, 8, 512>), dim3(batch), dim3(512), lds, s, a);
    else if (rows <= 128) GN_LAUNCH_BIG((k_constraint<2, 8, 1024>), dim3(batch), dim3(1024), lds, s, a);
    else if (rows <= 256) GN_LAUNCH_BIG((k_constraint<4, 8, 1024>), dim3(batch), dim3(1024), lds, s, a);
    else if (rows <= 512) GN_LAUNCH_BIG((k_constraint<8, 4, 1024>), dim3(batch), dim3(1024), lds, s, a);
    else GN_LAUNCH_BIG((k_constraint<16, 2, 1024>), dim3(batch), dim3(1024), lds, s, a);
}
static void launch_pivot(int rows, int batch, hipStream_t s, FinalArgs a) {
    final_carve(a.m, a.n, a.t, a.nv, a.matd);
    const size_t lds = final_lds_bytes(a.nv, a.matd);
    GN_ROUTE(rows <= 32 ? ENLSIP_GN_ROUTE_PIVOT_LDS_R1_256 : rows <= 64 ? ENLSIP_GN_ROUTE_PIVOT_LDS_R1_512 :
             rows <= 128 ? ENLSIP_GN_ROUTE_PIVOT_LDS_R2 : rows <= 256 ? ENLSIP_GN_ROUTE_PIVOT_LDS_R4 :
             rows <= 512 ? ENLSIP_GN_ROUTE_PIVOT_LDS_R8 : ENLSIP_GN_ROUTE_PIVOT_LDS_R16);
    if (rows <= 32) GN_LAUNCH_BIG((k_pivot_solve<1, 8, 256>), dim3(batch), dim3(256), lds, s, a);
    else if (rows <= 64) GN_LAUNCH_BIG((k_pivot_solve<1, 8, 512>), dim3(batch), dim3(512), lds, s, a);
    else if (rows <= 128) GN_LAUNCH_BIG((k_pivot_solve<2, 8, 1024>), dim3(batch), dim3(1024), lds, s, a);
    else if (rows <= 256) GN_LAUNCH_BIG((k_pivot_solve<4, 8, 1024>), dim3(batch), dim3(1024), lds, s, a);
    else if (rows <= 512) GN_LAUNCH_BIG((k_pivot_solve<8, 4, 1024>), dim3(batch), dim3(1024), lds, s, a);
    else GN_LAUNCH_BIG((k_pivot_solve<16, 2, 1024>), dim3(batch), dim3(1024), lds, s, a);
}

// J*Q1 of a solve: JQ1 = J Q1 into the working matrix W (and d_temp from rx), for the problems of the resident plan
static JQ1Args jq1_args(enlsip_gn_handle h, const double* J, long long ldj, long long strideJ, const double* rx) {
    const Plan& P = h->plan;
    JQ1Args qa{};
    qa.m = (int)P.m; qa.n = (int)P.n; qa.kA = P.kA; qa.ldw = P.ldw;
    qa.J = J; qa.ldj = ldj; qa.strideJ = strideJ; qa.rx = rx; qa.stride_rx = P.m;
    qa.FA = h->FA; qa.sFA = P.sFA; qa.TA = h->TA; qa.sTA = P.sTA; qa.p1 = h->p1; qa.sP1 = P.sP1;
    qa.W = h->W; qa.sW = P.sW; qa.state = h->state;
    qa.prob0 = 0; qa.plist = h->run_plist;
    // V T' of the fast path lives in the (still unused) working matrix of the pivoted QR
    qa.VT = (P.sM >= P.n * KBLK) ? h->qdM : nullptr; qa.sVT = P.sM;
    return qa;
}
static void launch_jq1_any(enlsip_gn_handle h, const JQ1Args& qa, int batch, hipStream_t s) {
    if (h->flags & ENLSIP_GN_UPDATE_REFLECTORS) launch_jq1(qa, batch, s);   // plain-FMA A/B partner
    else if (launch_jq1_rows(qa, batch, s)) {}                              // small n, few reflectors
    else if (!launch_jq1_v2(qa, batch, s)) launch_jq1_mfma(qa, batch, s);   // regular shapes / general shapes
}

// Problems the Jacobian-side launches of the running solve_dev cover: the whole part, or the listed problems of a changed-problems
// solve.  Only the GRIDS are sized by it: every kernel-form predicate keeps reading the part's whole problem count (plan.batch), so
// that a listed problem runs through the kernels a solve of the whole part would give it.
static long long launch_count(enlsip_gn_handle h) { return h->run_plist ? h->run_nlist : h->plan.batch; }

static CaqrArgs caqr_args(enlsip_gn_handle h, int k, const LevelPlan& L) {
    const Plan& P = h->plan;
    CaqrArgs a{};
    a.m = (int)P.m; a.n = (int)P.n; a.ldw = P.ldw;
    a.panel = k; a.level = L.level; a.F = P.F; a.nblocks = L.nblocks; a.S = L.S; a.tOff = L.tOff;
    a.W = h->W; a.sW = P.sW; a.Tbuf = h->Tbuf; a.sT = P.sT; a.state = h->state;
    a.ext_cols = 0; a.C = nullptr; a.sC = 0; a.reverse = 0;
    a.mode = L.mode; a.base = L.base; a.skip = L.skip; a.win = 0; a.pair = 0; a.tOff2 = 0;
    a.plist = h->run_plist;
    return a;
}

// the final kernel (pivoted QR of R0 in its LDS forms, the solves, the outputs of v) at launch width n2_launch
static FinalArgs final_args(enlsip_gn_handle h, const BatchOperands& v, double eps_rank, long long dimJ2_ov, int abs_shift, int n2_launch) {
    const Plan& P = h->plan;
    FinalArgs fa{};
    fa.m = (int)P.m; fa.n = (int)P.n; fa.t = (int)P.t; fa.kA = P.kA; fa.ldw = P.ldw; fa.ldr = P.ldr;
    fa.eps_rank = eps_rank; fa.abs_shift = abs_shift; fa.dimJ2_override = (int)dimJ2_ov; fa.refactor = 1;
    fa.W = h->W; fa.sW = P.sW; fa.Rt = h->Rt; fa.sRt = P.sRt; fa.tauJ = h->tauJ; fa.sTauJ = P.sTauJ;
    fa.jpvtJ = h->jpvtJ; fa.sJJ = P.sJJ; fa.FA = h->FA; fa.sFA = P.sFA; fa.tauA = h->tauA; fa.sTauA = P.sTauA;
    fa.p1 = h->p1; fa.sP1 = P.sP1; fa.bvec = h->bvec; fa.sB = P.sB; fa.zsave = h->zsave; fa.sZ = P.sZ;
    fa.p_out = v.p; fa.sPo = P.n; fa.b_out = v.b; fa.sBo = P.t; fa.d_out = v.d; fa.sDo = P.m;
    fa.jA_out = v.jpvtA; fa.sJAo = P.t; fa.jpvtA = h->jpvtA; fa.sJA = P.sJA;
    fa.jL_out = v.jpvtL; fa.sJLo = P.kA; fa.jpvtL = h->jpvtL; fa.sJL = P.sJL;
    fa.jJ_out = v.jpvtJ2; fa.sJJo = P.n;
    fa.state = h->state; fa.plist = h->run_plist;
    fa.n2cap = n2_launch;
    return fa;
}

static void launch_factor(enlsip_gn_handle h, const CaqrArgs& a, int groups, hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    dim3 grid(groups, (unsigned)launch_count(h));
    // one-tile problems of at most 256 rows: 4 waves x 8 columns issue ~20 % fewer instructions per step than 8 x 4
    // (measured on C5: panel stage 0.63 -> 0.57 ms); everywhere else the 8-wave form wins (a 16-wave form: 8.1 -> 11.2 ms)
    if (h->plan.m > 256) {
        // a tree level with ONE node of few blocks (the top of a tree; C2's first-panel trees: 8 blocks) needs only
        // ceil(blocks / 2) registers per lane and column: the smaller forms issue fewer multiply-adds per step on rows that hold
        // nothing (the geometry of a node is the same in every form: slot ln + 64 i = block (ln >> 5) + 2 i)
        int rpl = h->plan.RPL;
        if (a.level > 0 && groups == 1) {
            const int need = (a.nblocks + 1) / 2;
            const int fit = need <= 1 ? 1 : (need <= 2 ? 2 : (need <= 4 ? 4 : 8));
            if (fit < rpl) rpl = fit;
        }
        if (rpl == 8) hipLaunchKernelGGL((k_caqr_factor<8, 8>), grid, dim3(512), 0, st, a);
        else if (rpl == 4) hipLaunchKernelGGL((k_caqr_factor<4, 8>), grid, dim3(512), 0, st, a);
        else if (rpl == 2) hipLaunchKernelGGL((k_caqr_factor<2, 8>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((k_caqr_factor<1, 8>), grid, dim3(512), 0, st, a);
    } else {
        if (h->plan.RPL == 8) hipLaunchKernelGGL((k_caqr_factor<8, 4>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_caqr_factor<4, 4>), grid, dim3(256), 0, st, a);
    }
}
// nprob: the batch (the sweep), or 1 for one problem addressed through a.prob0 (caqr_apply_ext)
static void launch_update_refl(enlsip_gn_handle h, const CaqrArgs& a, int groups, int ncols, int nprob) {
    dim3 grid(groups, (ncols + 31) / 32, (unsigned)nprob);
    if (h->plan.RPL == 8) hipLaunchKernelGGL(k_caqr_update_refl<8>, grid, dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(k_caqr_update_refl<4>, grid, dim3(256), 0, h->stream, a);
}

// Apply Q0' (reverse = 0) or Q0 (reverse = 1) of the resident CAQR factors of problem `prob` to the external
// vector C (ldw doubles): every (panel, level) in forward or reverse order.
static void caqr_apply_ext(enlsip_gn_handle h, double* C, int prob, int npan, bool reverse) {
    const Plan& P = h->plan;
    for (int kk = 0; kk < npan; ++kk) {
        const int k = reverse ? npan - 1 - kk : kk;
        const auto& lv = P.panels[k].levels;
        for (size_t li = 0; li < lv.size(); ++li) {
            const LevelPlan& L = reverse ? lv[lv.size() - 1 - li] : lv[li];
            CaqrArgs a = caqr_args(h, k, L);
            a.ext_cols = 1; a.C = C; a.sC = 0; a.reverse = reverse ? 1 : 0; a.prob0 = prob;
            launch_update_refl(h, a, L.groups, 1, 1);
        }
    }
}

// the next event of a pool that grows on demand
static int next_event(enlsip_gn_handle h, std::vector<hipEvent_t>& pool, size_t& used, unsigned flags, hipEvent_t& e) {
    if (used >= pool.size()) {
        hipEvent_t ne;
        GN_HIP(hipEventCreateWithFlags(&ne, flags));
        pool.push_back(ne);
    }
    e = pool[used++];
    return 0;
}

// the CAQR sweep over [J2 | d]
// A step is a panel pair (k, k + 1) or one panel k.  Its CHAIN (the factorisations and, for a pair, the first panel's reflectors on
// the second panel's 32 columns) touches only the step's own columns; its WINDOW UPDATE is everything it applies to the trailing
// columns, one function of a column sub-window (sub0, subn) and a stream.  The one-stream schedule calls that function once for the
// whole window; the look-ahead schedule (two_streams) calls it for the near part on the main stream and for the rest on the second.
static int run_caqr(enlsip_gn_handle h, int n2_launch) {
    const Plan& P = h->plan;
    const int kp_launch = (int)std::min<long long>(P.m, n2_launch);
    const int npan = (kp_launch + PB - 1) / PB;
    const int nprob = (int)launch_count(h);       // grids only; P.batch below decides the forms
    const bool use_mfma = !(h->flags & ENLSIP_GN_UPDATE_REFLECTORS);
    GN_ROUTE(P.RPL == 8 ? ENLSIP_GN_ROUTE_SWEEP_TILE512 : ENLSIP_GN_ROUTE_SWEEP_TILE256);
    if (!use_mfma) GN_ROUTE(ENLSIP_GN_ROUTE_SWEEP_REFLECTORS);
    const double mpad = (double)rup(std::max<long long>(P.m, 1), 32);
    // the launch shape is the widest J2 of the batch; narrower ones exist only when some constraint matrix was rank deficient
    // (second attempt of solve_dev) or when the caller's problems differ
    const bool mixed = n2_launch != (int)(P.n - P.kA);
    // HIP events around a launch when `on`
    auto between_events = [&](bool on, std::vector<hipEvent_t>& pool, size_t& used, hipStream_t st, auto&& launch) -> int {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (on) {
            if (int rc = next_event(h, pool, used, hipEventDefault, e0)) return rc;
            if (int rc = next_event(h, pool, used, hipEventDefault, e1)) return rc;
            GN_HIP(hipEventRecord(e0, st));
        }
        launch();
        if (on) GN_HIP(hipEventRecord(e1, st));
        return 0;
    };
    // the level-0 far updates (the dominant kernel) are timed when profiling is on; `bytes` = SURVEY 8d's
    // B_trail = 8 (2 m_k n_k + m_k b + b^2) of every panel the launch applies, on the columns it applies them to
    auto timed = [&](double bytes, hipStream_t st, auto&& launch) -> int {
        if (int rc = between_events(h->profiling, h->upd_ev, h->upd_used, st, launch)) return rc;
        if (h->profiling) {
            h->upd_bytes += (double)P.batch * bytes;
            h->upd_launch_bytes.push_back((double)P.batch * bytes);
        }
        return 0;
    };
    // every other trailing-update launch (tree levels, the second panel's own columns): timed too, booked under
    // ENLSIP_GN_STAGE_UPDATE and reported by enlsip_gn_get_update_totals
    auto other = [&](hipStream_t st, auto&& launch) -> int {
        return between_events(h->profiling && h->profile_all_updates, h->oth_ev, h->oth_used, st, launch);
    };
    auto btrail = [&](int k, double ncols) { const double mk = mpad - (double)k * PB; return 8.0 * (2.0 * mk * ncols + mk * PB + PB * PB); };
    // a sub-window [sub0, sub0 + subn) of a trailing window of ntot columns (subn = 0: to its end); the carried right-hand side is
    // the window's last column, so a sub-window that ends before it has J2 columns only
    struct Window { int sub0, subn, ncols; bool has_rhs; };
    auto window = [](int ntot, int sub0, int subn) {
        const int ncols = subn > 0 ? std::min(subn, ntot - sub0) : ntot - sub0;
        return Window{sub0, subn, ncols, sub0 + ncols == ntot};
    };
    // The level-0 MFMA update of a window, on a grid over ngrid columns.  With the J2 columns filling whole 32-column blocks the
    // carried right-hand side (the 32 j + 1-th column: every panel of C2) would take a block of its own: it gets its own routine as
    // the last block index instead.  With a partial last block (C3: 24 columns) it simply rides in that block.
    auto update_l0 = [&](CaqrArgs a, const LevelPlan& L, const Window& w, int ngrid, hipStream_t st) {
        a.sub0 = w.sub0; a.subn = w.subn;
        if (w.has_rhs && (w.ncols - 1) % 32 == 0) {
            a.skip_rhs = 1;
            --ngrid;
        }
        launch_update_v4(P.RPL, a, L.groups, ngrid, nprob, st);
    };
    // every other update of a window (tree levels, the second panel's own columns): not the dominant kernel, booked as "other"
    auto update_other = [&](CaqrArgs a, const LevelPlan& L, const Window& w, int ngrid, hipStream_t st) -> int {
        a.sub0 = w.sub0; a.subn = w.subn;
        return other(st, [&] { launch_update_v4(P.RPL, a, L.groups, ngrid, nprob, st); });
    };
    // few problems with many tiles each: the far update of a pair reads its grid XCD-locally, so that a tile's V stays in one L2
    // between the tile's column blocks (k_caqr_update_v4_pair); batches keep the native order (a problem's tiles are neighbours)
    auto xmap_tiles = [&](int groups) -> int { return (P.batch <= 8 && groups >= 16 && !mixed) ? groups : 0; };
    // Look-ahead (chain-bound sweeps: one or a few problems with many tiles — C4): a pair's far update is split into the NEXT
    // pair's 64 columns (this stream) and the rest (second stream), so that the next pair's chain of small dependent launches
    // (two level-0 factorisations, their trees, the second panel's own columns) runs beside the bulk of the previous far update
    // instead of behind it.  Order: chain(K) -> E1 ; [wait E2(K-1)] near(K) ; second stream: wait E1, rest(K) -> E2.
    const long long far_wgs0 = P.batch * (((long long)mpad + 64 * P.RPL - 1) / (64 * P.RPL)) * ((n2_launch + 31) / 32);
    const bool la = P.pair && use_mfma && h->lookahead && !mixed &&
                    ((P.batch <= 8 && far_wgs0 >= 8192) || h->lookahead_forced);
    // The same idea for the PLAIN sweep of a chain-bound problem (a single C2 problem; a 32768-row shard of C4 where pairs do
    // not pay): the factorisations of a panel (tile level and tree levels: they only read the panel's own columns) run first,
    // its trailing updates are split into the next panel's 32 columns (this stream) and the rest (second stream), and the next
    // panel's factorisations run beside that rest.  Order per panel k: F(k) -> E1 ; [wait E2(k-1)] near(k) ; second stream:
    // wait E1, rest(k) -> E2.
    // Measured (MI355X, round 4): it does NOT pay at the sizes it was meant for — a single C2 problem 4.18 -> 4.38 ms, four of them
    // 4.59 -> 4.80 ms, a 32768 x 1024 shard 15.66 -> 15.63 ms: two event hand-overs per panel cost what the overlap of a ~25 us
    // update with a ~75 us factor chain brings.  Kept behind ENLSIP_GN_LOOKAHEAD=1 (parity-tested in both sweeps), off by default.
    const bool lap = !P.pair && use_mfma && h->lookahead && !mixed && npan >= 3 && h->lookahead_forced;
    const hipStream_t sA = h->stream;
    hipStream_t sB = nullptr;
    if (la || lap) {
        if (!h->stream2) {
            // lowest priority: the chain's small kernels on the main stream must not queue behind the thousands of workgroups
            // of the bulk update for a free CU slot
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            GN_HIP(hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, least));
        }
        sB = h->stream2;
        GN_ROUTE(ENLSIP_GN_ROUTE_SWEEP_LOOKAHEAD);
    }
    size_t la_used = 0;
    hipEvent_t la_prev = nullptr;                 // E2 of the previous step's rest (second stream), not yet waited for
    auto la_join = [&]() -> int {                 // this stream goes on only after the second stream's last window update
        if (la_prev) {
            GN_HIP(hipStreamWaitEvent(sA, la_prev, 0));
            la_prev = nullptr;
        }
        return 0;
    };
    // the window update of a step whose chain has just been issued on this stream, in two parts: columns [0, near) (the next
    // step's own) on this stream, the rest on the second
    auto two_streams = [&](int ncols, int near, auto&& update) -> int {
        if (ncols <= near) {                                    // nothing beyond the next step's columns: one part, this stream
            if (int rc = la_join()) return rc;
            return update(0, 0, sA);
        }
        hipEvent_t e1, e2;
        if (int rc = next_event(h, h->la_events, la_used, hipEventDisableTiming, e1)) return rc;
        if (int rc = next_event(h, h->la_events, la_used, hipEventDisableTiming, e2)) return rc;
        GN_HIP(hipEventRecord(e1, sA));                         // the step's reflectors and T factors are complete
        if (int rc = la_join()) return rc;                      // the previous step's rest covers the columns `near` touches
        if (int rc = update(0, near, sA)) return rc;
        GN_HIP(hipStreamWaitEvent(sB, e1, 0));
        if (int rc = update(near, 0, sB)) return rc;
        GN_HIP(hipEventRecord(e2, sB));
        la_prev = e2;
        return 0;
    };
    for (int k = 0; k < npan;) {
        const int bwk = std::min(PB, kp_launch - k * PB);
        const int ntrail = n2_launch + 1 - (k * PB + bwk);  // trailing columns incl. the augmented one
        if (h->profiling && ntrail > 0) h->upd_all_bytes += (double)P.batch * btrail(k, ntrail);   // every column right of the panel
        const auto& LA = P.panels[k].levels;
        if (P.pair && use_mfma && !(k & 1) && k + 1 < npan) {
            // ---- panel pair (k, k + 1): tiles shared, ONE pass over the far trailing columns for both (gn_kernels_caqr.hpp) ----
            GN_ROUTE(ENLSIP_GN_ROUTE_SWEEP_PAIRS);
            if (LA.size() > 1) GN_ROUTE(ENLSIP_GN_ROUTE_SWEEP_TREE);
            const int kb = k + 1;
            const auto& LB = P.panels[kb].levels;
            const int bwb = std::min(PB, kp_launch - kb * PB);
            const int nfar = ntrail - bwb;                   // columns beyond the pair, incl. the augmented one (>= 1)
            if (h->profiling && nfar > 0) h->upd_all_bytes += (double)P.batch * btrail(kb, nfar);
            // chain.  The first panel's level 0, applied to the second panel's columns only (win = 1); level 0 of the second panel:
            // the same tiles without their first 32 rows; the first panel's tree, applied likewise; the second panel's tree
            const Window own = window(bwb, 0, 0);
            auto first_panel_level = [&](const LevelPlan& L) -> int {
                CaqrArgs a = caqr_args(h, k, L);
                launch_factor(h, a, L.groups);
                a.win = 1;
                return update_other(a, L, own, bwb, sA);
            };
            if (int rc = first_panel_level(LA[0])) return rc;
            launch_factor(h, caqr_args(h, kb, LB[0]), LB[0].groups);
            for (size_t li = 1; li < LA.size(); ++li)
                if (int rc = first_panel_level(LA[li])) return rc;
            for (size_t li = 1; li < LB.size(); ++li) launch_factor(h, caqr_args(h, kb, LB[li]), LB[li].groups);
            // window update (win = 2): both level-0 reflectors in one pass, then the first panel's tree levels, then the second's.
            // Grid of the first panel's launches.  A problem whose J2 ends inside the pair has bwb fewer pair
            // columns and as many more far columns than the launch shape says, so with mixed widths the grid spans ntrail and the
            // column block past a problem's last column exits at once.  In a uniform batch that block is ALWAYS empty — and not
            // free: with 8 tiles in x (= the 8 XCDs) a grid whose y extent is a multiple of 4 hands the empty and the light
            // (right-hand side) block of every problem to the same two of an XCD's four dispatch queues, measured 5-20 % on the
            // far launches of pairs 1, 3, 5 of a C2 step (profiles/r4_notes.md).  The exact grid has an odd y extent.
            // (Mixed widths never meet a sub-window: both look-ahead forms need a uniform batch.)
            auto far_update = [&](int sub0, int subn, hipStream_t st) -> int {
                const Window w = window(nfar, sub0, subn);
                const int far_grid = mixed ? ntrail : w.ncols;
                CaqrArgs a = caqr_args(h, k, LA[0]);
                a.win = 2;
                a.pair = 1; a.tOff2 = LB[0].tOff;
                a.xmap = xmap_tiles(LA[0].groups);
                if (a.xmap) GN_ROUTE(ENLSIP_GN_ROUTE_SWEEP_XMAP);
                if (int rc = timed(btrail(k, w.ncols) + btrail(kb, w.ncols), st, [&] { update_l0(a, LA[0], w, far_grid, st); })) return rc;
                if (mixed) {        // problems whose J2 ends before the second panel: the first panel alone, every trailing column
                    a.pair = 2;
                    update_l0(a, LA[0], w, ntrail, st);
                }
                for (size_t li = 1; li < LA.size(); ++li) {
                    CaqrArgs t = caqr_args(h, k, LA[li]);
                    t.win = 2;
                    if (int rc = update_other(t, LA[li], w, far_grid, st)) return rc;
                }
                for (size_t li = 1; li < LB.size(); ++li)
                    if (int rc = update_other(caqr_args(h, kb, LB[li]), LB[li], w, w.ncols, st)) return rc;
                return 0;
            };
            if (int rc = la ? two_streams(nfar, 2 * PB, far_update) : far_update(0, 0, sA)) return rc;
            k += 2;
            continue;
        }
        // ---- one panel ----
        // last panel narrower than 32 with d as the only trailing column: d rides through the factor kernels (no update launch)
        const bool passenger = (ntrail == 1 && bwk < PB && kp_launch == n2_launch);
        GN_ROUTE(passenger ? ENLSIP_GN_ROUTE_SWEEP_PASSENGER : ENLSIP_GN_ROUTE_SWEEP_PLAIN);
        if (LA.size() > 1) GN_ROUTE(ENLSIP_GN_ROUTE_SWEEP_TREE);
        const bool updates = ntrail > 0 && !passenger;
        // window update of one level
        auto level_update = [&](const LevelPlan& L, int sub0, int subn, hipStream_t st) -> int {
            const Window w = window(ntrail, sub0, subn);
            const CaqrArgs a = caqr_args(h, k, L);
            if (L.level > 0) return update_other(a, L, w, w.ncols, st);
            return timed(btrail(k, w.ncols), st, [&] { update_l0(a, L, w, w.ncols, st); });
        };
        if (lap && updates) {       // every factorisation of the panel first, then the updates of the levels, in order
            for (const LevelPlan& L : LA) launch_factor(h, caqr_args(h, k, L), L.groups);
            int rc = two_streams(ntrail, PB, [&](int sub0, int subn, hipStream_t st) -> int {
                for (const LevelPlan& L : LA)
                    if (int rcl = level_update(L, sub0, subn, st)) return rcl;
                return 0;
            });
            if (rc) return rc;
            ++k;
            continue;
        }
        if (int rc = la_join()) return rc;
        for (const LevelPlan& L : LA) {     // one stream: factor and update level by level (F0 U0 F1 U1 ...)
            CaqrArgs a = caqr_args(h, k, L);
            a.npass = passenger ? 1 : 0;
            launch_factor(h, a, L.groups);
            if (!updates) continue;
            if (!use_mfma) launch_update_refl(h, a, L.groups, ntrail, nprob);      // reflector by reflector (A/B path)
            else if (int rc = level_update(L, 0, 0, sA)) return rc;
        }
        ++k;
    }
    if (int rc = la_join()) return rc;
    GN_HIP(hipGetLastError());
    return 0;
}

// the launch-per-step pivoted QR (gn_kernels_qrcp_dist.hpp): arguments of the stage on R0 out of the CAQR storage
static QdArgs qd_args_r0(enlsip_gn_handle h, int n2_launch) {
    const Plan& P = h->plan;
    QdArgs a{};
    a.n = (int)P.n; a.ldw = P.ldw; a.ldr = P.ldr; a.step = 0; a.prob0 = 0; a.plist = h->run_plist;
    a.W = h->W; a.sW = P.sW; a.M = h->qdM; a.sM = P.sM; a.Vb = h->qdVb; a.sVb = P.sVb; a.Rt = h->Rt; a.sRt = P.sRt;
    a.tau = h->tauJ; a.sTau = P.sTauJ; a.diag = h->qdDiag; a.sDiag = P.sDiag;
    a.vn1 = h->qdVn1; a.vn2 = h->qdVn2; a.sVn = P.sVn;
    a.chosen = h->qdChosen; a.pos = h->qdPos; a.colat = h->qdColat; a.sI = P.sQI;
    a.cand = (QdCand*)h->qdCand; a.sCand = P.sCand; a.Gmax = P.qdGmax;
    a.jpvt = h->jpvtJ; a.sJ = P.sJJ; a.state = h->state;
    a.n2cap = n2_launch;
    return a;
}
static dim3 qd_grid(int cols, long long batch) { return dim3((cols + 1 + QD_CPW - 1) / QD_CPW, (unsigned)batch); }
// k_qd_init (with the caller's a.step) and the pivot steps [0, nsteps), in the 16 (big: more than 512 rows) or 8 rows-per-lane
// form; a.step is left at the last step issued.  k_qd_assemble reads the sign of a.step (negative: the blocked form's single
// map), so it stays with the callers.
static void launch_qd_steps(dim3 grid, bool big, hipStream_t s, QdArgs& a, int nsteps) {
    if (big) hipLaunchKernelGGL(k_qd_init<16>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_qd_init<8>, grid, dim3(256), 0, s, a);
    for (int j = 0; j < nsteps; ++j) {
        a.step = j;
        if (big) hipLaunchKernelGGL(k_qd_step<16>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_qd_step<8>, grid, dim3(256), 0, s, a);
    }
}

// distributed column-pivoted QR of R0 (one launch per pivot step over all problems)
static int run_qrcp_dist(enlsip_gn_handle h, int n2_launch) {
    const Plan& P = h->plan;
    const int kp_launch = (int)std::min<long long>(P.m, n2_launch);
    QdArgs a = qd_args_r0(h, n2_launch);
    GN_ROUTE(ENLSIP_GN_ROUTE_PIVOT_STEPS);
    const dim3 grid = qd_grid(n2_launch, launch_count(h));
    launch_qd_steps(grid, kp_launch > 512, h->stream, a, kp_launch);
    hipLaunchKernelGGL(k_qd_assemble, grid, dim3(256), 0, h->stream, a);
    GN_HIP(hipGetLastError());
    return 0;
}

// blocked pivoted QR of R0 with verified pivots (gn_kernels_qrcp_block.hpp)
// More than 512 rows do not fit the register forms: the stage then opens with a launch-per-step HEAD (k_qd_step, 8.4 us per step)
// until 512 rows are left and hands the rest to the blocks (~3 us per step + ~50 us per block).  The two forms share their state
// (M, norms, maps, reflectors by position); the head ends on an even step so that the maps sit in parity 0, where the blocks keep
// them.  C4's 1024 x 1024 combine: 1024 head steps = 8.6 ms -> 512 head steps + 16 blocks.
static int run_qrcp_block(enlsip_gn_handle h, int n2_launch) {
    const Plan& P = h->plan;
    const int kp_launch = (int)std::min<long long>(P.m, n2_launch);
    int jhead = kp_launch > 512 ? kp_launch - 512 : 0;
    jhead += jhead & 1;
    GN_ROUTE(jhead > 0 ? ENLSIP_GN_ROUTE_PIVOT_HYBRID : ENLSIP_GN_ROUTE_PIVOT_BLOCKS);
    SbArgs a{};
    QdArgs& q = a.q;
    q = qd_args_r0(h, n2_launch);
    q.step = -1;
    a.info = (SbInfo*)h->sbInfo; a.inblk = h->sbInblk; a.sIn = P.sQI; a.blkid = 0;
    a.Tsb = h->sbT; a.sTsb = PB * PB; a.act = h->sbAct; a.sAct = P.sAct;
    a.dbg = nullptr;
    // a changed-problems solve: grids over the listed problems, the end-of-stage check over them too (the block records of the
    // others are whatever their own solve left); it neither uses nor renews the form hints, which belong to whole-part stages
    const bool listed = h->run_plist != nullptr;
    const long long nl = launch_count(h);
    auto prob_at = [&](long long i) -> long long { return listed ? h->refit[(size_t)i] : i; };
    const dim3 grid = qd_grid(n2_launch, nl);
    hipStream_t s = h->stream;
    // Row-count statistics per block id (see SbArgs::rows_stat).  Every block is launched in up to three forms of the select /
    // factor kernel and a problem runs in the one that fits its current row count; in a batch of similar problems two of the
    // three launches of every block id find nothing to do — 24-40 us each at batch 384 (a launch of 384 x 512 threads that only
    // reads its state), 1.3 ms of a C2 step.  The previous solve of the same shape on this handle tells which forms a block id
    // needs; a problem that a skipped form would have served simply makes no step in that block id, the end-of-stage check
    // sees it and the stage goes on WITHOUT hints, so the result never depends on them.
    {
        int rc = grow(h, h->sb_stat, 2 * SB_STAT_BLKS * sizeof(int));
        if (rc) return rc;
        if (!h->h_sb_stat) GN_HIP(hipHostMalloc((void**)&h->h_sb_stat, 2 * SB_STAT_BLKS * sizeof(int), hipHostMallocDefault));
        GN_HIP(hipMemsetAsync(h->sb_stat.p, 0, 2 * SB_STAT_BLKS * sizeof(int), s));
        a.rows_stat = (int*)h->sb_stat.p;
    }
    bool hints = !listed && h->sb_form_hints && h->sb_rows_kp == kp_launch && h->sb_rows_batch == P.batch && !h->sb_rows_max.empty();
    const bool hinted = hints;
    bool fell_back = false;
    launch_qd_steps(grid, jhead > 0, s, q, jhead);     // the head, if any: more than 512 rows
    q.step = -1;
    q.hyb = jhead;
    hipLaunchKernelGGL(k_sb_reset, dim3(((unsigned)P.n + 255) / 256, (unsigned)nl), dim3(256), 0, s, a, (int)P.n, jhead);
    const int kp_blk = kp_launch - jhead;           // steps (= rows) left to the blocks
    dim3 ugrid((n2_launch + 1 + SB_UCW - 1) / SB_UCW, (unsigned)nl);
    int it = 0;
    // blocks of <= 32 steps; the first chunk is sized from the previous solve on this handle (one host check per
    // solve in steady state), later chunks are small
    int chunk = std::min(kp_blk, (h->sb_hint > 0 && !listed) ? h->sb_hint : kp_blk / 16 + 4);
    SbInfo* hinfo = (SbInfo*)h->h_sbinfo;
    // the state records read back at the end of a chunk: into the handle's mirror, but for a changed-problems solve, whose mirror
    // keeps the records of the problems it leaves alone (a rescued one's is its rescue handle's, not the device's)
    std::vector<ProbState> own_states;
    if (listed) own_states.resize((size_t)P.batch);
    ProbState* hstate = listed ? own_states.data() : h->h_state;
    // rows_bound: an upper bound of kp - j0 over the problems.  A block in which EVERY form the bound asks for was launched
    // serves every unfinished problem, and a served problem makes at least one step: the bound then falls by one.  A block
    // in which the hints suppressed one of those forms may have left a problem unserved: the bound stays, and the read-back
    // at the end of the chunk replaces it by the exact maximum.  (Until round 5 the forms were gated on kp_blk - it, which
    // assumes a step per block for everybody: a problem that a hinted chunk had left behind above 256 rows was never served
    // once kp_blk - it had fallen to 256, and the loop ran out with wrong factors.)
    int rows_bound = kp_blk;
    const int max_blocks = 2 * kp_blk + 64;         // without hints kp_blk blocks always suffice; hinted chunks may idle
    bool done = kp_blk <= 0;
    while (!done) {
        for (int i = 0; i < chunk && rows_bound > 0; ++i, ++it) {
            a.blkid = it;
            GN_TRACE(h, "  qrcp block %d", it);
            // candidates in the registers of one workgroup (kp <= 512), block reflector applied to the still-active columns.
            // Up to three forms per block, each problem runs in the one that fits its current row count kp - j0
            // (gn_kernels_qrcp_block_reg.hpp): the large forms are no longer launched once the bound fits a smaller one.
            const dim3 fg((unsigned)nl);
            // a form of the select / factor kernel: its whole-part instantiation, or the one that reads the problem list
            auto factor_form = [&](void (*whole)(SbArgs), void (*by_list)(SbArgs)) {
                hipLaunchKernelGGL(listed ? by_list : whole, fg, dim3(512), 0, s, a);
            };
            const bool big0 = rows_bound > 256, med0 = rows_bound > 128;
            bool big = big0, med = med0, small = true;
            if (hints && it < (int)h->sb_rows_max.size() && h->sb_rows_max[it] > 0) {
                // what the previous solve saw at this block id, widened by a block's worth of steps either way
                const int lo = h->sb_rows_min[it] - 32, hi = h->sb_rows_max[it] + 32;
                big = big && hi > 256;
                med = med && hi > 128 && lo <= 256;
                small = lo <= 128;
            }
            if (big) {
                GN_ROUTE(kp_blk <= 448 ? ENLSIP_GN_ROUTE_PIVOT_BLOCKS_448 : ENLSIP_GN_ROUTE_PIVOT_BLOCKS_512);
                if (kp_blk <= 448) factor_form(k_sb_factor_reg<7, 8, 4>, k_sb_factor_reg<7, 8, 4, true>);
                else factor_form(k_sb_factor_reg<8, 8, 4>, k_sb_factor_reg<8, 8, 4, true>);
            }
            if (med) { GN_ROUTE(ENLSIP_GN_ROUTE_PIVOT_BLOCKS_256); factor_form(k_sb_factor_reg<4, 8, 2>, k_sb_factor_reg<4, 8, 2, true>); }
            if (small) { GN_ROUTE(ENLSIP_GN_ROUTE_PIVOT_BLOCKS_128); factor_form(k_sb_factor_reg<2, 8, 0>, k_sb_factor_reg<2, 8, 0, true>); }
            hipLaunchKernelGGL(k_sb_update_blk, ugrid, dim3(256), 0, s, a);
            if (big == big0 && med == med0 && small) --rows_bound;
        }
        GN_HIP(hipGetLastError());
        GN_HIP(hipMemcpyAsync(hinfo, h->sbInfo, (size_t)P.batch * sizeof(SbInfo), hipMemcpyDeviceToHost, s));
        GN_HIP(hipMemcpyAsync(hstate, h->state, (size_t)P.batch * sizeof(ProbState), hipMemcpyDeviceToHost, s));
        GN_HIP(hipMemcpyAsync(h->h_sb_stat, h->sb_stat.p, 2 * SB_STAT_BLKS * sizeof(int), hipMemcpyDeviceToHost, s));
        GN_HIP(hipStreamSynchronize(s));
        done = true;
        int rows_left = 0;                       // exact maximum of kp - j0 over the unfinished problems
        for (long long i = 0; i < nl; ++i) {
            const long long k = prob_at(i);
            if (hstate[k].n2 > n2_launch) continue;                // wider problems are skipped here
            const int left = hstate[k].kp - hinfo[k].j0;
            if (left > 0) {
                done = false;
                rows_left = std::max(rows_left, left);
            }
        }
        if (done && listed) break;
        if (done) {
            int used = 0;
            for (long long k = 0; k < P.batch; ++k) used = std::max(used, hinfo[k].blk + 1);
            h->sb_hint = used + 1;
            // statistics of this solve = hints of the next one (only of a stage that ran on hints it could trust or on none:
            // a block id in which some problem found no form to run in shows smaller counts than it should)
            if (hinted && fell_back) {      // the hints misled this stage: its statistics are incomplete; the next solve runs without
                h->sb_rows_max.clear();
                h->sb_rows_min.clear();
                h->sb_rows_kp = -1;
                break;
            }
            const int nb = std::min(it, SB_STAT_BLKS);
            h->sb_rows_max.assign(nb, 0);
            h->sb_rows_min.assign(nb, 0);
            for (int b = 0; b < nb; ++b) {
                h->sb_rows_max[b] = h->h_sb_stat[b];
                h->sb_rows_min[b] = h->h_sb_stat[b] > 0 ? SB_STAT_OFF - h->h_sb_stat[SB_STAT_BLKS + b] : 0;
            }
            h->sb_rows_kp = kp_launch;
            h->sb_rows_batch = P.batch;
            break;
        }
        if (it >= max_blocks) {
            // cannot happen with every form launched (a served problem makes a step per block); never assemble half-done factors
            h->sb_rows_max.clear();
            h->sb_rows_min.clear();
            h->sb_rows_kp = -1;
            h->err = "blocked pivoted QR of R0 did not finish within its block budget";
            return 996;
        }
        hints = false;          // somebody is not done: the rest of the stage launches every form
        fell_back = true;
        rows_bound = std::min(rows_left, 512);
        chunk = 4;
    }
    hipLaunchKernelGGL(k_qd_assemble, grid, dim3(256), 0, s, q);
    GN_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// rescale path (gn_rescale.hpp): scale the resident factors of ONE problem back to the caller's data
// ---------------------------------------------------------------------------------------------
static void scale_region(hipStream_t s, double* X, long long ld, long long rows, long long cols, int shift, int upper) {
    if (rows <= 0 || cols <= 0 || shift == 0) return;
    hipLaunchKernelGGL(k_scale_region, dim3((unsigned)std::min<long long>((rows + 255) / 256, 1024), (unsigned)cols), dim3(256), 0, s,
                       X, ld, (int)rows, (int)cols, shift, upper);
}
// F_A.R, F_L11.R, b (and the pieces the distributed constraint stage keeps for the re-solve): x 2^-sc_eA.  p1, every tau, every
// reflector vector and the T blocks of Q1 do not depend on the scale.
static int unscale_constraint_side(enlsip_gn_handle h) {
    const Plan& P = h->plan;
    hipStream_t s = h->stream;
    const int sh = -h->sc_eA;
    scale_region(s, h->FA, P.n, P.kA, P.t, sh, 1);
    scale_region(s, h->FL, P.t, std::min<long long>(P.t, P.kA), P.kA, sh, 1);
    scale_region(s, h->bvec, P.t, P.t, 1, sh, 0);
    if (h->cdist.valid) {
        scale_region(s, const_cast<double*>(h->cdist.L), h->cdist.ldL, P.t, P.kA, sh, 0);
        scale_region(s, const_cast<double*>(h->cdist.qb), P.t, P.t, 1, sh, 0);
    }
    GN_HIP(hipGetLastError());
    return 0;
}
// J1 = (J*Q1)[:, 1:rankA], the carried right-hand side d, the pivoted factor R of J2 with its carried column, the saved leading
// entries of Q0'd, and the outputs d (device): x 2^-sc_eJ.  (R0 inside W is consumed by the pivoted QR only; V and T of the CAQR
// and of the pivoted QR do not depend on the scale.)
static int unscale_jacobian_side(enlsip_gn_handle h, double* dd) {
    const Plan& P = h->plan;
    hipStream_t s = h->stream;
    const int sh = -h->sc_eJ;
    const ProbState& st = h->h_state[0];
    scale_region(s, h->W, P.ldw, P.ldw, st.rankA, sh, 0);
    scale_region(s, h->W + (size_t)P.n * P.ldw, P.ldw, P.ldw, 1, sh, 0);
    scale_region(s, h->Rt, P.ldr, st.kp, st.n2, sh, 1);
    scale_region(s, h->Rt + (size_t)st.n2 * P.ldr, P.ldr, st.kp, 1, sh, 0);
    scale_region(s, h->zsave, P.ldr, st.kp, 1, sh, 0);
    scale_region(s, h->qdDiag, P.ldr, st.kp, 1, sh, 0);
    if (dd) scale_region(s, dd, P.m, P.m, 1, sh, 0);
    GN_HIP(hipGetLastError());
    return 0;
}
// largest |entry| of the four inputs of problem 0 of a one-problem solve -> power-of-two shifts that bring J, rx / A', cx to
// magnitude ~1 (0: inside the band, zero, or not finite — nothing to rescale).  A null input side is not looked at.
static int extreme_shifts(enlsip_gn_handle h, const BatchOperands& v, int* shiftJ, int* shiftA) {
    hipStream_t s = h->stream;
    const long long m = v.m, n = v.n, t = v.t, ldj = v.ldj, ldat = v.ldat;
    const double *dJ = v.J, *drx = v.rx, *dAt = v.At, *dcx = v.cx;
    unsigned long long* dmx = h->small->amax;      // its first two words
    GN_HIP(hipMemsetAsync(dmx, 0, 16, s));
    if (dJ && drx) {
        hipLaunchKernelGGL(k_amax_bits, dim3((unsigned)n), dim3(256), 0, s, dJ, ldj, (int)m, (int)n, dmx);
        hipLaunchKernelGGL(k_amax_bits, dim3(1), dim3(256), 0, s, drx, m, (int)m, 1, dmx);
    }
    if (t > 0 && dAt && dcx) {
        hipLaunchKernelGGL(k_amax_bits, dim3((unsigned)t), dim3(256), 0, s, dAt, ldat, (int)n, (int)t, dmx + 1);
        hipLaunchKernelGGL(k_amax_bits, dim3(1), dim3(256), 0, s, dcx, t, (int)t, 1, dmx + 1);
    }
    GN_HIP(hipGetLastError());
    unsigned long long hb[2] = {0, 0};
    GN_HIP(hipMemcpyAsync(hb, dmx, 16, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    auto shift_of = [](unsigned long long bits) -> int {
        double a;
        memcpy(&a, &bits, 8);
        if (!(a > 0.0) || !std::isfinite(a)) return 0;
        int e;
        (void)std::frexp(a, &e);                    // a = f 2^e, 0.5 <= f < 1
        return (e > GN_RESCALE_BAND || e < -GN_RESCALE_BAND) ? -(e - 1) : 0;
    };
    *shiftJ = shift_of(hb[0]);
    *shiftA = shift_of(hb[1]);
    return 0;
}
// the copies of a one-problem solve's inputs scaled by 2^sJ (J, rx) and 2^sA (A', cx) in rs_buf; a zero shift copies nothing
static int scaled_copies(enlsip_gn_handle h, const BatchOperands& v, int sJ, int sA) {
    const long long m = v.m, n = v.n, t = v.t;
    const size_t nJ = (size_t)m * n, nA = (size_t)n * t;
    int rc = grow(h, h->rs_buf, (nJ + (size_t)m + nA + (size_t)t + 8) * 8);
    if (rc) return rc;
    h->rs_J = (double*)h->rs_buf.p; h->rs_rx = h->rs_J + nJ; h->rs_At = h->rs_rx + m; h->rs_cx = h->rs_At + nA;
    auto copy_scaled = [&](double* dst, long long ldd, const double* src, long long lds, long long rows, long long cols, int sh) {
        hipLaunchKernelGGL(k_scale_copy, dim3((unsigned)std::min<long long>((rows + 255) / 256, 1024), (unsigned)cols), dim3(256), 0,
                           h->stream, dst, ldd, src, lds, (int)rows, (int)cols, sh);
    };
    if (sJ) {
        copy_scaled(h->rs_J, m, v.J, v.ldj, m, n, sJ);
        copy_scaled(h->rs_rx, m, v.rx, m, m, 1, sJ);
    }
    if (sA) {
        copy_scaled(h->rs_At, n, v.At, v.ldat, n, t, sA);
        copy_scaled(h->rs_cx, t, v.cx, t, t, 1, sA);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// core: device-pointer batched solve
// ---------------------------------------------------------------------------------------------
// Constraint stage with many constraints: both pivoted factorisations through the distributed QR (one launch per pivot step),
// then k_constraint only does the rank decisions, the triangular solves and the T blocks.
// Ragged batch (tk != NULL): the launch shapes stay those of t_max; each problem's records carry its own column counts, F_L11 is
// factored as the t_max x kA matrix [L11; 0] (its padded rows and carried entries are zero, so they change nothing), and the copies
// out of the working storage take each problem's own sizes and write F_A's zero columns.
// A problem list (ca.plist, `launch` entries): every grid covers the listed problems only; the workspace keeps the whole batch's
// layout, so that the pieces the re-solve reads (L11, F_L11.Q' b_buff) of the problems left alone stay where they are.
static int run_constraint_dist(enlsip_gn_handle h, ConstraintArgs ca, long long batch, long long launch, long long n, long long t,
                               const int* tk = nullptr) {
    const Plan& P = h->plan;
    hipStream_t s = h->stream;
    const int kA = P.kA;
    CwsLayout C;
    int rc = place_dev(h, h->cws, C, batch, (long long)n, (long long)t, kA);
    if (rc) return rc;
    const long long ldc = C.ldc, sMc = C.sM, sVbc = C.sVb, sRtc = C.sRt, sLc = C.sL, sVec = C.sVec, sIc = C.sI, sCandc = C.sCand;
    const int Gc = C.G;
    double *cM = C.M, *cVb = C.Vb, *cRt = C.Rt, *cL = C.L, *cDiag = C.diag, *cVn1 = C.vn1, *cVn2 = C.vn2, *cBq = C.bq, *cQb = C.qb;
    int *cChosen = C.chosen, *cPos = C.pos, *cColat = C.colat;
    QdCand* cCand = (QdCand*)C.cand;
    ProbState *stA = C.stA, *stL = C.stL;
    const unsigned gb = (unsigned)((batch + 255) / 256);
    if (tk) {
        hipLaunchKernelGGL(k_fake_state_ragged, dim3(gb), dim3(256), 0, s, stA, (int)batch, (int)n, tk, 0);
        hipLaunchKernelGGL(k_fake_state_ragged, dim3(gb), dim3(256), 0, s, stL, (int)batch, (int)n, tk, 1);
    } else {
        hipLaunchKernelGGL(k_fake_state, dim3(gb), dim3(256), 0, s, stA, (int)batch, kA, (int)t);
        hipLaunchKernelGGL(k_fake_state, dim3(gb), dim3(256), 0, s, stL, (int)batch, kA, kA);
    }

    QdArgs q{};
    q.n = (int)n; q.ldw = 0; q.ldr = (int)ldc; q.prob0 = 0; q.plist = ca.plist;
    const int* plist = ca.plist;
    const unsigned nl = (unsigned)launch;
    q.M = cM; q.sM = sMc; q.Vb = cVb; q.sVb = sVbc; q.Rt = cRt; q.sRt = sRtc;
    q.diag = cDiag; q.sDiag = sVec; q.vn1 = cVn1; q.vn2 = cVn2; q.sVn = sVec;
    q.chosen = cChosen; q.pos = cPos; q.colat = cColat; q.sI = sIc;
    q.cand = cCand; q.sCand = sCandc; q.Gmax = Gc;
    auto factor = [&](int rows, int cols, int steps) {
        const dim3 grid = qd_grid(cols, launch);
        q.step = 0;
        launch_qd_steps(grid, rows > 512, s, q, steps);
        q.step = 0;
        hipLaunchKernelGGL(k_qd_assemble, grid, dim3(256), 0, s, q);
    };
    // ---- F_A: the n x t matrix C.A' -------------------------------------------------------------------------------
    q.rows = (int)n; q.in_mode = 1; q.Ain = ca.At; q.ldain = ca.ldat; q.sAin = ca.strideAt;
    q.tau = h->tauA; q.sTau = P.sTauA; q.jpvt = h->jpvtA; q.sJ = P.sJA; q.state = stA;
    factor((int)n, (int)t, kA);
    if (tk)
        hipLaunchKernelGGL(k_copy_cols_ragged, dim3((unsigned)t, nl), dim3(256), 0, s, h->FA, n, P.sFA, (const double*)cRt, ldc,
                           sRtc, (int)n, (int)t, (int)n, tk, 0, plist);
    else
        hipLaunchKernelGGL(k_copy_cols, dim3((unsigned)t, nl), dim3(256), 0, s, h->FA, n, P.sFA, cRt, ldc, sRtc, (int)n, (int)t, plist);
    // ---- F_L11: the t x kA lower trapezoid R_A', carrying b_buff = -cx[F_A.p] ----------------------------------------
    if (tk)
        hipLaunchKernelGGL(k_bbuff_ragged, dim3((unsigned)((t + 255) / 256), nl), dim3(256), 0, s, cBq, sVec, ca.cx,
                           ca.stride_cx, (const long long*)h->jpvtA, P.sJA, (int)t, tk, plist);
    else
        hipLaunchKernelGGL(k_bbuff, dim3((unsigned)((t + 255) / 256), nl), dim3(256), 0, s, cBq, sVec, ca.cx, ca.stride_cx,
                           h->jpvtA, P.sJA, (int)t, plist);
    q.rows = (int)t; q.in_mode = 2; q.Ain = h->FA; q.ldain = n; q.sAin = P.sFA; q.rin = cBq; q.sRin = sVec; q.Lout = cL; q.sLout = sLc;
    q.tau = h->tauL; q.sTau = P.sTauL; q.jpvt = h->jpvtL; q.sJ = P.sJL; q.state = stL;
    factor((int)t, kA, (int)std::min<long long>(t, kA));
    if (tk) {
        hipLaunchKernelGGL(k_copy_cols_ragged, dim3((unsigned)kA, nl), dim3(256), 0, s, h->FL, t, P.sFL, (const double*)cRt,
                           ldc, sRtc, (int)t, kA, (int)n, tk, 1, plist);
        hipLaunchKernelGGL(k_copy_cols_ragged, dim3(1, nl), dim3(256), 0, s, cQb, sVec, sVec, (const double*)cRt, ldc, sRtc,
                           (int)t, 1, (int)n, tk, 2, plist);
    } else {
        hipLaunchKernelGGL(k_copy_cols, dim3((unsigned)kA, nl), dim3(256), 0, s, h->FL, t, P.sFL, cRt, ldc, sRtc, (int)t, kA, plist);
        hipLaunchKernelGGL(k_copy_cols, dim3(1, nl), dim3(256), 0, s, cQb, sVec, sVec, cRt + (size_t)kA * ldc, ldc, sRtc, (int)t, 1, plist);
    }
    // ---- ranks, triangular solves, T blocks ---------------------------------------------------------------------------
    ca.fa_done = 1; ca.fl_done = 1; ca.need_T = 1;
    ca.Lmat = cL; ca.ldL = ldc; ca.sL = sLc; ca.qb = cQb; ca.sQb = sVec;
    h->cdist.L = cL; h->cdist.ldL = ldc; h->cdist.sL = sLc; h->cdist.qb = cQb; h->cdist.sQb = sVec; h->cdist.valid = true;
    launch_constraint((int)std::max(n, t), (int)launch, s, ca, tk);
    GN_HIP(hipGetLastError());
    return 0;
}

// F_A, rankA, F_L11, b, p1, block T of Q1 for every problem of the batch (plan already made)
// prob0 / code_ov: the re-solve of ONE resident problem (enlsip_gn_resolve) takes the same route as the solve that produced its
// factors, so that they are rewritten bit for bit by the same kernels.
// plist / nlist: a device list of problem indices (enlsip_gn_solve_factored_batched: the problems whose working set changed).  Every
// kernel of the stage is launched over the listed problems only and touches no slot of another one.
static int run_constraint_stage(enlsip_gn_handle h, long long batch, long long m, long long n, long long t, const double* dAt,
                                long long ldat, long long strideAt, const double* dcx, double eps_rank, long long dimA_ov,
                                int prob0 = 0, int code_ov = 0, const int* plist = nullptr, long long nlist = 0) {
    const Plan& P = h->plan;
    hipStream_t s = h->stream;
    const long long launch = plist ? nlist : batch;     // workgroups (grid rows) of every launch
    h->cstage_problems += launch;
    if (prob0 == 0 && code_ov == 0 && !plist) h->cdist.valid = false;
    // the resident problem was rescaled (sc_eA != 0: one problem): the stage runs on the scaled copies of A', cx with the absolute
    // rank threshold scaled alike, and what it leaves resident is scaled back below
    const bool scaledA = h->sc_eA != 0 && batch == 1 && prob0 == 0 && t > 0;
    if (scaledA) { dAt = h->rs_At; ldat = n; strideAt = n * t; dcx = h->rs_cx; }
    ConstraintArgs ca{};
    ca.n = (int)n; ca.t = (int)t; ca.kA = P.kA; ca.m = (int)m; ca.eps_rank = eps_rank;
    ca.abs_shift = scaledA ? h->sc_eA : 0;
    ca.dimA_override = (int)dimA_ov; ca.code_override = code_ov; ca.prob0 = prob0; ca.plist = plist;
    ca.At = dAt; ca.ldat = ldat; ca.strideAt = strideAt; ca.cx = dcx; ca.stride_cx = t;
    ca.FA = h->FA; ca.sFA = P.sFA; ca.tauA = h->tauA; ca.sTauA = P.sTauA; ca.jpvtA = h->jpvtA; ca.sJA = P.sJA;
    ca.FL = h->FL; ca.sFL = P.sFL; ca.tauL = h->tauL; ca.sTauL = P.sTauL; ca.jpvtL = h->jpvtL; ca.sJL = P.sJL;
    ca.TA = h->TA; ca.sTA = P.sTA; ca.p1 = h->p1; ca.sP1 = P.sP1; ca.bvec = h->bvec; ca.sB = P.sB;
    ca.state = h->state;
    const int* tk = h->h_tk.empty() ? nullptr : (const int*)h->tkbuf.p;     // ragged batch: each problem's own t
    // many constraints: both factorisations through the distributed pivoted QR
    if (t > 64 && (size_t)n * t > (size_t)CMAT_DOUBLES) {
        GN_ROUTE(ENLSIP_GN_ROUTE_CONSTRAINT_DIST);
        int rcd = run_constraint_dist(h, ca, batch, launch, n, t, tk);
        if (rcd) return rcd;
        return scaledA ? unscale_constraint_side(h) : 0;
    }
    // F_A of a matrix that does not fit the LDS area of k_constraint: whole matrix in registers (gn_kernels_geqp3_reg.hpp)
    if (t >= 1 && t <= 64 && n <= 512 && (size_t)n * t > (size_t)CMAT_DOUBLES) {
        Geqp3RegArgs ga{};
        ga.rows = (int)n; ga.cols = (int)t; ga.A = dAt; ga.lda = ldat; ga.strideA = strideAt;
        ga.F = h->FA; ga.sF = P.sFA; ga.tau = h->tauA; ga.sTau = P.sTauA; ga.jpvt = h->jpvtA; ga.sJ = P.sJA;
        ga.T = h->TA; ga.sT = P.sTA; ga.prob0 = prob0; ga.plist = plist;
        GN_ROUTE(n <= 256 ? ENLSIP_GN_ROUTE_CONSTRAINT_REG4 : ENLSIP_GN_ROUTE_CONSTRAINT_REG8);
        if (tk) {
            if (n <= 256) hipLaunchKernelGGL(k_geqp3_reg_ragged<4>, dim3((unsigned)launch), dim3(512), 0, s, ga, tk);
            else hipLaunchKernelGGL(k_geqp3_reg_ragged<8>, dim3((unsigned)launch), dim3(512), 0, s, ga, tk);
        } else if (n <= 256) hipLaunchKernelGGL(k_geqp3_reg<4>, dim3((unsigned)launch), dim3(512), 0, s, ga);
        else hipLaunchKernelGGL(k_geqp3_reg<8>, dim3((unsigned)launch), dim3(512), 0, s, ga);
        ca.fa_done = 1;
    }
    // with F_A done the kernel only factors the t x kA matrix R_A': size its rows-per-lane instantiation (and LDS) for that
    launch_constraint(ca.fa_done ? (int)std::max<long long>(t, 1) : (int)std::max(n, t), (int)launch, s, ca, tk);
    GN_HIP(hipGetLastError());
    return scaledA ? unscale_constraint_side(h) : 0;
}

static enlsip_gn_info info_of(const ProbState& st) {
    return {st.rankA, st.rankJ2, st.code, st.dimA, st.dimJ2, st.status};
}

// stage times of the last solve from its events and the event pairs around the trailing-update launches (profiling on)
static int collect_stage_ms(enlsip_gn_handle h) {
    float ms;
    GN_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1])); h->stage_ms[ENLSIP_GN_STAGE_CONSTRAINT] = ms;
    GN_HIP(hipEventElapsedTime(&ms, h->ev[1], h->ev[2])); h->stage_ms[ENLSIP_GN_STAGE_JQ1] = ms;
    GN_HIP(hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
    float upd = 0.f;
    h->upd_launch_ms.clear();
    for (size_t i = 0; i + 1 < h->upd_used; i += 2) {
        float u;
        GN_HIP(hipEventElapsedTime(&u, h->upd_ev[i], h->upd_ev[i + 1]));
        upd += u;
        h->upd_launch_ms.push_back(u);
    }
    h->upd_launches = (long long)(h->upd_used / 2);
    h->upd_avg_ms = h->upd_launches ? upd / (float)h->upd_launches : 0.f;
    // every trailing-update launch of the sweep is "update" (far level-0 passes AND tree levels / second-panel columns);
    // "panel" = the factorisations (and whatever else the sweep launches)
    float oth = 0.f;
    for (size_t i = 0; i + 1 < h->oth_used; i += 2) {
        float u;
        GN_HIP(hipEventElapsedTime(&u, h->oth_ev[i], h->oth_ev[i + 1]));
        oth += u;
    }
    h->oth_ms = oth;
    h->oth_launches = (long long)(h->oth_used / 2);
    h->stage_ms[ENLSIP_GN_STAGE_UPDATE] = upd + oth;
    h->stage_ms[ENLSIP_GN_STAGE_PANEL] = ms - upd - oth;
    GN_HIP(hipEventElapsedTime(&ms, h->ev[3], h->ev[4])); h->stage_ms[ENLSIP_GN_STAGE_PIVOT] = ms;
    GN_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[4])); h->stage_ms[ENLSIP_GN_STAGE_TOTAL] = ms;
    return 0;
}

// a handle of the library's own (pipeline half, rescue handle, TSQR sub-handle) with h's device, flags and tile rows
static int create_helper(enlsip_gn_handle h, enlsip_gn_handle* out, hipStream_t stream) {
    enlsip_gn_opts o{};
    o.device = h->device; o.flags = h->flags; o.panel_width = 0; o.tile_rows = h->tile_rows; o.stream = (void*)stream;
    return enlsip_gn_create(out, &o);
}

// the one-problem handle for the next rescaled problem of the batch on h (the rescue_prob.size()-th), created on first use
static int next_rescue_handle(enlsip_gn_handle h, enlsip_gn_handle* out) {
    const size_t j = h->rescue_prob.size();
    if (j >= 64) { h->err = "more than 64 problems of the batch need rescaling (magnitudes beyond 2^+-400): solve them separately"; return -18; }
    if (j >= h->rescue.size()) {
        enlsip_gn_handle r = nullptr;
        int rc = create_helper(h, &r, nullptr);
        if (rc) { h->err = "could not create a handle for a rescaled problem"; return rc; }
        r->is_rescue = true;
        r->pipeline = false;
        h->rescue.push_back(r);
    }
    *out = h->rescue[j];
    return 0;
}

// ---------------------------------------------------------------------------------------------
// the solve driver: solve_dev (and the constraint-only factor_dev) as a sequence of steps
// ---------------------------------------------------------------------------------------------
// The problems a solve_dev covers: its whole part, or the listed ones of a changed-problems solve (indices in the part).
struct Covered {
    long long count = 0;
    const int* list = nullptr;      // host; NULL: problems 0 .. count - 1
    long long operator[](long long i) const { return list ? list[(size_t)i] : i; }
};
constexpr int GN_NOMINATED = GN_FLAG_NONFINITE | GN_FLAG_TINY;       // the nomination bits of gn_rescale.hpp: host-internal

// Residency bookkeeping of a call that replaces the whole part: nothing of the previous one stays addressable.
// (The routing of the accessors to the pipeline child is re-established by the batched entry point, to the resident chunk by
// solve_chunked; a resident constraint stage keeps the scale enlsip_gn_factor_constraints gave it.)
static void begin_whole_part(enlsip_gn_handle h, const BatchOperands& inputs, bool keep_constraint_scale) {
    h->split = 0;
    h->chunk0 = 0;
    h->factors_valid = false;
    h->tsqr_stage = 0;
    h->held.clear();
    h->last = inputs;
    h->sc_eJ = 0;
    if (!keep_constraint_scale) h->sc_eA = 0;
    h->rescue_prob.clear();
}
// ... of a changed-problems solve: a held re-solve of a listed problem is dropped; a listed problem that lived on a rescue handle
// gives it back (the handle moves behind the ones in use)
static void release_listed(enlsip_gn_handle h, const std::vector<int>& list) {
    for (int k : list) {
        if ((size_t)k < h->held.size()) h->held[(size_t)k] = {};
        for (size_t j = 0; j < h->rescue_prob.size(); ++j)
            if (h->rescue_prob[j] == k) {
                enlsip_gn_handle r = h->rescue[j];
                h->rescue.erase(h->rescue.begin() + (long)j);
                h->rescue.push_back(r);
                h->rescue_prob.erase(h->rescue_prob.begin() + (long)j);
                break;
            }
    }
}

// ragged batch: every problem's own t, kept on the host for the accessors and copied to the device for the constraint kernels
static int upload_tk(enlsip_gn_handle h, const int* tk, long long batch) {
    h->h_tk.assign(tk, tk + batch);
    int rc = grow(h, h->tkbuf, (size_t)batch * sizeof(int));
    if (rc) return rc;
    GN_HIP(hipMemcpyAsync(h->tkbuf.p, h->h_tk.data(), (size_t)batch * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return 0;
}

static void mark(enlsip_gn_handle h, int i) {
    if (h->profiling) (void)hipEventRecord(h->ev[i], h->stream);
}

// The constraint step of a solve: for every problem (Fresh), or for the problems of h->refit only (Factored: those with a refactor
// flag, Changed: the listed ones, which from here on are the launch set of the solve).  Without a list the resident F_A, F_L11, b,
// p1, T and state records are those of enlsip_gn_factor_constraints*.
static int constraint_step(enlsip_gn_handle h, const BatchOperands& v, const SolveMode& mode) {
    if (mode.kind == SolveMode::Fresh) {
        h->fb.valid = false;
        return run_constraint_stage(h, v.batch, v.m, v.n, v.t, v.At, v.ldat, v.strideAt, v.cx, mode.eps_rank, mode.dimA_ov);
    }
    if (h->refit.empty()) return 0;
    const size_t nl = h->refit.size();
    int rc = grow(h, h->plist_buf, nl * sizeof(int));
    if (rc) return rc;
    GN_HIP(hipMemcpyAsync(h->plist_buf.p, h->refit.data(), nl * sizeof(int), hipMemcpyHostToDevice, h->stream));
    rc = run_constraint_stage(h, v.batch, v.m, v.n, v.t, v.At, v.ldat, v.strideAt, v.cx, mode.eps_rank, mode.dimA_ov, 0, 0,
                              (const int*)h->plist_buf.p, (long long)nl);
    if (rc) return rc;
    if (mode.kind == SolveMode::Changed) { h->run_plist = (const int*)h->plist_buf.p; h->run_nlist = (long long)nl; }
    return 0;
}

// The state records of the part from the device into the host mirror.  A changed-problems solve never writes the mirror's records
// of the problems it leaves alone (a rescued problem's holds its rescue handle's record, not the device's): it reads back into a
// buffer of its own and takes the listed records from there.
static int fetch_states(enlsip_gn_handle h, const Covered& cov) {
    const size_t batch = (size_t)h->plan.batch;
    std::vector<ProbState> own;
    if (cov.list) own.resize(batch);
    GN_HIP(hipMemcpyAsync(cov.list ? own.data() : h->h_state, h->state, batch * sizeof(ProbState), hipMemcpyDeviceToHost, h->stream));
    GN_HIP(hipStreamSynchronize(h->stream));
    for (long long i = 0; cov.list && i < cov.count; ++i) h->h_state[cov[i]] = own[(size_t)cov[i]];
    return 0;
}

// The Jacobian side (steps 2-4) of the covered problems for the J, rx given — the caller's, or their scaled copies with
// abs_shift = their power of two: the choice of the launch width, then up to two attempts of J*Q1, CAQR, pivoted QR of R0, final
// kernel, nomination and state read-back.  t_min: the smallest t of the part; upper_in: J is its own R0.
static int jacobian_side(enlsip_gn_handle h, const BatchOperands& v, const SolveMode& mode, const Covered& cov, int t_min, bool upper_in,
                         const double* dJ, long long ldj, long long strideJ, const double* drx, int abs_shift) {
    const Plan& P = h->plan;
    const long long batch = v.batch, m = v.m, n = v.n;
    const int nlaunch = (int)cov.count;
    hipStream_t s = h->stream;
    // speculate rankA = min(n, t) (ragged: the smallest min(n, t_k), so that only a rank-deficient A' widens J2); verified after the solve
    int n2_launch = (int)(n - std::min<long long>(n, t_min));
    // a changed-problems solve launches with the width a solve of the whole part on the final sets ends with: no narrower than the
    // widest J2 among the problems it leaves alone (one of them had a rank-deficient A')
    if (cov.list) {
        std::vector<char> in_list((size_t)batch, 0);
        for (long long i = 0; i < cov.count; ++i) in_list[(size_t)cov[i]] = 1;
        for (long long k = 0; k < batch; ++k)
            if (!in_list[(size_t)k]) n2_launch = std::max(n2_launch, h->h_state[k].n2);
    }
    h->jstage_problems = cov.count;
    for (int attempt = 0; attempt < 2; ++attempt) {
        // 2. JQ1 = J*Q1, d_temp
        const JQ1Args qa = jq1_args(h, dJ, ldj, strideJ, drx);
        // one 256-row tile, one narrow panel (C5): J*Q1 and the panel factorisation in ONE launch, the tile handed over in LDS
        const bool fused = h->fuse_small && !upper_in && !(h->flags & ENLSIP_GN_UPDATE_REFLECTORS) &&
                           small_fused_applies(m, n, P.kA, n2_launch);
        if (fused) {
            CaqrArgs ca = caqr_args(h, 0, P.panels[0].levels[0]);
            ca.npass = 1;
            launch_jq1_factor_small(qa, ca, nlaunch, s);
            GN_HIP(hipGetLastError());
        } else launch_jq1_any(h, qa, nlaunch, s);
        mark(h, 2);
        GN_TRACE(h, "attempt %d n2_launch=%d: J*Q1 done%s", attempt, n2_launch, fused ? " (fused with the panel factorisation)" : "");
        // 3. CAQR of [J2 | d]
        if (!upper_in && !fused) {
            int rc = run_caqr(h, n2_launch);
            if (rc) return rc;
        }
        if (upper_in) GN_ROUTE(ENLSIP_GN_ROUTE_SWEEP_UPPER_INPUT);
        if (attempt > 0) GN_ROUTE(ENLSIP_GN_ROUTE_SECOND_ATTEMPT);
        mark(h, 3);
        GN_TRACE(h, "CAQR done");
        // 4. pivoted QR of R0 + solves + outputs
        FinalArgs fa = final_args(h, v, mode.eps_rank, mode.dimJ2_ov, abs_shift, n2_launch);
        const int kp_launch = (int)std::min<long long>(m, n2_launch);
        if ((size_t)kp_launch * (n2_launch + 1) > (size_t)CMAT_DOUBLES) {
            // more than 512 rows do not fit the register form of the blocked factorisation: one launch per pivot step
            // (6.5 us per step; an LDS-slab blocked form was measured at 14 us per step and is gone)
            int rc = (kp_launch > 512 && !h->qrcp_hybrid) ? run_qrcp_dist(h, n2_launch) : run_qrcp_block(h, n2_launch);
            if (rc) return rc;
            fa.refactor = 2;
        }
        GN_TRACE(h, "pivoted QR of R0 done (refactor %d)", fa.refactor);
        if (!launch_pivot_small(kp_launch, n2_launch, (int)batch, s, fa, nlaunch)) launch_pivot((int)std::min<long long>(m, n), nlaunch, s, fa);
        mark(h, 4);
        GN_TRACE(h, "final kernel done");
        // nominate problems whose largest column norm overflowed or sits at the bottom of the exponent range (gn_rescale.hpp)
        if (h->rescale_enabled && !h->h_tk.empty())
            hipLaunchKernelGGL(k_extreme_flags_ragged, dim3((unsigned)((nlaunch + 255) / 256)), dim3(256), 0, s, h->state, (const double*)h->Rt,
                               P.sRt, (const double*)h->FA, P.sFA, P.kA, n2_launch, nlaunch, (const int*)h->tkbuf.p, h->run_plist);
        else if (h->rescale_enabled)
            hipLaunchKernelGGL(k_extreme_flags, dim3((unsigned)((nlaunch + 255) / 256)), dim3(256), 0, s, h->state, (const double*)h->Rt, P.sRt,
                               (const double*)h->FA, P.sFA, P.kA, n2_launch, nlaunch, h->run_plist);
        GN_HIP(hipGetLastError());
        if (int rc = fetch_states(h, cov)) return rc;
        int n2max = 0;
        for (long long i = 0; i < cov.count; ++i) n2max = std::max(n2max, h->h_state[cov[i]].n2);
        if (n2max <= n2_launch) break;
        n2_launch = n2max;  // some A was rank deficient: J2 is wider than speculated, redo from J*Q1
    }
    return 0;
}

static bool any_nominated(enlsip_gn_handle h, const Covered& cov) {
    for (long long i = 0; i < cov.count; ++i)
        if (h->h_state[cov[i]].status & GN_NOMINATED) return true;
    return false;
}

// Magnitudes beyond the range of plain sums of squares in a one-problem solve: LAPACK's result through a power-of-two scaling in
// place (gn_rescale.hpp).  A resident constraint stage is not looked at.
static int rescale_in_place(enlsip_gn_handle h, const BatchOperands& v, const SolveMode& mode, const Covered& cov, int t_min, bool upper_in) {
    int sJ = 0, sA = 0;
    BatchOperands looked = v;
    if (mode.kind != SolveMode::Fresh) { looked.At = nullptr; looked.cx = nullptr; }
    int rc = extreme_shifts(h, looked, &sJ, &sA);
    if (rc) return rc;
    if (!sJ && !sA) return 0;
    GN_TRACE(h, "rescale: J, rx by 2^%d, A', cx by 2^%d", sJ, sA);
    rc = scaled_copies(h, v, sJ, sA);
    if (rc) return rc;
    if (sA) {
        h->sc_eA = sA;      // the stage on the scaled copies; what it leaves resident is scaled back
        rc = run_constraint_stage(h, 1, v.m, v.n, v.t, v.At, v.ldat, v.strideAt, v.cx, mode.eps_rank, mode.dimA_ov);
        if (rc) return rc;
    }
    h->sc_eJ = sJ;
    if (!sA) {
        // the constraint stage is not run again, so nothing resets the status it wrote: take back the bit 0 that the
        // final kernel of the first pass ORed in on the unscaled data (a diagonal that underflowed to zero there)
        hipLaunchKernelGGL(k_clear_status_bits, dim3(1), dim3(256), 0, h->stream, h->state, 1, 1, (const int*)nullptr);
        GN_HIP(hipGetLastError());
        h->h_state[0].status &= ~1;
    }
    rc = sJ ? jacobian_side(h, v, mode, cov, t_min, upper_in, h->rs_J, v.m, v.m * v.n, h->rs_rx, sJ + mode.abs_shift)
            : jacobian_side(h, v, mode, cov, t_min, upper_in, v.J, v.ldj, v.strideJ, v.rx, mode.abs_shift);
    if (rc) return rc;
    if (sJ) {
        rc = unscale_jacobian_side(h, v.d);
        if (rc) return rc;
    }
    GN_ROUTE(ENLSIP_GN_ROUTE_RESCALED);
    return 0;
}

// A batch (or a ragged batch of one, whose problem is solved with its own t there): every nominated problem whose inputs are beyond
// the band goes to a one-problem handle of its own, on which `run` does the caller's work (and which rescales in place); the
// accessors are routed to it.  with_J: a shift of J, rx counts too (the constraint stage alone looks at A', cx only).
static int rescue_nominated(enlsip_gn_handle h, const BatchOperands& v, const Covered& cov, bool with_J,
                            const std::function<int(enlsip_gn_handle, const BatchOperands&)>& run) {
    for (long long i = 0; i < cov.count; ++i) {
        const long long k = cov[i];
        if (!(h->h_state[k].status & GN_NOMINATED)) continue;
        int sJ = 0, sA = 0;
        BatchOperands one = v.slice(k, 1);      // offsets with the batch's strides (t_max) ...
        if (v.tk) one.t = v.tk[k];              // ... and a problem of a ragged batch rescued with its own t
        one.dinfo = nullptr; one.hinfo = nullptr; one.tk = nullptr;
        int rc = extreme_shifts(h, one, &sJ, &sA);
        if (rc) return rc;
        if (!sA && !(with_J && sJ)) continue;
        enlsip_gn_handle r = nullptr;
        rc = next_rescue_handle(h, &r);
        if (rc) return rc;
        rc = run(r, one);
        if (rc) { h->err = r->err; return rc; }
        GN_HIP(hipSetDevice(h->device));
        h->h_state[k] = r->h_state[0];
        h->rescue_prob.push_back(k);
    }
    return 0;
}

// the nomination bits are host-internal: cleared on the host mirror and on the device
static int clear_nominations(enlsip_gn_handle h, const Covered& cov) {
    for (long long i = 0; i < cov.count; ++i) h->h_state[cov[i]].status &= ~GN_NOMINATED;
    hipLaunchKernelGGL(k_clear_status_bits, dim3((unsigned)((cov.count + 255) / 256)), dim3(256), 0, h->stream, h->state, GN_NOMINATED,
                       (int)cov.count, h->run_plist);
    GN_HIP(hipGetLastError());
    return 0;
}

// The info records of the covered problems, produced on the host from the state mirror: into the caller's host array, and / or
// uploaded to its device array — whole, or the listed records in list order, scattered by one launch.  constraints_only: nothing
// about J is resident, rankJ2 and dimJ2 are zero.
static int publish_info(enlsip_gn_handle h, const BatchOperands& v, const Covered& cov, bool constraints_only) {
    if (!v.hinfo && !v.dinfo) return 0;
    hipStream_t s = h->stream;
    std::vector<enlsip_gn_info> tmp((size_t)cov.count);
    for (long long i = 0; i < cov.count; ++i) {
        tmp[(size_t)i] = info_of(h->h_state[cov[i]]);
        if (constraints_only) tmp[(size_t)i].rankJ2 = tmp[(size_t)i].dimJ2 = 0;
        if (v.hinfo) v.hinfo[cov[i]] = tmp[(size_t)i];
    }
    if (!v.dinfo) return 0;
    if (cov.list) {
        int rc = grow(h, h->info_stage, tmp.size() * sizeof(enlsip_gn_info));
        if (rc) return rc;
        GN_HIP(hipMemcpyAsync(h->info_stage.p, tmp.data(), tmp.size() * sizeof(enlsip_gn_info), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_scatter_info, dim3((unsigned)((cov.count + 255) / 256)), dim3(256), 0, s, v.dinfo,
                           (const enlsip_gn_info*)h->info_stage.p, h->run_plist, (int)cov.count);
        GN_HIP(hipGetLastError());
    } else GN_HIP(hipMemcpyAsync(v.dinfo, tmp.data(), tmp.size() * sizeof(enlsip_gn_info), hipMemcpyHostToDevice, s));
    GN_HIP(hipStreamSynchronize(s));
    return 0;
}

// One solve of the problems of v on ONE handle (the caller's, a pipeline child, a rescue handle, the TSQR sub-handle); what kind of
// solve is in `mode` alone.  mode.flags are those of this part: a Factored / Changed solve lists its flagged problems from them.
static int solve_dev(enlsip_gn_handle h, const BatchOperands& v, SolveMode mode) {
    const long long batch = v.batch, m = v.m, n = v.n, t = v.t;
    gn_route_acc = 0;
    // a changed-problems solve (enlsip_gn_solve_changed_batched, which has checked the resident state): the flagged problems only,
    // constraint stage and Jacobian side, into their own slots of the resident batch; nothing else of it is touched
    const bool listed = mode.kind == SolveMode::Changed;
    const bool reuse = mode.kind != SolveMode::Fresh;
    h->refit.clear();
    for (long long k = 0; reuse && mode.flags && k < batch; ++k)
        if (mode.flags[k]) h->refit.push_back((int)k);
    struct ListGuard {      // no launch after this solve is sized by its list
        enlsip_gn_handle h;
        ~ListGuard() { h->run_plist = nullptr; h->run_nlist = 0; }
    } list_guard{h};
    const Covered cov{listed ? (long long)h->refit.size() : batch, listed ? h->refit.data() : nullptr};
    const bool upper_in = mode.upper_input && t == 0 && m <= n;   // J is upper triangular (and unconstrained): it IS its own R0, Q0 = I
    int rc = check_limits(h, batch, m, n, t);
    if (rc) return rc;
    if (v.ldj < m) { h->err = "ldj < m"; return -7; }
    if (t > 0 && v.ldat < n) { h->err = "ldat < n"; return -11; }
    GN_HIP(hipSetDevice(h->device));
    rc = make_plan(h, batch, m, n, t);
    if (rc) return rc;
    h->eps_rank = mode.eps_rank;
    if (listed) release_listed(h, h->refit);
    else begin_whole_part(h, v.inputs(), reuse);
    int t_min = (int)t;
    if (v.tk) {
        rc = upload_tk(h, v.tk, batch);
        if (rc) return rc;
        for (int tk : h->h_tk) t_min = std::min(t_min, tk);
    } else if (!reuse) {
        h->h_tk.clear();
    }
    if (h->profiling) {
        if (!h->ev_ready) {
            for (int i = 0; i < 8; ++i) GN_HIP(hipEventCreate(&h->ev[i]));
            h->ev_ready = true;
        }
        h->upd_used = 0;
        h->upd_bytes = 0.0;
        h->upd_launch_bytes.clear();
        h->oth_used = 0;
        h->upd_all_bytes = 0.0;
    }
    mark(h, 0);
    h->constraints_only = false;
    // 1. constraint stage
    GN_TRACE(h, "solve m=%lld n=%lld t=%lld batch=%lld: constraint stage%s", m, n, t, batch, reuse ? " (resident)" : "");
    h->cstage_problems = 0;
    h->jstage_problems = 0;
    rc = constraint_step(h, v, mode);
    if (rc) return rc;
    mark(h, 1);
    GN_TRACE(h, "constraint stage done");
    // 2-4. Jacobian side
    rc = jacobian_side(h, v, mode, cov, t_min, upper_in, v.J, v.ldj, v.strideJ, v.rx, mode.abs_shift);
    if (rc) return rc;
    if (any_nominated(h, cov)) {
        if (batch == 1 && !v.tk) rc = rescale_in_place(h, v, mode, cov, t_min, upper_in);
        else rc = rescue_nominated(h, v, cov, true, [&](enlsip_gn_handle r, const BatchOperands& one) {
            const unsigned long long route_here = gn_route_acc;
            const int rcr = solve_dev(r, one, mode.fresh());        // its outputs land in the caller's slots
            gn_route_acc = route_here | r->route;
            return rcr;
        });
        if (rc) return rc;
        rc = clear_nominations(h, cov);
        if (rc) return rc;
    }
    rc = publish_info(h, v, cov, false);
    if (rc) return rc;
    if (h->profiling) {
        rc = collect_stage_ms(h);
        if (rc) return rc;
    }
    h->factors_valid = true;
    h->tsqr_stage = 0;
    h->route = gn_route_acc;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static void tsqr_drop_comm(enlsip_gn_handle h);      // gn_tsqr.inc

extern "C" {

int enlsip_gn_version(void) { return 204; }

// why the last enlsip_gn_create of this thread failed (no handle exists to carry the message): enlsip_gn_last_error(NULL)
static thread_local std::string g_create_err;

int enlsip_gn_create(enlsip_gn_handle* out, const enlsip_gn_opts* opts) {
    if (!out) return -1;
    *out = nullptr;
    g_create_err.clear();
    enlsip_gn_context* h = new (std::nothrow) enlsip_gn_context();
    if (!h) { g_create_err = "out of host memory"; return 998; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) {
        delete h;
        g_create_err = std::string("no usable HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                       "): libenlsip_gn has no CPU code path";
        return e != hipSuccess ? (int)e : 100;  // hipErrorNoDevice
    }
    int dev = (opts && opts->device >= 0) ? opts->device : -1;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    if (dev >= ndev) {
        delete h;
        g_create_err = "opts->device is not a device ordinal of this process";
        return -2;
    }
    h->device = dev;
    h->flags = opts ? opts->flags : 0;
    h->tile_rows = (opts && opts->tile_rows == 256) ? 256 : 512;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            h->cu_count = prop.multiProcessorCount;
    }
    gn::read_env_switches(h);
    if (opts && opts->panel_width != 0 && opts->panel_width != PB) {
        delete h;
        return -2;
    }
    e = hipSetDevice(dev);
    if (e != hipSuccess) {
        delete h;
        return (int)e;
    }
    if (opts && opts->stream) {
        h->stream = (hipStream_t)opts->stream;
        h->own_stream = false;
    } else {
        e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete h;
            return (int)e;
        }
        h->own_stream = true;
    }
    // single-workgroup kernels use > 64 KB of dynamic LDS
    *out = h;
    return 0;
}

int enlsip_gn_destroy(enlsip_gn_handle h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->stream2) (void)hipStreamSynchronize(h->stream2);      // look-ahead sweep: an error return may have left work there
    if (h->ws.p) (void)hipFree(h->ws.p);
    if (h->in_stage.p) (void)hipFree(h->in_stage.p);
    if (h->out_stage.p) (void)hipFree(h->out_stage.p);
    if (h->lag.p) (void)hipFree(h->lag.p);
    if (h->newton.p) (void)hipFree(h->newton.p);
    if (h->lagb_io.p) (void)hipFree(h->lagb_io.p);
    if (h->lagb_scr.p) (void)hipFree(h->lagb_scr.p);
    if (h->rsb_dims.p) (void)hipFree(h->rsb_dims.p);
    if (h->rsb_io.p) (void)hipFree(h->rsb_io.p);
    for (hipEvent_t e : h->rsb_ev)
        if (e) (void)hipEventDestroy(e);
    if (h->nwb_ws.p) (void)hipFree(h->nwb_ws.p);
    if (h->nwb_io.p) (void)hipFree(h->nwb_io.p);
    if (h->tnw_ws.p) (void)hipFree(h->tnw_ws.p);
    if (h->tnw_io.p) (void)hipFree(h->tnw_io.p);
    if (h->ssb_req.p) (void)hipFree(h->ssb_req.p);
    if (h->ssb_io.p) (void)hipFree(h->ssb_io.p);
    if (h->rec_scr.p) (void)hipFree(h->rec_scr.p);
    for (hipEvent_t e : h->nwb_ev)
        if (e) (void)hipEventDestroy(e);
    for (PinnedBuf* b : {&h->h_ssb, &h->h_rec, &h->h_nwflag, &h->h_lagflag})
        if (b->p) (void)hipHostFree(b->p);
    if (h->cws.p) (void)hipFree(h->cws.p);
    if (h->plist_buf.p) (void)hipFree(h->plist_buf.p);
    if (h->info_stage.p) (void)hipFree(h->info_stage.p);
    if (h->scratch.p) (void)hipFree(h->scratch.p);
    if (h->xbuf.p) (void)hipFree(h->xbuf.p);
    if (h->tsqr_part.p) (void)hipFree(h->tsqr_part.p);
    if (h->tsqr_prod.p) (void)hipFree(h->tsqr_prod.p);
    tsqr_drop_comm(h);
    if (h->h_state) (void)hipHostFree(h->h_state);
    if (h->h_sbinfo) (void)hipHostFree(h->h_sbinfo);
    if (h->h_sb_stat) (void)hipHostFree(h->h_sb_stat);
    if (h->sb_stat.p) (void)hipFree(h->sb_stat.p);
    if (h->ev_ready)
        for (int i = 0; i < 8; ++i) (void)hipEventDestroy(h->ev[i]);
    for (hipEvent_t e : h->upd_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->oth_ev) (void)hipEventDestroy(e);
    if (h->rs_buf.p) (void)hipFree(h->rs_buf.p);
    for (enlsip_gn_handle r : h->rescue) (void)enlsip_gn_destroy(r);
    if (h->sub) (void)enlsip_gn_destroy(h->sub);
    if (h->child) (void)enlsip_gn_destroy(h->child);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (hipEvent_t e : h->la_events) (void)hipEventDestroy(e);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    if (h->own_stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

const char* enlsip_gn_last_error(enlsip_gn_handle h) {
    if (!h) return g_create_err.empty() ? "null handle" : g_create_err.c_str();
    if (h->err.empty() && h->child && !h->child->err.empty()) return h->child->err.c_str();
    return h->err.c_str();
}

int enlsip_gn_synchronize(enlsip_gn_handle h) {
    if (!h) return -1;
    GN_HIP(hipStreamSynchronize(h->stream));
    if (h->child) GN_HIP(hipStreamSynchronize(h->child->stream));
    return 0;
}

int enlsip_gn_set_profiling(enlsip_gn_handle h, int enable) {
    if (!h) return -1;
    h->profiling = enable != 0;
    h->profile_all_updates = enable >= 2;
    return 0;
}

int enlsip_gn_get_stage_ms(enlsip_gn_handle h, float* ms) {
    if (!h) return -1;
    if (!ms) return -2;
    for (int i = 0; i < ENLSIP_GN_STAGE_COUNT; ++i) ms[i] = h->stage_ms[i];
    return 0;
}

int enlsip_gn_get_update_table(enlsip_gn_handle h, int64_t cap, double* algorithmic_bytes, float* ms, int64_t* count) {
    if (!h) return -1;
    const size_t nl = std::min(h->upd_launch_ms.size(), h->upd_launch_bytes.size());
    if (count) *count = (int64_t)nl;
    for (size_t i = 0; i < nl && (int64_t)i < cap; ++i) {
        if (algorithmic_bytes) algorithmic_bytes[i] = h->upd_launch_bytes[i];
        if (ms) ms[i] = h->upd_launch_ms[i];
    }
    return 0;
}

// In-place read-modify-write stream over `bytes` of scratch memory with the trailing update's access shape (256-thread
// workgroups, 16-byte non-temporal loads and stores, 256 contiguous bytes per 16 lanes): the ceiling an in-place update of
// streamed data can reach on THIS device, measured with HIP events on the handle's stream.
__global__ __launch_bounds__(256) void k_stream_inplace(double* buf, long long n2pairs) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    d2* p = (d2*)buf;
    // one workgroup = 32 KB chunks of 256 x 16 B, eight of them (the update's 128 KB block of C per workgroup would be sixteen)
    const long long chunk = 256;
    for (long long c = (long long)blockIdx.x * 8; c < (long long)blockIdx.x * 8 + 8; ++c) {
        const long long i = c * chunk + threadIdx.x;
        if (i < n2pairs) {
            d2 x = __builtin_nontemporal_load(p + i);
            x[0] += 1.0; x[1] -= 1.0;
            __builtin_nontemporal_store(x, p + i);
        }
    }
}
int enlsip_gn_measure_stream(enlsip_gn_handle h, int64_t bytes, int reps, double* gbytes_per_s) {
    if (!h) return -1;
    GN_TRY
    if (bytes < (1 << 20) || reps < 1 || !gbytes_per_s) { h->err = "measure_stream: bytes >= 1 MiB, reps >= 1, non-NULL result"; return -2; }
    GN_HIP(hipSetDevice(h->device));
    int rc = grow(h, h->scratch, (size_t)bytes);
    if (rc) return rc;
    const long long pairs = bytes / 16;
    const unsigned grid = (unsigned)((pairs + 256 * 8 - 1) / (256 * 8));
    hipEvent_t e0, e1;
    GN_HIP(hipEventCreate(&e0));
    GN_HIP(hipEventCreate(&e1));
    GN_HIP(hipMemsetAsync(h->scratch.p, 0, (size_t)bytes, h->stream));
    hipLaunchKernelGGL(k_stream_inplace, dim3(grid), dim3(256), 0, h->stream, (double*)h->scratch.p, pairs);
    GN_HIP(hipEventRecord(e0, h->stream));
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_stream_inplace, dim3(grid), dim3(256), 0, h->stream, (double*)h->scratch.p, pairs);
    GN_HIP(hipEventRecord(e1, h->stream));
    GN_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    GN_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *gbytes_per_s = 2.0 * (double)(pairs * 16) * reps / ((double)ms * 1e-3) / 1e9;
    return 0;
    GN_CATCH(h)
}

// debugging aid: the working matrix W (ldw x (n + 1)) of problem `prob` as it stands
int enlsip_gn_debug_copy_W(enlsip_gn_handle h, int64_t prob, double* out, int64_t* ldw_out, int64_t cap_doubles) {
    if (!h || !h->have_plan) return -1;
    const Plan& P = h->plan;
    if (ldw_out) *ldw_out = P.ldw;
    const size_t need = (size_t)P.ldw * (P.n + 1);
    if (!out || (size_t)cap_doubles < need) return -3;
    GN_HIP(hipSetDevice(h->device));
    GN_HIP(hipStreamSynchronize(h->stream));
    GN_HIP(hipMemcpy(out, h->W + prob * P.sW, need * 8, hipMemcpyDeviceToHost));
    return 0;
}

int enlsip_gn_get_update_stats(enlsip_gn_handle h, float* avg_ms, int64_t* launches, double* bytes) {
    if (!h) return -1;
    if (avg_ms) *avg_ms = h->upd_avg_ms;
    if (launches) *launches = h->upd_launches;
    if (bytes) *bytes = h->upd_bytes;
    return 0;
}

int enlsip_gn_get_route(enlsip_gn_handle h, uint64_t* mask) {
    if (!h) return -1;
    if (!mask) return -2;
    *mask = (uint64_t)h->route;
    return 0;
}

const char* enlsip_gn_route_name(int bit) {
    static_assert(ENLSIP_GN_ROUTE_COUNT == 52, "one name per route bit");
    static const char* const names[ENLSIP_GN_ROUTE_COUNT] = {
        "constraint_wave32", "constraint_wave64", "constraint_lds_r1_256", "constraint_lds_r1_512", "constraint_lds_r2",
        "constraint_lds_r4", "constraint_lds_r8", "constraint_lds_r16", "constraint_global", "constraint_reg4", "constraint_reg8", "constraint_dist",
        "jq1_fused_small", "jq1_rows32", "jq1_rows2", "jq1_rows64", "jq1_v2_n128", "jq1_v2_n256", "jq1_v2_n384", "jq1_v2_n512",
        "jq1_mfma", "jq1_plain", "sweep_plain", "sweep_pairs", "sweep_lookahead", "sweep_passenger", "sweep_tree",
        "sweep_tile256", "sweep_tile512", "sweep_reflectors", "sweep_upper_input", "pivot_wave32", "pivot_wave64", "pivot_wave2",
        "pivot_lds_r1_256", "pivot_lds_r1_512", "pivot_lds_r2", "pivot_lds_r4", "pivot_lds_r8", "pivot_lds_r16", "pivot_blocks",
        "pivot_blocks_448", "pivot_blocks_512", "pivot_blocks_256", "pivot_blocks_128", "pivot_hybrid", "pivot_steps",
        "pipeline_split", "chunked", "second_attempt", "rescaled", "sweep_xmap"};
    return (bit >= 0 && bit < ENLSIP_GN_ROUTE_COUNT) ? names[bit] : nullptr;
}

int enlsip_gn_get_launch_plan(enlsip_gn_handle h, int64_t* pipeline_split, int* panel_pairs, int64_t* tile_rows) {
    if (!h) return -1;
    if (!h->have_plan) { h->err = "no solve on this handle yet"; return -1; }
    if (pipeline_split) *pipeline_split = h->split;
    if (panel_pairs) *panel_pairs = h->plan.pair ? 1 : 0;
    if (tile_rows) *tile_rows = 64LL * h->plan.RPL;
    return 0;
}

int enlsip_gn_get_update_totals(enlsip_gn_handle h, float* far_ms, float* other_ms, int64_t* other_launches, double* all_panels_bytes) {
    if (!h) return -1;
    if (far_ms) *far_ms = h->upd_avg_ms * (float)h->upd_launches;
    if (other_ms) *other_ms = h->oth_ms;
    if (other_launches) *other_launches = h->oth_launches;
    if (all_panels_bytes) *all_panels_bytes = h->upd_all_bytes;
    return 0;
}

// Where a batch is cut into two pipelined halves (see gn_context.hpp): problems [split, batch) run on the child handle; 0 = no split.
// one-tile problems of the wave-per-problem pipeline (n <= 64, m <= 512: C3, C5) are a handful of short, uniform launches with
// nothing latency-bound to hide behind them: the split costs C3 4 % (1.276 -> 1.325 M solves/s without it), C5 nothing
static long long pipeline_split_of(enlsip_gn_handle h, long long batch, long long m, long long n) {
    const bool small_uniform = (n <= 64 && m <= 512) && !h->pipeline_forced;
    return (h->pipeline && !h->profiling && batch >= h->pipeline_min && !small_uniform) ? (batch + 1) / 2 : 0;
}

// Orders `stream` (a pipeline child's) after everything the caller has enqueued on this handle's stream.
static int fork_after(enlsip_gn_handle h, hipStream_t stream) {
    if (!h->ev_fork) GN_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    GN_HIP(hipEventRecord(h->ev_fork, h->stream));
    GN_HIP(hipStreamWaitEvent(stream, h->ev_fork, 0));
    return 0;
}

// part(handle, first problem, count) for the two halves of a batch split at b0, on two streams: the child's stream is ordered after
// everything the caller has enqueued on this handle's stream (fork_after), the second half is driven by a host thread, and both
// halves are complete when this returns.  Records the split for the accessors.
static int on_both_halves(enlsip_gn_handle h, long long batch, long long b0,
                          const std::function<int(enlsip_gn_handle, long long, long long)>& part) {
    GN_HIP(hipSetDevice(h->device));
    if (!h->child) {
        int rc = create_helper(h, &h->child, nullptr);
        if (rc) { h->err = "could not create the second pipeline handle"; return rc; }
        h->child->pipeline = false;
    }
    int rc = fork_after(h, h->child->stream);
    if (rc) return rc;
    const long long b1 = batch - b0;
    enlsip_gn_handle c = h->child;
    int rc1 = 0;
    std::thread worker([&] {
        (void)hipSetDevice(c->device);
        try {
            rc1 = part(c, b0, b1);
        } catch (...) {
            c->err = "exception in the second pipeline half (out of host memory?)";
            rc1 = 997;
        }
    });
    int rc0;
    try {
        rc0 = part(h, 0LL, b0);
    } catch (...) {
        worker.join();
        throw;
    }
    worker.join();
    if (rc0) return rc0;
    if (rc1) { h->err = c->err; return rc1; }
    h->split = b0;
    h->route |= c->route | (1ull << ENLSIP_GN_ROUTE_PIPELINE_SPLIT);
    return 0;
}

// One launch set over at most GN_MAX_LAUNCH_BATCH problems: either two pipelined halves on two streams or one solve_dev.
// With a resident constraint stage (mode Factored) the halves are those the stage was placed on: enlsip_gn_factor_constraints_batched
// recorded its split, and the solve must come to the same one.
static int solve_launchable(enlsip_gn_handle h, const BatchOperands& v, SolveMode mode) {
    h->split = 0;
    const long long batch = v.batch, m = v.m, n = v.n;
    const bool plain = (mode.dimA_ov < 0 && mode.dimJ2_ov < 0);
    const long long b0 = plain ? pipeline_split_of(h, batch, m, n) : 0;
    if (mode.kind == SolveMode::Factored && b0 != (h->fb.valid ? h->fb.split : 0)) {
        h->err = "the batch would be split over the pipeline halves differently from the constraint stage that is resident "
                 "(profiling or the pipeline setting changed in between?): call enlsip_gn_factor_constraints_batched again";
        return -1;
    }
    if (b0 > 0)
        return on_both_halves(h, batch, b0, [&](enlsip_gn_handle hh, long long k0, long long cnt) {
            return solve_dev(hh, v.slice(k0, cnt), mode.part(k0));
        });
    return solve_dev(h, v, mode);
}

// Any batch: consecutive chunks of at most GN_MAX_LAUNCH_BATCH problems (the problem index is a grid y / z dimension).  The
// factors that stay resident are those of the LAST chunk; accessors address problems by their index in the whole batch and
// report an error for the earlier chunks (gn_accessors.inc: map_resident).
static int solve_chunked(enlsip_gn_handle h, const BatchOperands& v, SolveMode mode) {
    h->chunk0 = 0;
    const long long batch = v.batch;
    const long long nchunks = (batch + GN_MAX_LAUNCH_BATCH - 1) / GN_MAX_LAUNCH_BATCH;
    const long long per = (batch + nchunks - 1) / nchunks;
    unsigned long long route_all = nchunks > 1 ? (1ull << ENLSIP_GN_ROUTE_CHUNKED) : 0ull;
    for (long long c0 = 0; c0 < batch; c0 += per) {
        int rc = solve_launchable(h, v.slice(c0, std::min(per, batch - c0)), mode.part(c0));
        if (rc) return rc;
        h->chunk0 = c0;
        route_all |= h->route;
        h->route = route_all;
    }
    return 0;
}

int enlsip_gn_solve_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t,
                                const double* dJ, int64_t ldj, int64_t strideJ, const double* drx,
                                const double* dAt, int64_t ldat, int64_t strideAt, const double* dcx,
                                double eps_rank, double* dp, double* db, double* dd, enlsip_gn_info* dinfo,
                                int64_t* djpvtA, int64_t* djpvtL, int64_t* djpvtJ2) {
    if (!h) return -1;
    GN_TRY
    int rc = check_limits(h, batch, m, n, t);
    if (rc) return rc;
    if (!dJ) { h->err = "dJ is NULL"; return -6; }
    if (!drx) { h->err = "drx is NULL"; return -9; }
    if (t > 0 && (!dAt || !dcx)) { h->err = "dAt / dcx is NULL with t > 0"; return -10; }
    return solve_chunked(h, {batch, m, n, t, dJ, ldj, strideJ, drx, dAt, ldat, strideAt, dcx, dp, db, dd, dinfo, (long long*)djpvtA,
                             (long long*)djpvtL, (long long*)djpvtJ2}, {SolveMode::Fresh, nullptr, false, -1, -1, eps_rank});
    GN_CATCH(h)
}

static int solve_factored_core(enlsip_gn_handle h, const BatchOperands& v, const int64_t* refactor, double eps_rank, bool host_form);

// is any of the first `batch` refactor / changed flags set?  (NULL: none)
static bool any_flag(const int64_t* flags, int64_t batch) {
    for (int64_t k = 0; flags && k < batch; ++k)
        if (flags[k]) return true;
    return false;
}

// hv: the caller's host arrays (hinfo = the info records): staged packed (ld = m / n), solved, outputs copied back
// mode Factored: the constraint stage is resident and A', cx sit in their staging slots — of one problem (enlsip_gn_solve_factored),
// or, with per-problem t (hv.tk), of a whole batch (enlsip_gn_solve_factored_batched, which has checked the state), where the
// problems with a refactor flag bring new A', cx into their slots
static int solve_host(enlsip_gn_handle h, const BatchOperands& hv, SolveMode mode) {
    if (!h) return -1;
    GN_TRY
    const long long batch = hv.batch, m = hv.m, n = hv.n, t = hv.t, dimA_ov = mode.dimA_ov, dimJ2_ov = mode.dimJ2_ov;
    const bool factored = mode.kind == SolveMode::Factored, batched_factored = factored && hv.tk;
    const int64_t* refactor = mode.flags;
    int rc = check_limits(h, batch, m, n, t);
    if (rc) return rc;
    if (!hv.J) { h->err = "J is NULL"; return -6; }
    if (hv.ldj < m) { h->err = "ldj < m"; return -7; }
    if (!hv.rx) { h->err = "rx is NULL"; return -9; }
    if (factored && !batched_factored) {
        const Plan& P = h->plan;
        if (!(h->factors_valid && h->constraints_only && h->have_plan && P.batch == 1 && P.m == m && P.n == n && P.t == t)) {
            h->err = "enlsip_gn_solve_factored needs enlsip_gn_factor_constraints with the same m, n, t right before";
            return -1;
        }
    } else if (!factored) {
        if (t > 0 && (!hv.At || !hv.cx)) { h->err = "At / cx is NULL with t > 0"; return -10; }
        if (t > 0 && hv.ldat < n) { h->err = "ldat < n"; return -11; }
    }
    // truncation dimensions index the triangular factors: dimA <= min(n, t) = rows of F_L11.R, dimJ2 <= min(m, n) >= kp
    // (the kernels clamp dimJ2 to kp = min(m, n - rankA), which is only known on the device)
    if (dimA_ov > std::min(n, t)) { h->err = "dimA_override > min(n, t)"; return -16; }
    if (dimJ2_ov > std::min(m, n)) { h->err = "dimJ2_override > min(m, n)"; return -17; }
    GN_HIP(hipSetDevice(h->device));
    const int kA = (int)std::min(n, t);
    StageIn in;       // inputs packed (ld = m / n), outputs packed
    StageOut out;
    rc = place_dev(h, h->in_stage, in, batch, m, n, t);
    if (rc) return rc;
    rc = place_dev(h, h->out_stage, out, batch, m, n, t);
    if (rc) return rc;
    double *dJ = in.J, *drx = in.rx, *dAt = in.At, *dcx = in.cx, *dp = out.p, *db = out.b, *dd = out.d;
    long long *djA = out.jA, *djL = out.jL, *djJ = out.jJ;
    const BatchOperands dv{batch, m, n, t, dJ, m, m * n, drx, dAt, n, n * t, dcx, dp, db, dd, nullptr, djA, djL, djJ, hv.hinfo, hv.tk};
    hipStream_t s = h->stream;
    for (int64_t k = 0; k < batch; ++k) {
        GN_HIP(hipMemcpy2DAsync(dJ + (size_t)k * m * n, (size_t)m * 8, hv.J + (size_t)k * hv.strideJ, (size_t)hv.ldj * 8,
                                (size_t)m * 8, (size_t)n, hipMemcpyHostToDevice, s));
        if (t > 0 && (!factored || (refactor && refactor[k]))) {
            GN_HIP(hipMemcpy2DAsync(dAt + (size_t)k * n * t, (size_t)n * 8, hv.At + (size_t)k * hv.strideAt,
                                    (size_t)hv.ldat * 8, (size_t)n * 8, (size_t)t, hipMemcpyHostToDevice, s));
            if (factored) GN_HIP(hipMemcpyAsync(dcx + (size_t)k * t, hv.cx + (size_t)k * t, (size_t)t * 8, hipMemcpyHostToDevice, s));
        }
    }
    GN_HIP(hipMemcpyAsync(drx, hv.rx, (size_t)batch * m * 8, hipMemcpyHostToDevice, s));
    if (t > 0 && !factored) GN_HIP(hipMemcpyAsync(dcx, hv.cx, (size_t)batch * t * 8, hipMemcpyHostToDevice, s));
    rc = batched_factored ? solve_factored_core(h, dv, refactor, mode.eps_rank, true) : solve_chunked(h, dv, mode);
    if (rc) return rc;
    if (hv.p) GN_HIP(hipMemcpyAsync(hv.p, dp, (size_t)batch * n * 8, hipMemcpyDeviceToHost, s));
    if (hv.b && t > 0) GN_HIP(hipMemcpyAsync(hv.b, db, (size_t)batch * t * 8, hipMemcpyDeviceToHost, s));
    if (hv.d) GN_HIP(hipMemcpyAsync(hv.d, dd, (size_t)batch * m * 8, hipMemcpyDeviceToHost, s));
    if (hv.jpvtA && t > 0) GN_HIP(hipMemcpyAsync(hv.jpvtA, djA, (size_t)batch * t * 8, hipMemcpyDeviceToHost, s));
    if (hv.jpvtL && kA > 0) GN_HIP(hipMemcpyAsync(hv.jpvtL, djL, (size_t)batch * kA * 8, hipMemcpyDeviceToHost, s));
    if (hv.jpvtJ2) GN_HIP(hipMemcpyAsync(hv.jpvtJ2, djJ, (size_t)batch * n * 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    return 0;
    GN_CATCH(h)
}

// the constraint stage of ONE problem from device buffers (enlsip_gn_factor_constraints after its staging; a problem of
// enlsip_gn_factor_constraints_batched whose magnitudes need the rescaling, on its rescue handle)
static int factor_one_dev(enlsip_gn_handle h, long long m, long long n, long long t, const double* dAt, long long ldat, const double* dcx,
                          double eps_rank, enlsip_gn_info* info) {
    GN_HIP(hipSetDevice(h->device));
    h->fb.valid = false;
    int rc = make_plan(h, 1, m, n, t);
    if (rc) return rc;
    hipStream_t s = h->stream;
    BatchOperands v{1, m, n, t};     // no J, rx: the constraint side only
    v.At = dAt; v.ldat = ldat; v.strideAt = ldat * t; v.cx = dcx;
    h->eps_rank = eps_rank;
    begin_whole_part(h, v, false);
    h->h_tk.clear();
    rc = run_constraint_stage(h, 1, m, n, t, dAt, ldat, ldat * t, dcx, eps_rank, -1);
    if (rc) return rc;
    if (h->rescale_enabled && t > 0)
        hipLaunchKernelGGL(k_extreme_flags, dim3(1), dim3(256), 0, s, h->state, (const double*)nullptr, 0LL, (const double*)h->FA, h->plan.sFA,
                           h->plan.kA, 0, 1, (const int*)nullptr);
    GN_HIP(hipMemcpyAsync(h->h_state, h->state, sizeof(ProbState), hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    if (h->h_state[0].status & GN_NOMINATED) {
        // A', cx beyond the range of plain sums of squares: the stage again on copies scaled by a power of two (gn_rescale.hpp)
        int sJ = 0, sA = 0;
        rc = extreme_shifts(h, v, &sJ, &sA);
        if (rc) return rc;
        if (sA) {
            rc = scaled_copies(h, v, 0, sA);
            if (rc) return rc;
            h->sc_eA = sA;
            rc = run_constraint_stage(h, 1, m, n, t, dAt, ldat, ldat * t, dcx, eps_rank, -1);
            if (rc) return rc;
            GN_HIP(hipMemcpyAsync(h->h_state, h->state, sizeof(ProbState), hipMemcpyDeviceToHost, s));
            GN_HIP(hipStreamSynchronize(s));
            h->route |= (1ull << ENLSIP_GN_ROUTE_RESCALED);
        }
        rc = clear_nominations(h, {1});
        if (rc) return rc;
    }
    h->factors_valid = true;
    h->tsqr_stage = 0;
    h->constraints_only = true;
    v.hinfo = info;
    return publish_info(h, v, {1}, true);
}

int enlsip_gn_factor_constraints(enlsip_gn_handle h, int64_t m, int64_t n, int64_t t, const double* At, int64_t ldat,
                                 const double* cx, double eps_rank, enlsip_gn_info* info) {
    if (!h) return -1;
    int rc = check_limits(h, 1, m, n, t);
    if (rc) return rc;
    if (t > 0 && (!At || !cx)) return -5;
    if (t > 0 && ldat < n) return -6;
    GN_HIP(hipSetDevice(h->device));
    StageIn in;       // solve_host's: a following solve of the same shape finds A', cx in their slots
    rc = place_dev(h, h->in_stage, in, 1LL, (long long)m, (long long)n, (long long)t);
    if (rc) return rc;
    double *dAt = in.At, *dcx = in.cx;
    hipStream_t s = h->stream;
    if (t > 0) {
        GN_HIP(hipMemcpy2DAsync(dAt, (size_t)n * 8, At, (size_t)ldat * 8, (size_t)n * 8, (size_t)t, hipMemcpyHostToDevice, s));
        GN_HIP(hipMemcpyAsync(dcx, cx, (size_t)t * 8, hipMemcpyHostToDevice, s));
    }
    return factor_one_dev(h, m, n, t, dAt, n, dcx, eps_rank, info);
}

int enlsip_gn_solve_factored(enlsip_gn_handle h, int64_t m, int64_t n, int64_t t, const double* J, int64_t ldj,
                             const double* rx, double eps_rank, int64_t dimJ2_override, double* p, double* b, double* d,
                             enlsip_gn_info* info, int64_t* jpvtA, int64_t* jpvtL, int64_t* jpvtJ2) {
    return solve_host(h, {1, m, n, t, J, ldj, ldj * n, rx, nullptr, n, n * t, nullptr, p, b, d, nullptr, (long long*)jpvtA,
                          (long long*)jpvtL, (long long*)jpvtJ2, info}, {SolveMode::Factored, nullptr, false, -1, dimJ2_override, eps_rank});
}

int enlsip_gn_solve_batched(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t, const double* J,
                            int64_t ldj, int64_t strideJ, const double* rx, const double* At, int64_t ldat,
                            int64_t strideAt, const double* cx, double eps_rank, double* p, double* b, double* d,
                            enlsip_gn_info* info, int64_t* jpvtA, int64_t* jpvtL, int64_t* jpvtJ2) {
    return solve_host(h, {batch, m, n, t, J, ldj, strideJ, rx, At, ldat, strideAt, cx, p, b, d, nullptr, (long long*)jpvtA,
                          (long long*)jpvtL, (long long*)jpvtJ2, info}, {SolveMode::Fresh, nullptr, false, -1, -1, eps_rank});
}

// ---- ragged batch: one t per problem (update_working_set, src/enlsip_functions.jl:686-795, gives every problem its own W.t and
// calls gn_search_direction with it, :725, :743, :762, :771, :789).  The batch is planned and launched with t_max; the constraint
// kernels read each problem's t and write the identity padding up to t_max, so that everything downstream runs unchanged.
// Argument errors are LAPACK-style (position in the argument list), all checked before anything is launched.
static int check_ragged(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t, const double* J,
                        int64_t ldj, const double* rx, const double* At, int64_t ldat, int64_t strideAt, const double* cx,
                        std::vector<int>& tk, bool with_J = true, bool with_A = true, bool t_optional = false) {
    int rc = check_limits(h, batch, m, n, t_max);
    if (rc) return rc;
    if (!t && !t_optional) { h->err = "t is NULL"; return -6; }
    if (with_J) {
        if (!J) { h->err = "J is NULL"; return -7; }
        if (ldj < m) { h->err = "ldj < m"; return -8; }
        if (!rx) { h->err = "rx is NULL"; return -10; }
    }
    if (with_A) {
        if (t_max > 0 && !At) { h->err = "At is NULL with t_max > 0"; return -11; }
        if (t_max > 0 && ldat < n) { h->err = "ldat < n"; return -12; }
        if (t_max > 0 && strideAt < ldat * t_max) { h->err = "strideAt < ldat * t_max"; return -13; }
        if (t_max > 0 && !cx) { h->err = "cx is NULL with t_max > 0"; return -14; }
    }
    tk.assign((size_t)batch, (int)t_max);
    for (int64_t k = 0; t && k < batch; ++k) {
        if (t[k] < 0 || t[k] > t_max) {
            h->err = "t[" + std::to_string(k) + "] = " + std::to_string(t[k]) + " is outside 0..t_max";
            return -6;
        }
        tk[(size_t)k] = (int)t[k];
    }
    return 0;
}

int enlsip_gn_solve_batched_ragged(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                   const double* J, int64_t ldj, int64_t strideJ, const double* rx, const double* At, int64_t ldat,
                                   int64_t strideAt, const double* cx, double eps_rank, double* p, double* b, double* d,
                                   enlsip_gn_info* info, int64_t* jpvtA, int64_t* jpvtL, int64_t* jpvtJ2) {
    if (!h) return -1;
    GN_TRY
    std::vector<int> tk;
    int rc = check_ragged(h, batch, m, n, t_max, t, J, ldj, rx, At, ldat, strideAt, cx, tk);
    if (rc) return rc;
    return solve_host(h, {batch, m, n, t_max, J, ldj, strideJ, rx, At, ldat, strideAt, cx, p, b, d, nullptr, (long long*)jpvtA,
                          (long long*)jpvtL, (long long*)jpvtJ2, info, tk.data()}, {SolveMode::Fresh, nullptr, false, -1, -1, eps_rank});
    GN_CATCH(h)
}

int enlsip_gn_solve_batched_ragged_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                       const double* dJ, int64_t ldj, int64_t strideJ, const double* drx, const double* dAt,
                                       int64_t ldat, int64_t strideAt, const double* dcx, double eps_rank, double* dp, double* db,
                                       double* dd, enlsip_gn_info* dinfo, int64_t* djpvtA, int64_t* djpvtL, int64_t* djpvtJ2) {
    if (!h) return -1;
    GN_TRY
    std::vector<int> tk;
    int rc = check_ragged(h, batch, m, n, t_max, t, dJ, ldj, drx, dAt, ldat, strideAt, dcx, tk);
    if (rc) return rc;
    return solve_chunked(h, {batch, m, n, t_max, dJ, ldj, strideJ, drx, dAt, ldat, strideAt, dcx, dp, db, dd, dinfo,
                             (long long*)djpvtA, (long long*)djpvtL, (long long*)djpvtJ2, nullptr, tk.data()},
                         {SolveMode::Fresh, nullptr, false, -1, -1, eps_rank});
    GN_CATCH(h)
}

// ---- batched constraint stage and the solve that goes on with it (update_working_set, src/enlsip_functions.jl:700-704 before the
// deletion decision, :725 / :771 after it), see include/enlsip_gn.h -------------------------------------------------------------

// The constraint stage of the problems of v (device buffers, v.tk on the host) on ONE handle: the parent or a pipeline child.
// The steps are solve_dev's; what differs: only a shift of A', cx sends a problem to a rescue handle, what runs there is the
// constraint stage of one problem, and the info records carry nothing about J.
static int factor_dev(enlsip_gn_handle h, const BatchOperands& v, double eps_rank) {
    const long long batch = v.batch, m = v.m, n = v.n, t = v.t;
    const Covered cov{batch};
    GN_HIP(hipSetDevice(h->device));
    gn_route_acc = 0;
    h->cstage_problems = 0;
    h->jstage_problems = 0;
    int rc = make_plan(h, batch, m, n, t);
    if (rc) return rc;
    const Plan& P = h->plan;
    h->eps_rank = eps_rank;
    begin_whole_part(h, v.inputs(), false);         // J, rx absent: the consumers that need them say so
    hipStream_t s = h->stream;
    rc = upload_tk(h, v.tk, batch);
    if (rc) return rc;
    rc = run_constraint_stage(h, batch, m, n, t, v.At, v.ldat, v.strideAt, v.cx, eps_rank, -1);
    if (rc) return rc;
    if (h->rescale_enabled && t > 0)
        hipLaunchKernelGGL(k_extreme_flags_ragged, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, h->state, (const double*)nullptr, 0LL,
                           (const double*)h->FA, P.sFA, P.kA, 0, (int)batch, (const int*)h->tkbuf.p, (const int*)nullptr);
    GN_HIP(hipGetLastError());
    rc = fetch_states(h, cov);
    if (rc) return rc;
    // A', cx beyond the range of plain sums of squares (gn_rescale.hpp): the accessors and the first estimate are routed to the
    // rescue handle
    if (any_nominated(h, cov)) {
        rc = rescue_nominated(h, v, cov, false, [&](enlsip_gn_handle r, const BatchOperands& one) {
            const int rcr = factor_one_dev(r, m, n, one.t, one.At, one.ldat, one.cx, eps_rank, nullptr);
            if (!rcr) gn_route_acc |= r->route & (1ull << ENLSIP_GN_ROUTE_RESCALED);
            return rcr;
        });
        if (rc) return rc;
        rc = clear_nominations(h, cov);
        if (rc) return rc;
    }
    rc = publish_info(h, v, cov, true);
    if (rc) return rc;
    h->factors_valid = true;
    h->tsqr_stage = 0;
    h->constraints_only = true;
    h->route = gn_route_acc;
    return 0;
}

// Both forms of enlsip_gn_factor_constraints_batched after their checks (and the host form's staging): every problem's stage on the
// handle the following solve will run it on, and the record that lets that solve recognise it.
static int factor_batched_core(enlsip_gn_handle h, const BatchOperands& v, double eps_rank, bool host_form) {
    h->fb.valid = false;
    const long long batch = v.batch;
    const long long b0 = pipeline_split_of(h, batch, v.m, v.n);
    int rc = b0 > 0 ? on_both_halves(h, batch, b0, [&](enlsip_gn_handle hh, long long k0, long long cnt) {
                          return factor_dev(hh, v.slice(k0, cnt), eps_rank);
                      })
                    : factor_dev(h, v, eps_rank);
    if (rc) return rc;
    auto& F = h->fb;
    F.host = host_form;
    F.batch = batch; F.m = v.m; F.n = v.n; F.t = v.t; F.split = b0;
    F.At = v.At; F.ldat = v.ldat; F.strideAt = v.strideAt; F.cx = v.cx;
    F.tk.assign(v.tk, v.tk + batch);
    F.valid = true;
    h->constraint_refactored = h->cstage_problems + (b0 > 0 ? h->child->cstage_problems : 0);
    return 0;
}

// Is the resident constraint stage the one an enlsip_gn_solve_factored_batched call with these arguments goes on with?  (The host form
// asks before it stages anything over the resident inputs.)
static int check_factored_call(enlsip_gn_handle h, const BatchOperands& v, const int64_t* refactor, bool host_form) {
    const long long batch = v.batch;
    const auto& F = h->fb;
    auto resident = [&](enlsip_gn_handle hh, long long cnt) {
        return hh && hh->factors_valid && hh->constraints_only && hh->have_plan && hh->plan.batch == cnt && hh->plan.m == v.m &&
               hh->plan.n == v.n && hh->plan.t == v.t;
    };
    bool ok = F.valid && F.host == host_form && F.batch == batch && F.m == v.m && F.n == v.n && F.t == v.t;
    if (ok) ok = F.split > 0 ? (resident(h, F.split) && resident(h->child, batch - F.split)) : resident(h, batch);
    if (!ok) {
        h->err = "enlsip_gn_solve_factored_batched needs enlsip_gn_factor_constraints_batched (same form, host or device) with the same "
                 "batch, m, n, t_max right before";
        return -1;
    }
    for (long long k = 0; k < batch; ++k)
        if (!(refactor && refactor[k]) && v.tk[k] != F.tk[(size_t)k]) {
            h->err = "t[" + std::to_string(k) + "] = " + std::to_string(v.tk[k]) + " but problem " + std::to_string(k) +
                     " was factored with " + std::to_string(F.tk[(size_t)k]) + " constraints and has no refactor flag";
            return -6;
        }
    return 0;
}

// Both forms of enlsip_gn_solve_factored_batched (v: device buffers) after check_factored_call: the solve over the same halves; each
// half runs the constraint stage again for its problems with a refactor flag.
static int solve_factored_core(enlsip_gn_handle h, const BatchOperands& v, const int64_t* refactor, double eps_rank, bool host_form) {
    auto& F = h->fb;
    if (!host_form && v.t > 0 && (v.At != F.At || v.ldat != F.ldat || v.strideAt != F.strideAt || v.cx != F.cx)) {
        h->err = "dAt, ldat, strideAt, dcx must be the buffers of the enlsip_gn_factor_constraints_batched_dev call (the slots of the "
                 "problems with a refactor flag rewritten in place)";
        return -11;
    }
    h->chunk0 = 0;
    const int rc = solve_launchable(h, v, {SolveMode::Factored, refactor, false, -1, -1, eps_rank});
    F.valid = false;
    if (rc) return rc;
    h->constraint_refactored = h->cstage_problems + (h->split > 0 ? h->child->cstage_problems : 0);
    return 0;
}

static int check_launch_batch(enlsip_gn_handle h, int64_t batch) {
    if (batch > GN_MAX_LAUNCH_BATCH) {
        h->err = "batch above the launch limit (" + std::to_string(GN_MAX_LAUNCH_BATCH) + "): only the last chunk's factors would "
                 "stay resident, so the constraint stage cannot be kept for a following solve";
        return -2;
    }
    return 0;
}

int enlsip_gn_factor_constraints_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                             const double* dAt, int64_t ldat, int64_t strideAt, const double* dcx, double eps_rank,
                                             enlsip_gn_info* dinfo) {
    if (!h) return -1;
    GN_TRY
    std::vector<int> tk;
    int rc = check_ragged(h, batch, m, n, t_max, t, nullptr, 0, nullptr, dAt, ldat, strideAt, dcx, tk, false, true, true);
    if (rc) return rc;
    rc = check_launch_batch(h, batch);
    if (rc) return rc;
    BatchOperands v{batch, m, n, t_max};
    v.At = dAt; v.ldat = ldat; v.strideAt = strideAt; v.cx = dcx; v.dinfo = dinfo; v.tk = tk.data();
    return factor_batched_core(h, v, eps_rank, false);
    GN_CATCH(h)
}

int enlsip_gn_factor_constraints_batched(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                         const double* At, int64_t ldat, int64_t strideAt, const double* cx, double eps_rank,
                                         enlsip_gn_info* info) {
    if (!h) return -1;
    GN_TRY
    std::vector<int> tk;
    int rc = check_ragged(h, batch, m, n, t_max, t, nullptr, 0, nullptr, At, ldat, strideAt, cx, tk, false, true, true);
    if (rc) return rc;
    rc = check_launch_batch(h, batch);
    if (rc) return rc;
    GN_HIP(hipSetDevice(h->device));
    StageIn in;       // solve_host's for this batch, whole: the solve that follows finds A', cx in their slots (and must not grow it)
    rc = place_dev(h, h->in_stage, in, (long long)batch, (long long)m, (long long)n, (long long)t_max);
    if (rc) return rc;
    double *dAt = in.At, *dcx = in.cx;
    hipStream_t s = h->stream;
    if (t_max > 0) {
        for (int64_t k = 0; k < batch; ++k)
            GN_HIP(hipMemcpy2DAsync(dAt + (size_t)k * n * t_max, (size_t)n * 8, At + (size_t)k * strideAt, (size_t)ldat * 8, (size_t)n * 8,
                                    (size_t)t_max, hipMemcpyHostToDevice, s));
        GN_HIP(hipMemcpyAsync(dcx, cx, (size_t)batch * t_max * 8, hipMemcpyHostToDevice, s));
    }
    BatchOperands v{batch, m, n, t_max};
    v.At = dAt; v.ldat = n; v.strideAt = n * t_max; v.cx = dcx; v.hinfo = info; v.tk = tk.data();
    return factor_batched_core(h, v, eps_rank, true);
    GN_CATCH(h)
}

int enlsip_gn_solve_factored_batched(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                     const int64_t* refactor, const double* J, int64_t ldj, int64_t strideJ, const double* rx,
                                     const double* At, int64_t ldat, int64_t strideAt, const double* cx, double eps_rank, double* p,
                                     double* b, double* d, enlsip_gn_info* info, int64_t* jpvtA, int64_t* jpvtL, int64_t* jpvtJ2) {
    if (!h) return -1;
    GN_TRY
    std::vector<int> tk;
    int rc = check_ragged(h, batch, m, n, t_max, t, J, ldj, rx, At, ldat, strideAt, cx, tk, true, any_flag(refactor, batch), true);
    if (rc) return rc;
    rc = check_launch_batch(h, batch);
    if (rc) return rc;
    BatchOperands shape{batch, m, n, t_max};
    shape.tk = tk.data();
    rc = check_factored_call(h, shape, refactor, true);
    if (rc) return rc;
    return solve_host(h, {batch, m, n, t_max, J, ldj, strideJ, rx, At, ldat, strideAt, cx, p, b, d, nullptr, (long long*)jpvtA,
                          (long long*)jpvtL, (long long*)jpvtJ2, info, tk.data()}, {SolveMode::Factored, refactor, false, -1, -1, eps_rank});
    GN_CATCH(h)
}

int enlsip_gn_solve_factored_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                         const int64_t* refactor, const double* dJ, int64_t ldj, int64_t strideJ, const double* drx,
                                         const double* dAt, int64_t ldat, int64_t strideAt, const double* dcx, double eps_rank,
                                         double* dp, double* db, double* dd, enlsip_gn_info* dinfo, int64_t* djpvtA, int64_t* djpvtL,
                                         int64_t* djpvtJ2) {
    if (!h) return -1;
    GN_TRY
    std::vector<int> tk;
    int rc = check_ragged(h, batch, m, n, t_max, t, dJ, ldj, drx, dAt, ldat, strideAt, dcx, tk, true, any_flag(refactor, batch), true);
    if (rc) return rc;
    rc = check_launch_batch(h, batch);
    if (rc) return rc;
    BatchOperands shape{batch, m, n, t_max};
    shape.tk = tk.data();
    rc = check_factored_call(h, shape, refactor, false);
    if (rc) return rc;
    return solve_factored_core(h, {batch, m, n, t_max, dJ, ldj, strideJ, drx, dAt, ldat, strideAt, dcx, dp, db, dd, dinfo,
                                   (long long*)djpvtA, (long long*)djpvtL, (long long*)djpvtJ2, nullptr, tk.data()},
                               refactor, eps_rank, false);
    GN_CATCH(h)
}

// ---- changed-problems solve: update_working_set (src/enlsip_functions.jl:686-795) solves the subproblem again after the undo of a
// deletion (:728-743) and after a second-order deletion (:745-762 / :773-790), each time for the problems whose working set changed
// only; the direction itself is gn_search_direction's (:725 / :771).  See include/enlsip_gn.h. ---------------------------------------

// What the resident batch must be for enlsip_gn_solve_changed_batched*: a fully solved ragged batch of this shape, split as it would
// be split now.  Nothing is staged or launched before this has passed.
static int check_changed_call(enlsip_gn_handle h, long long batch, long long m, long long n, long long t_max, const std::vector<int>& tk,
                              const int64_t* changed) {
    const enlsip_gn_handle c = h->split > 0 ? h->child : nullptr;
    auto solved = [&](enlsip_gn_handle hh) { return hh && hh->factors_valid && hh->have_plan; };
    if (!solved(h) || (c && !solved(c))) {
        h->err = "enlsip_gn_solve_changed_batched needs a fully solved batch resident on the handle (nothing is, or the last solve was "
                 "a TSQR solve, which leaves no whole problem resident)";
        return -1;
    }
    if (h->constraints_only || (c && c->constraints_only)) { h->err = "enlsip_gn_solve_changed_batched: only F_A / F_L11 are resident (enlsip_gn_factor_constraints*): solve first";
        return -1;
    }
    if (h->h_tk.empty() || (c && c->h_tk.empty())) {
        h->err = "enlsip_gn_solve_changed_batched: the resident batch is a uniform one (enlsip_gn_solve_batched): it has no per-problem t";
        return -1;
    }
    const long long total = h->plan.batch + (c ? c->plan.batch : 0);
    if (h->chunk0 != 0 || total != batch || h->plan.m != m || h->plan.n != n || h->plan.t != t_max) {
        h->err = "enlsip_gn_solve_changed_batched: batch, m, n, t_max must be those of the resident solve";
        return -1;
    }
    if (pipeline_split_of(h, batch, m, n) != h->split) {
        h->err = "enlsip_gn_solve_changed_batched: the batch would now be split over the pipeline halves differently from the resident "
                 "solve (profiling or the pipeline setting changed in between?)";
        return -1;
    }
    for (long long k = 0; k < batch; ++k) {
        const int have = (c && k >= h->split) ? c->h_tk[(size_t)(k - h->split)] : h->h_tk[(size_t)k];
        if (!changed[k] && tk[(size_t)k] != have) {
            h->err = "t[" + std::to_string(k) + "] = " + std::to_string(tk[(size_t)k]) + " but problem " + std::to_string(k) +
                     " is resident with " + std::to_string(have) + " constraints and has no changed flag";
            return -6;
        }
    }
    return 0;
}

// Both forms after their checks (and the host form's staging).  v: device buffers; J, rx the resident ones.
static int solve_changed_core(enlsip_gn_handle h, const BatchOperands& v, const int64_t* changed, double eps_rank) {
    const long long batch = v.batch;
    const long long split = h->split;
    const enlsip_gn_handle c = split > 0 ? h->child : nullptr;
    const long long b0 = c ? split : batch;
    const SolveMode mode{SolveMode::Changed, changed, false, -1, -1, eps_rank};
    h->fb.valid = false;
    const bool part0 = any_flag(changed, b0), part1 = c && any_flag(changed + b0, batch - b0);     // the halves that run
    if (!part0) h->cstage_problems = h->jstage_problems = 0;
    if (c && !part1) c->cstage_problems = c->jstage_problems = 0;
    int rc = 0;
    if (part0 && part1) {
        rc = on_both_halves(h, batch, b0, [&](enlsip_gn_handle hh, long long k0, long long cnt) {
            return solve_dev(hh, v.slice(k0, cnt), mode.part(k0));
        });
    } else if (part0) {
        rc = solve_dev(h, v.slice(0, b0), mode);
        if (!rc && c) h->route |= (1ull << ENLSIP_GN_ROUTE_PIPELINE_SPLIT);
    } else if (part1) {
        GN_HIP(hipSetDevice(h->device));
        rc = fork_after(h, c->stream);
        if (rc) return rc;
        rc = solve_dev(c, v.slice(b0, batch - b0), mode.part(b0));
        if (rc) h->err = c->err;
        else h->route = c->route | (1ull << ENLSIP_GN_ROUTE_PIPELINE_SPLIT);
        GN_HIP(hipSetDevice(h->device));
    }
    h->split = split;
    if (rc) return rc;
    h->constraint_refactored = h->cstage_problems + (c ? c->cstage_problems : 0);
    return 0;
}

// argument checks shared by the two forms; tk: the checked t
static int check_changed_args(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t, const int64_t* changed,
                              const double* At, int64_t ldat, int64_t strideAt, const double* cx, std::vector<int>& tk, bool* any) {
    int rc = check_ragged(h, batch, m, n, t_max, t, nullptr, 0, nullptr, nullptr, 0, 0, nullptr, tk, false, false, false);
    if (rc) return rc;
    rc = check_launch_batch(h, batch);
    if (rc) return rc;
    if (!changed) { h->err = "changed is NULL"; return -7; }
    rc = check_changed_call(h, batch, m, n, t_max, tk, changed);
    if (rc) return rc;
    bool flagged = false, constrained = false;
    for (int64_t k = 0; k < batch; ++k)
        if (changed[k]) { flagged = true; constrained = constrained || t[k] > 0; }
    *any = flagged;
    if (constrained) {
        if (!At) { h->err = "At is NULL while a changed problem has t[k] > 0"; return -8; }
        if (ldat < n) { h->err = "ldat < n"; return -9; }
        if (strideAt < ldat * t_max) { h->err = "strideAt < ldat * t_max"; return -10; }
        if (!cx) { h->err = "cx is NULL while a changed problem has t[k] > 0"; return -11; }
    }
    return 0;
}

// a call without a flag: nothing launched, nothing written
static int nothing_changed(enlsip_gn_handle h) {
    h->cstage_problems = h->jstage_problems = 0;
    if (h->split > 0) h->child->cstage_problems = h->child->jstage_problems = 0;
    h->constraint_refactored = 0;
    return 0;
}

int enlsip_gn_solve_changed_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                        const int64_t* changed, const double* dAt, int64_t ldat, int64_t strideAt, const double* dcx,
                                        double eps_rank, double* dp, double* db, double* dd, enlsip_gn_info* dinfo, int64_t* djpvtA,
                                        int64_t* djpvtL, int64_t* djpvtJ2) {
    if (!h) return -1;
    GN_TRY
    std::vector<int> tk;
    bool any = false;
    int rc = check_changed_args(h, batch, m, n, t_max, t, changed, dAt, ldat, strideAt, dcx, tk, &any);
    if (rc) return rc;
    const BatchOperands& L = h->last;
    if (t_max > 0 && (dAt != L.At || ldat != L.ldat || strideAt != L.strideAt || dcx != L.cx)) {
        h->err = "dAt, ldat, strideAt, dcx must be the buffers the resident solve was made with (the slots of the changed problems "
                 "rewritten in place)";
        return -8;
    }
    if (!any) return nothing_changed(h);
    return solve_changed_core(h, {batch, m, n, t_max, L.J, L.ldj, L.strideJ, L.rx, L.At, L.ldat, L.strideAt, L.cx, dp, db, dd, dinfo,
                                  (long long*)djpvtA, (long long*)djpvtL, (long long*)djpvtJ2, nullptr, tk.data()}, changed, eps_rank);
    GN_CATCH(h)
}

int enlsip_gn_solve_changed_batched(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                    const int64_t* changed, const double* At, int64_t ldat, int64_t strideAt, const double* cx,
                                    double eps_rank, double* p, double* b, double* d, enlsip_gn_info* info, int64_t* jpvtA, int64_t* jpvtL,
                                    int64_t* jpvtJ2) {
    if (!h) return -1;
    GN_TRY
    std::vector<int> tk;
    bool any = false;
    int rc = check_changed_args(h, batch, m, n, t_max, t, changed, At, ldat, strideAt, cx, tk, &any);
    if (rc) return rc;
    const BatchOperands L = h->last;
    if (!h->in_stage.p || L.J != (const double*)h->in_stage.p) {
        h->err = "enlsip_gn_solve_changed_batched: the resident solve was made from device buffers: use enlsip_gn_solve_changed_batched_dev";
        return -1;
    }
    if (!any) return nothing_changed(h);
    GN_HIP(hipSetDevice(h->device));
    const int kA = (int)std::min(n, t_max);
    StageOut out;     // packed as solve_host packs them (the resident solve reads nothing of this buffer)
    rc = place_dev(h, h->out_stage, out, (long long)batch, (long long)m, (long long)n, (long long)t_max);
    if (rc) return rc;
    double *dp = out.p, *db = out.b, *dd = out.d;
    long long *djA = out.jA, *djL = out.jL, *djJ = out.jJ;
    hipStream_t s = h->stream;
    // the changed problems' A', cx into the slots of the staging area the resident solve reads
    double* sAt = const_cast<double*>(L.At);
    double* scx = const_cast<double*>(L.cx);
    for (int64_t k = 0; k < batch && t_max > 0; ++k) {
        if (!changed[k] || t[k] <= 0) continue;
        GN_HIP(hipMemcpy2DAsync(sAt + (size_t)k * L.strideAt, (size_t)L.ldat * 8, At + (size_t)k * strideAt, (size_t)ldat * 8, (size_t)n * 8,
                                (size_t)t_max, hipMemcpyHostToDevice, s));
        GN_HIP(hipMemcpyAsync(scx + (size_t)k * t_max, cx + (size_t)k * t_max, (size_t)t_max * 8, hipMemcpyHostToDevice, s));
    }
    rc = solve_changed_core(h, {batch, m, n, t_max, L.J, L.ldj, L.strideJ, L.rx, L.At, L.ldat, L.strideAt, L.cx, dp, db, dd, nullptr, djA, djL,
                                djJ, info, tk.data()}, changed, eps_rank);
    if (rc) return rc;
    for (int64_t k = 0; k < batch; ++k) {
        if (!changed[k]) continue;
        if (p) GN_HIP(hipMemcpyAsync(p + (size_t)k * n, dp + (size_t)k * n, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        if (b && t_max > 0) GN_HIP(hipMemcpyAsync(b + (size_t)k * t_max, db + (size_t)k * t_max, (size_t)t_max * 8, hipMemcpyDeviceToHost, s));
        if (d) GN_HIP(hipMemcpyAsync(d + (size_t)k * m, dd + (size_t)k * m, (size_t)m * 8, hipMemcpyDeviceToHost, s));
        if (jpvtA && t_max > 0) GN_HIP(hipMemcpyAsync(jpvtA + (size_t)k * t_max, djA + (size_t)k * t_max, (size_t)t_max * 8, hipMemcpyDeviceToHost, s));
        if (jpvtL && kA > 0) GN_HIP(hipMemcpyAsync(jpvtL + (size_t)k * kA, djL + (size_t)k * kA, (size_t)kA * 8, hipMemcpyDeviceToHost, s));
        if (jpvtJ2) GN_HIP(hipMemcpyAsync(jpvtJ2 + (size_t)k * n, djJ + (size_t)k * n, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    }
    GN_HIP(hipStreamSynchronize(s));
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_get_jacobian_resolved(enlsip_gn_handle h, int64_t* count) {
    if (!h) return -1;
    if (!count) return -2;
    *count = (int64_t)(h->jstage_problems + (h->split > 0 && h->child ? h->child->jstage_problems : 0));
    return 0;
}

int enlsip_gn_get_constraint_refactored(enlsip_gn_handle h, int64_t* count) {
    if (!h) return -1;
    if (!count) return -2;
    *count = (int64_t)h->constraint_refactored;
    return 0;
}

int enlsip_gn_solve(enlsip_gn_handle h, int64_t m, int64_t n, int64_t t, const double* J, int64_t ldj,
                    const double* rx, const double* At, int64_t ldat, const double* cx, double eps_rank,
                    int64_t dimA_override, int64_t dimJ2_override, double* p, double* b, double* d,
                    enlsip_gn_info* info, int64_t* jpvtA, int64_t* jpvtL, int64_t* jpvtJ2) {
    return solve_host(h, {1, m, n, t, J, ldj, ldj * n, rx, At, ldat, ldat * t, cx, p, b, d, nullptr, (long long*)jpvtA,
                          (long long*)jpvtL, (long long*)jpvtJ2, info}, {SolveMode::Fresh, nullptr, false, dimA_override, dimJ2_override, eps_rank});
}

}  // extern "C"

#include "gn_accessors.inc"
#include "gn_tsqr.inc"
#include "gn_lagrange.inc"
#include "gn_tsqr_products.inc"
#include "gn_lagrange_batched.inc"
#include "gn_resolve_batched.inc"
#include "gn_subspace_batched.inc"
#include "gn_deletion_batched.inc"
#include "gn_linesearch_batched.inc"
#include "gn_penalty_batched.inc"
#include "gn_linesearch_fit_batched.inc"
#include "gn_addition_batched.inc"
#include "gn_termination_batched.inc"
#include "gn_direction_batched.inc"
#include "gn_hessian_batched.inc"
#include "gn_newton.inc"
#include "gn_newton_batched.inc"
#include "gn_tsqr_newton.inc"
