// Row-sharded TSQR (config C4): local stage -> ONE exchange step -> combine stage.
//   enlsip_gn_solve_tsqr            the whole collective inside the library: the exchange is one all-gather of
//                                   [packed upper triangle | z | tail^2] per rank over RCCL (loaded at run time, so that the
//                                   library itself has no link-time dependency on it) or over a caller-supplied transport
//   enlsip_gn_tsqr_local_dev / _combine_dev   the two stages alone, exchange by the caller (INTEGRATION.md section 5)
// Included by enlsip_gn.hip.
#include <dlfcn.h>

namespace gn {

struct gn_nccl_id { char internal[128]; };      // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128), passed by value

// Rloc (packed n2 x n2, upper) and zloc from the CAQR result in W; partial sum of squares of the tail of d
__global__ void k_tsqr_extract(const double* W, int ldw, int n, int m, const ProbState* st, double* Rloc,
                               double* zloc, double* tail_sq) {
    const int rankA = st->rankA, n2 = st->n2, kp = st->kp;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * blockDim.x;
    for (long long e = tid; e < (long long)n2 * n2; e += nthreads) {
        const int i = (int)(e % n2), c = (int)(e / n2);
        Rloc[e] = (i <= c && i < kp) ? W[i + (size_t)(rankA + c) * ldw] : 0.0;
    }
    for (long long i = tid; i < n2; i += nthreads) zloc[i] = (i < kp) ? W[i + (size_t)n * ldw] : 0.0;
    double s = 0.0;
    for (long long i = kp + tid; i < m; i += nthreads) {
        const double x = W[i + (size_t)n * ldw];
        s += x * x;
    }
    s = wave_allsum(s);
    if ((threadIdx.x & 63) == 0 && s != 0.0) atomicAdd(tail_sq, s);
}

// stack G packed n2 x n2 blocks on top of each other: Jst is (G n2) x n2 with ld = G n2; rx = -zstack
__global__ void k_tsqr_stack(const double* Rstack, const double* zstack, int G, int n2, double* Jst, double* rxs) {
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * blockDim.x;
    const long long ld = (long long)G * n2;
    for (long long e = tid; e < (long long)G * n2 * n2; e += nthreads) {
        const int i = (int)(e % n2);
        const long long rest = e / n2;
        const int c = (int)(rest % n2), g = (int)(rest / n2);
        Jst[(long long)g * n2 + i + (long long)c * ld] = (i <= c) ? Rstack[e] : 0.0;   // only the upper triangles are the caller's to fill
    }
    for (long long i = tid; i < ld; i += nthreads) rxs[i] = -zstack[i];
}

// p = F_A.Q * [p1[0:rankA] ; p2]     (src/enlsip_functions.jl:151), one wave
__global__ __launch_bounds__(64) void k_tsqr_q1(const double* FA, int n, const double* tauA, int kA, const double* p1,
                                                const ProbState* st, const double* p2, double* pout) {
    const int rankA = st->rankA, n2 = st->n2;
    for (int i = threadIdx.x; i < n; i += 64) pout[i] = (i < rankA) ? p1[i] : ((i - rankA) < n2 ? p2[i - rankA] : 0.0);
    __syncthreads();
    wave_apply_reflectors<false>(FA, n, tauA, kA, n, pout);
}

// message of one rank, msg_len doubles (sized from n, the same on every rank whatever its n2):
//   [0] n2 of the sender (checked against the receiver's after the gather)   [1] tail^2 (zeroed by the caller, accumulated here)
//   [2] rank of the sender + 1, [3] the rank count the sender believes in: after the gather slot g must carry tag g + 1 — the
//       count of slots that do is what "did the collective see N ranks" can be answered from (enlsip_gn_tsqr_get_exchange)
//   [4 ...] packed upper triangle (column c at offset c (c + 1) / 2, c + 1 entries), then z (n2)
constexpr int TSQR_HDR = 4;
__global__ void k_tsqr_pack(const double* W, int ldw, int n, int m, const ProbState* st, double* msg, int rank, int ranks) {
    const int rankA = st->rankA, n2 = st->n2, kp = st->kp;
    const long long tri = (long long)n2 * (n2 + 1) / 2;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * blockDim.x;
    if (tid == 0) {
        msg[0] = (double)n2;
        msg[2] = (double)(rank + 1);
        msg[3] = (double)ranks;
    }
    double* body = msg + TSQR_HDR;
    for (int c = blockIdx.x; c < n2; c += gridDim.x) {
        double* dst = body + (long long)c * (c + 1) / 2;
        for (int i = threadIdx.x; i <= c; i += blockDim.x) dst[i] = (i < kp) ? W[i + (size_t)(rankA + c) * ldw] : 0.0;
    }
    for (long long i = tid; i < n2; i += nthreads) body[tri + i] = (i < kp) ? W[i + (size_t)n * ldw] : 0.0;
    double s = 0.0;
    for (long long i = kp + tid; i < m; i += nthreads) {
        const double x = W[i + (size_t)n * ldw];
        s += x * x;
    }
    s = wave_allsum(s);
    if ((threadIdx.x & 63) == 0 && s != 0.0) atomicAdd(msg + 1, s);
}

// G gathered messages -> the stacked problem: Jst is (G n2) x n2 with ld = G n2 (block g = triangle of rank g, zeros below),
// rxs = -[z_0; z_1; ...]; tails[0] = sum of the ranks' tail^2, tails[1] = number of ranks whose n2 differs from this rank's
// (their triangles would be read with the wrong layout: the caller turns that into an error)
__global__ void k_tsqr_unpack(const double* msgs, long long msg_len, int G, int n2, double* Jst, double* rxs, double* tails) {
    const long long ld = (long long)G * n2;
    const long long tri = (long long)n2 * (n2 + 1) / 2;
    for (long long cg = blockIdx.x; cg < (long long)G * n2; cg += gridDim.x) {
        const int g = (int)(cg / n2), c = (int)(cg % n2);
        const double* src = msgs + g * msg_len + TSQR_HDR + (long long)c * (c + 1) / 2;
        double* dst = Jst + (long long)g * n2 + (long long)c * ld;
        for (int i = threadIdx.x; i < n2; i += blockDim.x) dst[i] = (i <= c) ? src[i] : 0.0;
    }
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * blockDim.x;
    for (long long i = tid; i < ld; i += nthreads) rxs[i] = -msgs[(i / n2) * msg_len + TSQR_HDR + tri + (i % n2)];
    if (tid == 0) {
        double s = 0.0, bad = 0.0, tagged = 0.0;
        for (int g = 0; g < G; ++g) {
            s += msgs[g * msg_len + 1];
            if (msgs[g * msg_len] != (double)n2) bad += 1.0;
            if (msgs[g * msg_len + 2] == (double)(g + 1) && msgs[g * msg_len + 3] == (double)G) tagged += 1.0;
        }
        tails[0] = s;
        tails[1] = bad;
        tails[2] = tagged;       // slots whose message came from the rank the slot belongs to
    }
}

__global__ void k_sumsq(const double* x, long long lo, long long hi, double* out) {
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * blockDim.x;
    double s = 0.0;
    for (long long i = lo + tid; i < hi; i += nthreads) s += x[i] * x[i];
    s = wave_allsum(s);
    if ((threadIdx.x & 63) == 0 && s != 0.0) atomicAdd(out, s);
}

}  // namespace gn


// ---- RCCL, bound at run time -------------------------------------------------------------------------------------------------
namespace {
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, gn::gn_nccl_id, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string why;
};
static void rccl_bind(RcclApi& api);
RcclApi& rccl() {            // bound once, also when two handles initialise from two threads (C++11 static initialisation)
    static RcclApi api = [] { RcclApi a; rccl_bind(a); return a; }();
    return api;
}
static void rccl_bind(RcclApi& api) {
    const char* env = getenv("ENLSIP_GN_RCCL_LIB");
    const char* names[] = {env, "librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
    for (const char* nm : names) {
        if (!nm || !*nm) continue;
        api.lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
        if (api.lib) break;
        api.why = dlerror();
    }
    if (!api.lib) return;
    api.GetUniqueId = (int (*)(void*))dlsym(api.lib, "ncclGetUniqueId");
    api.CommInitRank = (int (*)(void**, int, gn::gn_nccl_id, int))dlsym(api.lib, "ncclCommInitRank");
    api.CommDestroy = (int (*)(void*))dlsym(api.lib, "ncclCommDestroy");
    api.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(api.lib, "ncclAllGather");
    api.GetErrorString = (const char* (*)(int))dlsym(api.lib, "ncclGetErrorString");
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllGather) {
        api.why = "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllGather";
        dlclose(api.lib);
        api.lib = nullptr;
    }
}
constexpr int GN_NCCL_FLOAT64 = 8;      // ncclFloat64 / ncclDouble (rccl.h: ncclDataType_t)

// the local stage up to the CAQR of [J2 | d_temp]; the factored W stays resident
int tsqr_local_core(enlsip_gn_handle h, int64_t m_loc, int64_t n, int64_t t, const double* dJ, int64_t ldj,
                    const double* drx, const double* dAt, int64_t ldat, const double* dcx, double eps_rank) {
    int rc = check_limits(h, 1, m_loc, n, t);
    if (rc) return rc;
    if (!dJ) { h->err = "dJ is NULL"; return -5; }
    if (ldj < m_loc) { h->err = "ldj < m_loc"; return -6; }
    if (!drx) { h->err = "drx is NULL"; return -7; }
    if (t > 0 && (!dAt || !dcx)) { h->err = "dAt / dcx is NULL with t > 0"; return -8; }
    if (t > 0 && ldat < n) { h->err = "ldat < n"; return -9; }
    GN_HIP(hipSetDevice(h->device));
    h->split = 0;
    h->chunk0 = 0;
    rc = make_plan(h, 1, m_loc, n, t);
    if (rc) return rc;
    const Plan& P = h->plan;
    hipStream_t s = h->stream;
    h->eps_rank = eps_rank;
    h->factors_valid = false;
    h->held.clear();
    h->last = {1, m_loc, n, t, dJ, ldj, 0, drx, dAt, ldat, 0, dcx};
    // same routing as a solve (register / distributed forms of F_A for the shapes that need them)
    h->sc_eJ = 0; h->sc_eA = 0;          // row shards are not rescaled (include/enlsip_gn.h: magnitude range of the TSQR entry points)
    h->rescue_prob.clear();
    h->h_tk.clear();
    rc = run_constraint_stage(h, 1, m_loc, n, t, dAt, ldat, 0, dcx, eps_rank, -1);
    if (rc) return rc;
    int n2_launch = (int)(n - P.kA);
    for (int attempt = 0; attempt < 2; ++attempt) {
        launch_jq1_any(h, jq1_args(h, dJ, ldj, 0, drx), 1, s);
        rc = run_caqr(h, n2_launch);
        if (rc) return rc;
        GN_HIP(hipMemcpyAsync(h->h_state, h->state, sizeof(ProbState), hipMemcpyDeviceToHost, s));
        GN_HIP(hipStreamSynchronize(s));
        if (h->h_state[0].n2 <= n2_launch) break;
        n2_launch = h->h_state[0].n2;
    }
    h->tsqr_n2 = h->h_state[0].n2;
    return 0;
}

// the stacked problem (Jst (G n2) x n2, rxs) is in place in h->scratch: factor, solve, p = Q1 [p1; p2]
int tsqr_combine_core(enlsip_gn_handle h, int64_t G, int64_t n2, double eps_rank, double* p, double* dlead,
                      double* comb_tail_sq, enlsip_gn_info* info, int64_t* jpvtJ2) {
    const Plan& P = h->plan;      // plan of the local stage: F_A, p1, state are resident
    hipStream_t s = h->stream;
    const long long n = P.n, ms = (long long)G * n2;
    const ProbState st = h->h_state[0];
    double* Jst = (double*)h->scratch.p;
    double* rxs = Jst + (size_t)ms * n2;
    double* dp2 = rxs + ms;
    double* dd = dp2 + n2;
    double* dpo = dd + ms;
    enlsip_gn_info sinfo = {0, 0, 1, 0, 0, 0};
    int rc;
    if (n2 > 0) {
        if (!h->sub) {
            rc = create_helper(h, &h->sub, h->stream);
            if (rc) { h->err = "tsqr_combine: cannot create the sub-handle"; return rc; }
        }
        // jpvt / info of the stacked (unconstrained) problem through the ordinary device-pointer solve
        rc = grow(h, h->out_stage, ((size_t)n2 * 8 + sizeof(enlsip_gn_info)) + 1024);
        if (rc) return rc;
        long long* djJ = (long long*)h->out_stage.p;
        const BatchOperands v{1, ms, n2, 0, Jst, ms, 0, rxs, nullptr, 1, 0, nullptr, dp2, nullptr, dd, nullptr, nullptr, nullptr, djJ};
        rc = solve_dev(h->sub, v, {SolveMode::Fresh, nullptr, G == 1, -1, -1, eps_rank});      // one rank: the stacked matrix is that rank's triangle
        if (rc) { h->err = std::string("tsqr_combine/sub: ") + h->sub->err; return rc; }
        sinfo = info_of(h->sub->h_state[0]);       // its rankJ2, dimJ2 and status
        if (jpvtJ2) GN_HIP(hipMemcpyAsync(jpvtJ2, djJ, (size_t)n2 * 8, hipMemcpyDeviceToHost, s));
        if (dlead) GN_HIP(hipMemcpyAsync(dlead, dd, (size_t)n2 * 8, hipMemcpyDeviceToHost, s));
        GN_HIP(hipMemsetAsync(h->small + 8, 0, 8, s));
        if (ms > n2) hipLaunchKernelGGL(k_sumsq, dim3(64), dim3(256), 0, s, dd, (long long)n2, ms, (double*)(h->small + 8));
        if (comb_tail_sq) GN_HIP(hipMemcpyAsync(comb_tail_sq, h->small + 8, 8, hipMemcpyDeviceToHost, s));
    } else if (comb_tail_sq) {
        *comb_tail_sq = 0.0;
    }
    hipLaunchKernelGGL(k_tsqr_q1, dim3(1), dim3(64), 0, s, h->FA, (int)n, h->tauA, P.kA, h->p1, h->state, dp2, dpo);
    GN_HIP(hipGetLastError());
    if (p) GN_HIP(hipMemcpyAsync(p, dpo, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    if (info) *info = {st.rankA, sinfo.rankJ2, st.code, st.dimA, sinfo.dimJ2, (int64_t)(st.status | sinfo.status)};
    return 0;
}

int tsqr_scratch(enlsip_gn_handle h, int64_t G, int64_t n2) {
    const size_t ms = (size_t)G * n2;
    // Jst (ms x n2) | rxs (ms) | p2 (n2) | d (ms) | pout (n)
    return grow(h, h->scratch, (ms * n2 + 2 * ms + (size_t)n2 + (size_t)h->plan.n + 64) * 8);
}
}  // namespace

extern "C" {

int enlsip_gn_tsqr_local_dev(enlsip_gn_handle h, int64_t m_loc, int64_t n, int64_t t, const double* dJ, int64_t ldj,
                             const double* drx, const double* dAt, int64_t ldat, const double* dcx, double eps_rank,
                             double* dRloc, double* dzloc, double* tail_sq, int64_t* n2_out) {
    if (!h) return -1;
    GN_TRY
    if (!dRloc || !dzloc) { h->err = "dRloc / dzloc is NULL"; return -12; }
    int rc = tsqr_local_core(h, m_loc, n, t, dJ, ldj, drx, dAt, ldat, dcx, eps_rank);
    if (rc) return rc;
    const Plan& P = h->plan;
    hipStream_t s = h->stream;
    GN_HIP(hipMemsetAsync(h->small + 8, 0, 8, s));     // scratch double for the tail sum
    double* dsum = (double*)(h->small + 8);
    hipLaunchKernelGGL(k_tsqr_extract, dim3(256), dim3(256), 0, s, h->W, P.ldw, (int)n, (int)m_loc, h->state, dRloc,
                       dzloc, dsum);
    GN_HIP(hipGetLastError());
    double ts = 0.0;
    GN_HIP(hipMemcpyAsync(&ts, dsum, 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    if (tail_sq) *tail_sq = ts;
    if (n2_out) *n2_out = h->tsqr_n2;
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_tsqr_combine_dev(enlsip_gn_handle h, int64_t G, int64_t n2, const double* dRstack, const double* dzstack,
                               double eps_rank, double* p, double* dlead, double* comb_tail_sq, enlsip_gn_info* info,
                               int64_t* jpvtJ2) {
    if (!h) return -1;
    GN_TRY
    if (G < 1) { h->err = "G < 1"; return -2; }
    if (h->tsqr_n2 < 0 || n2 != h->tsqr_n2) { h->err = "tsqr_combine: n2 does not match the last tsqr_local on this handle"; return -3; }
    if (n2 > 0 && (!dRstack || !dzstack)) { h->err = "dRstack / dzstack is NULL"; return -4; }
    GN_HIP(hipSetDevice(h->device));
    int rc = tsqr_scratch(h, G, n2);
    if (rc) return rc;
    if (n2 > 0) {
        double* Jst = (double*)h->scratch.p;
        hipLaunchKernelGGL(k_tsqr_stack, dim3(512), dim3(256), 0, h->stream, dRstack, dzstack, (int)G, (int)n2, Jst,
                           Jst + (size_t)G * n2 * n2);
        GN_HIP(hipGetLastError());
    }
    return tsqr_combine_core(h, G, n2, eps_rank, p, dlead, comb_tail_sq, info, jpvtJ2);
    GN_CATCH(h)
}

// ---- the communicator behind enlsip_gn_solve_tsqr --------------------------------------------------------------------------------
int enlsip_gn_tsqr_unique_id(void* id128) {
    if (!id128) return -1;
    RcclApi& r = rccl();
    if (!r.lib) return 996;
    return r.GetUniqueId(id128) == 0 ? 0 : 995;
}

static void tsqr_drop_comm(enlsip_gn_handle h) {
    if (h->tsqr_comm && h->tsqr_comm_owned && rccl().lib) (void)rccl().CommDestroy(h->tsqr_comm);
    h->tsqr_comm = nullptr;
    h->tsqr_comm_owned = false;
    h->tsqr_xfn = nullptr;
    h->tsqr_xctx = nullptr;
    h->tsqr_ranks = 1;
    h->tsqr_rank = 0;
    h->tsqr_broken = false;
}

int enlsip_gn_tsqr_init_rccl(enlsip_gn_handle h, const void* id128, int nranks, int rank) {
    if (!h) return -1;
    GN_TRY
    if (!id128) { h->err = "unique id is NULL"; return -2; }
    if (nranks < 1) { h->err = "nranks < 1"; return -3; }
    if (rank < 0 || rank >= nranks) { h->err = "rank out of range"; return -4; }
    RcclApi& r = rccl();
    if (!r.lib) { h->err = "RCCL could not be loaded (" + r.why + "); set ENLSIP_GN_RCCL_LIB or use enlsip_gn_tsqr_set_exchange"; return 996; }
    GN_HIP(hipSetDevice(h->device));
    tsqr_drop_comm(h);
    gn::gn_nccl_id id;
    memcpy(&id, id128, sizeof id);
    void* comm = nullptr;
    const int e = r.CommInitRank(&comm, nranks, id, rank);
    if (e != 0) {
        // the handle is left WITHOUT a communicator and says so: a later enlsip_gn_solve_tsqr must not quietly solve the local shard alone
        h->tsqr_broken = true;
        h->err = std::string("ncclCommInitRank: ") + (r.GetErrorString ? r.GetErrorString(e) : "error");
        return 995;
    }
    h->tsqr_comm = comm;
    h->tsqr_comm_owned = true;
    h->tsqr_ranks = nranks;
    h->tsqr_rank = rank;
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_tsqr_set_comm(enlsip_gn_handle h, void* nccl_comm, int nranks, int rank) {
    if (!h) return -1;
    GN_TRY
    if (nranks < 1) { h->err = "nranks < 1"; return -3; }
    if (rank < 0 || rank >= nranks) { h->err = "rank out of range"; return -4; }
    tsqr_drop_comm(h);
    if (nccl_comm) {
        RcclApi& r = rccl();
        if (!r.lib) { h->err = "RCCL could not be loaded (" + r.why + ")"; return 996; }
        h->tsqr_comm = nccl_comm;
        h->tsqr_ranks = nranks;
        h->tsqr_rank = rank;
    }
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_tsqr_set_exchange(enlsip_gn_handle h, enlsip_gn_allgather_fn fn, void* ctx, int nranks, int rank) {
    if (!h) return -1;
    GN_TRY
    if (nranks < 1) { h->err = "nranks < 1"; return -4; }
    if (rank < 0 || rank >= nranks) { h->err = "rank out of range"; return -5; }
    tsqr_drop_comm(h);
    h->tsqr_xfn = fn;
    h->tsqr_xctx = ctx;
    h->tsqr_ranks = fn ? nranks : 1;
    h->tsqr_rank = fn ? rank : 0;
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_solve_tsqr(enlsip_gn_handle h, int64_t m_loc, int64_t n, int64_t t, const double* dJ, int64_t ldj,
                         const double* drx, const double* dAt, int64_t ldat, const double* dcx, double eps_rank,
                         double* p, double* dlead, double* d_norm, enlsip_gn_info* info, int64_t* jpvtJ2) {
    if (!h) return -1;
    GN_TRY
    const int G = h->tsqr_ranks;
    if (h->tsqr_broken) { h->err = "the communicator of this handle could not be created (enlsip_gn_tsqr_init_rccl failed): set one again first"; return -1; }
    if (G > 1 && !h->tsqr_comm && !h->tsqr_xfn) { h->err = "no communicator: call enlsip_gn_tsqr_init_rccl / _set_comm / _set_exchange first"; return -1; }
    // A failure of ONE rank before the exchange (arguments, memory, a HIP error in its local stage) is fatal for the
    // communicator: its peers wait in the all-gather.  The message length depends on n alone, so the ranks' counts always agree.
    hipEvent_t* ev = nullptr;
    if (h->profiling) {
        if (!h->ev_ready) {
            for (int i = 0; i < 8; ++i) GN_HIP(hipEventCreate(&h->ev[i]));
            h->ev_ready = true;
        }
        ev = h->ev;
        GN_HIP(hipEventRecord(ev[5], h->stream));
    }
    int rc = tsqr_local_core(h, m_loc, n, t, dJ, ldj, drx, dAt, ldat, dcx, eps_rank);
    if (rc) return rc;
    const Plan& P = h->plan;
    hipStream_t s = h->stream;
    const int64_t n2 = h->tsqr_n2;
    const size_t msg_len = ((size_t)TSQR_HDR + (size_t)n * (n + 1) / 2 + (size_t)n + 1) & ~(size_t)1;   // doubles per rank (from n, not n2), 16-byte granules
    rc = grow(h, h->xbuf, (size_t)(G + 1) * msg_len * 8 + 256);
    if (rc) return rc;
    double* send = (double*)h->xbuf.p;
    double* recv = send + msg_len;
    GN_HIP(hipMemsetAsync(send, 0, TSQR_HDR * 8, s));
    hipLaunchKernelGGL(k_tsqr_pack, dim3(256), dim3(256), 0, s, h->W, P.ldw, (int)n, (int)m_loc, h->state, send, h->tsqr_rank, G);
    GN_HIP(hipGetLastError());
    if (ev) GN_HIP(hipEventRecord(ev[6], s));
    // ---- the one exchange step -----------------------------------------------------------------------------------------------
    // an attached RCCL communicator is USED, also with one rank (a self-gather of a few MB): the prototype, the datatype
    // constant and the count are then exercised on every box, not for the first time on an 8-GPU node
    if (h->tsqr_comm) {
        RcclApi& r = rccl();
        const int e = r.AllGather(send, recv, msg_len, GN_NCCL_FLOAT64, h->tsqr_comm, s);
        if (e != 0) {
            h->err = std::string("ncclAllGather: ") + (r.GetErrorString ? r.GetErrorString(e) : "error");
            return 995;
        }
        h->tsqr_transport = ENLSIP_GN_TRANSPORT_RCCL;
    } else if (G > 1) {
        GN_HIP(hipStreamSynchronize(s));
        const int e = h->tsqr_xfn(h->tsqr_xctx, send, recv, msg_len * 8, (void*)s);
        if (e != 0) { h->err = "the caller's all-gather reported error " + std::to_string(e); return 994; }
        h->tsqr_transport = ENLSIP_GN_TRANSPORT_CALLBACK;
    } else {
        GN_HIP(hipMemcpyAsync(recv, send, msg_len * 8, hipMemcpyDeviceToDevice, s));
        h->tsqr_transport = ENLSIP_GN_TRANSPORT_NONE;
    }
    if (ev) GN_HIP(hipEventRecord(ev[7], s));
    // ---- combine, redundantly on every rank ----------------------------------------------------------------------------------
    rc = tsqr_scratch(h, G, n2);
    if (rc) return rc;
    double* Jst = (double*)h->scratch.p;
    double* tails = (double*)(h->small + 12);
    if (n2 > 0) {
        hipLaunchKernelGGL(k_tsqr_unpack, dim3(1024), dim3(256), 0, s, recv, (long long)msg_len, G, (int)n2, Jst,
                           Jst + (size_t)G * n2 * n2, tails);
        GN_HIP(hipGetLastError());
    } else {
        GN_HIP(hipMemsetAsync(tails, 0, 24, s));
    }
    double ctail = 0.0;
    double tail_host[3] = {0.0, 0.0, -1.0};           // tail^2, the n2 check, the rank tags; complete before this frame can be left
    {
        const hipError_t e1 = hipMemcpyAsync(tail_host, tails, 24, hipMemcpyDeviceToHost, s);
        const hipError_t e2 = hipStreamSynchronize(s);
        GN_HIP(e1);
        GN_HIP(e2);
    }
    const double tail_sum = tail_host[0];
    h->tsqr_tags_seen = n2 > 0 ? (int)tail_host[2] : -1;       // n2 == 0: nothing was unpacked
    if (tail_host[1] != 0.0) {
        h->err = "enlsip_gn_solve_tsqr: the ranks disagree about n2 (rank of the constraint Jacobian / eps_rank differ between ranks)";
        return -13;
    }
    std::vector<double> dl((size_t)std::max<int64_t>(n2, 1));
    rc = tsqr_combine_core(h, G, n2, eps_rank, p, dl.data(), &ctail, info, jpvtJ2);
    if (rc) return rc;
    double lead = 0.0;
    for (int64_t i = 0; i < n2; ++i) lead += dl[i] * dl[i];
    if (dlead) memcpy(dlead, dl.data(), (size_t)n2 * 8);
    if (n2 == 0) {       // J2 is m x 0: d = d_temp, whole norm in the tails
        GN_HIP(hipStreamSynchronize(s));
    }
    if (d_norm) *d_norm = std::sqrt(tail_sum + ctail + lead);
    if (ev) {
        GN_HIP(hipEventRecord(ev[4], s));
        GN_HIP(hipEventSynchronize(ev[4]));
        float ms;
        GN_HIP(hipEventElapsedTime(&ms, ev[5], ev[6])); h->tsqr_ms[0] = ms;
        GN_HIP(hipEventElapsedTime(&ms, ev[6], ev[7])); h->tsqr_ms[1] = ms;
        GN_HIP(hipEventElapsedTime(&ms, ev[7], ev[4])); h->tsqr_ms[2] = ms;
    }
    h->held.clear();
    h->factors_valid = false;       // the resident pieces are those of a row shard, not of a whole problem
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_tsqr_get_transport(enlsip_gn_handle h, int* transport) {
    if (!h) return -1;
    if (!transport) return -2;
    *transport = h->tsqr_transport;
    return 0;
}

int enlsip_gn_tsqr_get_exchange(enlsip_gn_handle h, int* transport, int* ranks, int* rank_tags_seen) {
    if (!h) return -1;
    if (transport) *transport = h->tsqr_transport;
    if (ranks) *ranks = h->tsqr_ranks;
    if (rank_tags_seen) *rank_tags_seen = h->tsqr_tags_seen;
    return 0;
}

int enlsip_gn_tsqr_get_stage_ms(enlsip_gn_handle h, float* ms3) {
    if (!h) return -1;
    if (!ms3) return -2;
    for (int i = 0; i < 3; ++i) ms3[i] = h->tsqr_ms[i];
    return 0;
}

}  // extern "C"
