// Row-sharded TSQR (config C4): local stage -> ONE exchange step -> combine stage.
//   enlsip_gn_solve_tsqr            the whole collective inside the library: the exchange is one all-gather of
//                                   [packed upper triangle | z | tail^2] per rank over RCCL (loaded at run time, so that the
//                                   library itself has no link-time dependency on it) or over a caller-supplied transport
//   enlsip_gn_tsqr_local_dev / _combine_dev   the two stages alone, exchange by the caller (INTEGRATION.md section 5)
//   enlsip_gn_tsqr_local_scaled_dev / _combine_scaled_dev   the same with the shard's exponent beside its triangle
// Magnitudes (gn_rescale.hpp): a shard whose local result is nominated (k_tsqr_flags) and whose inputs lie outside the band is
// factored again on copies scaled by a power of two of ITS OWN choice, 2^-e_g; e_g travels in the message header and the combine
// brings the blocks to the common scale 2^-E, E = max e_g.  No agreement before the local stages, still one exchange step.
// Included by enlsip_gn.hip.
#include <dlfcn.h>

namespace gn {

struct gn_nccl_id { char internal[128]; };      // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128), passed by value

// *out = sum of x[lo .. hi)^2, taken in a FIXED order whatever the scheduling (every launch of one shape returns the same bits, and
// a power-of-two multiple of x the exact multiple of them): each thread its strided entries, the wave's butterfly, the
// workgroup's waves in order into part[blockIdx.x], and the workgroup that finishes last adds the partial sums in a fixed order.
// part: gridDim.x doubles; count: one word, zero before the launch and left zero.  Call from every thread of the grid.
constexpr int TSQR_SUM_BLOCKS = 256;           // largest grid of a kernel that calls it (size of the partial-sum area)
__device__ __forceinline__ void ordered_sumsq(const double* x, long long lo, long long hi, double* part, unsigned* count, double* out) {
    __shared__ double wsum[16];
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * blockDim.x;
    double s = 0.0;
    for (long long i = lo + tid; i < hi; i += nthreads) s += x[i] * x[i];
    s = wave_allsum(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    __shared__ int last;
    if (threadIdx.x == 0) {
        double b = 0.0;
        for (unsigned w = 0; w < (blockDim.x >> 6); ++w) b += wsum[w];
        __hip_atomic_store(part + blockIdx.x, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        last = atomicAdd(count, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last || threadIdx.x >= 64) return;
    // the first wave of the last workgroup: lane l adds part[l], part[l + 64], ... in that order, then the butterfly
    __threadfence();
    double total = 0.0;
    for (unsigned g = threadIdx.x; g < gridDim.x; g += 64) total += __hip_atomic_load(part + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    total = wave_allsum(total);
    if (threadIdx.x == 0) {
        *out = total;
        atomicExch(count, 0u);
    }
}

// Rloc (packed n2 x n2, upper) and zloc from the CAQR result in W; sum of squares of the tail of d
__global__ void k_tsqr_extract(const double* W, int ldw, int n, int m, const ProbState* st, double* Rloc,
                               double* zloc, double* tail_sq, double* part, unsigned* count) {
    const int rankA = st->rankA, n2 = st->n2, kp = st->kp;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * blockDim.x;
    for (long long e = tid; e < (long long)n2 * n2; e += nthreads) {
        const int i = (int)(e % n2), c = (int)(e / n2);
        Rloc[e] = (i <= c && i < kp) ? W[i + (size_t)(rankA + c) * ldw] : 0.0;
    }
    for (long long i = tid; i < n2; i += nthreads) zloc[i] = (i < kp) ? W[i + (size_t)n * ldw] : 0.0;
    ordered_sumsq(W + (size_t)n * ldw, kp, m, part, count, tail_sq);
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
//   [0] n2 of the sender (checked against the receiver's after the gather)   [1] tail^2
//   [2] rank of the sender + 1, [3] the rank count the sender believes in: after the gather slot g must carry tag g + 1 — the
//       count of slots that do is what "did the collective see N ranks" can be answered from (enlsip_gn_tsqr_get_exchange)
//   [4] e_g: triangle, z and tail^2 are those of the sender's shard times 2^-e_g (an exact small double; 0: not rescaled)
//   [5] spare (zero): keeps the body on a 16-byte granule
//   [6 ...] packed upper triangle (column c at offset c (c + 1) / 2, c + 1 entries), then z (n2)
constexpr int TSQR_HDR = 6;
__device__ __forceinline__ int tsqr_msg_exponent(const double* msg) {       // a header that is not a sane exponent counts as 0
    const double x = msg[4];
    return (x >= -2200.0 && x <= 2200.0) ? (int)x : 0;
}
__global__ void k_tsqr_pack(const double* W, int ldw, int n, int m, const ProbState* st, double* msg, int rank, int ranks, int e_g,
                            double* part, unsigned* count) {
    const int rankA = st->rankA, n2 = st->n2, kp = st->kp;
    const long long tri = (long long)n2 * (n2 + 1) / 2;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * blockDim.x;
    if (tid == 0) {
        msg[0] = (double)n2;
        msg[2] = (double)(rank + 1);
        msg[3] = (double)ranks;
        msg[4] = (double)e_g;
    }
    double* body = msg + TSQR_HDR;
    for (int c = blockIdx.x; c < n2; c += gridDim.x) {
        double* dst = body + (long long)c * (c + 1) / 2;
        for (int i = threadIdx.x; i <= c; i += blockDim.x) dst[i] = (i < kp) ? W[i + (size_t)(rankA + c) * ldw] : 0.0;
    }
    for (long long i = tid; i < n2; i += nthreads) body[tri + i] = (i < kp) ? W[i + (size_t)n * ldw] : 0.0;
    ordered_sumsq(W + (size_t)n * ldw, kp, m, part, count, msg + 1);
}

// G gathered messages -> the stacked problem: Jst is (G n2) x n2 with ld = G n2 (block g = triangle of rank g, zeros below),
// rxs = -[z_0; z_1; ...]; tails[0] = sum of the ranks' tail^2, tails[1] = number of ranks whose n2 differs from this rank's
// (their triangles would be read with the wrong layout: the caller turns that into an error).
// Scales: block g arrives times 2^-e_g; with E = max e_g (tails[3]) block g and z_g are multiplied by 2^(e_g - E) and tail_g^2 by
// its square, so that the stacked problem is the whole one times 2^-E.  A block far below the largest one may flush to zeros: a
// relative perturbation of 2^-600 at most.  Equal exponents (every in-band call): nothing is multiplied.
__global__ void k_tsqr_unpack(const double* msgs, long long msg_len, int G, int n2, double* Jst, double* rxs, double* tails) {
    const long long ld = (long long)G * n2;
    const long long tri = (long long)n2 * (n2 + 1) / 2;
    int E = tsqr_msg_exponent(msgs);
    for (int g = 1; g < G; ++g) {
        const int e = tsqr_msg_exponent(msgs + g * msg_len);
        E = e > E ? e : E;
    }
    for (long long cg = blockIdx.x; cg < (long long)G * n2; cg += gridDim.x) {
        const int g = (int)(cg / n2), c = (int)(cg % n2);
        const int sh = tsqr_msg_exponent(msgs + g * msg_len) - E;
        const double* src = msgs + g * msg_len + TSQR_HDR + (long long)c * (c + 1) / 2;
        double* dst = Jst + (long long)g * n2 + (long long)c * ld;
        if (sh == 0) for (int i = threadIdx.x; i < n2; i += blockDim.x) dst[i] = (i <= c) ? src[i] : 0.0;
        else for (int i = threadIdx.x; i < n2; i += blockDim.x) dst[i] = (i <= c) ? __builtin_ldexp(src[i], sh) : 0.0;
    }
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * blockDim.x;
    for (long long i = tid; i < ld; i += nthreads) {
        const double* msg = msgs + (i / n2) * msg_len;
        const int sh = tsqr_msg_exponent(msg) - E;
        const double z = msg[TSQR_HDR + tri + (i % n2)];
        rxs[i] = sh == 0 ? -z : -__builtin_ldexp(z, sh);
    }
    if (tid == 0) {
        double s = 0.0, bad = 0.0, tagged = 0.0;
        for (int g = 0; g < G; ++g) {
            const int sh = tsqr_msg_exponent(msgs + g * msg_len) - E;
            s += sh == 0 ? msgs[g * msg_len + 1] : __builtin_ldexp(msgs[g * msg_len + 1], 2 * sh);
            if (msgs[g * msg_len] != (double)n2) bad += 1.0;
            if (msgs[g * msg_len + 2] == (double)(g + 1) && msgs[g * msg_len + 3] == (double)G) tagged += 1.0;
        }
        tails[0] = s;
        tails[1] = bad;
        tails[2] = tagged;       // slots whose message came from the rank the slot belongs to
        tails[3] = (double)E;
    }
}

__global__ void k_sumsq(const double* x, long long lo, long long hi, double* out, double* part, unsigned* count) {
    ordered_sumsq(x, lo, hi, part, count, out);
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

// the partial-sum area and the counter of ordered_sumsq (the counter is zeroed here, on the stream, before every use)
static int tsqr_sum_area(enlsip_gn_handle h, double** part, unsigned** count) {
    int rc = grow(h, h->tsqr_part, (size_t)TSQR_SUM_BLOCKS * 8);
    if (rc) return rc;
    *part = (double*)h->tsqr_part.p;
    *count = &h->small->sum_count;
    GN_HIP(hipMemsetAsync(*count, 0, 4, h->stream));
    return 0;
}

// largest |entry| of the shard's J, of its rx and of A', cx -> the shard's power-of-two shifts (0: the larger of J, rx lies inside
// the band, or is zero or not finite — nothing to rescale; likewise A', cx).  J and rx share ONE shift, which brings the larger of
// the two to magnitude ~1; when the other lies more than 2^400 below it, the shift takes the middle of the two instead, so that
// the squares of BOTH stay in range (J 2^600 with an ordinary rx: R near 2^300, d near 2^-300, tail^2 near 2^-600).
static int tsqr_shifts(enlsip_gn_handle h, long long m, long long n, long long t, const double* dJ, long long ldj, const double* drx,
                       const double* dAt, long long ldat, const double* dcx, int* shiftJ, int* shiftA) {
    hipStream_t s = h->stream;
    unsigned long long* dmx = h->small->amax;
    GN_HIP(hipMemsetAsync(dmx, 0, 24, s));
    hipLaunchKernelGGL(k_amax_bits, dim3((unsigned)n), dim3(256), 0, s, dJ, ldj, (int)m, (int)n, dmx);
    hipLaunchKernelGGL(k_amax_bits, dim3(1), dim3(256), 0, s, drx, m, (int)m, 1, dmx + 1);
    if (t > 0) {
        hipLaunchKernelGGL(k_amax_bits, dim3((unsigned)t), dim3(256), 0, s, dAt, ldat, (int)n, (int)t, dmx + 2);
        hipLaunchKernelGGL(k_amax_bits, dim3(1), dim3(256), 0, s, dcx, t, (int)t, 1, dmx + 2);
    }
    GN_HIP(hipGetLastError());
    unsigned long long hb[3] = {0, 0, 0};
    GN_HIP(hipMemcpyAsync(hb, dmx, 24, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    // 0: zero; 1: finite, *e = its binary exponent (a = f 2^e, 0.5 <= f < 1); -1: not finite
    auto exponent_of = [](unsigned long long bits, int* e) -> int {
        double a;
        memcpy(&a, &bits, 8);
        if (!std::isfinite(a)) return -1;
        if (!(a > 0.0)) return 0;
        (void)std::frexp(a, e);
        return 1;
    };
    auto outside = [](int e) { return e > GN_RESCALE_BAND || e < -GN_RESCALE_BAND; };
    *shiftJ = 0;
    *shiftA = 0;
    int eJ = 0, er = 0, eA = 0;
    const int kJ = exponent_of(hb[0], &eJ), kr = exponent_of(hb[1], &er), kA = exponent_of(hb[2], &eA);
    if (kJ >= 0 && kr >= 0 && (kJ > 0 || kr > 0)) {
        const int hi = kJ == 0 ? er : kr == 0 ? eJ : std::max(eJ, er);
        const int lo = kJ == 0 ? er : kr == 0 ? eJ : std::min(eJ, er);
        if (outside(hi)) {
            int sh = hi - lo <= GN_RESCALE_BAND ? -(hi - 1) : -((hi + lo) / 2);
            sh = std::min(sh, GN_RESCALE_BAND - hi);      // more than 2^800 apart: the larger one stays inside the band
            *shiftJ = sh;
        }
    }
    if (kA > 0 && outside(eA)) *shiftA = -(eA - 1);
    return 0;
}

// one pass of the local stage on the J, rx given (the caller's, or their scaled copies; the constraint stage picks the scaled
// A', cx itself when sc_eA is set): constraint stage, then up to two attempts of J*Q1 and the CAQR of [J2 | d_temp]
static int tsqr_local_pass(enlsip_gn_handle h, int64_t m_loc, int64_t n, int64_t t, const double* dJ, int64_t ldj, const double* drx,
                           const double* dAt, int64_t ldat, const double* dcx, double eps_rank, bool detect) {
    const Plan& P = h->plan;
    hipStream_t s = h->stream;
    int rc = run_constraint_stage(h, 1, m_loc, n, t, dAt, ldat, 0, dcx, eps_rank, -1);
    if (rc) return rc;
    int n2_launch = (int)(n - P.kA);
    for (int attempt = 0; attempt < 2; ++attempt) {
        launch_jq1_any(h, jq1_args(h, dJ, ldj, 0, drx), 1, s);
        rc = run_caqr(h, n2_launch);
        if (rc) return rc;
        if (detect) {
            // nominate the shard on its local result (gn_rescale.hpp); the flags travel in the read-back below
            const long long work = (long long)n2_launch * (n2_launch + 1) / 2 + m_loc;
            const unsigned blocks = (unsigned)std::min<long long>(256, std::max<long long>(1, work / 2048));
            hipLaunchKernelGGL(k_tsqr_flags, dim3(blocks), dim3(256), 0, s, h->state, (const double*)h->W, P.ldw, (int)n, (int)m_loc,
                               (const double*)h->FA, P.kA, n2_launch, h->small->flag_acc);
            GN_HIP(hipGetLastError());
        }
        GN_HIP(hipMemcpyAsync(h->h_state, h->state, sizeof(ProbState), hipMemcpyDeviceToHost, s));
        GN_HIP(hipStreamSynchronize(s));
        if (h->h_state[0].n2 <= n2_launch) break;
        n2_launch = h->h_state[0].n2;
    }
    return 0;
}

// the local stage up to the CAQR of [J2 | d_temp]; the factored W stays resident.  scaled: the shard may be factored at a scale
// 2^-tsqr_e of its own (the entry points that carry the exponent); otherwise plain arithmetic on the caller's data, as ever.
int tsqr_local_core(enlsip_gn_handle h, int64_t m_loc, int64_t n, int64_t t, const double* dJ, int64_t ldj,
                    const double* drx, const double* dAt, int64_t ldat, const double* dcx, double eps_rank, bool scaled) {
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
    hipStream_t s = h->stream;
    h->eps_rank = eps_rank;
    h->factors_valid = false;
    h->tsqr_stage = 0;
    h->held.clear();
    h->last = {1, m_loc, n, t, dJ, ldj, 0, drx, dAt, ldat, 0, dcx};
    // same routing as a solve (register / distributed forms of F_A for the shapes that need them)
    h->sc_eJ = 0; h->sc_eA = 0;
    h->tsqr_e = 0; h->tsqr_E = 0;
    h->rescue_prob.clear();
    h->h_tk.clear();
    gn_route_acc = 0;
    const bool detect = scaled && h->rescale_enabled;
    if (detect) GN_HIP(hipMemsetAsync(h->small->flag_acc, 0, sizeof h->small->flag_acc, s));      // accumulator of k_tsqr_flags (it leaves it zero itself)
    rc = tsqr_local_pass(h, m_loc, n, t, dJ, ldj, drx, dAt, ldat, dcx, eps_rank, detect);
    if (rc) return rc;
    if (h->h_state[0].status & (GN_FLAG_NONFINITE | GN_FLAG_TINY)) {
        // nominated: beyond the band the shard is factored again on copies scaled by a power of two of its own (gn_rescale.hpp)
        int sJ = 0, sA = 0;
        rc = tsqr_shifts(h, m_loc, n, t, dJ, ldj, drx, dAt, ldat, dcx, &sJ, &sA);
        if (rc) return rc;
        if (sJ || sA) {
            GN_TRACE(h, "tsqr local: J, rx by 2^%d, A', cx by 2^%d", sJ, sA);
            rc = scaled_copies(h, h->last, sJ, sA);
            if (rc) return rc;
            h->sc_eA = sA;
            h->sc_eJ = sJ;
            rc = sJ ? tsqr_local_pass(h, m_loc, n, t, h->rs_J, m_loc, h->rs_rx, dAt, ldat, dcx, eps_rank, detect)
                    : tsqr_local_pass(h, m_loc, n, t, dJ, ldj, drx, dAt, ldat, dcx, eps_rank, detect);
            if (rc) return rc;
            h->tsqr_e = -sJ;
            GN_ROUTE(ENLSIP_GN_ROUTE_RESCALED);
        }
        // the nomination bits are host-internal
        h->h_state[0].status &= ~(GN_FLAG_NONFINITE | GN_FLAG_TINY);
        hipLaunchKernelGGL(k_clear_status_bits, dim3(1), dim3(256), 0, s, h->state, GN_FLAG_NONFINITE | GN_FLAG_TINY, 1, (const int*)nullptr);
        GN_HIP(hipGetLastError());
    }
    h->tsqr_n2 = h->h_state[0].n2;
    h->route = gn_route_acc;
    h->tsqr_stage = 1;
    return 0;
}

// the stacked problem (Jst (G n2) x n2, rxs) is in place in h->scratch: factor, solve, p = Q1 [p1; p2].
// E: the stacked problem is the whole one times 2^-E (k_tsqr_unpack); the absolute rank test follows (SolveMode::abs_shift), p, the
// ranks and the pivots need nothing, and dlead / comb_tail_sq come back AT THAT SCALE: the caller takes its norms there, where no
// square leaves the range, and scales back by 2^E afterwards.
// the stacked problem of G blocks of n2 columns in h->scratch (grown, never shrunk: a second call with the same shape places again)
int tsqr_scratch(enlsip_gn_handle h, int64_t G, int64_t n2, TsqrScratch& T) {
    return place_dev(h, h->scratch, T, (long long)G, (long long)n2, h->plan.n);
}
int tsqr_combine_core(enlsip_gn_handle h, int64_t G, int64_t n2, double eps_rank, int E, double* p, double* dlead,
                      double* comb_tail_sq, enlsip_gn_info* info, int64_t* jpvtJ2) {
    const Plan& P = h->plan;      // plan of the local stage: F_A, p1, state are resident
    hipStream_t s = h->stream;
    const long long n = P.n, ms = (long long)G * n2;
    const ProbState st = h->h_state[0];
    TsqrScratch T;
    int rc = tsqr_scratch(h, G, n2, T);      // grown by the caller that stacked the problem: places only
    if (rc) return rc;
    double *Jst = T.Jst, *rxs = T.rxs, *dp2 = T.p2, *dd = T.d, *dpo = T.pout;
    enlsip_gn_info sinfo = {0, 0, 1, 0, 0, 0};
    if (n2 > 0) {
        if (!h->sub) {
            rc = create_helper(h, &h->sub, h->stream);
            if (rc) { h->err = "tsqr_combine: cannot create the sub-handle"; return rc; }
        }
        // jpvt / info of the stacked (unconstrained) problem through the ordinary device-pointer solve
        rc = grow(h, h->out_stage, (size_t)n2 * 8);
        if (rc) return rc;
        long long* djJ = (long long*)h->out_stage.p;
        const BatchOperands v{1, ms, n2, 0, Jst, ms, 0, rxs, nullptr, 1, 0, nullptr, dp2, nullptr, dd, nullptr, nullptr, nullptr, djJ};
        const unsigned long long route_local = h->route;
        rc = solve_dev(h->sub, v, {SolveMode::Fresh, nullptr, G == 1, -1, -1, eps_rank, -E});      // one rank: the stacked matrix is that rank's triangle
        if (rc) { h->err = std::string("tsqr_combine/sub: ") + h->sub->err; return rc; }
        h->route = route_local | h->sub->route;
        sinfo = info_of(h->sub->h_state[0]);       // its rankJ2, dimJ2 and status
        if (jpvtJ2) GN_HIP(hipMemcpyAsync(jpvtJ2, djJ, (size_t)n2 * 8, hipMemcpyDeviceToHost, s));
        if (dlead) GN_HIP(hipMemcpyAsync(dlead, dd, (size_t)n2 * 8, hipMemcpyDeviceToHost, s));
        double* part = nullptr;
        unsigned* count = nullptr;
        rc = tsqr_sum_area(h, &part, &count);
        if (rc) return rc;
        GN_HIP(hipMemsetAsync(&h->small->tail_sum, 0, 8, s));
        if (ms > n2) hipLaunchKernelGGL(k_sumsq, dim3(64), dim3(256), 0, s, dd, (long long)n2, ms, &h->small->tail_sum, part, count);
        if (comb_tail_sq) GN_HIP(hipMemcpyAsync(comb_tail_sq, &h->small->tail_sum, 8, hipMemcpyDeviceToHost, s));
    } else if (comb_tail_sq) {
        *comb_tail_sq = 0.0;
    }
    hipLaunchKernelGGL(k_tsqr_q1, dim3(1), dim3(64), 0, s, h->FA, (int)n, h->tauA, P.kA, h->p1, h->state, dp2, dpo);
    GN_HIP(hipGetLastError());
    if (p) GN_HIP(hipMemcpyAsync(p, dpo, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    if (info) *info = {st.rankA, sinfo.rankJ2, st.code, st.dimA, sinfo.dimJ2, (int64_t)(st.status | sinfo.status)};
    h->tsqr_E = E;
    if (E != 0 || h->tsqr_e != 0) h->route |= (1ull << ENLSIP_GN_ROUTE_RESCALED);
    if (h->tsqr_stage == 1) h->tsqr_stage = 2;       // the shard's local stage of THIS handle went into the combine
    return 0;
}

}  // namespace

extern "C" {

// both forms of the local stage entry point: scaled = the shard may come back times 2^-*e_out
static int tsqr_local_stage(enlsip_gn_handle h, int64_t m_loc, int64_t n, int64_t t, const double* dJ, int64_t ldj,
                            const double* drx, const double* dAt, int64_t ldat, const double* dcx, double eps_rank,
                            double* dRloc, double* dzloc, double* tail_sq, int64_t* n2_out, bool scaled, int64_t* e_out) {
    if (!h) return -1;
    GN_TRY
    if (!dRloc || !dzloc) { h->err = "dRloc / dzloc is NULL"; return -12; }
    int rc = tsqr_local_core(h, m_loc, n, t, dJ, ldj, drx, dAt, ldat, dcx, eps_rank, scaled);
    if (rc) return rc;
    const Plan& P = h->plan;
    hipStream_t s = h->stream;
    double* dsum = &h->small->tail_sum;
    double* part = nullptr;
    unsigned* count = nullptr;
    rc = tsqr_sum_area(h, &part, &count);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tsqr_extract, dim3(TSQR_SUM_BLOCKS), dim3(256), 0, s, h->W, P.ldw, (int)n, (int)m_loc, h->state, dRloc,
                       dzloc, dsum, part, count);
    GN_HIP(hipGetLastError());
    double ts = 0.0;
    GN_HIP(hipMemcpyAsync(&ts, dsum, 8, hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    if (tail_sq) *tail_sq = ts;
    if (n2_out) *n2_out = h->tsqr_n2;
    if (e_out) *e_out = h->tsqr_e;
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_tsqr_local_dev(enlsip_gn_handle h, int64_t m_loc, int64_t n, int64_t t, const double* dJ, int64_t ldj,
                             const double* drx, const double* dAt, int64_t ldat, const double* dcx, double eps_rank,
                             double* dRloc, double* dzloc, double* tail_sq, int64_t* n2_out) {
    return tsqr_local_stage(h, m_loc, n, t, dJ, ldj, drx, dAt, ldat, dcx, eps_rank, dRloc, dzloc, tail_sq, n2_out, false, nullptr);
}

int enlsip_gn_tsqr_local_scaled_dev(enlsip_gn_handle h, int64_t m_loc, int64_t n, int64_t t, const double* dJ, int64_t ldj,
                                    const double* drx, const double* dAt, int64_t ldat, const double* dcx, double eps_rank,
                                    double* dRloc, double* dzloc, double* tail_sq, int64_t* n2_out, int64_t* e_out) {
    if (h && !e_out) { h->err = "e_out is NULL"; return -14; }
    return tsqr_local_stage(h, m_loc, n, t, dJ, ldj, drx, dAt, ldat, dcx, eps_rank, dRloc, dzloc, tail_sq, n2_out, true, e_out);
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
    TsqrScratch T;
    int rc = tsqr_scratch(h, G, n2, T);
    if (rc) return rc;
    if (n2 > 0) {
        hipLaunchKernelGGL(k_tsqr_stack, dim3(512), dim3(256), 0, h->stream, dRstack, dzstack, (int)G, (int)n2, T.Jst, T.rxs);
        GN_HIP(hipGetLastError());
    }
    return tsqr_combine_core(h, G, n2, eps_rank, 0, p, dlead, comb_tail_sq, info, jpvtJ2);
    GN_CATCH(h)
}

int enlsip_gn_tsqr_combine_scaled_dev(enlsip_gn_handle h, int64_t G, int64_t n2, const double* dRstack, const double* dzstack,
                                      const int64_t* e, const double* tail_sq, double eps_rank, double* p, double* dlead,
                                      double* d_norm, enlsip_gn_info* info, int64_t* jpvtJ2) {
    if (!h) return -1;
    GN_TRY
    if (G < 1) { h->err = "G < 1"; return -2; }
    if (h->tsqr_n2 < 0 || n2 != h->tsqr_n2) { h->err = "tsqr_combine: n2 does not match the last tsqr_local on this handle"; return -3; }
    if (n2 > 0 && (!dRstack || !dzstack)) { h->err = "dRstack / dzstack is NULL"; return -4; }
    if (!e || !tail_sq) { h->err = "e / tail_sq is NULL"; return -5; }
    int64_t E = e[0];
    for (int64_t g = 0; g < G; ++g) {
        if (e[g] < -2200 || e[g] > 2200) { h->err = "tsqr_combine: an exponent is out of range"; return -6; }
        E = std::max(E, e[g]);
    }
    GN_HIP(hipSetDevice(h->device));
    TsqrScratch T;
    int rc = tsqr_scratch(h, G, n2, T);
    if (rc) return rc;
    hipStream_t s = h->stream;
    if (n2 > 0) {
        double *Jst = T.Jst, *rxs = T.rxs;
        hipLaunchKernelGGL(k_tsqr_stack, dim3(512), dim3(256), 0, s, dRstack, dzstack, (int)G, (int)n2, Jst, rxs);
        GN_HIP(hipGetLastError());
        // block g arrived times 2^-e[g]: to the common scale 2^-E (nothing to do where the exponents agree)
        for (int64_t g = 0; g < G; ++g) {
            scale_region(s, Jst + (size_t)g * n2, (long long)G * n2, n2, n2, (int)(e[g] - E), 1);
            scale_region(s, rxs + (size_t)g * n2, (long long)G * n2, n2, 1, (int)(e[g] - E), 0);
        }
        GN_HIP(hipGetLastError());
    }
    double tail_sum = 0.0, ctail = 0.0;
    for (int64_t g = 0; g < G; ++g) tail_sum += std::ldexp(tail_sq[g], (int)(2 * (e[g] - E)));
    std::vector<double> dl((size_t)std::max<int64_t>(n2, 1));
    rc = tsqr_combine_core(h, G, n2, eps_rank, (int)E, p, dl.data(), &ctail, info, jpvtJ2);
    if (rc) return rc;
    double lead = 0.0;
    for (int64_t i = 0; i < n2; ++i) lead += dl[i] * dl[i];
    if (dlead) for (int64_t i = 0; i < n2; ++i) dlead[i] = std::ldexp(dl[i], (int)E);
    if (d_norm) *d_norm = std::ldexp(std::sqrt(tail_sum + ctail + lead), (int)E);
    return 0;
    GN_CATCH(h)
}

int enlsip_gn_tsqr_get_scale(enlsip_gn_handle h, int64_t* e_local, int64_t* e_common) {
    if (!h) return -1;
    if (e_local) *e_local = h->tsqr_e;
    if (e_common) *e_common = h->tsqr_E;
    return 0;
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

// The one exchange step of a collective on the handle's communicator (enlsip_gn_solve_tsqr, the enlsip_gn_tsqr_products family):
// every rank's `send` (msg_len doubles, device) into `recv` (ranks x msg_len, rank-major), on the handle's stream.
// An attached RCCL communicator is USED, also with one rank (a self-gather of a few MB): the prototype, the datatype
// constant and the count are then exercised on every box, not for the first time on an 8-GPU node.
static int tsqr_exchange_step(enlsip_gn_handle h, const double* send, double* recv, size_t msg_len) {
    hipStream_t s = h->stream;
    if (h->tsqr_comm) {
        RcclApi& r = rccl();
        const int e = r.AllGather(send, recv, msg_len, GN_NCCL_FLOAT64, h->tsqr_comm, s);
        if (e != 0) {
            h->err = std::string("ncclAllGather: ") + (r.GetErrorString ? r.GetErrorString(e) : "error");
            return 995;
        }
        h->tsqr_transport = ENLSIP_GN_TRANSPORT_RCCL;
    } else if (h->tsqr_ranks > 1) {
        GN_HIP(hipStreamSynchronize(s));
        const int e = h->tsqr_xfn(h->tsqr_xctx, send, recv, msg_len * 8, (void*)s);
        if (e != 0) { h->err = "the caller's all-gather reported error " + std::to_string(e); return 994; }
        h->tsqr_transport = ENLSIP_GN_TRANSPORT_CALLBACK;
    } else {
        GN_HIP(hipMemcpyAsync(recv, send, msg_len * 8, hipMemcpyDeviceToDevice, s));
        h->tsqr_transport = ENLSIP_GN_TRANSPORT_NONE;
    }
    return 0;
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
    int rc = tsqr_local_core(h, m_loc, n, t, dJ, ldj, drx, dAt, ldat, dcx, eps_rank, true);
    if (rc) return rc;
    const Plan& P = h->plan;
    hipStream_t s = h->stream;
    const int64_t n2 = h->tsqr_n2;
    const size_t msg_len = ((size_t)TSQR_HDR + (size_t)n * (n + 1) / 2 + (size_t)n + 1) & ~(size_t)1;   // doubles per rank (from n, not n2), 16-byte granules
    struct { double *send = nullptr, *recv = nullptr;      // the send message + G received messages
             void carve(Carver& c, size_t len, int G) { c.take(send, "send", len, 16); c.take(recv, "recv", (size_t)G * len, 16); } } X;
    rc = place_dev(h, h->xbuf, X, msg_len, G);
    if (rc) return rc;
    double *send = X.send, *recv = X.recv;
    GN_HIP(hipMemsetAsync(send, 0, TSQR_HDR * 8, s));
    double* part = nullptr;
    unsigned* count = nullptr;
    rc = tsqr_sum_area(h, &part, &count);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tsqr_pack, dim3(TSQR_SUM_BLOCKS), dim3(256), 0, s, h->W, P.ldw, (int)n, (int)m_loc, h->state, send, h->tsqr_rank, G,
                       h->tsqr_e, part, count);
    GN_HIP(hipGetLastError());
    if (ev) GN_HIP(hipEventRecord(ev[6], s));
    // ---- the one exchange step -----------------------------------------------------------------------------------------------
    rc = tsqr_exchange_step(h, send, recv, msg_len);
    if (rc) return rc;
    if (ev) GN_HIP(hipEventRecord(ev[7], s));
    // ---- combine, redundantly on every rank ----------------------------------------------------------------------------------
    TsqrScratch T;
    rc = tsqr_scratch(h, G, n2, T);
    if (rc) return rc;
    double* tails = h->small->tails;
    // n2 == 0: no triangle and no z to unpack (the loops over G n2 are empty), but the headers still carry what ||d|| is made of —
    // d = d_temp, so the ranks' tail^2 at the common scale are the whole norm
    hipLaunchKernelGGL(k_tsqr_unpack, dim3(n2 > 0 ? 1024 : 1), dim3(256), 0, s, recv, (long long)msg_len, G, (int)n2, T.Jst, T.rxs, tails);
    GN_HIP(hipGetLastError());
    double ctail = 0.0;
    double tail_host[4] = {0.0, 0.0, -1.0, 0.0};      // tail^2, the n2 check, the rank tags, E; complete before this frame can be left
    {
        const hipError_t e1 = hipMemcpyAsync(tail_host, tails, 32, hipMemcpyDeviceToHost, s);
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
    const int E = (int)tail_host[3];                  // the stacked problem, its d and the three sums of squares are at scale 2^-E
    std::vector<double> dl((size_t)std::max<int64_t>(n2, 1));
    rc = tsqr_combine_core(h, G, n2, eps_rank, E, p, dl.data(), &ctail, info, jpvtJ2);
    if (rc) return rc;
    double lead = 0.0;
    for (int64_t i = 0; i < n2; ++i) lead += dl[i] * dl[i];
    if (dlead && E == 0) memcpy(dlead, dl.data(), (size_t)n2 * 8);
    else if (dlead) for (int64_t i = 0; i < n2; ++i) dlead[i] = std::ldexp(dl[i], E);
    if (n2 == 0) {       // J2 is m x 0: d = d_temp, whole norm in the tails
        GN_HIP(hipStreamSynchronize(s));
    }
    if (d_norm) *d_norm = E == 0 ? std::sqrt(tail_sum + ctail + lead) : std::ldexp(std::sqrt(tail_sum + ctail + lead), E);
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
