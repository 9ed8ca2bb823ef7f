// Host-side state behind an enlsip_gn_handle: shape plan, device workspace carve, stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/enlsip_gn.h"
#include "gn_device_utils.hpp"
#include "gn_plan.hpp"

namespace gn {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// pinned host memory that a call sizes for itself (grow_pinned): the host end of its asynchronous copies
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
};

// The device scalars of a handle (WsLayout::small, 256 bytes of the main workspace): results of single-number reductions that the
// host reads back or a following kernel accumulates into.  The members keep the 128-byte lines they were measured on.
struct SmallScalars {
    unsigned char unused0[32];
    double tail_sum;                 // tail sum of squares of a TSQR stage (k_tsqr_extract, k_sumsq)
    double unused1;
    double tails[4];                 // k_tsqr_unpack: tail^2, the n2 check, the rank tags, E
    unsigned char unused2[48];
    // largest-magnitude bit patterns: J, A' (extreme_shifts: two words) or J, rx, A' (tsqr_shifts: three).  Shared on purpose: both
    // run on the handle's one stream, each reads its words back and synchronises before it returns, so they never run concurrently.
    unsigned long long amax[3];
    unsigned long long unused3;
    unsigned long long flag_acc[2];  // accumulator of k_tsqr_flags (it leaves it zero itself)
    unsigned sum_count;              // arrival counter of ordered_sumsq
    unsigned char unused4[76];
};
static_assert(sizeof(SmallScalars) == PLAN_SMALL_BYTES && sizeof(ProbState) == PLAN_STATE_BYTES, "gn_plan.hpp sizes the workspace with these");

// The operands of one batched solve: shape, inputs, outputs (device pointers, or host pointers before solve_host stages them).
// Problem k's part of each array starts at a fixed stride, and slice() is the one place that knows them: J, A' by strideJ,
// strideAt; rx, d by m; p, jpvtJ2 by n; cx, b, jpvtA by t (t_max of a ragged batch); jpvtL by min(n, t); the info records and
// tk by 1.  A null pointer is an absent operand and stays null.
struct BatchOperands {
    long long batch = 0, m = 0, n = 0, t = 0;
    const double* J = nullptr; long long ldj = 0, strideJ = 0;
    const double* rx = nullptr;
    const double* At = nullptr; long long ldat = 0, strideAt = 0;
    const double* cx = nullptr;
    double *p = nullptr, *b = nullptr, *d = nullptr;
    enlsip_gn_info* dinfo = nullptr;    // device info records
    long long *jpvtA = nullptr, *jpvtL = nullptr, *jpvtJ2 = nullptr;
    enlsip_gn_info* hinfo = nullptr;    // host info records
    const int* tk = nullptr;            // ragged batch: each problem's own t (host)

    BatchOperands slice(long long k0, long long count) const {
        auto at = [k0](auto* x, long long stride) { return x ? x + k0 * stride : nullptr; };
        BatchOperands s = *this;
        s.batch = count;
        s.J = at(J, strideJ); s.rx = at(rx, m); s.At = at(At, strideAt); s.cx = at(cx, t);
        s.p = at(p, n); s.b = at(b, t); s.d = at(d, m); s.dinfo = at(dinfo, 1);
        s.jpvtA = at(jpvtA, t); s.jpvtL = at(jpvtL, std::min(n, t)); s.jpvtJ2 = at(jpvtJ2, n);
        s.hinfo = at(hinfo, 1); s.tk = at(tk, 1);
        return s;
    }
    // what a handle keeps of its last solve: shape and inputs, no output or host array of the caller
    BatchOperands inputs() const { return {batch, m, n, t, J, ldj, strideJ, rx, At, ldat, strideAt, cx}; }
};

// What kind of solve one pass through the solve driver is (solve_host -> solve_chunked -> solve_launchable -> solve_dev), by value:
// nothing about it is kept on a handle.
struct SolveMode {
    enum Kind { Fresh, Factored, Changed } kind = Fresh;
    //   Fresh:    constraint stage and Jacobian side for every problem
    //   Factored: the constraint stage is resident; it is run again for the flagged problems, the Jacobian side for all
    //   Changed:  flagged problems only, both sides, into their own slots
    const int64_t* flags = nullptr;   // whole-batch refactor / changed flags (host), sliced with the operands; NULL: none
    bool upper_input = false;         // J is one gathered triangle (one-rank TSQR combine): upper triangular, no CAQR needed
    long long dimA_ov = -1, dimJ2_ov = -1;
    double eps_rank = 0.0;
    int abs_shift = 0;                // J, rx arrive scaled by 2^abs_shift (TSQR combine of rescaled shards): the absolute rank test follows

    // the mode of the problems from k0 on: goes with BatchOperands::slice(k0, count)
    SolveMode part(long long k0) const {
        SolveMode s = *this;
        if (flags) s.flags = flags + k0;
        return s;
    }
    // a rescaled problem on its rescue handle: solved whole, with the caller's truncation dimensions and threshold
    SolveMode fresh() const { return {Fresh, nullptr, false, dimA_ov, dimJ2_ov, eps_rank, abs_shift}; }
};

// the families whose last kernel form a handle records (enlsip_gn_context::form)
enum Form { FORM_CONSUMER, FORM_RESOLVE, FORM_NEWTON, FORM_SUBSPACE, FORM_DELETION, FORM_LINESEARCH, FORM_PENALTY, FORM_ADDITION,
            FORM_TERMINATION, FORM_DIRECTION, FORM_COUNT };

}  // namespace gn

struct enlsip_gn_context : gn::WsLayout {      // h->W, h->FA, ... : the placed main workspace
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int flags = 0;
    int tile_rows = 512;
    std::string err;
    gn::Plan plan;
    bool have_plan = false;
    bool factors_valid = false;
    gn::DevBuf cws;                      // workspace of the distributed constraint stage (many constraints)
    struct {                             // what the re-solve needs of it: unfactored L11 and F_L11.Q' b_buff of the last solve
        const double* L = nullptr; long long ldL = 0, sL = 0;
        const double* qb = nullptr; long long sQb = 0;
        bool valid = false;
    } cdist;
    bool trace = false;              // ENLSIP_GN_TRACE=1: stage names on stderr with a stream synchronisation after each (fault hunting)
    bool constraints_only = false;   // resident: F_A, F_L11 only (enlsip_gn_factor_constraints); everything about J is absent
    double eps_rank = 0.0;

    gn::DevBuf ws;                   // the main workspace: one allocation, placed by WsLayout
    // row counts the blocks of the previous blocked QRCP started with (min / max over the problems, by block id), valid for
    // sb_rows_kp == kp_launch and the same batch: which forms of the select / factor kernel a block id needs
    std::vector<int> sb_rows_min, sb_rows_max;
    int sb_rows_kp = -1;
    long long sb_rows_batch = -1;
    gn::DevBuf sb_stat;          // device statistics (2 x SB_STAT_BLKS ints)
    int* h_sb_stat = nullptr;    // pinned mirror
    bool sb_form_hints = true;   // ENLSIP_GN_SB_FORM_HINTS=0: every block id in all three forms (A/B)
    bool qrcp_hybrid = true;     // pivoted QR of more than 512 rows: launch-per-step head, register blocks for the last 512 (ENLSIP_GN_QRCP_HYBRID=0: A/B)
    int sb_hint = 0;             // blocks the previous blocked QRCP needed (+1): size of the first launch chunk
    void* h_sbinfo = nullptr;    // pinned mirror of sbInfo
    int cu_count = 256;
    enlsip_gn_context* sub = nullptr;   // handle for the stacked problem of the TSQR combine stage
    // Two-stream pipelining of large batches (enlsip_gn_solve_batched_dev): the second half of the problems runs on
    // a child handle (own stream + workspace) driven by a host thread, so the latency-bound kernels of one half
    // overlap the bandwidth-bound kernels of the other.  Accessors route a problem index to the half that owns it.
    enlsip_gn_context* child = nullptr;
    bool pair_forced = false;           // ENLSIP_GN_PAIR=1: pairs for every shape with three panels or more
    bool lookahead_forced = false;
    bool lookahead = true;              // ENLSIP_GN_LOOKAHEAD=0: chain-bound pair sweeps on one stream
    hipStream_t stream2 = nullptr;      // second stream of the look-ahead sweep (the bulk of a pair's far update)
    std::vector<hipEvent_t> la_events;
    bool fuse_small = true;             // ENLSIP_GN_FUSE_SMALL=0: two launches for J*Q1 + panel factorisation of one-tile problems
    bool pair_enabled = true;           // ENLSIP_GN_PAIR=0: one panel per pass over the trailing matrix
    bool pipeline = true;               // ENLSIP_GN_PIPELINE=0 disables
    bool pipeline_forced = false;   // ENLSIP_GN_PIPELINE=1
    long long pipeline_min = 128;       // smallest batch that is split
    long long split = 0;                // problems [split, batch) of the last solve live on `child` (0: not split)
    hipEvent_t ev_fork = nullptr;
    // Rescale path (gn_rescale.hpp): the resident problem of a one-problem solve whose inputs were beyond the range of plain sums
    // of squares was solved on copies scaled by 2^sc_eJ (J, rx) / 2^sc_eA (A', cx), kept in rs_buf for the entry points that run the
    // constraint stage again (re-solve, Newton); the resident factors are scaled back, i.e. they are those of the caller's data.
    // In a batch such a problem is handed to a one-problem rescue handle of its own, to which the accessors are routed.
    int sc_eJ = 0, sc_eA = 0;
    gn::DevBuf rs_buf;
    double *rs_J = nullptr, *rs_rx = nullptr, *rs_At = nullptr, *rs_cx = nullptr;
    bool rescale_enabled = true;        // ENLSIP_GN_RESCALE=0: detection and rescaling off (A/B; tests)
    bool is_rescue = false;
    std::vector<enlsip_gn_context*> rescue;     // one-problem handles of rescaled problems of the last batch
    std::vector<long long> rescue_prob;          // their problem indices (same length while the batch is resident)
    // Ragged batch (enlsip_gn_solve_batched_ragged*): each problem's own constraint count (plan.t = t_max); empty after a uniform
    // solve.  The device copy is what the RAGGED forms of the constraint kernels read; the host copy answers the accessors.
    std::vector<int> h_tk;
    gn::DevBuf tkbuf;
    // Batched constraint stage (enlsip_gn_factor_constraints_batched*) and the solve that goes on with it
    // (enlsip_gn_solve_factored_batched*).  On the handle the caller holds: what the constraint call was made with, so that the solve
    // can tell whether it follows it — shape, pipeline split, each problem's t, the input buffers (device form: the caller's; host
    // form: the staging area).  On every handle that runs a part (parent, pipeline child): the number of problems the constraint
    // kernels of its last call were launched over.
    struct {
        bool valid = false, host = false;
        long long batch = 0, m = 0, n = 0, t = 0, split = 0;
        const double* At = nullptr; long long ldat = 0, strideAt = 0;
        const double* cx = nullptr;
        std::vector<int> tk;
    } fb;
    // The flagged problems of the part a Factored / Changed solve_dev is running on this handle (indices in its part), built by
    // that solve_dev from its SolveMode's flags, and the device copy of the list.  Nothing fills them on behalf of a later call.
    std::vector<int> refit;
    gn::DevBuf plist_buf;
    gn::DevBuf info_stage;              // a changed-problems solve: the listed problems' info records in list order, before their scatter
    long long cstage_problems = 0;
    // Changed-problems solve (enlsip_gn_solve_changed_batched*): solve_dev redoes the problems of `refit` only, constraint stage AND
    // Jacobian side, from the resident J, rx.  run_plist / run_nlist are the launch set of the solve IN PROGRESS: the device list
    // every Jacobian-side launch is sized by (the launch helpers read it through launch_count).  They are set in exactly one place,
    // the constraint step of a Changed solve_dev, and cleared by that solve_dev's scope guard: NULL outside of it (the whole part).
    // jstage_problems counts the problems the Jacobian-side kernels of the last solve_dev were launched over
    // (enlsip_gn_get_jacobian_resolved sums the halves).
    const int* run_plist = nullptr;
    long long run_nlist = 0;
    long long jstage_problems = 0;
    long long constraint_refactored = 0;   // ... summed over the handles (enlsip_gn_get_constraint_refactored)
    unsigned long long route = 0;       // ENLSIP_GN_ROUTE_* bits of the last solve (enlsip_gn_get_route)
    long long chunk0 = 0;               // first problem (index in the caller's batch) of the resident chunk: batches above the launch limit run in chunks
    long long tsqr_n2 = -1;             // n2 of the last tsqr_local on this handle
    // exponents of the last TSQR call: the resident local stage is that of the shard times 2^-tsqr_e (0: not rescaled), the
    // combine ran on the stacked blocks times 2^-tsqr_E (the largest exponent among the ranks)
    int tsqr_e = 0, tsqr_E = 0;
    // communicator of enlsip_gn_solve_tsqr: an RCCL communicator (created here or handed in) or the caller's all-gather
    void* tsqr_comm = nullptr;
    bool tsqr_comm_owned = false;
    enlsip_gn_allgather_fn tsqr_xfn = nullptr;
    void* tsqr_xctx = nullptr;
    int tsqr_ranks = 1, tsqr_rank = 0;
    bool tsqr_broken = false;           // enlsip_gn_tsqr_init_rccl failed: enlsip_gn_solve_tsqr refuses until a communicator is set again
    int tsqr_tags_seen = -1;            // gathered messages of the last enlsip_gn_solve_tsqr whose header carried the rank of their slot
    int tsqr_transport = 0;             // what moved the triangles in the last enlsip_gn_solve_tsqr (ENLSIP_GN_TRANSPORT_*)
    gn::DevBuf xbuf;                    // send message + G received messages
    gn::DevBuf tsqr_part;               // per-workgroup partial sums of the TSQR stages' ordered sums of squares
    // What of a row shard is resident (beside factors_valid, which stays false for a shard): 0 nothing, 1 the local stage of
    // this handle's last tsqr_local, 2 local stage AND combine (enlsip_gn_solve_tsqr, enlsip_gn_tsqr_combine(_scaled)_dev): F_A,
    // tauA, the pivots of A' and `last` are those of the shard — what the enlsip_gn_tsqr_products family needs.  Every other
    // solve entry sets it back to 0.
    int tsqr_stage = 0;
    gn::DevBuf tsqr_prod;               // scratch and messages of the enlsip_gn_tsqr_products family
    float tsqr_ms[3] = {};              // local / exchange / combine of the last enlsip_gn_solve_tsqr (profiling on)
    // staging for the host-pointer API
    gn::DevBuf in_stage, out_stage, scratch, lag, newton;
    // batched consumers (gn_lagrange_batched.inc): staging of the host-buffer forms, device temporaries, pinned "some problem
    // flagged" word of the last launch; never a buffer the resident solve reads
    gn::DevBuf lagb_io, lagb_scr;
    gn::PinnedBuf h_lagflag;
    bool lagrange_small = true;         // ENLSIP_GN_LAGRANGE_SMALL=0: batched multiplier estimates in the general form only (A/B)
    // batched re-solve (gn_resolve_batched.inc): per-slot requests on the device, staging of the host-buffer form, and per
    // resident problem the (code, dimA) of a held call whose p1 and Q3' d_temp are still in p1 / vec (code 0: none)
    gn::DevBuf rsb_dims, rsb_io;
    hipEvent_t rsb_ev[2] = {};          // profiling on: around the Q0' launches of the last batched re-solve on this handle
    bool rsb_timed = false;
    float resolve_q0_ms = 0.f;          // ... summed over the handles that ran a part of the range
    struct Held { int code = 0, dimA = 0; };
    std::vector<Held> held;
    // batched Newton direction (gn_newton_batched.inc): device temporaries of a segment, staging of the host-buffer form, HIP
    // events around its four stages (profiling on) and their times summed over the handles that ran a part
    gn::DevBuf nwb_ws, nwb_io;
    gn::PinnedBuf h_nwflag;             // pinned "some slot flagged" word of the last launch on this handle
    hipEvent_t nwb_ev[5] = {};
    bool nwb_timed = false;
    float newton_ms[4] = {};
    // Newton direction on a row shard (gn_tsqr_newton.inc): the call's temporaries and the staging of its host form; the form of
    // its factorisation, ENLSIP_GN_NEWTON_WIDE=0 never / =1 always the device-wide one (default: from an n2 threshold on)
    gn::DevBuf tnw_ws, tnw_io;
    bool newton_wide = true, newton_wide_forced = false;
    // one-call subspace minimisation (gn_subspace_batched.inc): requests and previous iterates on the device, staging of the
    // host-buffer form and the pinned copy of the final requests (chosen dimensions, status)
    gn::DevBuf ssb_req, ssb_io;
    gn::PinnedBuf h_ssb;
    // The one record scratch of the eleven calls on the caller's device buffers (gn_batch_records.hpp): delete and
    // restore, line-search set-up, penalty weights, merit, fit, additions, termination test, direction check, Hessian sums (the
    // Hessian points need none).  A device buffer and its pinned mirror, grown and never shrunk, shared on this invariant: every
    // such call places its own layout at its start (place_records), nothing in the scratch is read before the call has written
    // it, and the call synchronises h->stream before it returns (round_trip).  So nothing in it outlives a call and nothing of
    // the resident state is in it.
    gn::DevBuf rec_scr;
    gn::PinnedBuf h_rec;
    // the kernel form the last call of each family took (1 wave / small, 0 general; the enlsip_gn_get_*_form getters), -1: none yet
    int form[gn::FORM_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    static_assert(gn::FORM_COUNT == 10, "one -1 per family in the initialiser of form");
    gn::ProbState* h_state = nullptr;   // pinned
    size_t h_state_cap = 0;
    // device-pointer inputs of the last solve (resolve, Newton direction, J*Q1, gradient, multiplier estimates)
    gn::BatchOperands last;

    // profiling
    bool profiling = false;
    bool profile_all_updates = false;   // enlsip_gn_set_profiling(h, 2): events around EVERY trailing-update launch (hundreds in a C4 sweep)
    hipEvent_t ev[8] = {};
    bool ev_ready = false;
    float stage_ms[ENLSIP_GN_STAGE_COUNT] = {};
    std::vector<hipEvent_t> upd_ev;   // pairs around level-0 update launches
    size_t upd_used = 0;
    double upd_bytes = 0.0;
    std::vector<double> upd_launch_bytes;   // per timed launch, same order as the event pairs
    std::vector<float> upd_launch_ms;
    float upd_avg_ms = 0.f;
    long long upd_launches = 0;
    // every OTHER trailing-update launch of the sweep (tree levels, a pair's second-panel columns): event pairs, summed time
    std::vector<hipEvent_t> oth_ev;
    size_t oth_used = 0;
    float oth_ms = 0.f;
    long long oth_launches = 0;
    double upd_all_bytes = 0.0;             // SURVEY 8d bytes of EVERY panel of the sweep on ALL its trailing columns
};

namespace gn {

// The run-time switches of a handle: every environment variable the library reads when a handle is created (helper, child, rescue
// and sub handles are created the same way and read them again), but for ENLSIP_GN_RCCL_LIB, which names a file (gn_tsqr.inc).
// One row per (variable, value): a value whose first character is `value` stores `set` in `field`; value 0 = the variable is set
// at all.  README.md lists the switches from this table.
struct EnvSwitch {
    const char* name;
    char value;
    bool enlsip_gn_context::*field;
    bool set;
};
inline constexpr EnvSwitch ENV_SWITCHES[] = {
    {"ENLSIP_GN_TRACE", 0, &enlsip_gn_context::trace, true},                     // stage names on stderr, a synchronisation after each
    {"ENLSIP_GN_PAIR", '0', &enlsip_gn_context::pair_enabled, false},            // plain sweep: one panel per pass over the trailing matrix
    {"ENLSIP_GN_PAIR", '1', &enlsip_gn_context::pair_forced, true},              // pairs for every shape with three panels or more
    {"ENLSIP_GN_PAIR", '2', &enlsip_gn_context::pair_forced, true},              // (once an A/B form of the far update: now the same as 1)
    {"ENLSIP_GN_LOOKAHEAD", '0', &enlsip_gn_context::lookahead, false},          // the pair sweep on one stream
    {"ENLSIP_GN_LOOKAHEAD", '1', &enlsip_gn_context::lookahead_forced, true},    // look-ahead in every sweep, the plain one too (tests)
    {"ENLSIP_GN_FUSE_SMALL", '0', &enlsip_gn_context::fuse_small, false},        // J*Q1 and the one-tile panel factorisation as two launches
    {"ENLSIP_GN_SB_FORM_HINTS", '0', &enlsip_gn_context::sb_form_hints, false},  // every block of the blocked pivoted QR in all of its forms
    {"ENLSIP_GN_QRCP_HYBRID", '0', &enlsip_gn_context::qrcp_hybrid, false},      // more than 512 rows: one launch per pivot step to the end
    {"ENLSIP_GN_RESCALE", '0', &enlsip_gn_context::rescale_enabled, false},      // no detection / rescaling of magnitudes beyond plain sums of squares
    {"ENLSIP_GN_PIPELINE", '0', &enlsip_gn_context::pipeline, false},            // never split a batch over two streams
    {"ENLSIP_GN_PIPELINE", '1', &enlsip_gn_context::pipeline_forced, true},      // split even the small uniform shapes
    {"ENLSIP_GN_LAGRANGE_SMALL", '0', &enlsip_gn_context::lagrange_small, false},  // batched multiplier estimates always in the general form
    {"ENLSIP_GN_NEWTON_WIDE", '0', &enlsip_gn_context::newton_wide, false},        // sharded Newton direction: never the device-wide Cholesky
    {"ENLSIP_GN_NEWTON_WIDE", '1', &enlsip_gn_context::newton_wide_forced, true},  // ... always
};

inline void read_env_switches(enlsip_gn_context* h) {
    for (const EnvSwitch& sw : ENV_SWITCHES) {
        const char* v = getenv(sw.name);
        if (v && (sw.value == 0 || v[0] == sw.value)) h->*sw.field = sw.set;
    }
}

}  // namespace gn
