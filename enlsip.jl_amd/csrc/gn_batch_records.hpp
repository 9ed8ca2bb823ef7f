// The eleven batched calls on the caller's device buffers (gn_deletion_batched.inc, gn_linesearch_batched.inc,
// gn_penalty_batched.inc, gn_linesearch_fit_batched.inc, gn_addition_batched.inc, gn_termination_batched.inc,
// gn_direction_batched.inc, gn_hessian_batched.inc): the records they upload and download, the checks and the packing of their
// host arguments (the working-set lists among them), and the layouts they place in the handle's one record scratch (DESIGN.md
// 5.7a).  Host-only, nothing of HIP: tests/batch_records_check.cpp runs the shared pieces on the CPU, tests/addition_walk_check.cpp,
// termination_check.cpp, direction_check.cpp and hessian_sums_check.cpp the checks and layouts of their calls.  The kernel headers
// include it for the records.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/enlsip_gn.h"
#include "gn_layout.hpp"

namespace gn {

// ---- records: the kernels read them as they stand; sizes and field offsets are pinned in tests/batch_records_check.cpp ------------
struct DeletionMeta {
    int t, q;        // the problem's constraint count (restore: after the deletion) and its number of equalities
    int take;        // delete: 0 leaves the problem alone
    int s;           // restore: the 1-based row to put back, 0 for none
};

struct LsMeta {
    int n_inactive;     // used entries of the problem's list
    int index_del;      // the row :2166 skips, 0 for none
};

struct LsOut {
    double alpha_upp;
    double sums[3];     // Jp.Jp, Jp.rx, rx.rx
    long long index_alpha_upp;
};

struct PenaltyMeta {
    double sums[3];     // Jp.Jp, Jp.rx, rx.rx as the set-up call returns them
    int t, dimA;
    int take;           // 0 leaves the problem alone
    int pad;
};

struct PenaltyOut {
    double scalars[3];  // dpsi0, psi0, atwa
    int branch;
    int pad;
};

struct MeritMeta {
    int t, n_inactive;
    int take;
    int pad;
};

struct AdditionMeta {
    int t, q;
    int take;               // 0 leaves the problem alone, 1 walk and rebuild, 2 rebuild only
    int index_alpha_upp;    // the constraint the delta arm of :623 looks at, 0 for none
};

struct AdditionOut {
    int t;                  // the count the walk left (take 2: as given)
    int added, status;      // of the walk (gn_violated_constraints.hpp), 0 without one
    int pad;
};

struct TermMeta {
    double psi0;            // enters progress only
    int t, q, dimJ2;
    int take;               // 0 leaves the problem alone
};

struct DirMeta {
    int t, q, dimA, dimJ2;
    int k_prev;             // entries of d under d1_asprev_sq: max(prev_dimJ2 + prev_t - t - 1, 0), at most m
    int take;               // 0 leaves the problem alone (not taken, or status 1)
};

struct HessMeta {
    int t;                  // used entries of the problem's active list; 0 for a problem that is left alone
    int slot;               // the problem's Gamma is at Gamma + slot * strideG; < 0 leaves the problem alone
};

constexpr int LS_SUM_ROWS = 1024;       // rows per partial-sum workgroup until nblk reaches LS_MAX_NBLK
constexpr int LS_MAX_NBLK = 64;         // one partial per lane of the adding wave
constexpr int BATCH_MAX_T = 1024;       // t_max of this build: the LDS copies of the general forms (k_delete_general, PW_MAX_T)

// ---- checks of the host arguments: 0, or the message in err and the code ------------------------------------------------------------
inline int fail(std::string& err, int code, std::string msg) { err = std::move(msg); return code; }

inline int check_batch(std::string& err, int64_t batch) {
    return batch < 1 || batch > 0x7fffffff ? fail(err, -2, "batch must be in 1..2^31-1") : 0;
}
inline int check_l(std::string& err, int64_t l) { return l < 0 || l > (1LL << 27) ? fail(err, -3, "l must be in 0..2^27") : 0; }
inline int check_t_max(std::string& err, int64_t t_max) {
    return t_max < 0 || t_max > BATCH_MAX_T ? fail(err, -3, "t_max must be in 0..1024 in this build") : 0;
}
inline int check_m(std::string& err, int64_t m) { return m < 0 || m > 0x7fffffff ? fail(err, -3, "m must be in 0..2^31-1") : 0; }
inline int check_n(std::string& err, int64_t n) { return n < 1 || n > 0x3fffffff ? fail(err, -3, "n must be at least 1") : 0; }
// t_max in the build's range and no larger than l
inline int check_t_max_in_l(std::string& err, int64_t t_max, int64_t l) {
    const int rc = check_t_max(err, t_max);
    return rc ? rc : t_max > l ? fail(err, -3, "t_max > l") : 0;
}
// the shape of the penalty, merit and fit calls
inline int check_shape(std::string& err, int64_t batch, int64_t l, int64_t t_max) {
    int rc;
    if ((rc = check_batch(err, batch)) || (rc = check_l(err, l))) return rc;
    return check_t_max_in_l(err, t_max, l);
}
// the shape of the calls that take both working-set lists with stride l (addition, termination, direction check), whose general
// forms keep a list in LDS: l is bounded like t_max.  The addition call has no m and passes 0.
inline int check_working_set_shape(std::string& err, int64_t batch, int64_t m, int64_t n, int64_t l, int64_t t_max) {
    int rc;
    if ((rc = check_batch(err, batch)) || (rc = check_m(err, m)) || (rc = check_n(err, n))) return rc;
    if (l < 0 || l > BATCH_MAX_T) return fail(err, -3, "l must be in 0..1024 in this build");
    return check_t_max_in_l(err, t_max, l);
}

struct Range { int64_t lo, hi; const char* text; };     // lo..hi, and what a message calls it ("0..t_max")

// the failing end of the two checks below, "name[k] outside <text>" or with i >= 0 "name[k][i] outside <text>": a function of its
// own so that the checks stay small enough to be inlined into the callers' loops over the batch
inline int outside(std::string& err, int code, const char* name, int64_t k, int64_t i, const char* text) {
    return fail(err, code, std::string(name) + "[" + std::to_string(k) + (i < 0 ? "]" : "][" + std::to_string(i) + "]") + " outside " + text);
}
// v = name[k] of a per-problem count
inline int check_count(std::string& err, int code, const char* name, int64_t k, int64_t v, Range r) {
    return v < r.lo || r.hi < v ? outside(err, code, name, k, -1, r.text) : 0;
}
// row k of a ragged list: its first cnt entries; nothing behind them is read
inline int check_list(std::string& err, int code, const char* name, int64_t k, const int64_t* row, int64_t cnt, Range r) {
    for (int64_t i = 0; i < cnt; ++i)
        if (row[i] < r.lo || r.hi < row[i]) return outside(err, code, name, k, i, r.text);
    return 0;
}

// problem k's working set of the calls above: t active entries, l - t inactive ones, all in 0..l (code -7)
inline int check_working_set(std::string& err, int64_t k, const int64_t* active, const int64_t* inactive, int64_t l, int64_t t) {
    const int rc = check_list(err, -7, "active", k, active + k * l, t, {0, l, "0..l"});
    return rc ? rc : check_list(err, -7, "inactive", k, inactive + k * l, l - t, {0, l, "0..l"});
}

// row k of `stride` ints: the first cnt entries of row k of src, 0 behind them; with cnt == 0 nothing of src is touched
inline void pack_row(int* dst, const int64_t* src, int64_t k, int64_t cnt, int64_t stride) {
    int* to = dst + k * stride;
    const int64_t* from = cnt > 0 ? src + k * stride : nullptr;
    for (int64_t i = 0; i < cnt; ++i) to[i] = (int)from[i];
    std::fill(to + cnt, to + stride, 0);
}
// batch such rows, row k with cnt[k] entries
inline void pack_rows(int* dst, const int64_t* src, const int64_t* cnt, int64_t batch, int64_t stride) {
    for (int64_t k = 0; k < batch; ++k) pack_row(dst, src, k, cnt[k], stride);
}

// A working-set list as the addition, termination and direction calls move it: [active, batch rows of l | inactive, batch rows of
// l].  The two halves of `list`, on either side (T: int in the scratch).
template <class T>
struct WorkingSets {
    T *act, *inact;
    WorkingSets(T* list, int64_t batch, int64_t l) : act(list), inact(list + batch * l) {}
};
// problem k's two rows of it from the caller's arrays: t active entries and l - t inactive ones.  t < 0, a problem that is not
// taken: two zero rows, and nothing of its source rows is read.  (The Hessian sums pack the active half alone: pack_row.)
inline void pack_working_sets(int* list, int64_t batch, int64_t l, int64_t k, const int64_t* active, const int64_t* inactive, int64_t t) {
    const WorkingSets<int> w(list, batch, l);
    pack_row(w.act, active, k, t < 0 ? 0 : t, l);
    pack_row(w.inact, inactive, k, t < 0 ? 0 : l - t, l);
}

inline int take_flag(const int64_t* take, int64_t k) { return (take && take[k] == 0) ? 0 : 1; }     // no array: every problem
// the three kinds of the addition call: 0 nothing, 2 rebuild only, anything else (and no array) walk and rebuild
inline int addition_take(const int64_t* take, int64_t k) { return !take_flag(take, k) ? 0 : (take && take[k] == 2) ? 2 : 1; }

// workgroups per problem of an ordered partial sum over m rows, and whether batch * max(per_problem, 1) workgroups fit a grid
inline int64_t sum_blocks(int64_t m) { return std::min<int64_t>(LS_MAX_NBLK, (m + LS_SUM_ROWS - 1) / LS_SUM_ROWS); }
inline bool grid_fits(int64_t batch, int64_t per_problem) { return batch * std::max<int64_t>(per_problem, 1) <= 0x7fffffff; }

// ---- scratch layouts (gn_layout.hpp) ------------------------------------------------------------------------------------------------
// A call places its layout twice, in its device buffer and in pinned memory, and moves the records by ONE copy up and ONE down.
// That needs the moved arrays at equal offsets on both sides, so they come first and the partial sums, which only the device side
// has (0 per problem in pinned memory), come last.  up_bytes / down_bytes are read off the placed arrays, never from the shape again.
template <class T>
size_t bytes_since(const Carver& c, const T* first) { return c.off - (size_t)((const char*)first - c.base); }

// up [meta | list], down out.  Deletion: no list (stride 0), out = s; set-up: list = inactive, 3 * nblk partial sums; penalty: active
template <class Meta, class Out>
struct RecordScratch {
    Meta* meta = nullptr;
    int* list = nullptr;
    Out* out = nullptr;
    double* part = nullptr;
    size_t up_bytes = 0, down_bytes = 0;
    void carve(Carver& c, int64_t batch, int64_t stride, int64_t part_per_problem) {
        c.take(meta, "meta", (size_t)batch);
        c.take(list, "list", (size_t)batch * (size_t)stride);
        up_bytes = bytes_since(c, meta);
        c.take(out, "out", (size_t)batch, 8);
        down_bytes = bytes_since(c, out);
        c.take(part, "part", (size_t)batch * (size_t)part_per_problem);
    }
};
using DeletionScratch = RecordScratch<DeletionMeta, int>;
using LinesearchScratch = RecordScratch<LsMeta, LsOut>;
using PenaltyScratch = RecordScratch<PenaltyMeta, PenaltyOut>;
// The addition call: list = [active, batch rows of l | inactive, batch rows of l] (stride 2 l), no partial sums.  The kernels edit
// the lists where they are, so what comes down in ONE copy is [list | out]: the two arrays are neighbours on both sides.
using AdditionScratch = RecordScratch<AdditionMeta, AdditionOut>;
inline size_t addition_down_bytes(const AdditionScratch& s, int64_t batch) {
    return (size_t)((const char*)(s.out + batch) - (const char*)s.list);
}

// ---- the addition call's checks of its host arguments (the codes of include/enlsip_gn.h); the pointers only as "is it there" -------
struct AdditionShape { int64_t batch, n, l, t_max, lda, strideA, ldat, strideAt; };
inline int check_addition(std::string& err, const AdditionShape& s, const int64_t* q, const int64_t* t, const int64_t* active,
                          const int64_t* inactive, const int64_t* index_alpha_upp, const int64_t* take, bool host_outputs,
                          bool device_inputs, bool device_outputs) {
    int rc;
    if ((rc = check_working_set_shape(err, s.batch, 0, s.n, s.l, s.t_max))) return rc;
    if (!q || !t || !host_outputs) return fail(err, -4, "q, t, added and status are host arrays of batch entries");
    if (s.l > 0 && (!active || !inactive)) return fail(err, -4, "active and inactive are host arrays of batch x l entries");
    if (s.t_max > 0 && (!device_inputs || !device_outputs))
        return fail(err, -4, "dA, dcx_all, dAt, dcx and ddiag_scale are required when t_max > 0");
    const int64_t bnd = std::min(s.l, s.n);
    for (int64_t k = 0; k < s.batch; ++k) {      // per problem: the lower k wins; nothing of a problem that is not taken is read
        const int tk = addition_take(take, k);
        if (!tk) continue;
        if ((rc = check_count(err, -5, "t", k, t[k], {0, s.t_max, "0..t_max"}))) return rc;
        if (tk == 1 && std::max(t[k], bnd) > s.t_max)
            return fail(err, -5, "t_max < max(t[" + std::to_string(k) + "], min(l, n)): the walk of problem " + std::to_string(k) +
                                     " could outgrow its slot");
        if ((rc = check_count(err, -6, "q", k, q[k], {0, t[k], "0..t[k]"})) ||
            (rc = check_working_set(err, k, active, inactive, s.l, t[k])) ||
            (index_alpha_upp && (rc = check_count(err, -7, "index_alpha_upp", k, index_alpha_upp[k], {0, s.l, "0..l"})))) return rc;
    }
    if (s.lda < s.l) return fail(err, -9, "lda < l");
    if (s.ldat < s.n) return fail(err, -9, "ldat < n");
    if (s.strideA < s.lda * s.n) return fail(err, -10, "strideA < lda * n");
    if (s.strideAt < s.ldat * s.t_max) return fail(err, -10, "strideAt < ldat * t_max");
    return 0;
}

// ---- the termination call: list = [active | inactive] as the addition call's, out = the sums as the header declares them, and the
// general form's nblk partial sums of rx.rx per problem.  Its checks (the codes of include/enlsip_gn.h) -------------------------------
using TerminationScratch = RecordScratch<TermMeta, enlsip_gn_term_sums>;
struct TerminationShape { int64_t batch, m, n, l, t_max, ldj, strideJ, ldat, strideAt; };
inline int check_termination(std::string& err, const TerminationShape& s, const enlsip_gn_term_state* state, const int64_t* active,
                             const int64_t* inactive, const int64_t* take, bool host_rest, bool dev_m, bool dev_l, bool dev_t,
                             bool dev_n) {
    int rc;
    if ((rc = check_working_set_shape(err, s.batch, s.m, s.n, s.l, s.t_max))) return rc;
    if (!state || !host_rest) return fail(err, -4, "state, tol, sums and exit_code are required");
    if (s.l > 0 && (!active || !inactive)) return fail(err, -4, "active and inactive are host arrays of batch x l entries");
    if (s.m > 0 && !dev_m) return fail(err, -4, "dJ and drx are required when m > 0");
    if (s.l > 0 && !dev_l) return fail(err, -4, "dcx_all and dw are required when l > 0");
    if (s.t_max > 0 && !dev_t) return fail(err, -4, "dlambda, dcx_active, ddiag_scale and dAt are required when t_max > 0");
    if (!dev_n) return fail(err, -4, "dx, dx_prev, dp, dd_gn and dgrad are required");
    for (int64_t k = 0; k < s.batch; ++k) {      // per problem: the lower k wins; nothing of a problem that is not taken is read
        if (!take_flag(take, k)) continue;
        const enlsip_gn_term_state& st = state[k];
        if ((rc = check_count(err, -5, "state.t", k, st.t, {0, s.t_max, "0..t_max"})) ||
            (rc = check_count(err, -5, "state.l", k, st.l, {s.l, s.l, "l"})) ||
            (rc = check_count(err, -6, "state.q", k, st.q, {0, st.t, "0..t[k]"})) ||
            (rc = check_working_set(err, k, active, inactive, s.l, st.t)) ||
            (rc = check_count(err, -8, "state.dimJ2", k, st.dimJ2, {0, s.n, "0..n"}))) return rc;
    }
    if (s.ldj < s.m) return fail(err, -9, "ldj < m");
    if (s.ldat < s.n) return fail(err, -9, "ldat < n");
    if (s.strideJ < s.ldj * s.n) return fail(err, -10, "strideJ < ldj * n");
    if (s.strideAt < s.ldat * s.t_max) return fail(err, -10, "strideAt < ldat * t_max");
    return 0;
}

// ---- the direction check: list = [active | inactive] as the termination call's, out = the sums as the header declares them, no
// partial sums.  Its checks (the codes of include/enlsip_gn.h; tests/direction_check.cpp runs them on the CPU) ------------------------
using DirectionScratch = RecordScratch<DirMeta, enlsip_gn_dir_sums>;
struct DirectionShape { int64_t batch, m, n, l, t_max; };
constexpr int64_t DIR_PREV_MAX = 1LL << 31;      // |prev_dimJ2| (a Newton step leaves t - n there): k_prev cannot overflow
inline int check_direction(std::string& err, const DirectionShape& s, const enlsip_gn_dir_state* state, const int64_t* active,
                           const int64_t* inactive, const int64_t* take, bool host_rest, bool dev_m, bool dev_l, bool dev_t) {
    int rc;
    if ((rc = check_working_set_shape(err, s.batch, s.m, s.n, s.l, s.t_max))) return rc;
    if (!state || !host_rest) return fail(err, -4, "state, sums, method_code, beta and status are required");
    if (s.l > 0 && (!active || !inactive)) return fail(err, -4, "active and inactive are host arrays of batch x l entries");
    if (s.m > 0 && !dev_m) return fail(err, -4, "dd is required when m > 0");
    if (s.l > 0 && !dev_l) return fail(err, -4, "dcx_all is required when l > 0");
    if (s.t_max > 0 && !dev_t) return fail(err, -4, "db, dlambda and ddiag_scale are required when t_max > 0");
    for (int64_t k = 0; k < s.batch; ++k) {      // per problem: the lower k wins; nothing of a problem that is not taken is read
        if (!take_flag(take, k)) continue;
        const enlsip_gn_dir_state& st = state[k];
        if ((rc = check_count(err, -5, "state.t", k, st.t, {0, s.t_max, "0..t_max"})) ||
            (rc = check_count(err, -5, "state.l", k, st.l, {s.l, s.l, "l"})) ||
            (rc = check_count(err, -6, "state.q", k, st.q, {0, st.t, "0..t[k]"})) ||
            (rc = check_working_set(err, k, active, inactive, s.l, st.t)) ||
            (rc = check_count(err, -8, "state.dimA", k, st.dimA, {0, st.t, "0..t[k]"})) ||
            (rc = check_count(err, -8, "state.dimJ2", k, st.dimJ2, {0, s.m, "0..m"})) ||
            (rc = check_count(err, -8, "state.prev_t", k, st.prev_t, {0, s.l, "0..l"})) ||
            (rc = check_count(err, -8, "state.prev_dimJ2", k, st.prev_dimJ2, {-DIR_PREV_MAX, DIR_PREV_MAX, "-2^31..2^31"}))) return rc;
    }
    return 0;
}

// ---- the Hessian sums: up [meta | active], nothing down, no partial sums.  Its checks and those of the points call (the codes of
// include/enlsip_gn.h; tests/hessian_sums_check.cpp runs them on the CPU) ------------------------------------------------------------
struct HessianScratch {
    HessMeta* meta = nullptr;
    int* list = nullptr;
    size_t up_bytes = 0;
    void carve(Carver& c, int64_t count, int64_t l, int64_t) {
        c.take(meta, "meta", (size_t)count);
        c.take(list, "list", (size_t)count * (size_t)l);
        up_bytes = bytes_since(c, meta);
    }
};
constexpr int64_t HESS_MAX_ELEMS = 1LL << 48;      // doubles of one evaluation or point buffer: every index stays far inside int64
// the pair range [pair0, pair0 + npairs) inside the triangle of n, and count x npairs x 4 x width doubles addressable
inline int check_hessian_range(std::string& err, int64_t count, int64_t n, int64_t pair0, int64_t npairs, int64_t width) {
    if (count < 1 || count > 0x7fffffff) return fail(err, -2, "count must be in 1..2^31-1");
    if (n < 1 || n > 0x7fffffff) return fail(err, -2, "n must be in 1..2^31-1");
    if (npairs < 1 || pair0 < 0) return fail(err, -2, "npairs must be at least 1 and pair0 at least 0");
    const int64_t pairs = n * (n + 1) / 2;
    if (pair0 > pairs || npairs > pairs - pair0) return fail(err, -2, "pair0 + npairs > n (n + 1) / 2");
    if (width > 0 && npairs > HESS_MAX_ELEMS / 4 / width / count) return fail(err, -2, "count x npairs x 4 x row length beyond 2^48 doubles");
    return 0;
}
inline int check_hessian_points(std::string& err, int64_t count, int64_t n, int64_t pair0, int64_t npairs, bool x, bool X) {
    int rc;
    if ((rc = check_hessian_range(err, count, n, pair0, npairs, n))) return rc;
    return !x || !X ? fail(err, -4, "x and X are required") : 0;
}
struct HessianShape { int64_t count, m, n, l, t_max, pair0, npairs, ldg, strideG; };
inline int check_hessian_sums(std::string& err, const HessianShape& s, const int64_t* t, const int64_t* active, const int64_t* slot,
                              bool x, bool F, bool rx, bool G, bool lambda, bool Gamma) {
    int rc;
    if (s.m < 0 || s.m > 0x7fffffff) return fail(err, -2, "m must be in 0..2^31-1");      // -2 here, not check_m's -3
    if (s.l < 0 || s.l > (1LL << 27) || s.t_max < 0 || s.t_max > 0x7fffffff) return fail(err, -2, "l must be in 0..2^27 and t_max in 0..2^31-1");
    if ((rc = check_hessian_range(err, s.count, s.n, s.pair0, s.npairs, std::max(s.m, s.l)))) return rc;
    const int64_t t_top = std::min(s.l, s.t_max);
    if (!t || !x || !Gamma) return fail(err, -4, "t, x and Gamma are required");
    if (s.m > 0 && (!F || !rx)) return fail(err, -4, "F and rx are required when m > 0");
    for (int64_t k = 0; k < s.count; ++k)        // nothing of a problem with slot[k] < 0 is read
        if (!(slot && slot[k] < 0) && t[k] > 0 && (!active || !G || !lambda))
            return fail(err, -4, "active, G and lambda are required when some t[k] > 0");
    for (int64_t k = 0; k < s.count; ++k) {      // the lower k wins
        if (slot && slot[k] < 0) continue;
        if ((rc = check_count(err, -5, "t", k, t[k], {0, t_top, "0..min(l, t_max)"})) ||
            (t[k] > 0 && (rc = check_list(err, -5, "active", k, active + k * s.l, t[k], {0, s.l, "0..l"}))) ||
            (slot && (rc = check_count(err, -5, "slot", k, slot[k], {0, 0x7fffffff, "below 2^31"})))) return rc;
    }
    if (s.ldg < s.n) return fail(err, -5, "ldg < n");
    if (s.ldg > INT64_MAX / s.n || s.strideG < s.ldg * s.n) return fail(err, -5, "strideG < ldg * n");
    if (slot) {
        std::vector<int64_t> used;
        for (int64_t k = 0; k < s.count; ++k)
            if (slot[k] >= 0) used.push_back(slot[k]);
        std::sort(used.begin(), used.end());
        if (std::adjacent_find(used.begin(), used.end()) != used.end()) return fail(err, -5, "two problems share a slot");
    }
    return 0;
}

// The merit call and, with fit, the polynomial fit: up [meta | act | inact | alpha], down [sums | psi] (a fit without psi_new
// leaves the last psi_bytes of it where they are); the partial sums of the fit (6 * nblk per problem) and of the merit kernels
// (nblk) stay on the device.  alpha, sums and part exist with fit only.
struct MeritScratch {
    MeritMeta* meta = nullptr;
    int *act = nullptr, *inact = nullptr;
    double *alpha = nullptr, *sums = nullptr, *psi = nullptr, *part = nullptr, *mpart = nullptr;
    size_t up_bytes = 0, down_bytes = 0, psi_bytes = 0;
    void carve(Carver& c, int64_t batch, int64_t t_max, int64_t l, bool fit, int64_t nblk) {
        c.take(meta, "meta", (size_t)batch, 8);
        c.take(act, "act", (size_t)batch * (size_t)t_max);
        c.take(inact, "inact", (size_t)batch * (size_t)l);
        if (fit) c.take(alpha, "alpha", (size_t)batch);
        up_bytes = bytes_since(c, meta);
        if (fit) c.take(sums, "sums", (size_t)batch * 6);
        c.take(psi, "psi", (size_t)batch);
        psi_bytes = bytes_since(c, psi);
        down_bytes = fit ? bytes_since(c, sums) : psi_bytes;
        if (fit) c.take(part, "part", (size_t)batch * (size_t)nblk * 6);
        c.take(mpart, "mpart", (size_t)batch * (size_t)nblk);
    }
};

}  // namespace gn
