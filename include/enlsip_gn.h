/*
 * enlsip_gn.h — C ABI of libenlsip_gn.so: the Gauss-Newton search-direction subproblem of
 * Enlsip.jl as MI355X-native (gfx950) HIP kernels.
 *
 * Drop-in boundary.  The reference has no FFI; the seam is two internal Julia
 * functions, and every entry point below names the reference lines it replaces
 * (paths relative to the Enlsip.jl repository):
 *
 *   enlsip_gn_solve*            gn_search_direction   src/enlsip_functions.jl:206-234
 *                               sub_search_direction  src/enlsip_functions.jl:116-153
 *                               + the QR / rank lines of update_working_set
 *                                                     src/enlsip_functions.jl:700, 768-769
 *                               pseudo_rank           src/enlsip_functions.jl:17-31
 *   enlsip_gn_solve_batched_ragged*   the same per problem with its own working-set size W.t
 *                               update_working_set    src/enlsip_functions.jl:686-795 (:725, :743, :762, :771, :789)
 *   enlsip_gn_resolve           sub_search_direction re-entry with truncated dimA/dimJ2
 *                                                     src/enlsip_functions.jl:1249-1253
 *   enlsip_gn_get_R / _diagR / _jpvt / _apply_qt / _apply_q / _get_JQ1
 *                               the QRPivoted accessors (.R, .p, .Q', .Q) and J*F_A.Q that
 *                               first/second_lagrange_mult_estimate!, search_direction_analys,
 *                               choose_subspace_dimensions, determine_solving_dim consume
 *                                                     src/enlsip_functions.jl:461-537, 1118-1291
 *   enlsip_gn_newton_direction  newton_search_direction after its Hessian sums    src/enlsip_functions.jl:348-423
 *   enlsip_gn_newton_direction_batched  the same for a range of the resident batch  src/enlsip_functions.jl:371-421
 *   enlsip_gn_solve_tsqr        (new design, no reference counterpart) the same subproblem with the ROWS of one
 *                               tall J sharded over the GPUs of a node: `JQ1 = J * F_A.Q` ... `qr(J2, ColumnNorm())`
 *                               (src/enlsip_functions.jl:219-223) as a TSQR whose one exchange step is an RCCL
 *                               all-gather over xGMI inside the library; enlsip_gn_tsqr_local_dev / _combine_dev are
 *                               its two stages for callers that bring their own transport.  INTEGRATION.md section 5.
 *
 * Conventions
 *   - All matrices column-major (Julia / LAPACK layout), fp64, explicit leading dimensions.
 *   - Permutations are returned as 1-based LAPACK jpvt (Julia's F.p), int64.
 *   - Integers that mirror Julia Int / BlasInt are int64_t.
 *   - Return value: 0 = ok; < 0 = -(index of the offending argument), LAPACK style;
 *     > 0 = HIP runtime error code (text via enlsip_gn_last_error).  No exceptions cross the ABI.
 *   - Caller owns every buffer passed in; the library owns device workspaces (grown lazily,
 *     freed by enlsip_gn_destroy).  One handle = one HIP stream; a handle is not thread-safe,
 *     distinct handles are independent.
 *   - "_dev" entry points take DEVICE pointers (hipMalloc memory on the handle's device) and
 *     leave results in device memory; the others take HOST pointers and stage through PCIe.
 *   - Factors stay resident on the device behind the handle until the next solve on it.
 *   - Magnitudes.  qr(., ColumnNorm()) of the reference is dgeqp3, whose norms and reflectors scale internally: inputs of any
 *     magnitude are factored alike and pseudo_rank's absolute first test (src/enlsip_functions.jl:19) decides the rank.  The
 *     kernels square plainly; enlsip_gn_solve*, _solve_batched*, _factor_constraints and _solve_factored therefore detect such
 *     inputs on their result: a problem is nominated when the first diagonal entry of F_A.R or of F_J2.R (the largest column norm)
 *     is above 2^440, not finite, or below 2^-440, and a nominated problem whose largest |entry| of J, rx or of A', cx lies outside
 *     the band 2^-400 .. 2^400 is solved again on copies scaled by a power of two, with the resident factors and the outputs scaled
 *     back: ranks, pivots, p, b, d and every accessor are those of the caller's data, as LAPACK would return
 *     them.  The range covered therefore starts at the band edge: inside the band plain sums of squares hold for every shape the
 *     library takes; beyond it nothing is left to the plain kernels.  The row shards of enlsip_gn_solve_tsqr and of
 *     enlsip_gn_tsqr_local_scaled_dev / _combine_scaled_dev are covered in the same way, shard by shard: the local result is
 *     nominated on the largest |entry| of its (unpivoted) R and of its carried column, each rank scales ITS shard by a power of two
 *     of its own, the exponent travels with the triangle and the combine stage brings the blocks to one scale.
 *     Only the older stage pair enlsip_gn_tsqr_local_dev / _combine_dev, whose arguments cannot carry an exponent, stays plain.
 */
#ifndef ENLSIP_GN_H
#define ENLSIP_GN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct enlsip_gn_context* enlsip_gn_handle;
typedef int (*enlsip_gn_allgather_fn)(void* ctx, const void* dsend, void* drecv, size_t bytes_per_rank, void* hip_stream);

/* which factorisation an accessor addresses */
enum {
    ENLSIP_GN_FACTOR_A = 0,   /* F_A   = qr(C.A', ColumnNorm())     n  x t   */
    ENLSIP_GN_FACTOR_L11 = 1, /* F_L11 = qr(F_A.R', ColumnNorm())   t  x kA  */
    ENLSIP_GN_FACTOR_J2 = 2   /* F_J2  = qr(J2,  ColumnNorm())      m  x n2  */
};

/* option flags */
enum {
    ENLSIP_GN_UPDATE_MFMA = 1,      /* trailing update through v_mfma_f64_16x16x4 (default on)   */
    ENLSIP_GN_UPDATE_REFLECTORS = 2 /* trailing update by sequential reflectors (debug / A-B)    */
};

typedef struct enlsip_gn_opts {
    int32_t device;        /* HIP device ordinal; -1 = current device                          */
    int32_t flags;         /* 0 = defaults; see enum above                                     */
    int32_t panel_width;   /* 0 = default (32)                                                 */
    int32_t tile_rows;     /* 0 = default (512); rows of one CAQR tile, 256 or 512             */
    void*   stream;        /* hipStream_t to run on, NULL = library creates its own            */
} enlsip_gn_opts;

/* per-problem scalar results, mirrors Iteration.{rankA,rankJ2,dimA,dimJ2} + code
 * (src/structures.jl:63-91, src/enlsip_functions.jl:217, 226-229) */
typedef struct enlsip_gn_info {
    int64_t rankA;
    int64_t rankJ2;
    int64_t code;   /* 1 = rankA == t, -1 = stabilised path */
    int64_t dimA;
    int64_t dimJ2;
    int64_t status; /* 0 ok; bit0: a triangular diagonal was exactly 0 (Julia would throw SingularException) */
} enlsip_gn_info;

int enlsip_gn_version(void);

int enlsip_gn_create(enlsip_gn_handle* h, const enlsip_gn_opts* opts);
int enlsip_gn_destroy(enlsip_gn_handle h);
/* message of the last failed call on h; h = NULL: why the last enlsip_gn_create of the calling thread failed */
const char* enlsip_gn_last_error(enlsip_gn_handle h);
int enlsip_gn_synchronize(enlsip_gn_handle h);

/*
 * One subproblem, host buffers.  Replaces, for given J (m x n), rx (m), At = C.A' (n x t,
 * column-major, i.e. the memory of Julia's t x n C.A read row-wise is NOT what is wanted: pass
 * the transpose explicitly), cx (t):
 *     F_A = qr(C.A', ColumnNorm()); rankA; F_L11 = qr(F_A.R', ColumnNorm());
 *     p_gn, F_J2 = gn_search_direction(J, rx, cx, F_A, F_L11, rankA, t, eps_rank, iter)
 * dimA_override / dimJ2_override: -1 = use rankA / rankJ2 (gn_search_direction);
 * Outputs: p (n), b (t), d (m), info, jpvtA (t), jpvtL (min(n,t)), jpvtJ2 (n - rankA; buffer of
 * n entries required).  Any output pointer may be NULL.
 */
int enlsip_gn_solve(enlsip_gn_handle h, int64_t m, int64_t n, int64_t t,
                    const double* J, int64_t ldj, const double* rx,
                    const double* At, int64_t ldat, const double* cx,
                    double eps_rank, int64_t dimA_override, int64_t dimJ2_override,
                    double* p, double* b, double* d, enlsip_gn_info* info,
                    int64_t* jpvtA, int64_t* jpvtL, int64_t* jpvtJ2);

/*
 * The constraint stage alone: F_A = qr(C.A', ColumnNorm()) (src/enlsip_functions.jl:700), rankA (:768, :17-31) and
 * F_L11 (:769) of one problem, left resident for enlsip_gn_first_lagrange (pass grad_fx), the F_A / F_L11 accessors and
 * apply_q / apply_qt — what update_working_set needs BEFORE it decides which constraint to drop (:700-704).  m is the row
 * count of the solve that follows (the workspace plan is shared).  J-related entries (F_J2, get_JQ1, resolve, gradient,
 * second estimate, jacobian_times) report an error until the next solve.  info: rankA, code, dimA (J2 fields zero).
 */
int enlsip_gn_factor_constraints(enlsip_gn_handle h, int64_t m, int64_t n, int64_t t, const double* At, int64_t ldat,
                                 const double* cx, double eps_rank, enlsip_gn_info* info);

/*
 * The solve that follows enlsip_gn_factor_constraints when the working set did not change: update_working_set factors C.A' once
 * (src/enlsip_functions.jl:700) and, in its s == 0 branch, goes on with that SAME factorisation (:768-771: rankA, F_L11,
 * gn_search_direction).  Same m, n, t as the enlsip_gn_factor_constraints call right before; F_A, F_L11, b, p1 stay as they are,
 * only J and rx are taken in.  Outputs as enlsip_gn_solve.
 */
int enlsip_gn_solve_factored(enlsip_gn_handle h, int64_t m, int64_t n, int64_t t, const double* J, int64_t ldj,
                             const double* rx, double eps_rank, int64_t dimJ2_override, double* p, double* b, double* d,
                             enlsip_gn_info* info, int64_t* jpvtA, int64_t* jpvtL, int64_t* jpvtJ2);

/*
 * Batch of independent subproblems of one shape, host buffers.  Problem k uses
 * J + k*strideJ, rx + k*m, At + k*strideAt, cx + k*t; outputs p + k*n, b + k*t, d + k*m,
 * info[k], jpvtA + k*t, jpvtL + k*min(n,t), jpvtJ2 + k*n.
 */
int enlsip_gn_solve_batched(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t,
                            const double* J, int64_t ldj, int64_t strideJ, const double* rx,
                            const double* At, int64_t ldat, int64_t strideAt, const double* cx,
                            double eps_rank,
                            double* p, double* b, double* d, enlsip_gn_info* info,
                            int64_t* jpvtA, int64_t* jpvtL, int64_t* jpvtJ2);

/*
 * Same, DEVICE buffers in, DEVICE buffers out (inputs are not modified).  Output pointers may be
 * NULL (results then stay only behind the handle).  The call returns after the work has been
 * enqueued and the per-problem info has been checked (one stream synchronisation).
 */
int enlsip_gn_solve_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t,
                                const double* dJ, int64_t ldj, int64_t strideJ, const double* drx,
                                const double* dAt, int64_t ldat, int64_t strideAt, const double* dcx,
                                double eps_rank,
                                double* dp, double* db, double* dd, enlsip_gn_info* dinfo,
                                int64_t* djpvtA, int64_t* djpvtL, int64_t* djpvtJ2);

/*
 * Ragged batch: one shape (m, n) and a working set of its own per problem.  update_working_set (src/enlsip_functions.jl:686-795)
 * adds and drops constraints per problem and calls gn_search_direction with that problem's W.t (:725, :743, :762, :771, :789).
 * t holds `batch` entries 0 <= t[k] <= t_max and is a HOST array in both variants (the working set is host bookkeeping).
 * Problem k: A'_k = the n x t[k] matrix at At + k*strideAt (ld ldat, strideAt >= ldat*t_max), cx_k = the first t[k] entries of
 * cx + k*t_max.  Outputs use the strides of enlsip_gn_solve_batched with t = t_max: p + k*n, b + k*t_max, d + k*m, info[k],
 * jpvtA + k*t_max, jpvtL + k*min(n,t_max), jpvtJ2 + k*n; entries past t[k] in b and jpvtA and past min(n,t[k]) in jpvtL are 0.
 * Every problem's results are those of enlsip_gn_solve on (J_k, rx_k, A'_k[:, :t[k]], cx_k[:t[k]]), the magnitude contract above
 * included; with all t[k] == t_max they are bitwise those of enlsip_gn_solve_batched.  The accessors answer for each problem's
 * own t[k] (F_A: min(n,t[k]) x t[k], F_L11: min(t[k],kA) x kA with kA = min(n,t[k]); lambda, Ap, L11 vectors: t[k]).
 * Work is padded to t_max.  Known cliff: the J-side kernels are chosen with n2 = n - min(n, min_k t[k]), so one t[k] = 0 member
 * of a C5-shaped batch (n = 32) makes n2 = 32 and the whole batch leaves the fused one-launch J*Q1 + panel path; in a C3-shaped
 * batch (n = 64) it makes n2 + 1 = 65 and the whole batch leaves the one-wave pivoted QR (measured: 0.41x the uniform throughput).
 * A ragged batch of one problem whose magnitudes need the rescaling is solved with its own t[0] (the padding is never read).
 * Errors before any launch: -6 t NULL or some t[k] outside 0..t_max, -5 t_max beyond the build limit, -12 ldat < n,
 * -13 strideAt < ldat*t_max, -11 / -14 At / cx NULL while t_max > 0.
 */
int enlsip_gn_solve_batched_ragged(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                   const double* J, int64_t ldj, int64_t strideJ, const double* rx,
                                   const double* At, int64_t ldat, int64_t strideAt, const double* cx,
                                   double eps_rank,
                                   double* p, double* b, double* d, enlsip_gn_info* info,
                                   int64_t* jpvtA, int64_t* jpvtL, int64_t* jpvtJ2);
/* Same, DEVICE buffers in and out (t stays a HOST array), as enlsip_gn_solve_batched_dev. */
int enlsip_gn_solve_batched_ragged_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                       const double* dJ, int64_t ldj, int64_t strideJ, const double* drx,
                                       const double* dAt, int64_t ldat, int64_t strideAt, const double* dcx,
                                       double eps_rank,
                                       double* dp, double* db, double* dd, enlsip_gn_info* dinfo,
                                       int64_t* djpvtA, int64_t* djpvtL, int64_t* djpvtJ2);

/*
 * The constraint stage of a whole ragged batch, nothing about J: F_A = qr(C.A', ColumnNorm()) (src/enlsip_functions.jl:700), rankA
 * (:768, :17-31), F_L11 (:769), b, p1 and the block T of Q1 of every problem, left resident — what a batched update_working_set
 * needs BEFORE it decides which constraint each problem drops (:700-704).  Packing, strides, padding and error numbering are those
 * of enlsip_gn_solve_batched_ragged without its J, rx arguments' checks; t is a HOST array in both forms, NULL = every problem has
 * t_max constraints.  m is the row count of the solve that follows.  Afterwards the handle holds only F_A / F_L11 for all `batch`
 * problems: info[k] carries rankA, code, dimA (J fields zero); the FACTOR_A / FACTOR_L11 accessors, apply_q / apply_qt and
 * enlsip_gn_get_diagR_batched answer per problem with its own t[k]; enlsip_gn_first_lagrange_batched* answers over any range when
 * grad_fx is given (pipelined halves included); everything that needs J reports "only F_A / F_L11 are resident".  A problem whose
 * A', cx lie beyond the plain magnitude range is factored on a one-problem handle of its own (the magnitude contract above).
 * A batch above the launch limit (32768) returns -2: only its last chunk would stay resident.
 */
int enlsip_gn_factor_constraints_batched(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                         const double* At, int64_t ldat, int64_t strideAt, const double* cx,
                                         double eps_rank, enlsip_gn_info* info);
/* Same, DEVICE buffers (t stays a HOST array; dinfo DEVICE or NULL). */
int enlsip_gn_factor_constraints_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                             const double* dAt, int64_t ldat, int64_t strideAt, const double* dcx,
                                             double eps_rank, enlsip_gn_info* dinfo);

/*
 * The Jacobian side on that resident constraint stage (src/enlsip_functions.jl:725 / :771: gn_search_direction on the working set
 * that survived the deletion test).  Needs enlsip_gn_factor_constraints_batched (same form, host or device) with the same batch, m,
 * n, t_max right before: -1 otherwise.  refactor is a HOST array of `batch` flags, NULL = none.  A problem with refactor[k] == 0
 * keeps its constraint stage and must come with the t[k] it was factored with (-6 names k); its At / cx slots are not read.  A
 * problem with refactor[k] != 0 (its working set changed) may have any t[k] in 0..t_max and gets its constraint stage again from
 * its At / cx slots first; the constraint kernels are launched over exactly those problems and write no slot of another one.
 * Host form: only the flagged problems' At / cx are staged.  Device form: dAt, ldat, strideAt, dcx must be the buffers of the
 * factor call, the flagged problems' slots rewritten in place (-11 otherwise).  Either way the resident inputs afterwards are the
 * final working sets.  Per problem the outputs, the resident factors and every later consumer are those of
 * enlsip_gn_solve_batched_ragged on the final (J, rx, At, cx, t), bit for bit (same kernels, same inputs), the second attempt after
 * a rank-deficient A' (which restarts from J*Q1) and the magnitude contract included.  The pipelined halves are those the constraint
 * stage was placed on; if the library would now split the batch differently (profiling toggled in between) the call returns -1.
 * A batch above the launch limit returns -2.
 */
int enlsip_gn_solve_factored_batched(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                     const int64_t* refactor,
                                     const double* J, int64_t ldj, int64_t strideJ, const double* rx,
                                     const double* At, int64_t ldat, int64_t strideAt, const double* cx,
                                     double eps_rank,
                                     double* p, double* b, double* d, enlsip_gn_info* info,
                                     int64_t* jpvtA, int64_t* jpvtL, int64_t* jpvtJ2);
/* Same, DEVICE buffers in and out (t and refactor stay HOST arrays), as enlsip_gn_solve_batched_ragged_dev. */
int enlsip_gn_solve_factored_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                         const int64_t* refactor,
                                         const double* dJ, int64_t ldj, int64_t strideJ, const double* drx,
                                         const double* dAt, int64_t ldat, int64_t strideAt, const double* dcx,
                                         double eps_rank,
                                         double* dp, double* db, double* dd, enlsip_gn_info* dinfo,
                                         int64_t* djpvtA, int64_t* djpvtL, int64_t* djpvtJ2);
/* Problems the constraint kernels of the last enlsip_gn_factor_constraints_batched* / enlsip_gn_solve_factored_batched* call on h were
 * launched over (on the handle and its pipeline half): batch after the former, the number of refactor flags after the latter (0 with
 * refactor == NULL: no constraint kernel is launched).  This, not the results, tells the call from a full re-solve. */
int enlsip_gn_get_constraint_refactored(enlsip_gn_handle h, int64_t* count);

/*
 * Solve again only the problems whose working set changed, in place (update_working_set, src/enlsip_functions.jl:686-795: the
 * second solve after the undo of a deletion, :728-743, and the third after a second-order deletion, :745-762 / :773-790; the
 * direction itself is gn_search_direction's, :725 / :771).  The handle must hold a FULLY SOLVED ragged batch left by
 * enlsip_gn_solve_batched_ragged*, enlsip_gn_solve_factored_batched* or an earlier call of this entry point, with the same batch, m,
 * n, t_max; every other state returns -1 with a message (nothing resident, only F_A / F_L11 resident, a uniform
 * enlsip_gn_solve_batched, a TSQR solve, a pipeline split that would now differ from the resident one).  A batch above the launch
 * limit returns -2.  Workspace strides and the plan are those of the resident solve; J and rx are the resident ones (as
 * enlsip_gn_gradient_batched reads them).
 * changed is a HOST array of `batch` flags (NULL: -7).  All zero is legal: 0 is returned, nothing is launched or written.  A problem
 * with changed[k] == 0 must come with the t[k] it is resident with (-6 names k); its At / cx slots are not read, no output slot of
 * it is written and no byte of its resident state changes (a result held by ENLSIP_GN_DIM_HOLD stays held).  A problem with
 * changed[k] != 0 may have any t[k] in 0..t_max: its constraint stage and its Jacobian side (J*Q1, the CAQR sweep, the pivoted QR of
 * R0, the final kernel) run again over a device list of exactly those problems, into their own slots.  It gets its outputs, its
 * resident factors and state record, its info and its t — bit for bit what enlsip_gn_solve_batched_ragged on the whole batch with
 * the final working sets leaves for it (kernel forms are chosen from the part's whole problem count, only the grids follow the
 * list; the launch width is max(n - min(n, min over all t[k]), widest resident J2 of the unchanged problems), widened for the
 * changed problems alone when one of their A' turns out rank deficient) — and every later consumer answers for it.  A held result
 * of a changed problem is dropped.  The magnitude contract holds: a changed problem beyond the plain range is solved on a
 * one-problem handle from the resident inputs, one that was there returns to the batch when its data no longer needs it.
 * Host form: the resident solve must be a host-form one; only the changed problems' At / cx are staged, into the staging area it
 * reads.  Device form: dAt, ldat, strideAt, dcx must be the buffers the resident solve was made with, the changed slots rewritten
 * in place (-8 otherwise).  Other argument errors: -9 ldat < n, -10 strideAt < ldat * t_max, -11 cx NULL while a changed t[k] > 0.
 * Every argument and state error is raised before anything is staged or launched and leaves the resident state usable.
 */
int enlsip_gn_solve_changed_batched(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                    const int64_t* changed,
                                    const double* At, int64_t ldat, int64_t strideAt, const double* cx,
                                    double eps_rank,
                                    double* p, double* b, double* d, enlsip_gn_info* info,
                                    int64_t* jpvtA, int64_t* jpvtL, int64_t* jpvtJ2);
/* Same, DEVICE buffers in and out (t and changed stay HOST arrays). */
int enlsip_gn_solve_changed_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t t_max, const int64_t* t,
                                        const int64_t* changed,
                                        const double* dAt, int64_t ldat, int64_t strideAt, const double* dcx,
                                        double eps_rank,
                                        double* dp, double* db, double* dd, enlsip_gn_info* dinfo,
                                        int64_t* djpvtA, int64_t* djpvtL, int64_t* djpvtJ2);
/* Problems the Jacobian-side kernels of the last solve on h were launched over, summed over the pipelined halves: batch after a
 * whole-batch solve, the number of flags after enlsip_gn_solve_changed_batched* (enlsip_gn_get_constraint_refactored reports the
 * same number then). */
int enlsip_gn_get_jacobian_resolved(enlsip_gn_handle h, int64_t* count);

/* ---- accessors on the resident factors of problem `prob` of the last solve (host buffers) ---- */

/* rows/cols of F.R for `which`: A: min(n,t) x t; L11: min(t,kA) x kA; J2: min(m,n2) x n2 */
int enlsip_gn_factor_shape(enlsip_gn_handle h, int which, int64_t prob, int64_t* rows, int64_t* cols);
/* F.R = triu(factors[1:min,:]) into R (ldr >= rows) */
int enlsip_gn_get_R(enlsip_gn_handle h, int which, int64_t prob, double* R, int64_t ldr);
int enlsip_gn_get_diagR(enlsip_gn_handle h, int which, int64_t prob, double* diag);
int enlsip_gn_get_jpvt(enlsip_gn_handle h, int which, int64_t prob, int64_t* jpvt);
/* v <- F.Q' * v  (length n for A, t for L11, m for J2) */
int enlsip_gn_apply_qt(enlsip_gn_handle h, int which, int64_t prob, double* v);
/* v <- F.Q * v */
int enlsip_gn_apply_q(enlsip_gn_handle h, int which, int64_t prob, double* v);
/* J * F_A.Q (m x n) into out (ld >= m) — src/enlsip_functions.jl:219, :526, :1249 */
int enlsip_gn_get_JQ1(enlsip_gn_handle h, int64_t prob, double* out, int64_t ld);
/*
 * sub_search_direction(J1, rx, cx, F_A, F_L11, F_J2, n, t, rankA, dimA, dimJ2, code) on the
 * resident factors (src/enlsip_functions.jl:1253 calls it with code = -1).  code must be 1 or -1.
 */
int enlsip_gn_resolve(enlsip_gn_handle h, int64_t prob, int64_t dimA, int64_t dimJ2, int64_t code,
                      double* p, double* b, double* d);

/* ---- multiplier estimates on the resident data of the last solve -------------------------
 * The two consumers the reference runs right after the subproblem, computed where F_A, J and J*F_A.Q already
 * are instead of on copies: host vectors in / out, `prob` = problem index of the last (batched) solve,
 * diag_scale = Constraint.diag_scale when row scaling is on (NULL: no back-transform), eps_rank as in the solve.
 *
 * enlsip_gn_gradient          grad = J' * rx                           src/enlsip_functions.jl:2690, :2734, :2830
 * enlsip_gn_first_lagrange    first_lagrange_mult_estimate!            src/enlsip_functions.jl:461-508
 *                             lambda (t) and iter.grad_res; grad_fx = NULL uses J' * rx of the resident J, rx
 * enlsip_gn_second_lagrange   second_lagrange_mult_estimate!           src/enlsip_functions.jl:514-537
 *                             b = J1' (rx + J p_gn) with the resident J1 = (J*F_A.Q)[:, 1:t] (the reference
 *                             recomputes J*F_A.Q here, :526).  Returns -7 if the pseudo-rank under eps_rank
 *                             exceeds the rank the solve used (those J1 columns were factored in place).
 * enlsip_gn_jacobian_times    Jp = J * p (m) and Ap = C.A * p (t, active rows), the products the line search sets up
 *                             with (src/enlsip_functions.jl:2226-2229: `Jp = J * p`, `active_Ap = (active_constraint.A) * p`),
 *                             on the J and A' of the last solve; either output may be NULL.  (The product with the FULL
 *                             constraint Jacobian, :2227: enlsip_gn_full_constraints_times.)
 * enlsip_gn_full_constraints_times   Ap = A * p with the FULL constraint Jacobian A (l x n, column-major, host; inactive rows
 *                             included): the other product of src/enlsip_functions.jl:2227 (`Ap = A * p`).  A is staged through
 *                             PCIe for one gemv — offered so that the whole line-search set-up can stay behind the ABI; a host
 *                             BLAS call is the faster choice for small l.  Needs no resident factors.
 * enlsip_gn_matrix_times_QA   out = M * F_A.Q for a HOST matrix M with the row count m of the last solve (rows x n, ldm >= rows):
 *                             what the reference writes as `J * F_A.Q` (src/enlsip_functions.jl:384, :526, :1249) for ANY such
 *                             matrix — one launch of the J*Q1 kernel on the resident reflectors; -3 when rows != m.  The Julia
 *                             glue's `Base.:*(::AbstractMatrix, ::DeviceQ)` rests on it.
 */
int enlsip_gn_gradient(enlsip_gn_handle h, int64_t prob, double* grad);
int enlsip_gn_full_constraints_times(enlsip_gn_handle h, int64_t l, int64_t n, const double* A, int64_t lda, const double* p,
                                     double* Ap);
int enlsip_gn_matrix_times_QA(enlsip_gn_handle h, int64_t prob, int64_t rows, const double* M, int64_t ldm, double* out,
                              int64_t ldo);
int enlsip_gn_jacobian_times(enlsip_gn_handle h, int64_t prob, const double* p, double* Jp, double* Ap);
int enlsip_gn_first_lagrange(enlsip_gn_handle h, int64_t prob, const double* grad_fx, const double* diag_scale,
                             double eps_rank, double* lambda, double* grad_res);
int enlsip_gn_second_lagrange(enlsip_gn_handle h, int64_t prob, const double* p_gn, const double* diag_scale,
                              double eps_rank, double* lambda);

/* ---- the same consumers over a range of the resident batch ----------------------------------------------------------------------
 * update_working_set needs the first estimate on every outer iteration (src/enlsip_functions.jl:700-704) and the second whenever
 * t == rankA && rankJ2 == min(m, n - rankA) (:745-747, :773-776); the line search needs J p and A p (:2226-2229).  These forms
 * answer for problems prob0 .. prob0+count-1 (indices in the caller's whole batch, as the accessors count them) in a fixed number
 * of launches whatever count is.  Slot j holds problem prob0 + j; strides are those of enlsip_gn_solve_batched with t = t_max:
 *   grad, p, p_gn, grad_fx: n    Jp: m    Ap, lambda, diag_scale: t_max    grad_res, status: 1
 * After a ragged solve each problem uses its own t[k]; lambda and Ap entries past t[k] are exactly 0.
 *
 * enlsip_gn_gradient_batched*         grad = J' rx                         src/enlsip_functions.jl:2690, :2734, :2830
 * enlsip_gn_jacobian_times_batched*   Jp = J p, Ap = C.A p (active rows)   src/enlsip_functions.jl:2226-2229
 *                                     Jp or Ap may be NULL, not both.
 * enlsip_gn_first_lagrange_batched*   first_lagrange_mult_estimate!        src/enlsip_functions.jl:461-508
 *                                     grad_fx = NULL: J' rx of the resident J, rx; grad_res and status may be NULL.  A problem with
 *                                     t[k] = 0 gets grad_res = ||grad|| (grad = grad_fx or J' rx); the per-problem entry point
 *                                     reports 0 there when grad_fx is NULL (it has no gradient), so that case is checked against the
 *                                     reference's definition, not against enlsip_gn_first_lagrange.
 * enlsip_gn_second_lagrange_batched*  second_lagrange_mult_estimate!       src/enlsip_functions.jl:514-537
 * diag_scale = NULL: no back-transform.  status[j]: 0; 1 singular triangular system (the per-problem return 1); 2 the pseudo-rank
 * under eps_rank exceeds the rank the solve used, whose J1 columns are no longer resident (the per-problem -7).
 * Returns 0 when every status is 0, 1 when some problem is flagged; argument and state errors are negative (last_error):
 *   -1 no resident factors or a resident input missing (as the per-problem entry points; after enlsip_gn_factor_constraints:
 *      grad_fx is required and there is no second estimate), -2 count < 1, -3 the range leaves the resident batch or reaches into
 *      an earlier chunk of a batch above the launch limit (need_factors' message), -4 a required pointer is NULL.
 * The range may straddle the two pipelined halves of a batch; problems solved on a rescue handle (magnitudes beyond the plain
 * range) are answered by the per-problem entry points, bitwise.  The _dev forms take DEVICE buffers and return after one
 * synchronisation of each stream that ran a part of the range (the rescue route synchronises more).  The host forms stage through
 * a buffer of their own, never through a buffer the resident solve reads.
 * Results: gradient and products bitwise those of the per-problem entry points; estimates bitwise in the general form (one
 * workgroup per problem, the per-problem kernel's body) and to rounding in the wave-per-problem form, used for n <= 64 and
 * t_max <= 64 unless ENLSIP_GN_LAGRANGE_SMALL=0 (read at handle creation).
 */
int enlsip_gn_gradient_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, double* grad);
int enlsip_gn_gradient_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, double* dgrad);
int enlsip_gn_jacobian_times_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* p, double* Jp, double* Ap);
int enlsip_gn_jacobian_times_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* dp,
                                         double* dJp, double* dAp);
int enlsip_gn_first_lagrange_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* grad_fx,
                                     const double* diag_scale, double eps_rank, double* lambda, double* grad_res, int* status);
int enlsip_gn_first_lagrange_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* dgrad_fx,
                                         const double* ddiag_scale, double eps_rank, double* dlambda,
                                         double* dgrad_res, int* dstatus);
int enlsip_gn_second_lagrange_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* p_gn,
                                      const double* diag_scale, double eps_rank, double* lambda, int* status);
int enlsip_gn_second_lagrange_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* dp_gn,
                                          const double* ddiag_scale, double eps_rank, double* dlambda, int* dstatus);
/* form of the last batched multiplier estimate on this handle: 0 general, 1 wave per problem, -1 none yet */
int enlsip_gn_get_consumer_form(enlsip_gn_handle h, int* form);

/* ---- the subspace re-solve over a range of the resident batch ----------------------------------------------------------------
 * search_direction_analys inspects the Gauss-Newton direction of every problem on every outer iteration; where
 * check_gn_direction asks for subspace minimisation it computes b = F_L11.Q' * (-cx[F_A.p]) (src/enlsip_functions.jl:1249-1253),
 * lets choose_subspace_dimensions (src/enlsip_functions.jl:1118-1176) pick dimA from b and diag(F_L11.R), form
 * d = F_J2.Q' * (-(rx + J1*p1(dimA))) (:1156-1163) and pick dimJ2 from d and diag(F_J2.R), and calls sub_search_direction
 * (src/enlsip_functions.jl:116-153) with them (:1253).  These forms do that for problems prob0 .. prob0+count-1 in a number of
 * launches and synchronisations that does not depend on count; nothing is factored again (F_A, F_L11, F_J2, their pivots and T
 * blocks are not rewritten).  Slot j is problem prob0 + j; strides are those of enlsip_gn_solve_batched with t = t_max:
 * p n, b t_max (zero past a ragged problem's t[k]), d m, info and status 1.  dimA, dimJ2, code are HOST arrays of count entries in
 * both forms (host bookkeeping, like t of the ragged solve); any output pointer may be NULL.
 *
 * enlsip_gn_resolve_batched*   per problem what enlsip_gn_resolve(h, prob0 + j, dimA[j], dimJ2[j], code[j], ...) computes:
 *     sub_search_direction    src/enlsip_functions.jl:116-153 (called at :1253), with
 *     code[j] = 1 or -1;  code[j] = 0 leaves the problem alone: none of its output slots is written, its state is untouched.
 *     dimJ2[j] = ENLSIP_GN_DIM_HOLD   b (:1251) and d = F_J2.Q' d_temp (:1156-1163) only: b and d are written, p is not, and b,
 *                             p1 and F_J2.Q' d_temp stay resident for the form below.  When every request of a call is
 *                             held and d is NULL, b alone is computed (F_J2.Q' is not applied) and nothing is held.
 *     dimA[j]  = ENLSIP_GN_DIM_HOLD   the rest alone: the triangular solve with dimJ2[j], the scatter and p = F_A.Q [p1; p2] on the
 *                             held p1 and d (code and dimA are the held call's; code[j] only has to be non-zero).
 *     Together: code = -1, dimA = rankA, dimJ2 = HOLD gives b (:1251); dimA chosen, dimJ2 = HOLD gives d (:1162);
 *     dimA = HOLD, dimJ2 chosen gives p (:1253) — one F_J2.Q' application per problem where the reference's literal flow has two.
 *   status[j] (written for code[j] != 0): 0; 1 dimA outside 0..min(n, t[k]); 2 dimJ2 outside 0..min(m, n - rankA);
 *     3 dimA = HOLD without a held result (a solve, enlsip_gn_resolve, apply_q / apply_qt on F_J2 or a call without HOLD on that
 *     problem came in between); 4 code not 1 / -1 / 0, or code 1 with rankA < t[k].  A flagged problem is skipped.
 *   Returns 0, 1 when some problem is flagged; negative: -1 no resident factors (also after enlsip_gn_factor_constraints),
 *     -2 count < 1, -3 the range leaves the resident batch or reaches into an earlier chunk of a batch above the launch limit,
 *     -4 dimA, dimJ2 or code is NULL.
 *   Afterwards the resident p1, b, state record and enlsip_gn_info of a re-solved problem are what enlsip_gn_resolve leaves, so
 *   enlsip_gn_second_lagrange, enlsip_gn_newton_direction and a later enlsip_gn_resolve behave the same.  Results agree with
 *   enlsip_gn_resolve to rounding (other summation order in F_J2.Q'; p1 is not recomputed by a factorisation).  The range may
 *   straddle the pipelined halves; problems on a rescue handle are answered by enlsip_gn_resolve.  The _dev form takes DEVICE
 *   output buffers and returns after one synchronisation of each stream that ran a part of the range.
 * enlsip_gn_get_diagR_batched  diag(F.R) of every problem of the range, what choose_subspace_dimensions reads
 *     (src/enlsip_functions.jl:1118-1176: diag(F_L11.R), diag(F_J2.R)): HOST array, `stride` doubles per slot, zeros past each
 *     problem's own length; -6 when stride is smaller than the longest diagonal of the range.
 * enlsip_gn_get_resolve_form   kernel form of the last enlsip_gn_resolve_batched* on this handle: 0 general (a workgroup per
 *     problem), 1 one wave per problem (n <= 64 and t_max <= 64), -1 none yet.
 */
enum { ENLSIP_GN_DIM_HOLD = -2 };
int enlsip_gn_resolve_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const int64_t* dimA, const int64_t* dimJ2,
                              const int64_t* code, double* p, double* b, double* d, enlsip_gn_info* info, int* status);
int enlsip_gn_resolve_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const int64_t* dimA, const int64_t* dimJ2,
                                  const int64_t* code, double* dp, double* db, double* dd, enlsip_gn_info* dinfo, int* dstatus);
int enlsip_gn_get_diagR_batched(enlsip_gn_handle h, int which, int64_t prob0, int64_t count, double* diag, int64_t stride);
int enlsip_gn_get_resolve_form(enlsip_gn_handle h, int* form);
/* HIP-event time (ms) of the F_J2.Q0' launches of the last enlsip_gn_resolve_batched* on this handle, summed over the pipelined
 * halves that ran a part of the range; 0 unless enlsip_gn_set_profiling was on (the events add stream bubbles) */
int enlsip_gn_get_resolve_q0_ms(enlsip_gn_handle h, float* ms);

/* ---- subspace minimisation in ONE call: the dimension choice on the device ---------------------------------------------------
 * The three-call held flow above leaves choose_subspace_dimensions (src/enlsip_functions.jl:1118-1176) to the host: b and d cross
 * PCIe so that determine_solving_dim (src/enlsip_functions.jl:1041-1113, with gn_previous_step :909-932 and
 * subspace_min_previous_step :864-904) can read a vector, a diagonal and six scalars of the previous iterate.  These forms run
 * that choice where b, d and the diagonals are, so the subspace branch of search_direction_analys
 * (src/enlsip_functions.jl:1249-1253, code = -1) is one call for problems prob0 .. prob0+count-1.
 *
 * enlsip_gn_determine_solving_dim   determine_solving_dim (src/enlsip_functions.jl:1041-1113) on HOST data, no handle and no GPU:
 *     *newdim; eta is not computed (its only caller discards it, :1150, :1169).  diagR, y: rankR entries.  Returns 0; 5 when the
 *     reference would index outside tau / rho (previous_dimR > rankR outside a restart; Julia throws there); -2 newdim NULL or
 *     rankR < 0, -4 diagR or y NULL with rankR > 0.  The same routine, compiled for the device, makes the choices below.
 * enlsip_gn_subspace_prev           per problem, what choose_subspace_dimensions reads of previous_iter (host bookkeeping).
 * enlsip_gn_subspace_direction_batched*   per taken problem (take: HOST array of count entries, NULL = all; take[j] == 0:
 *     no output slot written, no state touched):
 *         b = F_L11.Q' (-cx[F_A.p])                                             :1251
 *         dimA by determine_solving_dim on b, diag(F_L11.R)                     :1144-1150   (rankA <= 0: dimA = 0, :1136-1140)
 *         d = F_J2.Q' (-(rx + J1 p1(dimA)))                                     :1156-1163
 *         dimJ2 by determine_solving_dim on d, diag(F_J2.R)                     :1165-1169
 *         dimA, dimJ2 = max with the previous ones if !restart && alpha >= 0.2  :1171-1174
 *         p = sub_search_direction with the final pair                          :1253
 *     Where the max raised dimA, b, p1 and d are formed again with the final dimA before p, as the reference's call at :1253
 *     does: p, b, d, info and the state afterwards are bitwise those of enlsip_gn_resolve_batched(dimA*, dimJ2*, -1) with the
 *     returned pair (the same stage kernels), and a held result of a taken problem is dropped.  info[j].dimA / .dimJ2 carry the
 *     chosen dimensions.  Slots, strides, ragged t[k] and zero padding are those of enlsip_gn_resolve_batched; prev is a HOST
 *     array in both forms and goes up with the one request copy; any output pointer may be NULL.
 *   status[j] (written for taken problems): 0; 1 / 2 the final dimA / dimJ2 lies outside 0..min(n, t[k]) / 0..min(m, n - rankA)
 *     (the max with a previous dimension can do that): no p; b, the d the choice of dimJ2 read and info (with the pair) are
 *     written; 5 the reference would index out of bounds (b[1:previous_dimA] with previous_dimA > t[k], d[1:previous_dimJ2] with
 *     previous_dimJ2 > m, tau / rho past rankR): nothing is written.  What the previous dimensions and the resident ranks decide
 *     is found before any launch and leaves the problem untouched; the one case that depends on the data (previous_dimR ==
 *     rankR + 1 after a step shorter than 0.2) is found on the device, for dimJ2 after b, p1 and the state record were set for the
 *     chosen dimA (a held result of that problem is dropped; one of a problem flagged earlier is kept).
 *   Returns 0, 1 when some problem is flagged; negative as enlsip_gn_resolve_batched: -1 no resident factors (also after
 *     enlsip_gn_factor_constraints), -2 count < 1, -3 the range leaves the resident batch, -4 prev is NULL.
 *   The number of launches does not depend on count; ONE synchronisation per stream that ran a part of the range; no byte of b, d
 *   or a diagonal crosses PCIe between the stages.  The range may straddle the pipelined halves; a problem on a rescue handle is
 *   answered through enlsip_gn_resolve with the dimensions chosen by the host instantiation of the same routine.
 * enlsip_gn_get_subspace_form   kernel form of the last call on this handle: 0 general (256 threads per problem), 1 one wave per
 *     problem (n <= 64 and t_max <= 64), -1 none yet.
 */
typedef struct enlsip_gn_subspace_prev {
    int64_t previous_dimA;        /* :1144  abs(previous_iter.dimA) + t - previous_iter.t   */
    int64_t previous_dimJ2;       /* :1165  abs(previous_iter.dimJ2) + previous_iter.t - t  */
    int64_t restart;              /* current_iter.restart                                    */
    double  previous_alpha;       /* previous_iter.alpha                                     */
    double  constraint_progress;  /* :1147  dot(prev.cx, prev.cx) - active_cx_sum            */
    double  residual_progress;    /* :1168  dot(prev.rx, prev.rx) - rx_sum                   */
} enlsip_gn_subspace_prev;
int enlsip_gn_determine_solving_dim(int64_t previous_dimR, int64_t rankR, double predicted_linear_progress, double obj_progress,
                                    double prelin_previous_dim, const double* diagR, const double* y, double previous_alpha,
                                    int64_t restart, int64_t* newdim);
int enlsip_gn_subspace_direction_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const int64_t* take,
                                         const enlsip_gn_subspace_prev* prev, double* p, double* b, double* d,
                                         enlsip_gn_info* info, int* status);
int enlsip_gn_subspace_direction_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const int64_t* take,
                                             const enlsip_gn_subspace_prev* prev, double* dp, double* db, double* dd,
                                             enlsip_gn_info* dinfo, int* dstatus);
int enlsip_gn_get_subspace_form(enlsip_gn_handle h, int* form);

/* ---- the deletion test and the working-set edit of a batch, on the caller's device buffers -------------------------------------
 * Between the stages of a batched update_working_set (src/enlsip_functions.jl:686-795: enlsip_gn_factor_constraints_batched_dev,
 * enlsip_gn_first_lagrange_batched_dev, enlsip_gn_solve_factored_batched_dev, enlsip_gn_solve_changed_batched_dev,
 * enlsip_gn_second_lagrange_batched_dev) stands check_constraint_deletion (:574-603), the removal of row s from C.A, C.cx,
 * C.diag_scale and lambda (:708-719, :748-756, :776-785) and the re-insertion after a failed feasibility test (:731-739).  These
 * entry points do that where lambda, grad_res, diag_scale, A' and cx are, so that "the flagged problems' slots rewritten in
 * place" of the _dev solves needs no download, host loop and upload.  What stays with the caller is the bookkeeping the ragged
 * ABI keeps on the host anyway: t, the active / inactive index lists, the 0/1 flags.
 *
 * enlsip_gn_check_constraint_deletion   check_constraint_deletion (src/enlsip_functions.jl:574-603) on HOST data, no handle and no
 *     GPU: *s = the 1-based index of the constraint to delete, 0 for none.  lambda, diag_scale: t entries; q: the equalities, never
 *     candidates (:591).  lambda_max is taken over all t entries and propagates a NaN as Julia's maximum does (then s = 0); row_i is
 *     an IEEE division when scaling != 0 (:592); both tests of :593 are <=, so among equal minima the last index wins; the gate is
 *     grad_res > -10 e (:598).  Returns 0; -2 s NULL, t < 0, q < 0 or q > t; -4 lambda or diag_scale NULL while t > q.  The same
 *     routine, compiled for the device, makes the decisions below.
 * enlsip_gn_delete_constraints_batched_dev   for every taken problem k (take: HOST array of batch entries, NULL = all) the test on
 *     dlambda[k, 0:t[k]), ddiag_scale[k, 0:t[k]), q[k] and dgrad_res[k] (dgrad_res NULL: 0.0 for every problem, the second-order
 *     test of :747 / :775), and where s[k] != 0, in place:
 *         dsaved[k] = A_s (n), cx_s, lambda_s, diag_scale_s                                    :708-711   (dsaved may be NULL when
 *                                                                                                no restore will follow)
 *         columns s .. t-1 of the A' block one to the left, column t-1 zero                     :719 / :756 / :785
 *         cx, lambda, diag_scale likewise; the vacated slot gets 0.0, 0.0 and 1.0               :713-715 / :751-753 / :779-781
 *     i.e. the padded layout a host caller would upload.  t, q, take and s are HOST arrays of batch entries; s[k] (1-based, 0 =
 *     nothing, also for a problem not taken) comes back in the host array; t is not written, the caller decrements it.  Device
 *     buffers have the strides of the ragged solve: dlambda, ddiag_scale, dcx t_max per problem, dAt problem k's n x t[k]
 *     column-major block at dAt + k * strideAt, dgrad_res 1, dsaved n + 3.  Nothing of a problem with s[k] == 0 or take[k] == 0 is
 *     written, nor any byte between rows n and ldat or between ldat * t_max and strideAt.
 * enlsip_gn_restore_constraints_batched_dev   for every problem with s[k] != 0 the exact inverse, t[k] being the count AFTER the
 *     deletion: columns s-1 .. t-1 one to the right, the saved column at s-1, the same for cx, lambda and diag_scale (:731-733 and
 *     what :739 rebuilds).  Afterwards the slot is byte for byte what it was before the delete.  The feasibility rule itself
 *     (:728-729) stays a host line of the driver: its dot(A_s, p_gn) arm needs rankA > W.t, which cannot happen (rankA <=
 *     min(n, t); quirk Q1 of SURVEY App. C), so there is no device dot product for it.
 * enlsip_gn_get_deletion_form   kernel form of the last of the two calls on this handle: 0 general (one workgroup per problem, one
 *     lane runs the routine above on an LDS copy), 1 one wave per problem (n <= 64 and t_max <= 64: four problems per workgroup,
 *     the decision by cross-lane operations), -1 none yet.  The two forms give the same s on the same inputs.
 * Both calls need no resident factors: they are legal in every handle state, between a factor call and its solve included, and
 * touch nothing resident.  The number of launches does not depend on batch; one copy of the host records goes up, one copy of s
 * comes back (delete), and the call returns after ONE synchronisation of the handle's stream.  The records live in a scratch the
 * handle keeps.  Argument errors are raised before anything is launched and leave every buffer untouched (last_error names k):
 *   -1 h NULL; -2 batch < 1; -3 n < 1 or t_max outside 0..1024 (this build); -4 t, q or s NULL, or dlambda,
 *   ddiag_scale, dAt or dcx NULL while t_max > 0; -5 some t[k] outside 0..t_max (restore: 0..t_max-1 where s[k] != 0); -6 some q[k]
 *   outside 0..t[k]; -7 restore: some s[k] outside 0..t[k]+1; -9 ldat < n; -10 strideAt < ldat * t_max; -12 restore: dsaved NULL
 *   while some s[k] != 0.
 */
int enlsip_gn_check_constraint_deletion(int64_t q, int64_t t, const double* lambda, const double* diag_scale, int scaling,
                                        double grad_res, int64_t* s);
int enlsip_gn_delete_constraints_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t n, int64_t t_max,
                                             const int64_t* t, const int64_t* q, const int64_t* take, int scaling,
                                             double* dlambda, double* ddiag_scale, const double* dgrad_res,
                                             double* dAt, int64_t ldat, int64_t strideAt, double* dcx,
                                             double* dsaved, int64_t* s);
int enlsip_gn_restore_constraints_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t n, int64_t t_max,
                                              const int64_t* t, const int64_t* s,
                                              double* dlambda, double* ddiag_scale,
                                              double* dAt, int64_t ldat, int64_t strideAt, double* dcx,
                                              const double* dsaved);
int enlsip_gn_get_deletion_form(enlsip_gn_handle h, int* form);

/* ---- the line-search set-up of a batch, on the caller's device buffers ---------------------------------------------------------
 * What compute_steplength (src/enlsip_functions.jl:2197-2293) does with the direction before the line search itself: the product
 * with the FULL constraint Jacobian, `Ap = A * p` (:2226-2229), upper_bound_steplength on it (:2149-2178), and the three sums
 * through which `Jp` enters the scalars of the set-up: dot(Jp,Jp), dot(Jp,rx) and dot(rx,rx) of penalty_weight_update (:1561-1584)
 * and of the predicted reduction (:2269).  Jp itself is what enlsip_gn_jacobian_times_batched_dev leaves on the device.  The penalty
 * weights, the merit function and the polynomial fit are the calls of the next two sections; the callbacks stay with the caller.
 *
 * enlsip_gn_upper_bound_steplength   upper_bound_steplength (src/enlsip_functions.jl:2149-2178) on HOST data, no handle and no GPU,
 *     on an Ap that has already been formed.  inactive: n_inactive 1-based row indices, 0 for padding; cx, Ap: l entries.  The list is
 *     walked in list order; an all-zero list looks at nothing (:2163); the entry equal to index_del is skipped (:2166); alpha_j =
 *     -cx[j] / Ap[j] is an IEEE division; the test is cx[j] > 0 && Ap[j] < 0 && alpha_j < alpha_upper with a strict <, so among equal
 *     minima the first list position wins and a row with a NaN is skipped; *alpha_upp = min(3.0, alpha_upper) while *index_alpha_upp
 *     stays the minimising row even when its alpha_j is 3 or more; no row qualifies: 3.0 and 0.  Returns 0; -2 an output pointer
 *     NULL, l < 0 or n_inactive outside 0..l; -4 inactive, cx or Ap NULL while n_inactive > 0; -5 a list entry outside 0..l.  The same
 *     routine, compiled for the device, makes the decisions below.
 * enlsip_gn_linesearch_setup_batched_dev   for every problem k: dAp[k, 0:l) = A_k * p_k (A_k: l x n column-major at dA + k *
 *     strideA, lda >= l; dp n per problem), the bound on dcx[k, 0:l) (ALL constraint values), that product, the first n_inactive[k]
 *     entries of inactive[k, 0:l) and index_del[k] (index_del NULL: 0 everywhere), and, when dJp, drx and sums are given (all three
 *     or none), sums[3k .. 3k+2] = Jp.Jp, Jp.rx, rx.rx over the m entries of dJp[k], drx[k].  inactive, n_inactive, index_del,
 *     alpha_upp, index_alpha_upp and sums are HOST arrays; everything with a d is a device buffer.  In the general form dAp[k] is bit
 *     for bit what enlsip_gn_full_constraints_times returns for problem k (columns summed in ascending order); alpha_upp and
 *     index_alpha_upp are what enlsip_gn_upper_bound_steplength returns on that dAp.  The sums are plain sums of products added in a
 *     fixed order without floating-point atomics: a sum depends on m and the operands alone, not on the slot, the batch or the
 *     call.  They are covered for operands inside the 2^+-400 band; beyond it they are not part of the magnitude contract (a product
 *     may overflow or underflow where a scaled norm would not).  l == 0: 3.0 and 0 for every problem, the sums are still computed.
 *     No byte outside dAp[k, 0:l) is written; no input is.
 * enlsip_gn_get_linesearch_form   kernel form of the last call on this handle: 0 general (product: one thread per row, p in LDS;
 *     bound: one workgroup per problem; sums: partial sums per workgroup, added in index order), 1 one wave per problem (n <= 64 and
 *     l <= 64: four problems per workgroup, one launch, the arg-min by cross-lane operations), -1 none yet.  The two forms name the
 *     same row on the same dAp.
 * The call needs no resident factors: it is legal in every handle state, between a factor call and its solve included, and touches
 * nothing resident.  The number of launches does not depend on batch (which may exceed the grid's y limit); one copy of the host
 * records goes up, one copy of the five scalars per problem comes back, and the call returns after ONE synchronisation of the
 * handle's stream.  The records live in a scratch the handle keeps.  Argument errors are raised before anything is launched and
 * leave every buffer untouched (last_error names k):
 *   -1 h NULL; -2 batch < 1 (or batch times the workgroups per problem beyond 2^31-1); -3 n outside 1..1024 (this build), l < 0 (or
 *   above 2^27), or m < 1 while the sums are asked for; -4 n_inactive, alpha_upp or index_alpha_upp NULL, dp, dA, dcx, inactive or
 *   dAp NULL while l > 0, or exactly one or two of dJp / drx / sums missing; -5 some n_inactive[k] outside 0..l; -6 a list entry or
 *   index_del[k] outside 0..l; -9 lda < l; -10 strideA < lda * n.
 */
int enlsip_gn_upper_bound_steplength(int64_t l, int64_t n_inactive, const int64_t* inactive, int64_t index_del,
                                     const double* cx, const double* Ap, double* alpha_upp, int64_t* index_alpha_upp);
int enlsip_gn_linesearch_setup_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t l,
                                           const double* dp, const double* dA, int64_t lda, int64_t strideA,
                                           const double* dcx, const int64_t* inactive, const int64_t* n_inactive,
                                           const int64_t* index_del, const double* dJp, const double* drx,
                                           double* dAp, double* alpha_upp, int64_t* index_alpha_upp, double* sums);
int enlsip_gn_get_linesearch_form(enlsip_gn_handle h, int* form);

/* ---- the penalty weights and the merit function of a batch, on the caller's device buffers -------------------------------------
 * What compute_steplength (src/enlsip_functions.jl:2197-2293) does next with what the set-up left: penalty_weight_update (:2238,
 * :1545-1629, with max_norm_weight_update! :1504-1539, euclidean_norm_weight_update :1429-1497, min_norm_w! :1374-1423 and assort!
 * :1344-1360), psi(0) of :2243, atwa of :2268, and the merit function psi (:1307-1340) of trial points whose residuals and
 * constraints the caller has evaluated into device buffers.  The polynomial fit (linesearch_constrained, :1940-2147) is the next
 * section; the callbacks, check_derivatives and the first guess alpha0 stay with the caller.
 *
 * enlsip_gn_penalty_weight_update   penalty_weight_update on HOST data, no handle and no GPU.  active: t 1-based constraint numbers,
 *     distinct as a working set's are; active_Ap: the t entries of C.A * p, already divided by diag_scale where scaling is on
 *     (:2231-2233); w_old, cx: l entries; norm_code 0 (maximum norm) or 2 (Euclidean norm) (:1606-1611); K: the four histories of
 *     l entries, row ii (K[ii+1] of the reference) at K + ii*l, in and out; w: the new weights, l entries (w == w_old is allowed);
 *     scalars = dpsi0 (:1628), psi0 = 0.5 * (rxrx + sum w[k] cx[k]^2 over active) (:2243), atwa = sum w[k] active_Ap[i]^2 (:2268);
 *     *branch: 0 norm_code 0, or t == 0; 1 ztw >= mu && dimA < t; 2 ztw < mu && dimA < t; 3 ztw < mu && dimA == t (the ctrl = 1
 *     arm); 4 ztw >= mu && dimA == t (or a NaN ztw), the arm that changes nothing but still runs assort!.
 *     One stated deviation: Jp and rx enter only through the three sums the set-up call returns.  nrm_Jp = sqrt(JpJp), nrm_Jp^2 is
 *     nrm_Jp * nrm_Jp as in the Julia, Jp_rx = Jprx instead of the dot of the two normalised vectors multiplied back (:1567-1584),
 *     and nrm_rx is unused.  Everything on the t- and l-vectors is literal, the divide by nrm_Ap / nrm_cx and the multiply back at
 *     :1610 included, and so are the reference's quirks: min_norm_w! starts from w[:] = K[4] over all l entries, not from
 *     previous_w (:1383, :1447); buff >= w_old[i], y_elem > 0, w[k] > K[ii][k] and abs(alpha_w - 1) <= delta keep their strictness;
 *     norm(y, Inf) <= eps gives c = 1 (:1398) and is taken over the whole of y, stale entries included; assort! does not stop after
 *     an insertion (:1351-1357); the maximum-norm arm reads and writes only K[ii][1] and reads w[active[1]], with active[1] == 0
 *     (t == 0) treated as 1 (:1515-1518); rmy / nrm_Ap is an IEEE division, also by zero (:1514).  With norm_code 0 and l == 0,
 *     where the Julia would throw at :1516, w stays empty and K untouched (both may then be NULL).  All sums run in index order,
 *     norm(y) is the square root of that sum of squares, and only + - * / and sqrt are used, never contracted: host and device
 *     give the same bits.  Like the three sums, the routine is covered for operands inside the 2^+-400 band and is not part of the
 *     magnitude contract.  Returns 0; before anything is written: -2 scalars or branch NULL (K or w NULL while l > 0), l < 0,
 *     t outside 0..l, dimA outside 0..t, or norm_code not 0 / 2; -4 w_old NULL while l > 0, or active, active_Ap or cx NULL while
 *     t > 0; -5 an active entry outside 1..l.  The same routine, compiled for the device, does the work below.
 * enlsip_gn_penalty_weights_batched_dev   for every taken problem k (take: HOST array of batch entries, NULL = all; the problems of
 *     the method_code == 2 arm, :2284-2290, are not taken) that routine on dw_old[k], dcx[k], dK[k] (l, l and 4*l per problem, row
 *     ii at + ii*l), dactive_Ap[k, 0:t[k]) divided by ddiag_scale[k, 0:t[k]) when scaling != 0 (an IEEE division, both t_max per
 *     problem: exactly what enlsip_gn_jacobian_times_batched_dev and the ragged layout leave), active[k, 0:t[k]) (HOST, batch x
 *     t_max, 0 padded), dimA[k] and sums[3k .. 3k+2] = Jp.Jp, Jp.rx, rx.rx as the set-up call returns them.  dw[k] (l per problem)
 *     and dK[k] are written on the device; scalars (3 per problem) and branch come back in HOST arrays.  t, dimA, active, take,
 *     sums, scalars, branch are HOST arrays; everything with a d is a device buffer.  w, K, scalars and branch of problem k are bit
 *     for bit what enlsip_gn_penalty_weight_update returns on the downloaded inputs of problem k.  dw == dw_old (the same
 *     pointer) is legal; any other overlap of an output with an input is not checked and not supported.  A problem with
 *     take[k] == 0 has no byte written on the device; its host outputs are 0.  Nothing past t[k] of a t_max-strided buffer is
 *     read, and an entry of K that does not move is not written.
 * enlsip_gn_get_penalty_form   kernel form of the last enlsip_gn_penalty_weights_batched_dev on this handle: 0 general (one
 *     workgroup per problem: it gathers the active entries into LDS, one lane runs the routine, the workgroup does the l-wide copy,
 *     the scatter and assort!), 1 one wave per problem (t_max <= 64 and l <= 64: four problems per workgroup, the same steps),
 *     -1 none yet.  The serial part is the same code in both, so the two forms give the same bits.
 * enlsip_gn_merit_batched_dev   psi[k] = 0.5 * (dot(rx_k, rx_k) + sum over active[k, 0:t[k]) of w[j] cx[j]^2 + sum over the j of
 *     inactive[k, 0:n_inactive[k]) with cx[j] < 0 of w[j] cx[j]^2) (:1322-1339) on drx (m per problem), dcx and dw (l per problem).
 *     The test cx[j] < 0 is literal: -0.0, 0 and a NaN do not enter.  A 0 in either list is padding and is skipped.  rx.rx is the
 *     ordered partial-sum scheme of the set-up call's general form; the constraint terms are added one by one in list order, the
 *     active list first.  No floating-point atomics: a value depends on m, l, the lists and the operands alone, not on the slot,
 *     the batch or the call.  psi of a problem not taken is 0.  t, active (batch x t_max), inactive (batch x l), n_inactive, take
 *     and psi are HOST arrays.
 * All three device calls need no resident factors: they are legal in every handle state and touch nothing resident.  The number
 * of launches does not depend on batch (which may exceed the grid's y limit); one copy of the host records goes up, one copy of
 * the scalars comes back, and a call returns after ONE synchronisation of the handle's stream.  The records live in a scratch
 * the handle keeps.  t_max is at most 1024 in this build, l at most 2^27.  Argument errors are raised before anything is launched
 * and leave every buffer untouched (last_error names k):
 *   -1 h NULL; -2 batch < 1; -3 l or t_max out of range, t_max > l, norm_code not 0 / 2 (merit: m < 0); -4 a required pointer
 *   NULL (penalty: t, dimA, sums, scalars, branch; dw_old, dK, dw while l > 0; active, dactive_Ap, dcx while t_max > 0;
 *   ddiag_scale only while scaling != 0 and t_max > 0; merit: t, n_inactive, psi; drx while m > 0; dcx, dw, inactive while l > 0;
 *   active while t_max > 0); -5 some t[k] outside 0..t_max (merit: or n_inactive[k] outside 0..l); -6 penalty: some dimA[k] outside
 *   0..t[k] or an active entry outside 1..l within the first t[k]; merit: a list entry outside 0..l.
 */
int enlsip_gn_penalty_weight_update(int64_t l, int64_t t, const int64_t* active, int64_t dimA, int norm_code,
                                    const double* w_old, const double* active_Ap, const double* cx,
                                    double JpJp, double Jprx, double rxrx, double* K, double* w,
                                    double* scalars, int* branch);
int enlsip_gn_penalty_weights_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t l, int64_t t_max,
                                          const int64_t* t, const int64_t* dimA, const int64_t* active,
                                          const int64_t* take, int norm_code, int scaling,
                                          const double* dw_old, const double* dactive_Ap, const double* ddiag_scale,
                                          const double* dcx, double* dK, const double* sums, double* dw,
                                          double* scalars, int* branch);
int enlsip_gn_get_penalty_form(enlsip_gn_handle h, int* form);
int enlsip_gn_merit_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t l, int64_t t_max,
                                const int64_t* t, const int64_t* active, const int64_t* inactive,
                                const int64_t* n_inactive, const int64_t* take,
                                const double* drx, const double* dcx, const double* dw, double* psi);

/* ---- the polynomial fit of the line search, on host scalars and on the caller's device buffers ---------------------------------
 * What linesearch_constrained (src/enlsip_functions.jl:1940-2143) does between two callback evaluations.  At its first trial point,
 * and once more on the arm of :2078-2092, it builds v0, v_buff and v2 of length m + l (coefficients_linesearch!, :1665-1689, through
 * concatenate!, :1635-1659), scales v1 = [Jp; Ap] (:1986-1998), takes six dot products of them (minrm, :1849; parameters_rm,
 * :1749-1751) and turns the six numbers into the next step length (:1739-1862 and the choice of :2023-2026).  With these calls every
 * step of the line search between two evaluations of the callbacks exists in the library; the callbacks stay with the caller.
 *
 * enlsip_gn_linesearch_coefficients   the six sums on HOST data, no handle and no GPU.  active: t 1-based constraint numbers,
 *     inactive: n_inactive of them, together a partition of 1..l as a working set's lists are (t + n_inactive == l; duplicates are
 *     the caller's contract and are not checked); rx, rx_new, Jp: m entries; cx, cx_new, Ap, w: l entries, Ap the UNSCALED A * p.
 *     No vector is materialised; the elements are formed literally: residual i: v0 = rx[i], v1 = Jp[i], vb = rx_new[i]; constraint
 *     k: v0 = sqrt(w[k]) * cx[k], v1 = sqrt(w[k]) * Ap[k], vb = sqrt(w[k]) * cx_new[k], where an INACTIVE entry is 0 instead when
 *     cx[k] > 0 (v0, and v1: it reads the OLD cx, :1996) or cx_new[k] > 0 (vb); v2 = ((vb - v0) / alpha_k - v1) / alpha_k, two IEEE
 *     divisions, alpha_k == 0 not special-cased.  sums = v0.v0, v0.v1, v0.v2, v1.v1, v1.v2, v2.v2, each product rounded and then
 *     added, never contracted, in this order: the m residual terms in index order, then the active list in list order, then the
 *     inactive list in list order.  The reference scales JpAp in place (:1986); this routine writes neither Jp nor Ap.  Returns 0;
 *     -2 sums NULL or a size out of range (m, l < 0, t or n_inactive outside 0..l); -4 a needed input pointer NULL; -5
 *     t + n_inactive != l; -6 a list entry outside 1..l.
 * enlsip_gn_linesearch_fit   minrm (:1841-1862) with parameters_rm, newton_raphson, one_root, two_roots and bounds on the six sums,
 *     and the choice alpha_kp1 != beta && p_beta < pk && beta <= alpha_k (:2023-2026).  out = alpha_kp1, pk (after the choice),
 *     alpha_hat, s_alpha, beta_hat, s_beta (as minrm returns them); *arm 0 Newton-Raphson, 1 one root, 2 two roots.  Kept as
 *     written: the d = 1.0 sentinel (:1747), so the Newton arm ends in beta_hat = alpha_hat; (a3, a2, a1) are the FIRST three
 *     coefficients of ds (:1757); alpha_old == beta_hat is tested on the unclamped value after bounds (:1854-1856); the Newton loop
 *     runs while (error > 1e-4 || iter < 3) && iter < 50 and leaves on |dds| < eps; every comparison keeps its strictness.  Horner
 *     evaluation is unfused (Polynomials.jl may fuse, which moves a value by a rounding); a^2, a^3 are products; pow, cbrt, acos,
 *     cos are the host libm's.  Where the Julia would throw or divide by zero (dds_best == 0, normv2 == 0 on the analytic arm, an
 *     acos argument that rounding pushed past 1) the IEEE value is taken; the Newton loop is bounded, so a NaN input ends the
 *     routine.  Returns 0; -2 out or arm NULL; -4 sums NULL.
 * enlsip_gn_minrn   minrn (:1708-1735) with minimize_quadratic (:1692-1702): (0, 0) when two of the abscissae are closer than
 *     sqrt(eps) / p_max (:1719), else the clamped minimiser of the parabola and its value there.  Returns 0; -2 an output NULL.
 * enlsip_gn_check_reduction   check_reduction (:1870-1886): *likely 1 or 0.  Returns 0; -2 likely NULL.
 * enlsip_gn_linesearch_fit_batched_dev   for every taken problem k the six sums on drx, drx_new, dJp (m per problem) and dcx,
 *     dcx_new, dAp, dw (l per problem) with the HOST records t, active (batch x t_max), inactive (batch x l), n_inactive, take
 *     (NULL = all) and alpha_k; then enlsip_gn_linesearch_fit on the HOST, inside the call, with alpha_k[k], x_min[k], alpha_min[k],
 *     alpha_max[k]: out[6k .. 6k+5] and arm[k] are bit for bit that routine on the returned sums[6k .. 6k+5].  (The scalar stage
 *     branches on cbrt, acos and cos, which differ between the host libm and the device library, and the step length has to reach
 *     the host for the next callback evaluation anyway.)  The m residual terms are added by the ordered partial-sum scheme of the
 *     set-up call's general form with six accumulators, the constraint terms one by one in list order, the active list first.  No
 *     floating-point atomics: a sum depends on m, l, the lists and the operands alone, not on the slot, the batch or the call; it
 *     lies within 2 (m + l) u sum |x||y| of the exact dot product of the elements.  psi_new (HOST, may be NULL): psi of (drx_new,
 *     dcx_new, dw) by the merit kernels in the same call from the same uploaded records, bit for bit what
 *     enlsip_gn_merit_batched_dev returns (the reference needs both at the same point, :2000 with :2010).  A problem with
 *     take[k] == 0 gets zeros in sums, out, arm and psi_new.  No device buffer of the caller is written.  The call needs no
 *     resident factors: it is legal in every handle state and touches nothing resident.  The number of launches does not depend on
 *     batch (which may exceed the grid's y limit); one copy of the host records goes up, one copy of the sums (and psi) comes back,
 *     and the call returns after ONE synchronisation of the handle's stream.  t_max is at most 1024 in this build, l at most 2^27.
 *     Argument errors are raised before anything is launched and leave everything untouched (last_error names k):
 *       -1 h NULL; -2 batch < 1; -3 m, l or t_max out of range, t_max > l; -4 a required pointer NULL (t, n_inactive, alpha_k,
 *       x_min, alpha_min, alpha_max, sums, out, arm; drx, drx_new, dJp while m > 0; dcx, dcx_new, dAp, dw, inactive while l > 0;
 *       active while t_max > 0); -5 some t[k] outside 0..t_max, n_inactive[k] outside 0..l, or t[k] + n_inactive[k] != l; -6 a list
 *       entry outside 1..l within the used part of a list.
 */
int enlsip_gn_linesearch_coefficients(int64_t m, int64_t l, int64_t t, const int64_t* active, const int64_t* inactive,
                                      int64_t n_inactive, const double* rx, const double* rx_new, const double* Jp,
                                      const double* cx, const double* cx_new, const double* Ap, const double* w,
                                      double alpha_k, double* sums);
int enlsip_gn_linesearch_fit(const double* sums, double alpha_k, double x_min, double alpha_min, double alpha_max,
                             double* out, int* arm);
int enlsip_gn_minrn(double x1, double y1, double x2, double y2, double x3, double y3, double alpha_min, double alpha_max,
                    double p_max, double* alpha, double* p_alpha);
int enlsip_gn_check_reduction(double psi_alpha, double psi_k, double approx_k, double eta, double diff_psi, int* likely);
int enlsip_gn_linesearch_fit_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t l, int64_t t_max,
                                         const int64_t* t, const int64_t* active, const int64_t* inactive,
                                         const int64_t* n_inactive, const int64_t* take,
                                         const double* alpha_k, const double* x_min, const double* alpha_min,
                                         const double* alpha_max, const double* drx, const double* drx_new,
                                         const double* dJp, const double* dcx, const double* dcx_new, const double* dAp,
                                         const double* dw, double* sums, double* out, int* arm, double* psi_new);

/* ---- the working-set additions of a batch and the rebuild of its active constraints, on the caller's device buffers -----------
 * After new_point! the outer iteration runs evaluate_violated_constraints (src/enlsip_functions.jl:608-650), rebuilds
 * active_C.cx / active_C.A from the full cx and A (:2854-2855) and scales them at the top of the next iteration
 * (evaluate_scaling!, src/structures.jl:160-178, called at :2783).  These entry points do that where the full A (l x n per
 * problem) and cx already are for enlsip_gn_linesearch_setup_batched_dev, and leave the padded slot of the ragged solve: the
 * loop working-set update -> line search -> next update of a batch exchanges only per-problem scalars and index lists.
 *
 * enlsip_gn_evaluate_violated_constraints   the walk on HOST data, no handle and no GPU.  active, inactive: l entries each, the
 *     first *t / l - *t used (1-based, sorted), 0 behind; cx: l entries.  eps = sqrt(DBL_EPSILON), delta = 0.1, bnd = min(l, n);
 *     inactive[i] = k is violated when cx[k] < eps || (k == index_alpha_upp && cx[k] < delta): a NaN never is (nor is an entry
 *     0).  At capacity (*t >= bnd) the worst active inequality is the FIRST maximum of cx over the positions q+1..t by a strict
 *     >, and the swap happens only when worst_val > cx[k]; after the removal the inactive list is re-sorted and inactive[i],
 *     whatever it now is, is added (the reference's behaviour, quirk included).  Both sorts are a single insertion into a sorted
 *     list.  *added = 0 / 1; *status = 0 the walk ended as the reference's does; 1 a swap pass would put back the very
 *     constraint it removes, so (active, inactive, t, i) would be unchanged and the reference would repeat that pass for ever:
 *     the routine stops there with the lists in that unchanged state, *added is what earlier passes set; 2 the defensive cap of
 *     (l+1)^2 passes was exceeded, the lists are as they are at the cap (never observed: the one-pass cycle is the only one
 *     seen, not proved to be the only one).  Returns 0; -2 t, added or status NULL, l, n or q negative, q > *t or *t > l; -4
 *     active, inactive or cx NULL while l > 0; -5 a list entry or index_alpha_upp outside 0..l.
 * enlsip_gn_gather_active_constraints   the rebuild on HOST data: column c of At (n x t column-major, ldat >= n) is row active[c]
 *     of A (l x n column-major, lda >= l); a list entry 0 gives a row of zeros.  row_i = sqrt of the sum of squares in ONE fixed
 *     order that depends on n alone: 64 strided partials (s = j mod 64, ascending j), added by the butterfly of a wave
 *     all-reduce (x[s] += x[s ^ mask], mask = 1, 2, 7, 15, 16, 32); products and additions rounded separately, one IEEE square
 *     root.  scaling == 0: diag_scale = row_i, the row and cx are copied.  scaling != 0: row_i < DBL_EPSILON gives the divisor 1.0,
 *     the row and cx are divided by the divisor (IEEE) and diag_scale = 1.0 / divisor.  Plain sums of squares: covered for
 *     entries inside the 2^+-400 band, as the sums of the line-search set-up.  Nothing between rows n and ldat is written.
 *     Returns 0; -2 a bad shape (l < 0, n < 1, t outside 0..l, lda < l, ldat < n); -4 a NULL while t > 0; -5 an entry outside 0..l.
 * enlsip_gn_add_constraints_batched_dev   per problem k, by take[k] (HOST array, NULL = 1 everywhere): 0 nothing of problem k is
 *     read or written; 1 the walk on dcx_all[k] (l per problem), then the rebuild; 2 the rebuild only, from the lists as given
 *     (the first iteration after init_working_set, and the rebuild of :739).  q, t, active, inactive (batch x l each),
 *     index_alpha_upp (NULL: 0) are HOST arrays; t, active, inactive come back updated where a walk ran (all l entries of a
 *     row, 0 behind the used part), and added / status (HOST, batch entries; 0 for a problem without a walk) as above.  dA: problem
 *     k's l x n column-major block at dA + k * strideA, as in the line-search set-up.  The rebuild writes the padded slot a
 *     host caller would upload: columns 0..t[k]-1 of the block at dAt + k * strideAt gathered (and scaled when scaling != 0),
 *     columns t[k]..t_max-1 0.0 in rows 0..n-1; dcx[k] (t_max per problem) likewise with 0.0 behind, ddiag_scale[k] with 1.0
 *     behind.  No byte between rows n and ldat, behind ldat * t_max or of any input is written.  After a walk with status 1 or 2
 *     the rebuild still runs on the lists as left.  The results are bitwise those of the two host routines on the same data in
 *     both kernel forms and do not depend on the slot, the batch or the take of other problems; no floating-point atomics.
 * enlsip_gn_get_addition_form   kernel form of the last call on this handle: 0 general (a walk kernel, one workgroup per problem
 *     with one lane on LDS copies, l <= 1024 in this build; then a gather kernel per 64-column tile of A' and problem through a
 *     padded LDS tile), 1 one wave per problem (n <= 64 and l <= 64: four problems per workgroup, one launch, cross-lane
 *     operations), -1 none yet.
 * The call needs no resident factors: it is legal in every handle state and touches nothing resident.  The number of launches
 * does not depend on batch; one copy of the records goes up, one comes down, and the call returns after ONE synchronisation of
 * the handle's stream.  l == 0 or t_max == 0 launches nothing.  Argument errors are raised before anything is launched and
 * leave every buffer untouched (last_error names k):
 *   -1 h NULL; -2 batch < 1 (or batch * ceil(t_max / 64) beyond the grid); -3 n < 1, l outside 0..1024, t_max outside 0..1024
 *   or > l; -4 q, t, added or status NULL, active or inactive NULL while l > 0, a device pointer NULL while t_max > 0; -5 some
 *   t[k] outside 0..t_max or, where take[k] == 1, max(t[k], min(l, n)) > t_max (the largest t a walk can leave, so that no
 *   slot can overflow); -6 some q[k] outside 0..t[k]; -7 a list entry or index_alpha_upp[k] outside 0..l; -9 lda < l or
 *   ldat < n; -10 strideA < lda * n or strideAt < ldat * t_max.  Problems with take[k] == 0 are not checked.
 */
int enlsip_gn_evaluate_violated_constraints(int64_t l, int64_t n, int64_t q, int64_t* t, int64_t* active, int64_t* inactive,
                                            const double* cx, int64_t index_alpha_upp, int64_t* added, int64_t* status);
int enlsip_gn_gather_active_constraints(int64_t l, int64_t n, int64_t t, const int64_t* active, const double* A, int64_t lda,
                                        const double* cx, int scaling, double* At, int64_t ldat, double* cx_active,
                                        double* diag_scale);
int enlsip_gn_add_constraints_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t n, int64_t l, int64_t t_max,
                                          const int64_t* q, int64_t* t, int64_t* active, int64_t* inactive,
                                          const int64_t* index_alpha_upp, const int64_t* take, int scaling,
                                          const double* dA, int64_t lda, int64_t strideA, const double* dcx_all,
                                          double* dAt, int64_t ldat, int64_t strideAt, double* dcx, double* ddiag_scale,
                                          int64_t* added, int64_t* status);
int enlsip_gn_get_addition_form(enlsip_gn_handle h, int* form);

/* ---- the termination test of a batch, on the caller's device buffers ----------------------------------------------------------
 * What stands between new_point! and evaluate_violated_constraints in the outer loop (src/enlsip_functions.jl:2828-2839): rx_sum,
 * grad_fx = J' rx, minmax_lagrangian_mult (:540-564) and check_termination_criteria (:2399-2517), with iter.progress (:2279-2280).
 * The exit code of a problem is also the take mask of every other batched call of the next iteration, and dgrad is the dgrad_fx
 * of the next enlsip_gn_first_lagrange_batched_dev.  Delta_time, max_iter and the error_code / Psi_error bookkeeping stay with the
 * caller as inputs.
 *
 * enlsip_gn_minmax_lagrangian_mult   :540-564 on HOST data, no handle and no GPU.  t <= q: *sigma_min = +Inf, *lambda_abs_max =
 *     0.0.  Otherwise lambda_abs_max = max |lambda_i| over ALL t entries and sigma_min the smallest lambda_i of the positions
 *     q+1..t with lambda_i * rows_i <= -sqrt(DBL_EPSILON) (strict < against the running minimum, in order), rows_i = 1.0 /
 *     diag_scale_i (IEEE) when scaling != 0, diag_scale_i otherwise; +Inf when none passes.  A NaN never passes.  A NaN among the
 *     t entries of lambda makes lambda_abs_max the quiet NaN (as Julia's maximum does), here and in both kernel forms.
 *     Returns 0; -2 an output NULL, q < 0 or t < 0; -4 lambda or diag_scale NULL while t > q.
 * enlsip_gn_check_termination_criteria   the decision of :2420-2516 on scalars, statement for statement: the preliminary
 *     condition, the necessary conditions, the codes 10000 / 2000 / 300 / 40 summed, the feas negation of :2471-2481 (unreachable
 *     in the reference, whose necessary condition already excludes it; kept, from n_inactive_le0), then the abnormal chain in its
 *     order: -2, error_code (-3..-5), -9, -6, -10, -11.  alfnoi = DBL_EPSILON / (p_nrm + DBL_EPSILON); eps_rel^2 is eps_rel *
 *     eps_rel.  Returns 0; -2 a NULL.
 * enlsip_gn_termination_sums   fills enlsip_gn_term_sums from HOST arrays of ONE problem, in the orders of the kernels: every
 *     n-, t- and l-length sum as 64 strided partials (s = j mod 64, ascending j, from +0.0) added by the butterfly of a wave
 *     all-reduce (masks 1, 2, 7, 15, 16, 32), products and additions rounded separately; entry j of At * cx_active as a running
 *     sum over the columns in ascending order; norms as a plain sum of squares and one IEEE square root (not nrm2's scaled form:
 *     covered for operands inside the 2^+-400 band, as the sums of the line-search set-up and of the gather).  J: m x n
 *     column-major, ldj; At: n x t column-major, ldat (the OLD active slot, as lambda, cx_active, diag_scale); active / inactive:
 *     the first t / l - t entries used, 1-based, an entry 0 contributes nothing.  grad_in (n) / rx_sum_in: when not NULL the
 *     gradient / rx_sum are taken as given (what the device formed: they follow k_gemv_t and the line-search set-up's dot(rx, rx),
 *     which this routine does not restate bit for bit); otherwise both are formed in the strided order.  grad_out (n) may be NULL.
 *     Returns 0; -2 sums NULL or a bad shape (m, l < 0, n < 1, t outside 0..l, q outside 0..t, dimJ2 outside 0..n, ldj < m,
 *     ldat < n); -4 a NULL array that would be read; -5 a list entry outside 0..l; 998 out of host memory.
 * enlsip_gn_termination_batched_dev   for every problem k with take[k] != 0 (HOST array, NULL = all; take[k] == 0: nothing of
 *     problem k is read or written, sums[k] and exit_code[k] included), on the device: dgrad[k] = J_k' rx_k (n per problem) and the
 *     fields of sums[k]; then, on the host inside the same call, exit_code[k] by enlsip_gn_check_termination_criteria on
 *     (state[k], sums[k], tol): the decision has one implementation.  Padded ragged layout: dlambda, dcx_active, ddiag_scale hold
 *     t_max entries per problem and dAt the n x t_max block at dAt + k * strideAt, of which problem k uses its first state[k].t;
 *     they are the OLD active slot (what active_C holds at :2838).  dJ, drx, dcx_all (l), dx are the NEW point; dx_prev, dp, dd_gn
 *     (n per problem, the first state[k].dimJ2 used), dw (l) belong to the iteration that just ended.  active / inactive: HOST,
 *     batch x l, 1-based, 0 behind.  state[k].psi0 enters progress = 2 psi0 - rx_sum - whsum only.
 *     Arithmetic: no floating-point atomics; every field is bitwise enlsip_gn_termination_sums on the same data given the dgrad
 *     and the rx_sum the call produced, in both kernel forms, whatever the slot, the batch and the take of other problems.  dgrad
 *     is bitwise what enlsip_gn_gradient_batched_dev returns once the same J, rx are resident; rx_sum is bitwise the dot(rx, rx)
 *     of enlsip_gn_linesearch_setup_batched_dev on the same rx (which depends on the kernel form, as there).
 * enlsip_gn_get_termination_form   kernel form of the last call on this handle: 0 general (the J' rx kernel, the partial sums of
 *     rx, one workgroup per problem for every short reduction), 1 one wave per problem (n <= 64 and l <= 64: four problems per
 *     workgroup, one launch, cross-lane operations only), -1 none yet.
 * The call needs no resident factors: it is legal in every handle state and touches nothing resident.  The number of launches
 * does not depend on batch; one copy of the records goes up, one comes down, and the call returns after ONE synchronisation of
 * the handle's stream.  l == 0, t_max == 0 and m == 0 are legal (m == 0: rx_sum = 0.0 and dgrad = 0.0).  Argument errors are raised
 * before anything is launched and leave every buffer untouched (last_error names k):
 *   -1 h NULL; -2 batch < 1 (or batch * max(ceil(n / 4), partial-sum workgroups) beyond the grid); -3 m < 0, n < 1, l outside
 *   0..1024, t_max outside 0..1024 or > l; -4 state, tol, sums or exit_code NULL, active or inactive NULL while l > 0, dJ or drx
 *   NULL while m > 0, dcx_all or dw NULL while l > 0, dlambda, dcx_active, ddiag_scale or dAt NULL while t_max > 0, any of dx,
 *   dx_prev, dp, dd_gn, dgrad NULL; -5 some state[k].t outside 0..t_max, or state[k].l != l; -6 some state[k].q outside
 *   0..state[k].t; -7 a list entry outside 0..l; -8 some state[k].dimJ2 outside 0..n; -9 ldj < m or ldat < n; -10 strideJ <
 *   ldj * n or strideAt < ldat * t_max.  Problems with take[k] == 0 are not checked.
 */
typedef struct enlsip_gn_term_state {
    int64_t restart;              /* :2425  iter.restart (0 / 1)                                                  */
    int64_t code;                 /* :2425  iter.code                                                             */
    int64_t del;                  /* :2430  iter.del (0 / 1)                                                      */
    double  grad_res;             /* :2430  iter.grad_res                                                         */
    int64_t nb_iter;              /* :2492  nb_iter                                                               */
    int64_t nb_newton_steps;      /* :2500  iter.nb_newton_steps                                                  */
    int64_t error_code;           /* :2496  error_code of search_direction_analys                                 */
    int64_t psi_error;            /* :2503  Psi_error of compute_steplength                                       */
    double  delta_time;           /* :2511  Delta_time                                                            */
    int64_t q;                    /* :2437  W.q                                                                   */
    int64_t t;                    /* :2431  W.t                                                                   */
    int64_t l;                    /* :2431  W.l                                                                   */
    int64_t dimJ2;                /* :2448  iter.dimJ2                                                            */
    double  psi0;                 /* :2279  psi0 of compute_steplength (enters progress only)                     */
} enlsip_gn_term_state;
typedef struct enlsip_gn_term_tol {
    int64_t max_iter;             /* :2492  max_iter                                                              */
    double  eps_abs;              /* :2456  eps_abs                                                               */
    double  eps_rel;              /* :2430  eps_rel                                                               */
    double  eps_x;                /* :2460  eps_x                                                                 */
    double  eps_c;                /* :2430  eps_c                                                                 */
} enlsip_gn_term_tol;
typedef struct enlsip_gn_term_sums {
    double  rx_sum;               /* :2828  dot(rx, rx)                                                           */
    double  grad_nrm;             /* :2430  norm(grad_fx), grad_fx = J' rx (:2829)                                */
    double  p_nrm;                /* :2422  norm(iter.p)                                                          */
    double  active_cx_nrm;        /* :2430  norm(active_C.cx)                                                     */
    int64_t n_inactive_nonpos;    /* :2434  inactive cx that are not > 0 (a NaN counts)                           */
    int64_t n_inactive_le0;       /* :2475  inactive cx that are <= 0 (a NaN does not count)                      */
    double  sigma_min;            /* :559   sigma_min of minmax_lagrangian_mult                                   */
    double  lambda_abs_max;       /* :554   lambda_abs_max of minmax_lagrangian_mult                              */
    double  d1_sq;                /* :2452  dot(d1, d1), d1 = iter.d_gn[1:dimJ2]                                  */
    double  x_diff;               /* :2449  norm(prev_iter.x - x)                                                 */
    double  x_nrm;                /* :2460  norm(x)                                                               */
    double  Atcx_nrm;             /* :2488  norm(transpose(active_C.A) * active_C.cx)                             */
    double  active_penalty_sum;   /* :2489  dot(w[active], w[active])                                             */
    double  whsum;                /* :2279  sum of w[active] * cx_new[active]^2                                   */
    double  progress;             /* :2280  2 psi0 - rx_sum - whsum                                               */
} enlsip_gn_term_sums;
int enlsip_gn_minmax_lagrangian_mult(int64_t q, int64_t t, const double* lambda, const double* diag_scale, int scaling,
                                     double* sigma_min, double* lambda_abs_max);
int enlsip_gn_check_termination_criteria(const enlsip_gn_term_state* s, const enlsip_gn_term_sums* v,
                                         const enlsip_gn_term_tol* tol, int64_t* exit_code);
int enlsip_gn_termination_sums(int64_t m, int64_t n, int64_t l, int64_t t, int64_t q, int64_t dimJ2, double psi0,
                               const int64_t* active, const int64_t* inactive, const double* J, int64_t ldj, const double* rx,
                               const double* cx_all, const double* x, const double* x_prev, const double* p, const double* d_gn,
                               const double* lambda, const double* cx_active, const double* diag_scale, const double* At,
                               int64_t ldat, const double* w, int scaling, const double* grad_in, const double* rx_sum_in,
                               double* grad_out, enlsip_gn_term_sums* sums);
int enlsip_gn_termination_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t l, int64_t t_max,
                                      const enlsip_gn_term_state* state, const enlsip_gn_term_tol* tol, const int64_t* active,
                                      const int64_t* inactive, const int64_t* take, int scaling, const double* dJ, int64_t ldj,
                                      int64_t strideJ, const double* drx, const double* dcx_all, const double* dx,
                                      const double* dx_prev, const double* dp, const double* dd_gn, const double* dlambda,
                                      const double* dcx_active, const double* ddiag_scale, const double* dAt, int64_t ldat,
                                      int64_t strideAt, const double* dw, double* dgrad, enlsip_gn_term_sums* sums,
                                      int64_t* exit_code);
int enlsip_gn_get_termination_form(enlsip_gn_handle h, int* form);

/* ---- the Gauss-Newton direction check of a batch, on the caller's device buffers ---------------------------------------------
 * search_direction_analys (src/enlsip_functions.jl:1191-1291) up to its branch: the norms of :1222-1231 and check_gn_direction
 * (:943-1030).  After a solve b, d, lambda, diag_scale and cx are on the device; this call forms every scalar of the decision
 * there, brings one 64-byte record per problem down and makes the decision on the host inside the same call.  method_code == -1
 * is the take of enlsip_gn_subspace_direction_batched_dev, method_code == 2 the take of enlsip_gn_newton_direction_batched_dev.
 * Callbacks and the Hessian sums of the Newton branch stay with the caller.
 *
 * enlsip_gn_check_gn_direction   :943-1030 on scalars, statement for statement, HOST, no handle and no GPU.  b1nrm, d1nrm,
 *     d1nrm_as_km1, dnrm = sqrt of b1_sq, d1_sq, d1_asprev_sq, d_sq (one IEEE square root each); *beta = sqrt(d1nrm * d1nrm +
 *     b1nrm * b1nrm); c1..c5 = 0.5, 0.1, 4.0, 10.0, 0.05, delta = 0.1, eps = max(1e-2, 10 DBL_EPSILON).  lagrange_mult_cond =
 *     n_lm_ge > 0 && n_lm_neg > 0 enters to_reduce only when q < t, n_inactive_lt_delta > 0 only when l - t > 0.  *method_code: 1
 *     the Gauss-Newton direction is accepted, -1 subspace minimisation, 2 the method of Newton.  Returns 0; -2 a NULL.
 * enlsip_gn_direction_sums   fills enlsip_gn_dir_sums from HOST arrays of ONE problem, in the order of the kernels: every sum as
 *     64 strided partials (s = j mod 64, ascending j, from +0.0) added by the butterfly of a wave all-reduce (the masks of
 *     enlsip_gn_termination_sums), products and additions rounded separately; norms are a plain sum of squares (covered for
 *     operands inside the 2^+-400 band).  b: the first dimA entries are read, d: m, lambda and diag_scale: t, cx_all: l; active / inactive: the first
 *     t / l - t entries used, 1-based, an entry 0 contributes nothing.  A NaN passes none of the three comparisons behind the
 *     counts.  *status as status[k] below; with status 1 sums is left untouched.  Returns 0; -2 a NULL among s, sums, status or a
 *     bad shape (m, l < 0, n < 1, s->l != l, t outside 0..l, q outside 0..t, dimA outside 0..t, dimJ2 outside 0..m, prev_t
 *     outside 0..l, |prev_dimJ2| > 2^31); -4 a NULL
 *     array that would be read; -5 a list entry outside 0..l.
 * enlsip_gn_direction_check_batched_dev   for every problem k with take[k] != 0 (HOST array, NULL = all; take[k] == 0: nothing
 *     of problem k is read, written or checked, sums[k], method_code[k], beta[k] and status[k] included), on the device the fields
 *     of sums[k]; then, on the host inside the same call, method_code[k] and beta[k] by enlsip_gn_check_gn_direction on (state[k],
 *     sums[k], m, n).  db, dd, dlambda, ddiag_scale are where the preceding solve and multiplier calls left them, in the padded
 *     ragged layout: db + k * t_max, dd + k * m, dlambda and ddiag_scale + k * t_max; dcx_all holds l entries per problem.  state,
 *     active, inactive (batch x l, 1-based, 0 behind the used part) are HOST arrays.
 *     status[k]: 0 the decision was made; 1 k_prev = prev_dimJ2 + prev_t - t - 1 > m: the reference throws a BoundsError at
 *     :1231, nothing but status[k] is written; 2 the decision was made, but a prefix of d (dimJ2 or k_prev entries) reaches past
 *     n - rankA, where d is this library's and differs from LAPACK's by an orthogonal transform of the tail.
 *     Arithmetic: no floating-point atomics; every field is bitwise enlsip_gn_direction_sums on the same data, in both kernel
 *     forms, whatever the slot, the batch and the take of other problems.
 * enlsip_gn_get_direction_form   kernel form of the last call on this handle: 0 general (one workgroup of four waves per
 *     problem: one pass over d, b and the active list, the multiplier counts, the inactive count), 1 one wave per problem (m <=
 *     1024, l <= 64 and t_max <= 64: four problems per workgroup, cross-lane operations only), -1 none yet.  One launch either
 *     way; the bound on m changes no result.
 * The call needs no resident factors: it is legal in every handle state and touches nothing resident.  One copy of the records
 * goes up, one comes down, and the call returns after ONE synchronisation of the handle's stream.  l == 0, t_max == 0 and m == 0
 * are legal.  Argument errors are raised before anything is launched and leave every buffer untouched (last_error names k):
 *   -1 h NULL; -2 batch < 1; -3 m < 0, n < 1, l outside 0..1024, t_max outside 0..1024 or > l; -4 state, sums, method_code, beta
 *   or status NULL, active or inactive NULL while l > 0, dd NULL while m > 0, dcx_all NULL while l > 0, db, dlambda or
 *   ddiag_scale NULL while t_max > 0; -5 some state[k].t outside 0..t_max, or state[k].l != l; -6 some state[k].q outside
 *   0..state[k].t; -7 a list entry outside 0..l; -8 some state[k].dimA outside 0..state[k].t, state[k].dimJ2 outside 0..m,
 *   state[k].prev_t outside 0..l or |state[k].prev_dimJ2| > 2^31.
 *   Problems with take[k] == 0 are not checked.
 */
typedef struct enlsip_gn_dir_state {
    int64_t iter_number;               /* :981   iter_number                                                      */
    int64_t restart;                   /* :974   current_iter.restart (0 / 1)                                     */
    int64_t add;                       /* :983   current_iter.add (0 / 1)                                         */
    int64_t del;                       /* :983   current_iter.del (0 / 1)                                         */
    int64_t q;                         /* :998   W.q                                                              */
    int64_t t;                         /* :998   W.t                                                              */
    int64_t l;                         /* :1007  W.l                                                              */
    int64_t rankA;                     /* :1015  current_iter.rankA                                               */
    int64_t dimA;                      /* :1222  current_iter.dimA                                                */
    int64_t dimJ2;                     /* :1228  current_iter.dimJ2                                               */
    int64_t prev_code;                 /* :974   previous_iter.code                                               */
    int64_t prev_dimJ2;                /* :1230  previous_iter.dimJ2                                              */
    int64_t prev_t;                    /* :1230  previous_iter.t                                                  */
    double  prev_beta;                 /* :984   previous_iter.beta                                               */
    double  prev_progress;             /* :985   previous_iter.progress                                           */
    double  prev_predicted_reduction;  /* :985   previous_iter.predicted_reduction                                */
    double  prev_alpha;                /* :1020  previous_iter.alpha                                              */
} enlsip_gn_dir_state;
typedef struct enlsip_gn_dir_sums {
    double  b1_sq;                     /* :1222  dot(b1, b1), b1 = b_gn[1:dimA]                                   */
    double  d_sq;                      /* :1227  dot(d_gn, d_gn), all m entries                                   */
    double  d1_sq;                     /* :1228  dot(d1, d1), d1 = d_gn[1:dimJ2]                                  */
    double  d1_asprev_sq;              /* :1231  the same over d_gn[1:k_prev] (k_prev <= 0: 0.0)                  */
    double  active_c_sum;              /* :1013  sum of cx[active]^2 (active_cx_sum)                              */
    int64_t n_lm_ge;                   /* :1004  i in q+1..t with lambda_i * rows_i >= -sqrt(eps)                 */
    int64_t n_lm_neg;                  /* :1004  i in q+1..t with lambda_i < 0                                    */
    int64_t n_inactive_lt_delta;       /* :1009  inactive cx below delta = 0.1                                    */
} enlsip_gn_dir_sums;
int enlsip_gn_check_gn_direction(const enlsip_gn_dir_state* s, const enlsip_gn_dir_sums* v, int64_t m, int64_t n,
                                 int64_t* method_code, double* beta);
int enlsip_gn_direction_sums(int64_t m, int64_t n, int64_t l, const enlsip_gn_dir_state* s, const int64_t* active,
                             const int64_t* inactive, const double* b, const double* d, const double* lambda,
                             const double* diag_scale, const double* cx_all, int scaling, enlsip_gn_dir_sums* sums,
                             int64_t* status);
int enlsip_gn_direction_check_batched_dev(enlsip_gn_handle h, int64_t batch, int64_t m, int64_t n, int64_t l, int64_t t_max,
                                          const enlsip_gn_dir_state* state, const int64_t* active, const int64_t* inactive,
                                          const int64_t* take, int scaling, const double* db, const double* dd,
                                          const double* dlambda, const double* ddiag_scale, const double* dcx_all,
                                          enlsip_gn_dir_sums* sums, int64_t* method_code, double* beta, int64_t* status);
int enlsip_gn_get_direction_form(enlsip_gn_handle h, int* form);

/* ---- the finite-difference Hessian sums of the Newton branch, around the caller's evaluations ---------------------------------
 * hessian_res! and hessian_cons! (src/enlsip_functions.jl:243-328) are callback-bound only in their evaluations: the stencil
 * points and the contractions are streaming work.  A caller whose residuals and constraints are batched device functions forms
 * the points of a pair range for every problem in one call, evaluates them all at once, and hands the evaluations to the sums
 * call, which writes Gamma = r_mat - c_mat (:393) where enlsip_gn_newton_direction_batched_dev reads it.
 *
 * Pair index: a pair is (k, j), 0 <= j <= k < n, P = k (k + 1) / 2 + j (the loop order `for k in 1:n, j in 1:k` of :255).  Every
 * call takes a pair range [pair0, pair0 + npairs), so the caller bounds the size of its evaluation buffers.
 * Steps: eps1 = eps(Float64)^(1/3) (:252), formed once on the host as pow(DBL_EPSILON, 1.0 / 3.0); eps_k = max(|x[k]|, 1.0) * eps1
 * (:256-257; a NaN in x[k] stays a NaN, as Julia's max).
 *
 * enlsip_gn_hessian_points   HOST, one problem, no handle and no GPU.  X (npairs, 4, n): slot s of pair (k, j) is x_work before
 *     evaluation f_{s+1} (:259-265) bit for bit: a copy of x, entry j +- eps_j FIRST, then entry k +- eps_k, signs (+,+), (-,+),
 *     (+,-), (-,-) in the order (j, k).  On the diagonal k == j these are two successive roundings of one entry (f2 is
 *     (x[k] - eps) + eps, not x[k]).  Returns 0; -2 n < 1, npairs < 1, pair0 < 0 or pair0 + npairs > n (n + 1) / 2; -4 a NULL.
 * enlsip_gn_hessian_points_batched_dev   the same for count problems on DEVICE buffers: dx (count, n) in, dX (count, npairs, 4,
 *     n) out, bitwise the host routine's.  One launch, one synchronisation of the handle's stream.  -1 h NULL; -2 count < 1 or
 *     a bad range as above; -4 dx or dX NULL.
 * enlsip_gn_hessian_sums   HOST, one problem and one pair range.  F (npairs, 4, m) and G (npairs, 4, l) hold the residuals and ALL
 *     l constraints at the points above; per pair
 *         s_r = sum_{i<m} (((f1[i] - f2[i]) - f3[i]) + f4[i]) * rx[i]                          :268-271
 *         r   = s_r / ((4 * eps_j) * eps_k)                                                    :272
 *         s_c = sum_{i<t} (((g1[a] - g2[a]) - g3[a]) + g4[a]) * lambda[i], a = active[i] - 1   :317-321
 *         c   = s_c / ((4.0 * eps_k) * eps_j)                                                  :322
 *         Gamma[k, j] = Gamma[j, k] = r - c                                                    :393
 *     every difference, product and divisor rounded as written (the two divisors associate differently in the reference; both
 *     forms are kept).  The two sums are taken in the order of enlsip_gn_termination_sums: 64 strided partials (s = i mod 64,
 *     ascending i, from +0.0) added by the butterfly of a wave all-reduce, NOT the reference's left-to-right order.  An active
 *     entry 0 contributes nothing; with t == 0 c = +0.0 and G, lambda and active are not read.  Gamma is column-major with
 *     ldg >= n; only the (k, j) and (j, k) entries of the pairs in the range are written.  Returns 0; -2 m < 0, n < 1, l < 0 or a
 *     bad range; -4 x or Gamma NULL, F or rx NULL while m > 0, active, G or lambda NULL while t > 0; -5 t outside 0..l, an active
 *     entry outside 0..l, or ldg < n.
 * enlsip_gn_hessian_sums_batched_dev   the same for count problems on DEVICE buffers: dx (count, n), dF (count, npairs, 4, m), drx
 *     (count, m), dG (count, npairs, 4, l), dlambda (count, t_max); t (count), active (count x l, 1-based, 0 behind the used
 *     part) and slot (count) are HOST arrays.  Gamma of problem k is written column-major at dGamma + slot[k] * strideG (slot
 *     NULL: slot[k] = k), the layout enlsip_gn_newton_direction_batched_dev reads, so a compacted list of problems can be run
 *     against the Gamma slots of the resident batch.  slot[k] < 0 leaves problem k alone: nothing of it is read, written or
 *     checked.  Rows >= n of a column (ldg > n) and the gap up to strideG are never touched.  Where no taken problem has t[k] > 0,
 *     dG, dlambda and active may be NULL.  One wave owns one (problem, pair), four pairs per workgroup; no LDS, no barrier, no floating-point
 *     atomics; every entry is bitwise enlsip_gn_hessian_sums on the same data, whatever the slot, the batch and the split of the
 *     triangle into pair ranges.  One copy of the records goes up, one launch, one synchronisation of the handle's stream.
 *     Argument errors are raised before anything is launched and leave every buffer untouched (last_error names k):
 *       -1 h NULL; -2 count < 1, n < 1, m < 0, l < 0, t_max < 0, npairs < 1, pair0 < 0 or pair0 + npairs > n (n + 1) / 2 (also: a
 *       buffer beyond 2^48 doubles); -4 t, dx or dGamma NULL, dF or drx NULL while m > 0, active, dG or dlambda NULL while some
 *       taken t[k] > 0; -5 an active entry outside 0..l, t[k] outside 0..min(l, t_max), ldg < n, strideG < ldg * n, a slot
 *       beyond 2^31 - 1, or two non-negative slot values equal.
 * The batched calls need no resident factors: they are legal in every handle state and touch nothing resident. */
int enlsip_gn_hessian_points(int64_t n, int64_t pair0, int64_t npairs, const double* x, double* X);
int enlsip_gn_hessian_points_batched_dev(enlsip_gn_handle h, int64_t count, int64_t n, int64_t pair0, int64_t npairs,
                                         const double* dx, double* dX);
int enlsip_gn_hessian_sums(int64_t m, int64_t n, int64_t l, int64_t t, int64_t pair0, int64_t npairs, const int64_t* active,
                           const double* x, const double* F, const double* rx, const double* G, const double* lambda,
                           double* Gamma, int64_t ldg);
int enlsip_gn_hessian_sums_batched_dev(enlsip_gn_handle h, int64_t count, int64_t m, int64_t n, int64_t l, int64_t t_max,
                                       int64_t pair0, int64_t npairs, const int64_t* t, const int64_t* active,
                                       const int64_t* slot, const double* dx, const double* dF, const double* drx,
                                       const double* dG, const double* dlambda, double* dGamma, int64_t ldg, int64_t strideG);

/* ---- Newton direction on the resident data of the last solve -------------------------------------------------
 * newton_search_direction (src/enlsip_functions.jl:348-423) after its two Hessian sums (:391-396), which are callback-bound and
 * stay with the caller: Gamma = r_mat - c_mat (n x n, host, column-major, ldg >= n).  Computes E = F_A.Q' Gamma F_A.Q (:398),
 * W22 = E22 + J2'J2, W21 = E21 + J2'J1 (:405-409), d = -W21 p1 - J2' rx (:411), cholesky((W22 + W22')/2) and the two triangular
 * solves (:414-420), p = F_A.Q [p1; p2] (:421) on the resident F_A, p1, J (J * F_A.Q is recomputed, as at :384).
 * *not_posdef = 1 (and p = 0) when the symmetrised W22 is not positive definite (:417-420: `error = true`).  With rankA == n the
 * reference returns p1 as it is (:374-376); so does this.  A rank-deficient working set (t > rankA) takes the reference's other
 * branch: p1 = F_L11.P[1:rankA, 1:rankA] * dp1 (:371-373) and E = E[F_L11.p, F_L11.p] (:396-399) — defined for t >= n only,
 * because F_L11.p has min(n, t) entries and :402-403 read rows up to n; with n > t > rankA the reference runs out of bounds and
 * this entry point returns -7. */
int enlsip_gn_newton_direction(enlsip_gn_handle h, int64_t prob, const double* Gamma, int64_t ldg, double* p, int64_t* not_posdef);

/* ---- the Newton direction over a range of the resident batch -----------------------------------------------------------------
 * newton_search_direction (src/enlsip_functions.jl:348-423) is the direction check_gn_direction picks with method_code == 2; the
 * members of a multi-start batch reach it together, near convergence.  These forms take the step for problems
 * prob0 .. prob0+count-1 in a number of launches and synchronisations that does not depend on count.  Slot j is problem
 * prob0 + j: Gamma_j = r_mat - c_mat (the Hessian sums :391-396 stay with the caller; n x n, column-major, ldg >= n) at
 * Gamma + j*strideG (strideG >= ldg*n), p_j at p + j*n, status[j].  take is a HOST array of count entries in both forms (NULL =
 * all): take[j] == 0 leaves the problem alone — no output slot written, no state touched.
 *
 * Per taken problem the result is what enlsip_gn_newton_direction(h, prob0 + j, Gamma_j, ldg, p_j, &e) computes, with the
 * problem's own t[k] after a ragged solve and the DEFAULT p1 (dimA = rankA), also after a truncated re-solve:
 *     p1 of the rank-deficient working set           :371-373
 *     rankA == n: p1 returned as it is               :374-376
 *     E = F_A.Q' Gamma F_A.Q                         :398      by the kA resident reflectors from both sides, Q is not formed
 *     E = E[F_L11.p, F_L11.p] where t >= n > rankA   :396-399
 *     W22 = E22 + J2'J2, d = -W21 p1 - J2'rx         :405-411  from the resident F_J2 (J2 Pi = Q R): J2'J2 = Pi R'R Pi' and
 *                                                              d = -E21 p1 + Pi R' (F_J2.Q' d_temp)[1:kp], d_temp = -(rx + J1 p1);
 *                                                              no row of J, J*F_A.Q or rx is read for W22
 *     cholesky((W22 + W22')/2), the two solves       :414-420  LAPACK dpotrf semantics (a pivot <= 0 or NaN: not positive definite)
 *     p = F_A.Q [p1; p2]                             :421
 *   status[j] (written for taken problems): 0; 1 the symmetrised W22 is not positive definite (p_j = 0, the reference's
 *     error = true); 2 rank-deficient working set with t[k] < n (enlsip_gn_newton_direction's -7; p_j is not written).
 *   Returns 0, 1 when some taken problem is flagged; negative: -1 no resident J-side factors (also after
 *     enlsip_gn_factor_constraints), -2 count < 1, -3 the range leaves the resident batch or reaches into an earlier chunk of a
 *     batch above the launch limit, -4 Gamma or p is NULL, -5 ldg < n or strideG < ldg*n, -7 the batch went through the
 *     distributed constraint stage (as enlsip_gn_newton_direction).  Argument errors are raised before any launch.
 *   Nothing is factored again: F_A, F_L11, F_J2, their pivots and T blocks are not rewritten; W, Rt and the resident vec are only
 *   read (F_J2.Q' d_temp goes to a buffer of the call).  Afterwards the resident b and p1 of a taken problem are the default ones
 *   and its state record is what it was — what the loop of enlsip_gn_newton_direction calls leaves — so
 *   enlsip_gn_second_lagrange, enlsip_gn_resolve, enlsip_gn_newton_direction and the accessors answer the same.  A result held
 *   by ENLSIP_GN_DIM_HOLD is DROPPED for a taken problem (its p1 is gone): a later dimA = HOLD reports status 3.  Results agree
 *   with enlsip_gn_newton_direction to rounding (J2'J2 from R instead of J).  The range may straddle the pipelined halves;
 *   problems on a rescue handle are answered by enlsip_gn_newton_direction.  The host form stages Gamma in and p, status out
 *   through a buffer of its own, one copy each way; the _dev form takes DEVICE buffers (take stays a host array) and returns after
 *   one synchronisation of each stream that ran a part of the range.
 *   Workspace: 2 n^2 + n + ldw doubles per problem of each pipelined half (1.5 GiB for 384 problems of n = 512), kept on the
 *   handle until it is destroyed.
 * enlsip_gn_get_newton_form      kernel form of the last enlsip_gn_newton_direction_batched* on this handle: 0 general (256
 *     threads per problem in the factorisation), 1 one wave per problem (n <= 64), -1 none yet; after
 *     enlsip_gn_tsqr_newton_direction* also 2, the device-wide factorisation of its one matrix.
 * enlsip_gn_get_newton_stage_ms  HIP-event times (ms) of the four stages of the last call (b / p1 / d with the default
 *     dimensions; E; W22 and the right-hand side; factorisation, solves and p), summed over the pipelined halves that ran a part of
 *     the range; zeros unless enlsip_gn_set_profiling was on.  ms: 4 floats.
 */
int enlsip_gn_newton_direction_batched(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* Gamma, int64_t ldg,
                                       int64_t strideG, const int64_t* take, double* p, int* status);
int enlsip_gn_newton_direction_batched_dev(enlsip_gn_handle h, int64_t prob0, int64_t count, const double* dGamma, int64_t ldg,
                                           int64_t strideG, const int64_t* take, double* dp, int* dstatus);
int enlsip_gn_get_newton_form(enlsip_gn_handle h, int* form);
int enlsip_gn_get_newton_stage_ms(enlsip_gn_handle h, float* ms);

/* ---- row-sharded TSQR building blocks (multi-GPU config C4) ----------
 * One tall residual Jacobian whose ROWS are sharded over G GPUs; the (small) constraint data
 * At, cx are replicated.  Same mathematics as enlsip_gn_solve:  F_A, rankA, F_L11, p1 are
 * computed redundantly on every rank (bitwise identical), J*Q1 and d_temp = -J1 p1 - rx are
 * row-local, the unpivoted QR of [J2 | d_temp] is done on the local rows, and only the
 * n2 x n2 triangles travel.
 *
 * Local stage (device buffers in, device buffers out):
 *   dRloc  n2 x n2 upper-triangular factor of the local rows, column-major, PACKED (ld = n2), so the
 *          first n2*n2 doubles can be all-gathered as they are; the caller provides n*n doubles
 *          (n2 = n - rankA <= n is only known afterwards and is returned in *n2_out)
 *   dzloc  (Q_loc' d_loc)[1:n2]             (n doubles provided)
 *   tail_sq  ||(Q_loc' d_loc)[n2+1:]||^2    (host)
 *
 * Magnitudes: this pair computes plainly on the caller's data and is OUTSIDE the magnitude contract above — a J of magnitude 2^600
 * comes back with rankJ2 = 0 or not finite.  Its arguments cannot carry a shard's exponent; use enlsip_gn_tsqr_local_scaled_dev /
 * enlsip_gn_tsqr_combine_scaled_dev (below) or enlsip_gn_solve_tsqr where the inputs may leave the band 2^-400 .. 2^400.
 */
int enlsip_gn_tsqr_local_dev(enlsip_gn_handle h, int64_t m_loc, int64_t n, int64_t t,
                             const double* dJ, int64_t ldj, const double* drx,
                             const double* dAt, int64_t ldat, const double* dcx, double eps_rank,
                             double* dRloc, double* dzloc, double* tail_sq, int64_t* n2_out);
/*
 * Combine stage, run redundantly on every rank after the all-gather (RCCL) of the G local results:
 *   dRstack  G blocks of n2 x n2 (each column-major, ld = n2, i.e. the dRloc buffers packed to n2*n2)
 *   dzstack  G blocks of n2
 * Factors the stacked (G*n2) x n2 matrix (unpivoted CAQR, then the pivoted QR of its R — the same
 * plan as a single-GPU solve), solves, and applies Q1 of the handle's resident F_A (from the
 * local stage on the SAME handle).  HOST outputs: p (n), dlead (n2) = leading entries of
 * F_J2.Q' d, comb_tail_sq = squared norm of the remaining entries of the stacked rhs (add the
 * ranks' tail_sq for ||d||^2), info, jpvtJ2 (n2).
 */
int enlsip_gn_tsqr_combine_dev(enlsip_gn_handle h, int64_t G, int64_t n2,
                               const double* dRstack, const double* dzstack, double eps_rank,
                               double* p, double* dlead, double* comb_tail_sq,
                               enlsip_gn_info* info, int64_t* jpvtJ2);
/*
 * The two stages with the magnitude contract of enlsip_gn_solve.  A shard whose local result is nominated (largest |entry| of its R
 * or of its carried column above 2^440, not finite, or below 2^-440) and whose J, rx (A', cx) lie outside the band is factored
 * again on copies scaled by a power of two chosen by this rank alone; *e_out is the exponent (0: not rescaled):
 *   dRloc, dzloc, tail_sq are those of the shard times 2^-e (tail_sq times 2^-2e).
 * J and rx share the exponent: it brings the larger of the two near 1, or both to the two sides of 1 when they lie more than 2^400
 * apart, so that tail_sq stays a number.  A', cx are replicated: every rank reaches the same rankA and n2.
 * The combine takes every rank's exponent e[g] and tail_sq[g] (HOST arrays of G entries, tail_sq[g] at rank g's scale) beside the
 * gathered triangles, brings block g to the common scale 2^-max(e) (a block more than 2^1000 below the largest becomes zeros),
 * and returns d_norm = ||d||_2 over all ranks instead of a partial sum of squares, so that the caller never adds squares that
 * may overflow.  p, dlead (n2), d_norm, info, jpvtJ2 are those of the caller's data.
 */
int enlsip_gn_tsqr_local_scaled_dev(enlsip_gn_handle h, int64_t m_loc, int64_t n, int64_t t,
                                    const double* dJ, int64_t ldj, const double* drx,
                                    const double* dAt, int64_t ldat, const double* dcx, double eps_rank,
                                    double* dRloc, double* dzloc, double* tail_sq, int64_t* n2_out, int64_t* e_out);
int enlsip_gn_tsqr_combine_scaled_dev(enlsip_gn_handle h, int64_t G, int64_t n2,
                                      const double* dRstack, const double* dzstack,
                                      const int64_t* e, const double* tail_sq, double eps_rank,
                                      double* p, double* dlead, double* d_norm,
                                      enlsip_gn_info* info, int64_t* jpvtJ2);
/* Exponents of the last TSQR call on the handle (either stage pair, or enlsip_gn_solve_tsqr): *e_local = this rank's shard was
 * factored times 2^-e_local, *e_common = the combine ran at 2^-e_common (the largest exponent among the ranks).  Both 0 for
 * inputs inside the band; then ENLSIP_GN_ROUTE_RESCALED is clear in enlsip_gn_get_route, otherwise set. */
int enlsip_gn_tsqr_get_scale(enlsip_gn_handle h, int64_t* e_local, int64_t* e_common);

/* ---- the same, as ONE collective call (every rank of the communicator calls it with its row block) -------------------------
 *
 * Communicator of a handle (default: one rank, no exchange).  Exactly one of:
 *   enlsip_gn_tsqr_init_rccl     the library creates an RCCL communicator: rank 0 obtains 128 bytes from
 *                                enlsip_gn_tsqr_unique_id, the caller hands them to every rank by whatever means it has (Julia:
 *                                Distributed / MPI.jl; Python: torch.distributed broadcast), every rank calls init_rccl (collective,
 *                                ncclCommInitRank).  The handle's device must be the rank's GPU.  RCCL is loaded at run time
 *                                (librccl.so.1; ENLSIP_GN_RCCL_LIB overrides): the library has no link-time dependency on it.
 *   enlsip_gn_tsqr_set_comm      an existing ncclComm_t of the caller (not destroyed by the library); NULL = back to one rank.
 *   enlsip_gn_tsqr_set_exchange  any other transport: fn(ctx, dsend, drecv, bytes_per_rank, hip_stream) must all-gather
 *                                bytes_per_rank bytes of DEVICE memory from every rank into drecv (rank-major) and return 0 once
 *                                drecv is complete or the transfer is enqueued on hip_stream; dsend is complete when fn is called.
 *
 * enlsip_gn_solve_tsqr: rank g passes its m_loc rows of J and rx (device pointers; the row blocks may have different heights)
 * and the replicated At, cx.  One message per rank travels: the packed upper triangle of the local R (8 n2 (n2 + 1) / 2 bytes:
 * 4.2 MB at n2 = 1024), z = (Q_loc' d_loc)[1:n2], the squared norm of the local tail, the sender's n2 and the power of two its
 * shard was scaled by (0 inside the band: see "Magnitudes" above); its length depends on n
 * alone, so the ranks' counts agree even if their n2 do not — that case (the ranks see different constraint ranks) returns -13.
 * A rank that fails BEFORE the exchange (bad arguments, out of memory, a HIP error in its local stage) leaves its peers waiting
 * in the all-gather: such a failure is fatal for the communicator.  After a failed enlsip_gn_tsqr_init_rccl the handle has no
 * communicator and enlsip_gn_solve_tsqr returns an error until one is set again.  Every rank returns the same HOST
 * outputs: p (n), dlead (n2 <= n entries: leading entries of F_J2.Q' d), d_norm = ||d||_2 over all ranks, info, jpvtJ2 (n2 <= n).
 */
int enlsip_gn_tsqr_unique_id(void* id128);
int enlsip_gn_tsqr_init_rccl(enlsip_gn_handle h, const void* id128, int nranks, int rank);
int enlsip_gn_tsqr_set_comm(enlsip_gn_handle h, void* nccl_comm, int nranks, int rank);
int enlsip_gn_tsqr_set_exchange(enlsip_gn_handle h, enlsip_gn_allgather_fn fn, void* ctx, int nranks, int rank);
int enlsip_gn_solve_tsqr(enlsip_gn_handle h, int64_t m_loc, int64_t n, int64_t t,
                         const double* dJ, int64_t ldj, const double* drx,
                         const double* dAt, int64_t ldat, const double* dcx, double eps_rank,
                         double* p, double* dlead, double* d_norm, enlsip_gn_info* info, int64_t* jpvtJ2);
/* local / exchange / combine time (ms, HIP events) of the last enlsip_gn_solve_tsqr with profiling enabled */
int enlsip_gn_tsqr_get_stage_ms(enlsip_gn_handle h, float* ms3);
/* what moved the messages in the last enlsip_gn_solve_tsqr of this handle: an attached RCCL communicator is used for the
 * exchange even when it has ONE rank (a self-gather), so that the RCCL leg runs on a one-GPU box too */
enum {
    ENLSIP_GN_TRANSPORT_NONE = 0,     /* one rank, no communicator: a device copy */
    ENLSIP_GN_TRANSPORT_RCCL = 1,     /* ncclAllGather on the handle's stream */
    ENLSIP_GN_TRANSPORT_CALLBACK = 2  /* the caller's all-gather (enlsip_gn_tsqr_set_exchange) */
};
int enlsip_gn_tsqr_get_transport(enlsip_gn_handle h, int* transport);
/* The same with the evidence that the collective really spanned the communicator: *ranks = the handle's rank count, and
 * *rank_tags_seen = how many of the gathered messages carried, in their header, the rank their slot belongs to AND the same rank
 * count (every message is tagged by its sender; -1: nothing was gathered, n2 = 0).  transport == RCCL and rank_tags_seen == ranks
 * on every rank is "RCCL moved one message from each of N distinct ranks" (bench.py --config C4 prints and asserts it). */
int enlsip_gn_tsqr_get_exchange(enlsip_gn_handle h, int* transport, int* ranks, int* rank_tags_seen);

/* ---- the consumers around the subproblem on a row-sharded J -------------------------------------------------------------------
 * What Enlsip runs around the subproblem, for a J whose rows stay on their ranks: grad = J' (rx + J p) (p NULL: J' rx,
 * src/enlsip_functions.jl:2690, :2734, :2830), J p and A p of the line-search set-up (:2226-2229), the three sums dot(rx,rx),
 * dot(Jp,Jp), dot(Jp,rx) (:1561-1584, :2269) and the two multiplier estimates (:461-508, :514-537).  Rank g forms the products of its
 * shard (J_g p is row-local and stays on the rank), packs ONE message
 *     [ rank + 1 | rank count | n | 0 | g_g = J_g' v_g (n) | dot(rx_g,rx_g) | dot(Jp_g,Jp_g) | dot(Jp_g,rx_g) ]   v_g = rx_g + J_g p
 * of enlsip_gn_tsqr_products_msg_len(n) doubles (a multiple of two: 16-byte granules; the length depends on n alone), the messages
 * move in ONE exchange step the way the triangles of enlsip_gn_solve_tsqr move (RCCL where a communicator is attached, also with one
 * rank; the callback otherwise; a device copy for one rank without a communicator; errors 994 / 995 as there), and every rank adds the
 * G messages in RANK order, 0 first, with plain additions: every rank holds the same bits.  A message whose header names another n,
 * another rank count than G or another slot than the one it lies in returns -13 (rank and rank count 0 = "not stated" pass).
 *
 * Order of summation: fixed by m_loc, n, ldj and the operands alone (chunks of a fixed height, 64 strided partial sums and a
 * butterfly inside a chunk, chunks ascending, ranks ascending; no floating-point atomics): a call repeats its bits on any handle and
 * after any history, and a shard read in place (any start row, ldj = the whole height; only the 8-byte alignment of a double is
 * assumed) gives the bits of a copy of its rows.  Two different splits of the same rows differ by rounding.
 *
 * Magnitudes: these calls compute plainly on the caller's data and are OUTSIDE the magnitude contract above, like the stage pair
 * enlsip_gn_tsqr_local_dev / _combine_dev.  When the handle's last sharded solve was rescaled (enlsip_gn_tsqr_get_scale not (0, 0),
 * or A', cx were factored on a scaled copy) the resident F_A may belong to a scaled copy: the collective forms return -15 and
 * compute nothing.  enlsip_gn_tsqr_products_local_dev is stateless and unaffected.
 *
 * enlsip_gn_tsqr_products_local_dev    the local stage alone, for callers that move the messages themselves; needs NOTHING resident and
 *     leaves the handle's resident data alone.  dJ (m_loc x n, column-major, ldj >= m_loc), drx (m_loc), dp (n) or NULL, dJp (m_loc;
 *     receives J_g p when dp is given, else untouched) or NULL, dmsg (msg_len doubles): device.  m_loc = 0 is legal and gives a zero
 *     message.  The header carries the rank and rank count of the handle's communicator, or 0 / 0 without one (the caller may fill
 *     them in).  Returns 0; before anything is launched: -2 m_loc, -3 n (1..1024), -4 dJ NULL, -5 ldj < m_loc, -6 drx NULL,
 *     -8 dmsg NULL.
 * enlsip_gn_tsqr_products_combine_dev  dmsgs: G messages, rank-major (device); grad (n) and sums (3): host, either may be NULL.
 *     -2 G, -3 n, -4 dmsgs NULL, -13 a header does not fit (nothing is written).
 * The collective forms work on the shard (dJ, drx, dAt, dcx: kept alive and unchanged by the caller, as for the one-GPU consumers)
 * and the communicator of the handle's last successful enlsip_gn_solve_tsqr, or enlsip_gn_tsqr_combine_dev / _combine_scaled_dev after a
 * local stage on the same handle; every other solve entry withdraws that.  Without it they return -7 and launch nothing.  Every rank
 * calls them; a rank that fails before the exchange leaves its peers waiting, as in the solve.  One synchronisation of the handle's
 * stream per call (the callback transport adds the one before it calls out).
 * enlsip_gn_tsqr_products         p (host n) or NULL; dJp (device m_loc, receives this rank's J_g p) or NULL; grad (host n), sums
 *     (host 3), Ap (host t: C.A p on the active rows, from the replicated A' of the solve, no exchange; needs p) or NULL each.
 * enlsip_gn_tsqr_first_lagrange   first_lagrange_mult_estimate! (:461-508) on the resident F_A: grad_fx (host n), or NULL for J' rx
 *     over the ranks (then collective); diag_scale (host t) or NULL; lambda (host t), grad_res.  The arithmetic is that of
 *     enlsip_gn_first_lagrange.  Returns 1 for a singular triangular system.
 * enlsip_gn_tsqr_second_lagrange  second_lagrange_mult_estimate! (:514-537), collective: b = J1' (rx + J p_gn) with
 *     J1 = (J F_A.Q)[:, 1:t] is formed as (F_A.Q' (J' (rx + J p_gn)))[1:t], from the product above and F_A.Q' on an n-vector.  It
 *     reads no factored workspace, so the -7 of enlsip_gn_second_lagrange has no counterpart; the ROUNDING ORDER differs from the
 *     one-GPU call (which forms J1 first), the results agree within the bound of either.
 */
int64_t enlsip_gn_tsqr_products_msg_len(int64_t n);
int enlsip_gn_tsqr_products_local_dev(enlsip_gn_handle h, int64_t m_loc, int64_t n, const double* dJ, int64_t ldj, const double* drx,
                                      const double* dp, double* dJp, double* dmsg);
int enlsip_gn_tsqr_products_combine_dev(enlsip_gn_handle h, int64_t G, int64_t n, const double* dmsgs, double* grad, double* sums);
int enlsip_gn_tsqr_products(enlsip_gn_handle h, const double* p, double* dJp, double* grad, double* sums, double* Ap);
int enlsip_gn_tsqr_first_lagrange(enlsip_gn_handle h, const double* grad_fx, const double* diag_scale, double eps_rank,
                                  double* lambda, double* grad_res);
int enlsip_gn_tsqr_second_lagrange(enlsip_gn_handle h, const double* p_gn, const double* diag_scale, double eps_rank,
                                   double* lambda);

/* ---- Newton direction on a row-sharded J --------------------------------------------------------------------------------------
 * newton_search_direction (src/enlsip_functions.jl:348-423) after its Hessian sums, for the sharded caller whose
 * check_gn_direction answered method_code == 2.  Gamma = r_mat - c_mat (n x n, column-major, ldg >= n; the Hessian sums stay with
 * the caller, as everywhere else).  The step is the batched one (enlsip_gn_newton_direction_batched above) on what the combine stage
 * of a sharded solve leaves resident on EVERY rank, replicated and bitwise equal:
 *     from the handle:      F_A, tauA, F_L11.p, p1 and rankA, n2, code, dimA of its state record
 *     from its sub-handle:  R and Pi of the stacked problem (J2 Pi = Q R), d = F_J2.Q' d_stack carried beside R, rankJ2, dimJ2
 *     E = F_A.Q' Gamma F_A.Q, sW22 = sym(E22) + Pi R'R Pi', rhs = -E21 p1 + Pi R' d[1:kp], cholesky, two solves, p = F_A.Q [p1; p2]
 * No row of any shard is read and NOTHING IS EXCHANGED: the call is not collective, a rank may call it alone, and ranks that pass the
 * same Gamma get the same bits.  Special cases as in the batched form: rankA == n returns p1 as it is (:379-381); a rank-deficient
 * working set with t >= n > rankA takes E = E[F_L11.p, F_L11.p] (:396-399).
 *
 * It works on the resident result of the handle's last successful enlsip_gn_solve_tsqr, or enlsip_gn_tsqr_combine_dev /
 * _combine_scaled_dev after a local stage on the same handle; every other solve entry withdraws that, as for the
 * enlsip_gn_tsqr_products family.  Nothing resident is rewritten: F_A, p1, both state records, the sub-handle's factors, pivots and
 * carried d, the shard pointers and what the enlsip_gn_tsqr_products family answers stay as they were.  The call has a workspace of
 * its own (2 n^2 + n doubles and a few words), kept on the handle until it is destroyed.
 *
 * Host form: Gamma, p (n), not_posdef (may be NULL) on the host, Gamma staged in and p out through a buffer of the call, one copy
 * each way.  *not_posdef = 1 with p = 0 when the symmetrised W22 is not positive definite (:413-421; LAPACK dpotrf semantics: a pivot
 * <= 0 or NaN), else 0.  _dev form: dGamma, dp (n) and dstatus (one int, 0 or 1; may be NULL) are DEVICE buffers.  Either form
 * returns after one synchronisation of the handle's stream.
 * Returns 0, or, before anything is launched and with nothing written: -1 h is NULL, -3 Gamma is NULL, -5 p is NULL, -7 no sharded
 * solve is resident, -4 ldg < n (n is the resident sharded solve's, so this is tested after -7: without one the answer is -7 whatever
 * ldg is), -15 the sharded solve was rescaled (enlsip_gn_tsqr_get_scale not (0, 0), or A', cx factored on
 * a scaled copy: the rule and the reason of enlsip_gn_tsqr_products), -8 rank-deficient working set with t < n (the reference
 * indexes out of bounds there; enlsip_gn_newton_direction's -7).
 *
 * The factorisation of the one n2 x n2 matrix takes one of two forms: the one-workgroup kernel of the batched call (one problem), or
 * a right-looking blocked Cholesky spread over the device, two launches per 32-column panel and no synchronisation but the kernel
 * boundary.  ENLSIP_GN_NEWTON_WIDE=0 / 1 (read at handle creation) never / always takes the device-wide form; DESIGN.md section 7
 * has the measurement behind the default.  enlsip_gn_get_newton_form reports 2 after a call that took the device-wide form, else 0 / 1
 * as above (a call with rankA == n factors nothing and reports 0 / 1 under either setting); enlsip_gn_get_newton_stage_ms returns the four stage times (set-up; E; W22 and the right-hand side; factorisation, solves
 * and p) when profiling is on.  The two forms agree to rounding, not bit for bit.
 */
int enlsip_gn_tsqr_newton_direction(enlsip_gn_handle h, const double* Gamma, int64_t ldg, double* p, int64_t* not_posdef);
int enlsip_gn_tsqr_newton_direction_dev(enlsip_gn_handle h, const double* dGamma, int64_t ldg, double* dp, int* dstatus);

/* ---- instrumentation: HIP-event time (ms) of the stages of the last solve ------------------ */
enum {
    ENLSIP_GN_STAGE_CONSTRAINT = 0, /* F_A, F_L11, p1, T factor            */
    ENLSIP_GN_STAGE_JQ1 = 1,        /* J*Q1 and d_temp                      */
    ENLSIP_GN_STAGE_PANEL = 2,      /* all CAQR panel factorisations (tiles and tree nodes)                     */
    ENLSIP_GN_STAGE_UPDATE = 3,     /* EVERY trailing-update launch of the sweep: the level-0 far passes, the tree
                                     * levels and a pair's second-panel columns (sum of their HIP-event times)  */
    ENLSIP_GN_STAGE_PIVOT = 4,      /* pivoted QR of R0 + triangular solves */
    ENLSIP_GN_STAGE_TOTAL = 5,
    ENLSIP_GN_STAGE_COUNT = 6
};
/* enable = 1 records events per stage and around the level-0 far updates (adds stream bubbles; off by default); enable = 2 also
 * around every other trailing-update launch of the sweep (tree levels, second-panel columns): ENLSIP_GN_STAGE_UPDATE then is the
 * sum over ALL update launches and enlsip_gn_get_update_totals reports them; with enable = 1 it is the far passes alone and the
 * other update launches stay inside ENLSIP_GN_STAGE_PANEL (hundreds of event pairs would stretch a C4 sweep by ~3 %) */
int enlsip_gn_set_profiling(enlsip_gn_handle h, int enable);
int enlsip_gn_get_stage_ms(enlsip_gn_handle h, float* ms /* ENLSIP_GN_STAGE_COUNT */);
/* average duration (ms) and count of the level-0 trailing-update launches of the last solve,
 * measured with HIP events on the handle's stream (bench.py roofline leg) */
int enlsip_gn_get_update_stats(enlsip_gn_handle h, float* avg_ms, int64_t* launches,
                               double* algorithmic_bytes);
/* the same launch by launch (sweep order: one entry per panel, or per panel pair where two panels share a pass): SURVEY 8d
 * bytes 8 (2 m_k n_k + m_k b + b^2) of the panels the launch applies, and its HIP-event time.  *count = launches recorded;
 * at most cap entries are written. */
int enlsip_gn_get_update_table(enlsip_gn_handle h, int64_t cap, double* algorithmic_bytes, float* ms, int64_t* count);
/* How the last solve on this handle was launched (what the library chose on its own): *pipeline_split = number of problems the
 * first of the two pipelined halves owned (0: one stream), *panel_pairs = 1 when the CAQR sweep applied two panels per pass over
 * the far trailing columns, *tile_rows = rows of a level-0 CAQR tile.  Tests use it to assert that a configuration really took
 * the path a benchmark times. */
int enlsip_gn_get_launch_plan(enlsip_gn_handle h, int64_t* pipeline_split, int* panel_pairs, int64_t* tile_rows);
/* All trailing-update launches of the last profiled solve: HIP-event time of the level-0 far passes (the launches of
 * enlsip_gn_get_update_table) and of every OTHER update launch (tree levels, second-panel columns), and SURVEY 8d's
 * 8 (2 m_k n_k + m_k b + b^2) summed over EVERY panel of the sweep with n_k = all columns right of the panel (times the batch):
 * bytes / (far_ms + other_ms) is the trailing update's rate counted over all of its kernels (bench.py: roofline.all_update_kernels) */
int enlsip_gn_get_update_totals(enlsip_gn_handle h, float* far_ms, float* other_ms, int64_t* other_launches,
                                double* all_panels_bytes);
/* GB/s (read + write) of an in-place non-temporal read-modify-write stream over `bytes` of the handle's scratch memory with the
 * trailing update's access shape, HIP events around `reps` passes: the same-box ceiling of an in-place update (bench.py) */
int enlsip_gn_measure_stream(enlsip_gn_handle h, int64_t bytes, int reps, double* gbytes_per_s);
/* Which kernel-selection branches of the host code the last solve on this handle took: one bit per branch (and per template
 * instantiation a branch chooses between), ORed over both pipeline halves, every chunk and both attempts of a solve.  Every
 * place in the library that picks a kernel from the shape sets a bit; tests/test_dispatch_grid.py derives a stratified shape
 * list from the same conditions and asserts that every bit is hit by a case that is compared against the oracle — a new fast
 * path gets a bit here and cannot ship without such a case.  enlsip_gn_route_name(bit) = its name, NULL past the last bit. */
enum {
    ENLSIP_GN_ROUTE_CONSTRAINT_WAVE32 = 0,   /* k_constraint_small<32>: n, t <= 32                                     */
    ENLSIP_GN_ROUTE_CONSTRAINT_WAVE64,       /* k_constraint_small<64>: n <= 64, t <= 63                               */
    ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R1_256,   /* k_constraint, matrices in LDS, rows <= 32                              */
    ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R1_512,   /* rows <= 64                                                             */
    ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R2,       /* rows <= 128                                                            */
    ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R4,       /* rows <= 256                                                            */
    ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R8,       /* rows <= 512                                                            */
    ENLSIP_GN_ROUTE_CONSTRAINT_LDS_R16,      /* rows <= 1024                                                           */
    ENLSIP_GN_ROUTE_CONSTRAINT_GLOBAL,       /* k_constraint factoring in global memory (beyond the LDS area, n > 512) */
    ENLSIP_GN_ROUTE_CONSTRAINT_REG4,         /* F_A by k_geqp3_reg<4> (n <= 256, beyond the LDS area)                  */
    ENLSIP_GN_ROUTE_CONSTRAINT_REG8,         /* F_A by k_geqp3_reg<8> (n <= 512)                                       */
    ENLSIP_GN_ROUTE_CONSTRAINT_DIST,         /* more than 64 constraints beyond the LDS area: launch-per-step QR       */
    ENLSIP_GN_ROUTE_JQ1_FUSED_SMALL,         /* k_jq1_factor_small: J*Q1 + the one narrow panel in one launch          */
    ENLSIP_GN_ROUTE_JQ1_ROWS32,              /* k_jq1_rows<32>: a lane per row, n <= 32                                */
    ENLSIP_GN_ROUTE_JQ1_ROWS2,               /* k_jq1_rows2: two lanes per row, 32 < n <= 64                           */
    ENLSIP_GN_ROUTE_JQ1_ROWS64,              /* k_jq1_rows<64> (leading dimensions beyond 2^23)                        */
    ENLSIP_GN_ROUTE_JQ1_V2_N128,             /* k_jq1_v2<2,4,2>: kA = 64, n = 128, m multiple of 32                    */
    ENLSIP_GN_ROUTE_JQ1_V2_N256,
    ENLSIP_GN_ROUTE_JQ1_V2_N384,
    ENLSIP_GN_ROUTE_JQ1_V2_N512,
    ENLSIP_GN_ROUTE_JQ1_MFMA,                /* k_jq1_mfma: every other shape                                          */
    ENLSIP_GN_ROUTE_JQ1_PLAIN,               /* k_jq1 (ENLSIP_GN_UPDATE_REFLECTORS; also behind get_JQ1 / Newton)      */
    ENLSIP_GN_ROUTE_SWEEP_PLAIN,             /* CAQR: one panel per pass over the trailing columns                     */
    ENLSIP_GN_ROUTE_SWEEP_PAIRS,             /* two panels per pass over the far columns                               */
    ENLSIP_GN_ROUTE_SWEEP_LOOKAHEAD,         /* a pair's far update split over two streams                             */
    ENLSIP_GN_ROUTE_SWEEP_PASSENGER,         /* last narrow panel: d rides through the factor kernel                   */
    ENLSIP_GN_ROUTE_SWEEP_TREE,              /* more than one tile: tree levels                                        */
    ENLSIP_GN_ROUTE_SWEEP_TILE256,           /* 256-row tiles (m <= 256 or opts.tile_rows = 256)                       */
    ENLSIP_GN_ROUTE_SWEEP_TILE512,
    ENLSIP_GN_ROUTE_SWEEP_REFLECTORS,        /* trailing update reflector by reflector (ENLSIP_GN_UPDATE_REFLECTORS)   */
    ENLSIP_GN_ROUTE_SWEEP_UPPER_INPUT,       /* J already upper triangular (TSQR combine of one shard): no sweep       */
    ENLSIP_GN_ROUTE_PIVOT_WAVE32,            /* k_pivot_small<32>: kp <= 32, n2 + 1 <= 64, one problem                 */
    ENLSIP_GN_ROUTE_PIVOT_WAVE64,            /* k_pivot_small<64>: kp <= 64, n2 + 1 <= 64                              */
    ENLSIP_GN_ROUTE_PIVOT_WAVE2,             /* k_pivot_small2: two problems per wave, kp <= 32, n2 + 1 <= 32, batch   */
    ENLSIP_GN_ROUTE_PIVOT_LDS_R1_256,        /* k_pivot_solve (pivoted QR of R0 in LDS, or only the solves behind the  */
    ENLSIP_GN_ROUTE_PIVOT_LDS_R1_512,        /*                blocked form), by rows min(m, n): <= 32, 64, 128, ...   */
    ENLSIP_GN_ROUTE_PIVOT_LDS_R2,
    ENLSIP_GN_ROUTE_PIVOT_LDS_R4,
    ENLSIP_GN_ROUTE_PIVOT_LDS_R8,
    ENLSIP_GN_ROUTE_PIVOT_LDS_R16,
    ENLSIP_GN_ROUTE_PIVOT_BLOCKS,            /* run_qrcp_block: register blocks (R0 beyond the LDS area, kp <= 512)    */
    ENLSIP_GN_ROUTE_PIVOT_BLOCKS_448,        /*   forms of the block kernel that were launched: 448 rows               */
    ENLSIP_GN_ROUTE_PIVOT_BLOCKS_512,
    ENLSIP_GN_ROUTE_PIVOT_BLOCKS_256,
    ENLSIP_GN_ROUTE_PIVOT_BLOCKS_128,
    ENLSIP_GN_ROUTE_PIVOT_HYBRID,            /* kp > 512: launch-per-step head, then the register blocks               */
    ENLSIP_GN_ROUTE_PIVOT_STEPS,             /* kp > 512 with ENLSIP_GN_QRCP_HYBRID=0: one launch per step to the end  */
    ENLSIP_GN_ROUTE_PIPELINE_SPLIT,          /* batch >= 128: two halves on two streams                                */
    ENLSIP_GN_ROUTE_CHUNKED,                 /* batch > 32768: consecutive chunks                                      */
    ENLSIP_GN_ROUTE_SECOND_ATTEMPT,          /* some A was rank deficient: J2 wider than speculated, redone            */
    ENLSIP_GN_ROUTE_RESCALED,                /* inputs beyond the range of plain sums of squares: solved on a copy     */
                                             /* scaled by a power of two (LAPACK's dnrm2 / dlarfg behaviour)           */
    ENLSIP_GN_ROUTE_SWEEP_XMAP,              /* a pair's far update read its grid XCD-locally (batch <= 8, >= 16 tiles) */
    ENLSIP_GN_ROUTE_COUNT
};
int enlsip_gn_get_route(enlsip_gn_handle h, uint64_t* mask);
const char* enlsip_gn_route_name(int bit);
/* Debugging aid: copies the working matrix W of problem `prob` (ldw x (n + 1): J*Q1 with the CAQR factors of [J2 | d] in place) as
 * it stands after the last solve to host memory; *ldw_out = its leading dimension; -3 when cap_doubles is too small.  Comparing
 * the copies of two handles (ENLSIP_GN_PAIR=0 against the default, say) locates a defect of the sweep panel by panel. */
int enlsip_gn_debug_copy_W(enlsip_gn_handle h, int64_t prob, double* out, int64_t* ldw_out, int64_t cap_doubles);

#ifdef __cplusplus
}
#endif
#endif /* ENLSIP_GN_H */
