"""CPU premises of tests/test_gpu_constraint_conditioning.py (cases: tests/constraint_cases.py), from NumPy and the oracle alone, so
that a failure on the GPU means the kernel is wrong and not the case:

* coverage: every constraint_* bit of the header is reached by a leader_cluster and a graded case (a shape with t >= n admits no
  cluster: it carries graded and row_scaled instead, listed by test_coverage_of_every_constraint_bit);
* reference agreement: the restatement of dlaqp2 (oracle/lapack_semantics.py: geqp2) and LAPACK's dgeqp3 (oracle/gn_oracle.py:
  qr_colnorm) give the same pivots over the leading rankA positions of F_A and of F_L11, and the same rankA and code at every
  eps_rank of the case;
* recompute count: a counting copy of the restatement (kept here) takes the `temp2 <= sqrt(eps)` branch at least t - 1 times on a
  leader_cluster case and at least once on a graded one;
* tie freedom, every case of every kind: the smallest relative lead of a chosen pivot of F_A over its runner-up (the computation of
  tests/test_tsqr_edges_host.py::test_pivot_margins) is at least LEAD_FLOOR = 100 x the largest relative difference between the
  restatement's and LAPACK's |diag R| over the same cases;
* sensitivity: the counting copy with a mutated step — the recompute branch removed, the recompute taken over rows j.. instead of
  j+1.., the partial norms not carried along on a pivot exchange — changes at least one of the leading rankA pivots of every
  leader_cluster case.  One more mutation, vn2 left at its old value by a recompute, changes no pivot on inputs whose leads
  exceed the error of the norm downdate (all of these): a stale vn2 is never smaller than the true one, so temp2 is never larger,
  the branch is taken at least as often, and every norm taken there is the exact one.  The test asserts what that mutation does
  change (the branch count: every later step recomputes every cluster column) and that its pivots stay LAPACK's, so that this
  stays on record; a kernel with that defect is slower, not wrong, on such inputs;
* rank margins: for every plateau, dependent and zero case the last kept and the first dropped |R_ii| / |R_00| lie at least 10x
  either side of sqrt(kA) eps_rank (tests/test_tsqr_edges_host.py::test_rank_margins);
* the reference floors of the two allowances the GPU test measures with (|R| against the oracle's, and the column-pivoting
  inequality), from LAPACK's own factors: see FLOOR_* below.

Measured here over every case (pytest -s prints them per case):
  largest relative difference of |diag R|, restatement against LAPACK ......... 9.7e-10 (the 1e-8 ends of graded and plateau
                                                                                 diagonals); asserted under DIAG_DIFF_MAX = 2e-9, so
                                                                                 LEAD_FLOOR = 2e-7 and RANK_GAP_FLOOR = 2e-5
  smallest lead of a chosen pivot, leader_cluster ............................. 8.0e-7 on the A side, 8.0e-7 on R0 of the J side;
                                                                                 every other kind at least 2.0e-5
  recomputes: leader_cluster t - 1 (7 .. 81), graded 3 .. 158; closest |R_ii| of a graded / row_scaled / cluster diagonal to the rank
  tolerance 5.2e-3 (relative)
  |R| of the restatement against LAPACK's over the leading rankA rows ......... 5.3e-16 of |R_00|
  column-pivoting inequality on LAPACK's and the restatement's R .............. violated nowhere (0)
"""
import math

import numpy as np
import pytest

from oracle import gn_oracle as go, lapack_semantics as ls

import constraint_cases as cc
import dispatch_grid as dg

CASES = cc.cases()
IDS = [c["id"] for c in CASES]
MUTATIONS = ("no_recompute", "rows_from_j", "swap_not_carried", "vn2_stale")

# ---- measured floors (asserted below; repeated in the GPU test's head and DESIGN.md §2) -----------------------------------------
DIAG_DIFF_MAX = 2.0e-9          # restatement against LAPACK, relative |diag R| over the leading rankA entries, every case
LEAD_FLOOR = 100.0 * DIAG_DIFF_MAX
RANK_GAP_FLOOR = 1e4 * DIAG_DIFF_MAX    # kinds without designed ranks: no |R_ii| within this relative distance of the rank tolerance


# ---- the counting copy of the restatement -------------------------------------------------------------------------------------------
def geqp2_counting(A, mutation=None):
    """oracle/lapack_semantics.py: geqp2 without carried columns, counting the recompute branch; mutation: one of MUTATIONS.
    Returns (factors, jpvt 1-based, recomputes)."""
    A = np.array(A, dtype=np.float64, order="F", copy=True)
    rows, cols = A.shape
    k = min(rows, cols)
    jpvt = np.arange(1, cols + 1, dtype=np.int64)
    vn1 = np.linalg.norm(A, axis=0)
    vn2 = vn1.copy()
    count = 0
    for j in range(k):
        pvt = j + int(np.argmax(vn1[j:cols]))
        if pvt != j:
            A[:, [j, pvt]] = A[:, [pvt, j]]
            jpvt[[j, pvt]] = jpvt[[pvt, j]]
            if mutation != "swap_not_carried":
                vn1[pvt] = vn1[j]
                vn2[pvt] = vn2[j]
        beta, t_j, scale = ls.dlarfg(A[j, j], A[j + 1:, j])
        if t_j != 0.0:
            A[j + 1:, j] *= scale
            v = np.concatenate([[1.0], A[j + 1:, j]])
            if j + 1 < cols:
                w = v @ A[j:, j + 1:]
                A[j:, j + 1:] -= t_j * np.outer(v, w)
        A[j, j] = beta
        for c in range(j + 1, cols):
            if vn1[c] != 0.0:
                temp = max(1.0 - (abs(A[j, c]) / vn1[c]) ** 2, 0.0)
                temp2 = temp * (vn1[c] / vn2[c]) ** 2
                if temp2 <= ls.TOL3Z and mutation != "no_recompute":
                    count += 1
                    lo = j if mutation == "rows_from_j" else j + 1
                    if j + 1 < rows:
                        vn1[c] = float(np.linalg.norm(A[lo:, c]))
                        if mutation != "vn2_stale":
                            vn2[c] = vn1[c]
                    else:
                        vn1[c] = 0.0
                        vn2[c] = 0.0
                else:
                    vn1[c] *= math.sqrt(temp)
    return A, jpvt, count


# ---- shared references, computed once ------------------------------------------------------------------------------------------------
_cache = {}


def solved(c):
    """(J, rx, A, cx, {eps_rank: oracle solution}, restatement (factors, jpvt, count) of A')"""
    if c["id"] not in _cache:
        J, rx, A, cx = cc.build(c)
        refs = {e: go.gn_subproblem(J, rx, A, cx, e) for e in c["eps_ranks"]}
        _cache[c["id"]] = (J, rx, A, cx, refs, geqp2_counting(A.T))
    return _cache[c["id"]]


def smallest_lead(M, jpvt, steps):
    """tests/test_tsqr_edges_host.py::test_pivot_margins: the remaining column norms at step k are those of rows k.. of the
    unpivoted QR of M with its columns in pivot order."""
    R = np.linalg.qr(M[:, np.asarray(jpvt) - 1], mode="r")
    rem = np.sqrt(np.cumsum((R ** 2)[::-1], axis=0)[::-1])
    worst = np.inf
    for k in range(min(steps, R.shape[0])):
        if k + 1 < R.shape[1] and rem[k, k + 1:].max() > 0:
            worst = min(worst, float(rem[k, k] / rem[k, k + 1:].max()) - 1.0)
    return worst


def pivots_certified(c) -> bool:
    """Cases whose pivots the GPU test compares with the oracle's: the lead of every chosen pivot of F_A is above LEAD_FLOOR.
    Always so for a leader cluster (asserted); by measurement for the other kinds."""
    J, rx, A, cx, refs, _ = solved(c)
    ref = refs[c["eps_ranks"][-1]]
    if ref.rankA == 0:
        return False
    return smallest_lead(A.T, ref.jpvtA, ref.rankA) >= LEAD_FLOOR


def pivots_L_certified(c) -> bool:
    """The same for F_L11 = qr(R_A'): only full-rank cases (below rankA the rows of R_A past rankA are rounding dust)."""
    J, rx, A, cx, refs, _ = solved(c)
    ref = refs[c["eps_ranks"][-1]]
    if ref.rankA == 0 or ref.code != 1:
        return False
    return smallest_lead(np.asarray(ref.F_A.R).T, ref.jpvtL, ref.rankA) >= LEAD_FLOOR


# ---- 1. shapes and coverage --------------------------------------------------------------------------------------------------------
def test_listed_shapes_reach_their_bits():
    for (n, t), want in cc.LISTED_SHAPES.items():
        got = cc.constraint_bits(dg.expected_route(1, cc.rows_of(n), n, t))
        assert got == want, ((n, t), got, want)


def test_derived_shapes_are_the_smallest_of_their_bits():
    shapes = cc.constraint_shapes()
    print("derived shapes:", [(n, t, sorted(b)) for n, t, b in shapes], flush=True)
    for n, t, bits in shapes:
        assert cc.constraint_bits(dg.expected_route(1, cc.rows_of(n), n, t)) == bits
        for (n2, t2) in ((n - 1, t), (n, t - 1)):                  # one step smaller leaves the set (or the lattice)
            if t2 >= cc.T_MIN and n2 >= cc.T_MIN and n2 != t2 and (t2 > n2) == (t > n):
                assert cc.constraint_bits(dg.expected_route(1, cc.rows_of(n2), n2, t2)) != bits, ((n, t), (n2, t2))


def test_coverage_of_every_constraint_bit():
    cov = cc.coverage()
    assert set(cov) == set(cc.header_constraint_bits()) and len(cov) == 12
    for bit, kinds in cov.items():
        assert {"leader_cluster", "graded"} <= kinds, (bit, kinds)
    # shapes without a cluster (t >= n): each has a graded and a row_scaled case
    without = sorted({(c["n"], c["t"]) for c in CASES if not cc.admits_leader(c["n"], c["t"])})
    print("shapes that admit no leader_cluster:", without, flush=True)
    for (n, t) in without:
        kinds = {c["kind"] for c in CASES if (c["n"], c["t"]) == (n, t)}
        assert {"graded", "row_scaled"} <= kinds and "leader_cluster" not in kinds, ((n, t), kinds)
    # every form has the full set of kinds
    for f, (n, t) in cc.form_shapes().items():
        kinds = {c["kind"] for c in CASES if (c["n"], c["t"]) == (n, t)}
        assert kinds == {"leader_cluster", "graded", "row_scaled", "plateau", "dependent", "zero"}, (f, kinds)
    assert set(cc.form_shapes()) == set(cc.FORMS)


# ---- 2. reference agreement, recompute count, leads ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatement_agrees_with_lapack(c):
    J, rx, A, cx, refs, (fac, jp, count) = solved(c)
    n, t = c["n"], c["t"]
    kA = min(n, t)
    dg_r = np.abs(np.diag(fac[:kA, :kA]))
    for i, e in enumerate(c["eps_ranks"]):
        ref = refs[e]
        rank = ls.pseudo_rank(np.diag(fac[:kA, :kA]), e)
        assert (rank, 1 if rank == t else -1) == (ref.rankA, ref.code), (c["id"], e, rank, ref.rankA)
        if c["ranks"] is not None:
            assert ref.rankA == c["ranks"][i], (c["id"], e, ref.rankA, c["ranks"])
        assert np.array_equal(jp[:ref.rankA], ref.jpvtA[:ref.rankA]), (c["id"], e)
    ref = refs[c["eps_ranks"][-1]]
    r = ref.rankA
    diff = float((np.abs(dg_r[:r] - np.abs(ref.F_A.diagR()[:r])) / np.abs(ref.F_A.diagR()[:r])).max()) if r else 0.0
    # F_L11 = qr(R_A') by the restatement, on LAPACK's R_A: same pivots over the leading rankA positions where they are certified
    facL, jpL, _ = geqp2_counting(np.asarray(ref.F_A.R).T)
    lead = smallest_lead(A.T, ref.jpvtA, r) if r else np.inf
    leadL = smallest_lead(np.asarray(ref.F_A.R).T, ref.jpvtL, r) if r else np.inf
    if pivots_L_certified(c):
        assert np.array_equal(jpL[:r], ref.jpvtL[:r]), c["id"]
    print(f"{c['id']}: rankA {[refs[e].rankA for e in c['eps_ranks']]} recomputes {count} lead F_A {lead:.2e} F_L11 {leadL:.2e} "
          f"|diag R| restatement vs LAPACK {diff:.2e}", flush=True)
    assert diff <= DIAG_DIFF_MAX, (c["id"], diff)
    if r:                                       # tie freedom of F_A, every kind: jpvtA is compared on the device for every case
        assert lead >= LEAD_FLOOR and pivots_certified(c), (c["id"], lead)
    if c["kind"] == "leader_cluster":
        assert count >= t - 1, (c["id"], count)
    if c["kind"] == "graded":
        assert count >= 1, (c["id"], count)
    # a graded diagonal passes the rank tolerance somewhere: no entry may sit close enough to it for rounding to decide the rank
    if c["kind"] in ("graded", "row_scaled", "leader_cluster"):
        d = np.abs(ref.F_A.diagR())
        gap = float(np.abs(d / (d[0] * math.sqrt(d.size) * c["eps_ranks"][-1]) - 1.0).min())
        print(f"{c['id']}: closest |R_ii| to the rank tolerance: {gap:.2e} (relative)", flush=True)
        assert gap >= RANK_GAP_FLOOR, (c["id"], gap)


def test_every_route_keeps_its_certified_cases():
    """Every constraint bit keeps a graded case (ranks, |R|, identities certified above) and a leader_cluster whose pivots are
    certified."""
    for bit in cc.header_constraint_bits():
        assert any(bit in c["bits"] and c["kind"] == "graded" for c in CASES), bit
        assert any(bit in c["bits"] and c["kind"] == "leader_cluster" and pivots_certified(c) for c in CASES), bit


# ---- 3. sensitivity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in CASES if c["kind"] == "leader_cluster"], ids=[i for i in IDS if i.startswith("leader")])
def test_cluster_pivots_feel_a_wrong_recompute(c):
    J, rx, A, cx, refs, (fac, jp, count) = solved(c)
    r = refs[c["eps_ranks"][-1]].rankA
    assert r == c["t"]
    changed = {}
    for mut in MUTATIONS:
        _, jm, cm = geqp2_counting(A.T, mut)
        changed[mut] = (int((jm[:r] != jp[:r]).sum()), cm)
    print(f"{c['id']}: pivots changed / recomputes under {changed} (unmutated: {count} recomputes)", flush=True)
    assert changed["no_recompute"][0] >= 1 and changed["rows_from_j"][0] >= 1 and changed["swap_not_carried"][0] >= 1, (c["id"], changed)
    # a stale vn2 only adds recomputes (module head): no pivot moves, the branch count rises
    assert changed["vn2_stale"][0] == 0 and changed["vn2_stale"][1] > count, (c["id"], changed)


# ---- 4. rank margins ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in CASES if c["kind"] in ("plateau", "dependent", "zero")],
                         ids=[c["id"] for c in CASES if c["kind"] in ("plateau", "dependent", "zero")])
def test_rank_margins(c):
    J, rx, A, cx, refs, _ = solved(c)
    for e in c["eps_ranks"]:
        ref = refs[e]
        d = np.abs(ref.F_A.diagR())
        if c["kind"] == "zero":
            assert ref.rankA == 0 and np.all(d == 0.0)
            continue
        tol = math.sqrt(d.size) * e
        r = ref.rankA
        kept = float(d[r - 1] / d[0])
        dropped = float(d[r:].max() / d[0]) if r < d.size else 0.0
        print(f"{c['id']} eps_rank {e:.1e}: rank {r} of {d.size}, last kept {kept:.2e}, first dropped {dropped:.2e}, "
              f"tolerance {tol:.2e} (of |R_00|)", flush=True)
        assert d[0] >= e and kept >= 10.0 * tol and dropped <= 0.1 * tol, (c["id"], e, kept, dropped, tol)


# ---- 5. the floors of the GPU test's allowances, from LAPACK's factors --------------------------------------------------------
FLOOR_R = 6.0e-16               # | |R| - |R_restatement| | / |R_00| over the leading rankA rows, LAPACK against the restatement
FLOOR_PIVOT_INEQ = 0.0          # max_k (max_{j>k} sum_{i>=k} R_ij^2 / R_kk^2 - 1) on LAPACK's and the restatement's R, where positive


def r_difference(R, Rref, rank):
    """max | |R| - |Rref| | over the leading `rank` rows, relative to |Rref_00|"""
    if rank == 0:
        return 0.0
    return float(np.abs(np.abs(R[:rank]) - np.abs(Rref[:rank])).max() / abs(Rref[0, 0]))


def pivot_inequality(R, rank):
    """The column-pivoting inequality R_kk^2 >= max_{j>k} sum_{i>=k} R_ij^2 over the leading `rank` steps: its worst violation
    relative to R_kk^2 (0 when it holds everywhere)."""
    R = np.asarray(R)
    if rank == 0 or R.size == 0:
        return 0.0
    rem = np.cumsum((R ** 2)[::-1], axis=0)[::-1]                # rem[k, j] = sum_{i >= k} R_ij^2
    worst = 0.0
    for k in range(min(rank, R.shape[0])):
        if k + 1 < R.shape[1]:
            worst = max(worst, float(rem[k, k + 1:].max() / R[k, k] ** 2) - 1.0)
    return worst


def test_reference_floors_over_every_case():
    worst_r = worst_rl = worst_i = 0.0
    for c in CASES:
        J, rx, A, cx, refs, (fac, jp, _) = solved(c)
        ref = refs[c["eps_ranks"][-1]]
        r = ref.rankA
        kA = min(c["n"], c["t"])
        if r:
            assert pivots_certified(c), c["id"]
            # same pivots over the leading r positions: the rows of R agree up to sign on the columns both put in the same place
            same = np.nonzero(jp == ref.jpvtA)[0]
            worst_r = max(worst_r, r_difference(np.triu(fac[:kA])[:, same], np.asarray(ref.F_A.R)[:, same], r))
        worst_i = max(worst_i, pivot_inequality(ref.F_A.R, r), pivot_inequality(ref.F_L11.R, r), pivot_inequality(np.triu(fac[:kA]), r))
    print(f"floors over {len(CASES)} cases: |R| restatement against LAPACK {worst_r:.2e}, pivoting inequality on LAPACK's R "
          f"{worst_i:.2e}", flush=True)
    assert worst_r <= FLOOR_R and worst_i <= FLOOR_PIVOT_INEQ, (worst_r, worst_i)


# ---- 6. the J side and the second attempt --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.j_side_cases(), ids=[c["id"] for c in cc.j_side_cases()])
def test_j_side_cluster_reaches_R0_intact(c):
    """t = 0: J2 = J.  The lead floor is measured on R0 of the restatement of the HIP plan (unpivoted QR, then the pivoted QR of
    its R factor), not on J."""
    J, rx = cc.j_side_problem(c["seed"], c["m"], c["n"])
    n = c["n"]
    ref = go.gn_subproblem(J, rx, np.zeros((0, n)), np.zeros(0))
    assert ref.rankJ2 == n and n <= c["m"] - 8
    f0, _ = ls.geqr2(J)
    R0 = np.triu(f0[:n, :n])
    fac, jp, count = geqp2_counting(R0)
    assert np.array_equal(jp, ref.jpvtJ2)
    lead = smallest_lead(R0, ref.jpvtJ2, n)
    diff = float((np.abs(np.abs(np.diag(fac)) - np.abs(ref.F_J2.diagR())) / np.abs(ref.F_J2.diagR())).max())
    changed = {mut: int((geqp2_counting(R0, mut)[1] != jp).sum()) for mut in MUTATIONS}
    print(f"{c['id']}: recomputes {count} lead on R0 {lead:.2e} |diag R| plan vs LAPACK {diff:.2e} pivots changed {changed}", flush=True)
    assert count >= n - 1 and lead >= LEAD_FLOOR and diff <= DIAG_DIFF_MAX
    assert changed["no_recompute"] >= 1 and changed["rows_from_j"] >= 1 and changed["swap_not_carried"] >= 1
    assert changed["vn2_stale"] == 0


@pytest.mark.parametrize("batch", [1, 5])
def test_second_attempt_cases_cross_their_boundaries(batch):
    names = set()
    for c in cc.second_attempt_cases(batch):
        J, rx, A, cx = cc.build_second(c)
        ref = go.gn_subproblem(J, rx, A, cx)
        d = np.abs(ref.F_A.diagR())
        tol = math.sqrt(d.size) * go.SQRT_EPS
        r = c["t"] - c["q"]
        print(f"{c['id']}: only in the first attempt {sorted(c['first'] - c['second'])}, only in the second "
              f"{sorted(c['second'] - c['first'])}", flush=True)
        assert (ref.rankA, ref.code) == (r, -1)
        assert d[r - 1] / d[0] >= 10 * tol and d[r:].max() / d[0] <= 0.1 * tol
        assert smallest_lead(A.T, ref.jpvtA, r) >= LEAD_FLOOR
        assert (c["first"] != c["second"]) == (c["name"] != "same_kernels")
        # the launch is planned for the smallest t of its members: none of the ragged batch has fewer than the deficient one
        assert min(cc.RAGGED_EXTRA) == 0 and cc.RAGGED_EXTRA[2] == 0 and c["t"] + max(cc.RAGGED_EXTRA) <= dg.Q1R_MAXK
        names.add(c["name"])
    assert len({(c["m"], c["n"], c["t"], c["q"]) for c in cc.second_attempt_cases(batch)}) == len(names) == 6
