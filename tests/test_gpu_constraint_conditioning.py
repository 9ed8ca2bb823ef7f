"""The constraint stage on ill-conditioned A, on every route (cases: tests/constraint_cases.py; their premises — reference
agreement, recompute counts, pivot leads, sensitivity to a wrong recompute, rank margins — are certified on the CPU by
tests/test_constraint_cases_host.py, so a failure here means a kernel is wrong).

Every case runs on a fresh GNSolver through both entry flows (factor_constraints + solve_factored, and the one-call solve) and is
held to the oracle (oracle/gn_oracle.py, LAPACK): route bits, (rankA, code, dimA) at every eps_rank of the case, jpvtA over the
leading rankA positions, jpvtL where the host test certified it, |R| of F_A and F_L11 over the leading rankA rows, the defining
identities of tests/factor_identities.py with that module's TOL_COL / TOL_GRAM, the column-pivoting inequality on the returned R,
b, and p — against the oracle within the conditioning of the kept constraints and by its definition (feasibility on consistent
constraints, no descent left in the null space of the kept constraints; the method of tests/test_gpu_defining_properties.py).
Then: dependent(q) problems whose second attempt runs other kernels than the first, alone and inside a ragged batch of five whose
other members must not feel the defect; batches of mixed kinds against their single solves, bit for bit; and the leader cluster
on the J side (t = 0), where it reaches the pivoted QR of R0 — the blocked form included — intact.

Allowances (floors measured by the host test on LAPACK's factors and the restatement of dlaqp2, times factor_identities.MARGIN for
the reduction orders LAPACK does not have, under a cap that keeps a 1e-9 change of R failing):
  |R| over the leading rankA rows, relative to |R_00| ....... floor 5.3e-16, TOL_R = 1.2e-14 (cap 1e-10)
  column-pivoting inequality, relative to R_kk^2 ............ floor 0 on LAPACK's R and on the restatement's; the allowance is one
                                                              rounding of each of the two sums compared, eps, times the margin:
                                                              TOL_INEQ = 4.4e-15.  The cluster's leads are 1.6e-6 in the squares.
  |diag R| of F_J2 on the J side, relative to each entry .... floor 1.5e-11 (eps / DELTA-conditioned), TOL_DIAG_J = 3e-10 (cap 1e-9)
MI355X maxima over every case (the module prints those of a run when it is done, pytest -s): |R| 6.2e-16 (F_A), 5.1e-16 (F_L11); pivoting
inequality violated nowhere; identities 9.3e-16 (columns), 1.5e-15 (Gram); feasibility 2.1e-16; p 9.8e-15 on well-conditioned kept
rows, 4.2e-3 of 1e-13 cond otherwise; b of code -1 1.8e-4 of its bound; projected gradient 1.6 eps cond; J side |diag R| 1.4e-11.
Batches: the constraint side of every member is its single solve's bit for bit; p differs by at most 4.4e-16 where the batch takes
pivot_wave2.  Ragged batch with a deficient member: the others move by nothing where the second attempt runs the first one's
kernels, and by at most 1.8e-15 (p) / 7.0e-16 (d) where the launch crosses a dispatch boundary (allowance TOL_MOVED = 5e-14)."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import gn_oracle as go, synth

sys.path.insert(0, str(Path(__file__).resolve().parent))
import constraint_cases as cc                     # noqa: E402
import factor_identities as fi                    # noqa: E402
import test_constraint_cases_host as host         # noqa: E402

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
FLOOR_R = 6.0e-16
TOL_R = min(fi.MARGIN * FLOOR_R, 1e-10)
TOL_INEQ = fi.MARGIN * max(0.0, EPS)
FLOOR_DIAG_J = 1.5e-11
TOL_DIAG_J = min(fi.MARGIN * FLOOR_DIAG_J, 1e-9)
TOL_P = 1e-11                 # well conditioned (tests/test_gpu_parity.py); ill conditioned: 1e-13 cond of the kept constraints
TOL_MOVED = fi.MARGIN * fi.FLOOR_COL      # p, d of a well-conditioned problem redone by other kernels (second attempt of a launch): two
                                          # backward-stable factorisations of the same Gaussian J, the floor of the column identities
TOL_B = 1e-10                 # code -1: b = Q_L' (-cx[p]) (tests/test_gpu_ragged_batch.py: check_problem)

MEASURED = {}                 # maxima of the current run (test_zz_report)
CASES = cc.cases()
FACTOR_A, FACTOR_L11 = fi.FACTOR_A, fi.FACTOR_L11


def note(key, value):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(value))


@pytest.fixture
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def rel(a, b):
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / (nb if nb > 0 else 1.0))


def same(a, b):
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return a.shape == b.shape and np.array_equal(a, b)


def cond_of(M):
    if M.size == 0:
        return 1.0
    s = np.linalg.svd(M, compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else math.inf


# ---- checks of one solved problem ----------------------------------------------------------------------------------------------------
def check_factors(s, A, ref, c, prob=0, L_certified=False):
    """F_A and F_L11 resident on `s` for problem `prob`: pivots, |R|, identities, pivoting inequality."""
    r = ref.rankA
    FA, FL = s.factor(FACTOR_A, prob), s.factor(FACTOR_L11, prob)
    RA, pA = np.asarray(FA.R), np.asarray(FA.p)
    assert np.array_equal(pA[:r], ref.jpvtA[:r]), (c["id"], "jpvtA", pA[:r], ref.jpvtA[:r])
    same_cols = np.nonzero(pA == ref.jpvtA)[0]
    dR = host.r_difference(RA[:, same_cols], np.asarray(ref.F_A.R)[:, same_cols], r)
    note("R.A", dR)
    assert dR <= TOL_R, (c["id"], "|R| of F_A", dR)
    res = fi.check_factor_identity(FA, A.T)
    RL, pL = np.asarray(FL.R), np.asarray(FL.p)
    resL = fi.check_factor_identity(FL, RA.T)
    for k, v in zip(("id.qt", "id.q", "id.gram"), np.maximum(res, resL)):
        note(k, v)
    assert max(res[0], res[1], resL[0], resL[1]) <= fi.TOL_COL and max(res[2], resL[2]) <= fi.TOL_GRAM, (c["id"], res, resL)
    ineq = host.pivot_inequality(RA, r)
    note("ineq.A", ineq)
    assert ineq <= TOL_INEQ, (c["id"], "pivoting inequality F_A", ineq)
    if L_certified:
        assert np.array_equal(pL[:r], ref.jpvtL[:r]), (c["id"], "jpvtL")
    if r and np.array_equal(pL[:r], ref.jpvtL[:r]):
        same_cols = np.nonzero(pL == ref.jpvtL)[0]
        dL = host.r_difference(RL[:, same_cols], np.asarray(ref.F_L11.R)[:, same_cols], r)
        note("R.L11", dL)
        assert dL <= TOL_R, (c["id"], "|R| of F_L11", dL)
        ineqL = host.pivot_inequality(RL, r)
        note("ineq.L11", ineqL)
        assert ineqL <= TOL_INEQ, (c["id"], "pivoting inequality F_L11", ineqL)


def check_direction(out, J, rx, A, cx, ref, c, consistent=True):
    """b and p of one solve: against the oracle, and p by its definition on the constraints the pivoted QR kept."""
    m, n = J.shape
    t = A.shape[0]
    r = ref.rankA
    assert (out.rankA, out.code, out.dimA) == (ref.rankA, ref.code, ref.rankA), (c["id"], out.rankA, out.code, out.dimA, ref.rankA)
    assert out.rankJ2 == ref.rankJ2 == min(m, n - r), (c["id"], out.rankJ2, ref.rankJ2)
    assert np.array_equal(out.jpvtA[:r], ref.jpvtA[:r]), (c["id"], "jpvtA")
    assert np.all(np.isfinite(out.p)) and np.all(np.isfinite(out.b)) and np.all(np.isfinite(out.d))
    S = ref.jpvtA[:r] - 1
    AS, cS = A[S], cx[S]
    kS = cond_of(AS)
    if ref.code == 1:
        assert np.array_equal(out.b, -cx[out.jpvtA - 1]), (c["id"], "b")
    elif r:
        # b = Q_L' (-cx[p]) with Q_L from the pivoted QR of R_A': its leading rankA columns are those of a matrix of condition
        # cond(A_S), so they, and b[:rankA] with them, are defined to eps cond(A_S) (the suite's 1e-13 cond rule for forward errors)
        eb = float(np.linalg.norm(out.b[:r] - ref.b[:r]) / max(np.linalg.norm(ref.b), 1e-300))
        note("b.code-1/(tol)", eb / max(TOL_B, 1e-13 * kS))
        assert eb <= max(TOL_B, 1e-13 * kS), (c["id"], "b", eb, kS)
        assert abs(np.linalg.norm(out.b) - np.linalg.norm(ref.b)) <= TOL_B * np.linalg.norm(ref.b), (c["id"], "||b||")
    nJ = float(np.linalg.norm(J, 2))
    scale = nJ * (nJ * np.linalg.norm(out.p) + np.linalg.norm(rx))
    unique = m >= n - r
    if unique:
        ep = rel(out.p, ref.p)
        note("p/(1e-13 cond)" if kS > 100 else "p", ep / (1e-13 * kS) if kS > 100 else ep)
        assert ep <= max(TOL_P, 1e-13 * kS), (c["id"], "p against the oracle", ep, kS)
    # definition: feasible where the constraints can all hold, and no descent left in the null space of the kept constraints
    if r and (ref.code == 1 or (c["kind"] == "dependent" and consistent)):
        feas = float(np.linalg.norm(A @ out.p + cx) / (np.linalg.norm(A, 2) * np.linalg.norm(out.p) + np.linalg.norm(cx)))
        note("feasibility", feas)
        assert feas <= 1e-13, (c["id"], "feasibility", feas)          # backward error: free of cond (test_gpu_defining_properties.py)
    if r < n:
        Z = np.linalg.svd(AS, full_matrices=True)[2][r:].T if r else np.eye(n)
        g = float(np.linalg.norm(Z.T @ (J.T @ (J @ out.p + rx))) / scale)
        note("projected gradient/(eps cond)", g / (EPS * max(kS, 1.0)))
        # Z comes from an SVD of A_S: its columns are defined to eps cond(A_S), and so is the projection (a few roundings: 8)
        assert g <= max(1e-13, 8 * EPS * kS), (c["id"], "projected gradient", g, kS)
    if c["kind"] == "zero":
        pu = np.linalg.lstsq(J, -rx, rcond=None)[0]
        assert rel(out.p, pu) <= TOL_P, (c["id"], "unconstrained minimiser", rel(out.p, pu))


def reference(c, eps):
    """the oracle's solution of a case, shared with the host test's certificates"""
    return host.solved(c)[4][eps]


@pytest.fixture(scope="module", autouse=True)
def report_maxima():
    """prints the maxima of the run beside their allowances when the module is done (pytest -s)"""
    yield
    print("\nmaxima of this run:", {k: f"{v:.2e}" for k, v in sorted(MEASURED.items())}, flush=True)
    print(f"allowances: TOL_R {TOL_R:.1e} TOL_INEQ {TOL_INEQ:.1e} TOL_COL {fi.TOL_COL:.1e} TOL_GRAM {fi.TOL_GRAM:.1e} "
          f"TOL_DIAG_J {TOL_DIAG_J:.1e} TOL_MOVED {TOL_MOVED:.1e}", flush=True)


# ---- 1. every case, both flows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_case_on_both_flows(c, solver):
    J, rx, A, cx = cc.build(c)
    m, n, t = c["m"], c["n"], c["t"]
    L_cert = host.pivots_L_certified(c)
    consistent = bool(c["params"].get("consistent", 1))
    for i, eps in enumerate(c["eps_ranks"]):
        ref = reference(c, eps)
        if c["ranks"] is not None:
            assert ref.rankA == c["ranks"][i]
        last = i == len(c["eps_ranks"]) - 1
        # flow 1: the constraint stage alone, then the solve that goes on with it
        # (enlsip_gn_get_route speaks of the last SOLVE: the one-problem constraint stage alone records none, so the bits are
        # asserted on flow 2, which goes through the same run_constraint_stage)
        got = solver.factor_constraints(m, A, cx, eps_rank=eps)
        assert got == (ref.rankA, ref.code, ref.rankA), (c["id"], eps, got, ref.rankA, ref.code)
        if last:
            check_factors(solver, A, ref, c, L_certified=L_cert)
        out1 = solver.solve_factored(J, rx, t, eps_rank=eps)
        check_direction(out1, J, rx, A, cx, ref, c, consistent)
        # flow 2: the one-call solve
        out2 = solver.solve(J, rx, A, cx, eps_rank=eps)
        route = solver.route()
        assert c["bits"] <= route, (c["id"], c["bits"], route)
        assert ("second_attempt" in route) == (ref.rankA < min(n, t)), (c["id"], route)
        check_direction(out2, J, rx, A, cx, ref, c, consistent)
        if last:
            check_factors(solver, A, ref, c, L_certified=L_cert)
        assert np.array_equal(out1.jpvtA, out2.jpvtA) and np.array_equal(out1.jpvtL, out2.jpvtL), (c["id"], "the two flows differ")


# ---- 2. second attempt across a dispatch boundary --------------------------------------------------------------------------------
SECOND = [c for c in cc.second_attempt_cases() if c["name"] != "same_kernels"]


def _second_reference(c):
    J, rx, A, cx = cc.build_second(c)
    return J, rx, A, cx, go.gn_subproblem(J, rx, A, cx)


@pytest.mark.parametrize("c", SECOND, ids=[c["id"] for c in SECOND])
def test_second_attempt_runs_other_kernels(c, solver):
    J, rx, A, cx, ref = _second_reference(c)
    cd = dict(id=c["id"], kind="dependent")
    out = solver.solve(J, rx, A, cx)
    route = solver.route()
    assert "second_attempt" in route, route
    moved = c["first"] ^ c["second"]
    assert moved and moved <= route, (c["id"], moved, route)          # both attempts' kernels ran
    assert ref.rankA == c["t"] - c["q"]
    check_direction(out, J, rx, A, cx, ref, cd)
    check_factors(solver, A, ref, cd)


SECOND5 = cc.second_attempt_cases(5)


@pytest.mark.parametrize("c", SECOND5, ids=[c["id"] for c in SECOND5])
def test_second_attempt_inside_a_ragged_batch(c, solver):
    """Five problems with their own t_k >= t; member 2 has t constraints and is rank deficient by q.  A ragged launch is planned
    for its smallest t_k, so the first attempt runs at n2 = n - t and the second at n - t + q: the cases are those whose routes
    for a launch of five differ there, and both attempts' bits must be reported.  The other members are held to the batch in
    which member 2 has full rank (bit for bit where the two attempts run the same kernels, see below), and member 2 is its single
    solve's and the oracle's."""
    from enlsip_gn import GNSolver
    m, n, t = c["m"], c["n"], c["t"]
    ts = [t + e for e in cc.RAGGED_EXTRA]
    probs = [synth.make_problem(c["seed"] + 10 + k, m, n, tk) for k, tk in enumerate(ts)]
    Jd, rxd, Ad, cxd, ref = _second_reference(c)
    outs = []
    for deficient in (True, False):
        ps = list(probs)
        ps[2] = (Jd, rxd, Ad, cxd) if deficient else cc.build_second(c, deficient=False)
        At, cx, tv = GNSolver.pack_ragged([p[2] for p in ps], [p[3] for p in ps], n)
        J = np.stack([np.asfortranarray(p[0]).T for p in ps])
        rx = np.stack([p[1] for p in ps])
        outs.append(solver.solve_batched_ragged(J, rx, At, cx, tv))
        route = solver.route()
        assert ("second_attempt" in route) == deficient
        assert c["first"] <= route, (c["id"], deficient, c["first"] - route)
        if deficient:
            assert c["second"] <= route, (c["id"], c["second"] - route)           # both attempts' kernels ran
        else:
            assert not (c["second"] - c["first"]) & route, (c["id"], route)
    (p, b, d, infos, jA, jL, jJ), other = outs
    # the second attempt redoes EVERY member of the launch at the launch's new width: the panel count, the passenger rule, the
    # pivot form and the J*Q1 form are chosen per launch.  Where both attempts run the same kernels (the control case) nothing of
    # the untouched members may move.  Where the launch crosses a boundary they go through other arithmetic, and bit for bit cannot
    # hold: then their constraint side is still bit for bit, their pivots equal, and p, d agree to TOL_MOVED.  MI355X: 0 on the
    # control; p / d move by 4.2e-16 / 3.7e-16 (wave -> wave64), 8.0e-16 / 6.3e-16 (wave64 -> lds), 1.2e-15 / 6.1e-16 (lds ->
    # blocks), 1.8e-15 / 7.0e-16 (fused -> rows), 5.8e-16 / 5.9e-16 (passenger).
    same_j_kernels = c["first"] == c["second"]
    for k in (0, 1, 3, 4):
        assert infos[k] == other[3][k] and infos[k][0] == ts[k]
        for name, a, o in (("b", b, other[1]), ("jpvtA", jA, other[4]), ("jpvtL", jL, other[5])):
            assert same(a[k], o[k]), (c["id"], k, name)
        assert np.array_equal(jJ[k, :n - ts[k]], other[6][k, :n - ts[k]]), (c["id"], k, "jpvtJ2")
        dp, dd = rel(p[k], other[0][k]), rel(d[k], other[2][k])
        print(f"{c['id']} member {k}: p differs by {dp:.2e}, d by {dd:.2e} from the batch without the defect", flush=True)
        if same_j_kernels:
            assert same(p[k], other[0][k]) and same(d[k], other[2][k]), (c["id"], k, dp, dd)
        else:
            note("moved p, d (launch crossed a boundary)", max(dp, dd))
            assert dp <= TOL_MOVED and dd <= TOL_MOVED, (c["id"], k, dp, dd)
    single = GNSolver(device=0)
    try:
        sk = single.solve(Jd, rxd, Ad, cxd)
    finally:
        single.close()
    r = ref.rankA
    assert infos[2][:4] == (r, ref.rankJ2, -1, r) == (sk.rankA, sk.rankJ2, sk.code, sk.dimA)
    assert np.array_equal(jA[2, :r], ref.jpvtA[:r]) and np.array_equal(jA[2, :t], sk.jpvtA)
    assert rel(p[2], sk.p) <= TOL_P and rel(d[2], sk.d) <= TOL_P
    if m >= n - r:
        assert rel(p[2], ref.p) <= TOL_P


# ---- 3. batch forms ------------------------------------------------------------------------------------------------------------------
def _batch_members(form, count):
    n, t = cc.form_shapes()[form]
    pool = [c for c in CASES if (c["n"], c["t"]) == (n, t)]
    want = (lambda c: c["kind"] == "leader_cluster", lambda c: c["kind"] == "graded",
            lambda c: c["kind"] == "dependent" and c["params"]["q"] == 2, lambda c: c["kind"] == "row_scaled",
            lambda c: c["kind"] == "dependent" and not c["params"]["consistent"])      # every kind certified at the default eps_rank
    return [next(c for c in pool if ok(c)) for ok in want][:count]


@pytest.mark.parametrize("form,count", [("constraint_wave32", 5), ("constraint_wave64", 5), ("constraint_reg4", 2),
                                        ("constraint_dist", 2)])
def test_batches_of_mixed_kinds_match_their_single_solves(form, count, solver):
    from enlsip_gn import GNSolver
    members = _batch_members(form, count)
    probs = [cc.build(c) for c in members]
    n, t = members[0]["n"], members[0]["t"]
    J = np.stack([np.asfortranarray(q[0]).T for q in probs])
    rx = np.stack([q[1] for q in probs])
    At = np.stack([q[2] for q in probs])
    cx = np.stack([q[3] for q in probs])
    p, b, d, infos, jA, jL, jJ = solver.solve_batched(J, rx, At, cx)
    assert form in solver.route(), solver.route()
    m = members[0]["m"]
    j_bits = lambda batch: {x for x in cc.dg.expected_route(batch, m, n, t) if not x.startswith("constraint_")}
    same_j = j_bits(count) == j_bits(1)
    for k, (c, q) in enumerate(zip(members, probs)):
        ref = reference(c, cc.SQRT_EPS)
        r = ref.rankA
        assert infos[k][:4] == (r, ref.rankJ2, ref.code, r), (c["id"], infos[k])
        assert np.array_equal(jA[k, :r], ref.jpvtA[:r]), c["id"]
        check_factors(solver, q[2], ref, c, prob=k, L_certified=host.pivots_L_certified(c))
        single = GNSolver(device=0)
        sk = single.solve(*q)
        assert infos[k] == (sk.rankA, sk.rankJ2, sk.code, sk.dimA, sk.dimJ2, sk.status), c["id"]
        # the constraint side (the wave forms hold several problems per workgroup): bit for bit
        for name, a, o in (("b", b[k], sk.b), ("jpvtA", jA[k], sk.jpvtA), ("jpvtL", jL[k], sk.jpvtL)):
            assert same(a, o), (c["id"], name, "batch member differs from its single solve")
        for which in (FACTOR_A, FACTOR_L11):
            assert same(solver.factor(which, k).R, single.factor(which, 0).R), (c["id"], which, "R differs from the single solve's")
        # the J side: bit for bit where batch and single solve run the same kernels; a batch of small problems takes
        # pivot_wave2, which a single problem never does: then equal pivots, p and d within the conditioning of the kept rows
        assert np.array_equal(jJ[k, :n - r], sk.jpvtJ2), (c["id"], "jpvtJ2")
        dp, dd = rel(p[k], sk.p), rel(d[k], sk.d)
        print(f"{c['id']} in a batch of {count}: p differs by {dp:.2e}, d by {dd:.2e} from its single solve "
              f"(same J-side kernels: {same_j})", flush=True)
        if same_j:
            assert same(p[k], sk.p) and same(d[k], sk.d), (c["id"], dp, dd)
        else:
            kS = cond_of(q[2][ref.jpvtA[:r] - 1])
            assert dp <= max(TOL_P, 1e-13 * kS) and dd <= max(TOL_P, 1e-13 * kS), (c["id"], dp, dd, kS)
        single.close()


# ---- 4. the cluster on the J side ------------------------------------------------------------------------------------------------
JSIDE = cc.j_side_cases()


@pytest.mark.parametrize("c", JSIDE, ids=[c["id"] for c in JSIDE])
def test_cluster_reaches_the_pivoted_qr_of_R0(c, solver):
    m, n, batch = c["m"], c["n"], c["batch"]
    probs = [cc.j_side_problem(c["seed"] + k, m, n) for k in range(batch)]
    none, nocx = np.zeros((0, n)), np.zeros(0)
    if batch == 1:
        o = solver.solve(probs[0][0], probs[0][1], none, nocx)
        outs = [(o.rankJ2, o.jpvtJ2, o.p)]
    else:
        J = np.stack([np.asfortranarray(q[0]).T for q in probs])
        p, b, d, infos, jA, jL, jJ = solver.solve_batched(J, np.stack([q[1] for q in probs]), np.zeros((batch, 0, n)), np.zeros((batch, 0)))
        outs = [(infos[k][1], jJ[k], p[k]) for k in range(batch)]
    assert c["bits"] <= solver.route(), (c["id"], c["bits"], solver.route())
    for k, ((J, rx), (rankJ2, jp, p)) in enumerate(zip(probs, outs)):
        ref = go.gn_subproblem(J, rx, none, nocx)
        assert rankJ2 == ref.rankJ2 == n
        assert np.array_equal(jp[:n], ref.jpvtJ2), (c["id"], k, int((jp[:n] != ref.jpvtJ2).sum()), "pivots differ")
        dg_ = np.abs(solver.factor(fi.FACTOR_J2, k).diagR())
        dd = float((np.abs(dg_ - np.abs(ref.F_J2.diagR())) / np.abs(ref.F_J2.diagR())).max())
        note("J side |diag R|", dd)
        assert dd <= TOL_DIAG_J, (c["id"], dd)
        kJ = cond_of(J)
        assert rel(p, ref.p) <= max(TOL_P, 1e-13 * kJ), (c["id"], rel(p, ref.p), kJ)
