"""The solve on structurally sparse J and bound-constraint A, on every route (cases: tests/sparse_cases.py; their premises — the
oracle's identities on them, LAPACK's identity reflectors, zero diagonals and signed-permutation Q_A, pivot leads, the teeth of
the exact checks — are certified on the CPU by tests/test_sparse_cases_host.py, so a failure here means a kernel is wrong).

Every case runs on a fresh GNSolver (with the environment, flags and tile height of its forced variant), must report the route it
was picked for, and is held to
  1. the defining identities of tests/factor_identities.py with that module's tolerances; rankA, rankJ2, code of the oracle; jpvtJ2
     of the oracle where the host test certified the leads; p against the oracle within max(1e-11, 1e-13 cond) (cond: of the kept
     columns of J2 and of the kept rows of A) where the dropped columns are fixed by structure; the column-pivoting inequality on
     F_J2.R (TOL_INEQ of tests/test_gpu_constraint_conditioning.py); finite outputs;
  2. exact pass-through, `upper`: Q'v and Qv equal v bit for bit on rows kp.. and |d| = |rx| there (tau = 0 makes T = 0 and every
     update C - V 0; the pivoted QR of R0 works on rows < kp only).  Rows of an all-zero tile (lastrows, any kind that has one):
     ||Q'e_i|| = 1 within TOL_COL — no bit claim, the tree moves such rows;
  3. zero columns: rankJ2 = the number of non-zero columns, diagR() exactly 0.0 on the dropped positions, p exactly 0.0 on the zero
     columns, the dropped positions hold exactly the zero columns — on pivot_wave32 / wave64 / wave2 (the batch of five) / the LDS
     form / pivot_blocks_128 / _256 / _448 / _512 / pivot_hybrid / pivot_steps;
  4. bounds: jpvtA of the oracle (bounds_tied: the idamax rule), the explicit Q_A within TOL_COL of LAPACK's entries in {0, +-1},
     feasibility 1e-13, p[i_k] = -cx_k / a_k within 1e-13 of the largest bound value (entry by entry LAPACK itself is off by
     9.0e-13 where |cx_k| = 2.7e-5: sparse_cases.check_bounds), check_direction of tests/test_gpu_constraint_conditioning.py against
     the oracle; bounds_dup: second_attempt, rank t - 1, code -1, the kept pivots, |R_A| (TOL_R), |b| entry by entry (TOL_B),
     feasibility, p against the oracle (check_dup says why b is compared in magnitude and jpvtJ2 is not compared);
  5. a batch of five kinds and a ragged batch of three with bounds against their single solves (bit for bit where batch and single
     solve run the same J-side kernels, TOL_MOVED elsewhere);
  6. handle health: after its case the same handle solves a Gaussian problem of another shape within 1e-11 of the oracle.
Every figure is printed before it is asserted (pytest -s); the module prints the maxima of the run when it is done.

Oracle floors on these cases (host test): columns 1.1e-15, Gram 9.5e-16, d 6.4e-16, under FLOOR_COL / FLOOR_GRAM / FLOOR_D.
MI355X maxima over the 155 tests (31 s): columns 1.5e-15 (TOL_COL 5e-14), Gram 2.0e-15 (4e-14), d 1.8e-15 (6e-14), pivoting
inequality violated nowhere, p 2.2e-14 (1e-11) and 1.7e-3 of 1e-13 cond, |Q_A - LAPACK's| 4.4e-16, feasibility 1.3e-16, p[i_k]
3.8e-16, rows of zero tiles | ||Q'e_i|| - 1 | 1.1e-16, bounds_dup |R_A| 2.0e-16 and |b| 1.8e-16, handle health 1.3e-15; every
exact assertion (pass-through on every sweep route and forced variant, zero diagonals, p == 0.0, tied pivots) held as ==; the
batch of five and the ragged batch equal their single solves bit for bit, pivot_wave2 included."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import factor_identities as fi                        # noqa: E402
import sparse_cases as sc                             # noqa: E402
import test_constraint_cases_host as cch              # noqa: E402
import test_gpu_constraint_conditioning as gcc        # noqa: E402
import test_sparse_cases_host as host                 # noqa: E402

pytestmark = pytest.mark.gpu

CASES = sc.cases()
TOL_P = gcc.TOL_P
TOL_INEQ = gcc.TOL_INEQ
TOL_MOVED = gcc.TOL_MOVED
MEASURED = {}


def note(key, value):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def report_maxima():
    yield
    print("\nmaxima of this run:", {k: f"{v:.2e}" for k, v in sorted(MEASURED.items())}, flush=True)
    print(f"allowances: TOL_COL {fi.TOL_COL:.1e} TOL_GRAM {fi.TOL_GRAM:.1e} TOL_D {fi.TOL_D:.1e} TOL_INEQ {TOL_INEQ:.1e} "
          f"TOL_P {TOL_P:.1e} TOL_MOVED {TOL_MOVED:.1e}", flush=True)


def _handle(c):
    from enlsip_gn import GNSolver
    with fi.handle_env(c["env"]):
        return GNSolver(device=0, flags=c["flags"], tile_rows=c["tile_rows"])


class _Out:
    def __init__(self, p, d, rankA):
        self.p, self.d, self.rankA = p, d, rankA


def check_problem(s, c, k, prob, out_p, out_d, info, jJ):
    """checks 1 to 3 of the module head for problem k of case c, resident on handle s as problem `prob`; info = (rankA, rankJ2, code)"""
    (J, rx, A, cx), ref = sc.solved(c, k)
    m, n = J.shape
    tag = (c["id"], k)
    kind = c["kinds"][k] if c["kinds"] else c["kindJ"]
    assert info == (ref.rankA, ref.rankJ2, ref.code), (tag, info, (ref.rankA, ref.rankJ2, ref.code))
    assert np.all(np.isfinite(out_p)) and np.all(np.isfinite(out_d)), tag
    res = fi.check_solve_identities(fi.SolverAccess(s, m, n, prob), J, rx, A, cx, _Out(out_p, out_d, ref.rankA))
    print(f"identities {c['id']} prob {k}: " + " ".join(f"{key}={v:.1e}" for key, v in sorted(res.items())), flush=True)
    for key, v in res.items():
        note("gram" if key.endswith(".gram") else key if key in ("d", "d_cond") else "columns", v)
    fi.assert_within(res, "full", tag)
    FJ = s.factor(fi.FACTOR_J2, prob)
    r2 = ref.rankJ2
    certified = host.pivots_certified(c, k)
    if certified:
        assert np.array_equal(np.asarray(jJ)[:r2], ref.jpvtJ2[:r2]), (tag, "jpvtJ2", int((np.asarray(jJ)[:r2] != ref.jpvtJ2[:r2]).sum()))
    ineq = cch.pivot_inequality(np.asarray(FJ.R), r2)
    note("pivoting inequality", ineq)
    drop = sc.structural_drop(c, k)
    # p is unique where the dropped columns are fixed by structure (or nothing is dropped) and the kept ones have full rank
    if ref.rankJ2 == min(m, n - ref.rankA) - len(drop) and m >= n - ref.rankA:
        cond = max(sc.cond_kept(ref, J), gcc.cond_of(A[ref.jpvtA[:ref.rankA] - 1]) if ref.rankA else 1.0)
        ep = gcc.rel(out_p, ref.p)
        note("p/(1e-13 cond)" if cond > 100 else "p", ep / (1e-13 * cond) if cond > 100 else ep)
        print(f"{c['id']} prob {k}: p against the oracle {ep:.2e} (cond {cond:.1e}), pivoting inequality {ineq:.2e}, jpvtJ2 "
              f"compared: {certified}", flush=True)
        assert ep <= max(TOL_P, 1e-13 * cond), (tag, "p", ep, cond)
    assert ineq <= TOL_INEQ, (tag, "pivoting inequality", ineq)
    # 2. exact pass-through, and the rows of all-zero tiles
    if kind == "upper" and ref.rankA == 0:
        sc.check_pass_through(FJ, out_d, rx, min(m, n), c["seed"] + k)
    for i in sc.zero_tile_rows(J, c["tile"]):
        e = np.zeros(m)
        e[i] = 1.0
        dn = abs(float(np.linalg.norm(FJ.Qt_mul(e))) - 1.0)
        note("||Q'e_i|| - 1, rows of zero tiles", dn)
        print(f"{c['id']} prob {k}: row {i} of an all-zero tile: | ||Q'e_i|| - 1 | = {dn:.2e}", flush=True)
        assert dn <= fi.TOL_COL, (tag, i, dn)
    # 3. zero columns
    if kind == "zerocols" and ref.rankA == 0:
        sc.check_zero_columns(FJ, out_p, info[1], drop, n)
    if kind == "mixed_scale" and ref.rankA == 0:
        assert sorted((np.asarray(FJ.p)[r2:] - 1).tolist()) == drop and np.all(np.asarray(out_p)[drop] == 0.0), (tag, "tiny columns")
    return ref


def check_dup(s, c, out, route, A, cx, ref):
    """bounds_dup: the second attempt, the oracle's rank, code and kept pivots, |R_A|, b and feasibility (p against the oracle:
    check_problem).  b = Q_L'(-cx[p]) is compared entry by entry in magnitude: the duplicate column is exactly zero in LAPACK after
    the first step and a residue of eps where a fl(1 / a) != 1 (the device's reciprocal is good to 1 - 2 ulp), so a later
    reflector of F_L11 is I in the one and I - 2 e e' in the other, and that entry of b changes its sign with the row of R —
    the signs of Q's columns are implementation-defined."""
    t, r = c["t"], ref.rankA
    assert "second_attempt" in route and (out.rankA, out.code, out.dimA) == (t - 1, -1, t - 1), (c["id"], sorted(route), out.rankA, out.code)
    assert np.array_equal(out.jpvtA[:r], ref.jpvtA[:r]), (c["id"], "jpvtA", out.jpvtA, ref.jpvtA)
    RA = np.asarray(s.factor(fi.FACTOR_A, 0).R)
    dR = cch.r_difference(RA, np.asarray(ref.F_A.R), r)
    residue = float(np.abs(RA[np.asarray(ref.F_A.R) == 0.0]).max())
    eb = float(np.linalg.norm(np.abs(out.b[:r]) - np.abs(ref.b[:r])) / np.linalg.norm(ref.b))
    nb = abs(float(np.linalg.norm(out.b) - np.linalg.norm(ref.b))) / float(np.linalg.norm(ref.b))
    feas = float(np.linalg.norm(A @ out.p + cx) / (np.linalg.norm(A, 2) * np.linalg.norm(out.p) + np.linalg.norm(cx)))
    note("bounds_dup |R_A|", dR)
    note("bounds_dup |b|", eb)
    note("feasibility", feas)
    print(f"{c['id']}: |R_A| against LAPACK's {dR:.2e} (largest entry where LAPACK has an exact zero {residue:.2e}), |b| {eb:.2e}, "
          f"||b|| {nb:.2e}, feasibility {feas:.2e}", flush=True)
    assert dR <= gcc.TOL_R and eb <= gcc.TOL_B and nb <= gcc.TOL_B and feas <= 1e-13, (c["id"], dR, eb, nb, feas)


def check_health(s, c):
    """6. the handle after its case: a Gaussian problem of another shape"""
    shape = sc.HEALTH_SHAPE if (c["m"], c["n"]) != sc.HEALTH_SHAPE[:2] else sc.HEALTH_SHAPE_2
    P, ref = sc.health_problem(shape)
    out = s.solve(*P)
    e = gcc.rel(out.p, ref.p)
    note("handle health p", e)
    print(f"{c['id']}: the handle then solves Gaussian {shape} within {e:.2e} of the oracle", flush=True)
    assert (out.rankA, out.rankJ2, out.code) == (ref.rankA, ref.rankJ2, ref.code) and e <= TOL_P, (c["id"], "health", e)
    assert np.array_equal(out.jpvtA, ref.jpvtA) and np.array_equal(out.jpvtJ2, ref.jpvtJ2), (c["id"], "health pivots")


# ---- 1 - 4, 6: every case ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_case(c):
    (J, rx, A, cx), ref = sc.solved(c)
    s = _handle(c)
    try:
        out = s.solve(J, rx, A, cx)
        route = s.route()
        print(f"{c['id']}: route {sorted(route)}", flush=True)
        assert c["want"] <= route, (c["id"], sorted(c["want"] - route), sorted(route))
        assert "rescaled" not in route, (c["id"], sorted(route))
        assert np.all(np.isfinite(out.b))
        check_problem(s, c, 0, 0, out.p, out.d, (out.rankA, out.rankJ2, out.code), out.jpvtJ2)
        if c["kindA"] in ("bounds", "bounds_tied"):
            assert np.array_equal(out.jpvtA, ref.jpvtA), (c["id"], "jpvtA", out.jpvtA, ref.jpvtA)
            dq, feas, ep = sc.check_bounds(s.factor(fi.FACTOR_A, 0), out.p, A, cx, ref, c["kindA"])
            note("|Q_A - LAPACK's|", dq)
            note("feasibility", feas)
            note("p[i_k] against the bound", ep)
        if c["kindA"] == "bounds_dup":
            check_dup(s, c, out, route, A, cx, ref)
        elif c["kindA"]:
            gcc.check_direction(out, J, rx, A, cx, ref, dict(id=c["id"], kind=c["kindA"]))
        check_health(s, c)
    finally:
        s.close()


# ---- 5. batches ------------------------------------------------------------------------------------------------------------------------
def _singles(c):
    """the single solves of a batch's members, each on a fresh handle: [(p, d, b, jpvtA, jpvtJ2, (rankA, rankJ2, code))]"""
    from enlsip_gn import GNSolver
    out = []
    for k in range(c["batch"]):
        (J, rx, A, cx), _ = sc.solved(c, k)
        s = GNSolver(device=0)
        try:
            o = s.solve(J, rx, A, cx)
            out.append((o.p, o.d, o.b, o.jpvtA, o.jpvtJ2, (o.rankA, o.rankJ2, o.code)))
        finally:
            s.close()
    return out


def _check_batch(s, c, p, b, d, infos, jA, jJ, same_j):
    n = c["n"]
    singles = _singles(c)
    for k in range(c["batch"]):
        tk = c["t_list"][k] if c["t_list"] else c["t"]
        info = infos[k][:3]
        ref = check_problem(s, c, k, k, p[k], d[k], info, jJ[k, :n - infos[k][0]])
        sp, sd, sb, sjA, sjJ, sinfo = singles[k]
        assert info == sinfo, (c["id"], k, info, sinfo)
        assert np.array_equal(jA[k, :tk], sjA) and gcc.same(b[k, :tk], sb), (c["id"], k, "constraint side differs from the single solve")
        assert np.array_equal(jJ[k, :ref.rankJ2], sjJ[:ref.rankJ2]), (c["id"], k, "jpvtJ2 differs from the single solve")
        dp, dd = gcc.rel(p[k], sp), gcc.rel(d[k], sd)
        print(f"{c['id']} member {k}: p differs by {dp:.2e}, d by {dd:.2e} from its single solve (same J-side kernels: {same_j[k]})", flush=True)
        if same_j[k]:
            assert gcc.same(p[k], sp) and gcc.same(d[k], sd), (c["id"], k, dp, dd)
        else:
            note("batch member against its single solve", max(dp, dd))
            assert dp <= TOL_MOVED and dd <= TOL_MOVED, (c["id"], k, dp, dd)


def _j_side(batch, m, n, t):
    return {x for x in sc.dg.expected_route(batch, m, n, t) if not x.startswith("constraint_")}


def test_batch_of_five_kinds_matches_its_single_solves():
    from enlsip_gn import GNSolver
    c = sc.batch_case()
    probs = [sc.solved(c, k)[0] for k in range(c["batch"])]
    s = GNSolver(device=0)
    try:
        J = np.stack([np.ascontiguousarray(P[0].T) for P in probs])
        p, b, d, infos, jA, jL, jJ = s.solve_batched(J, np.stack([P[1] for P in probs]), None, None)
        route = s.route()
        print(f"{c['id']}: route {sorted(route)}", flush=True)
        assert c["want"] <= route and "pivot_wave2" in route, (sorted(c["want"] - route), sorted(route))
        same_j = _j_side(c["batch"], c["m"], c["n"], 0) == _j_side(1, c["m"], c["n"], 0)
        _check_batch(s, c, p, b, d, infos, jA, jJ, [same_j] * c["batch"])
        check_health(s, c)
    finally:
        s.close()


def test_ragged_batch_with_bounds_matches_its_single_solves():
    from enlsip_gn import GNSolver
    c = sc.ragged_case()
    probs = [sc.solved(c, k)[0] for k in range(c["batch"])]
    s = GNSolver(device=0)
    try:
        At, cxb, tk = GNSolver.pack_ragged([P[2] for P in probs], [P[3] for P in probs], n=c["n"])
        J = np.stack([np.ascontiguousarray(P[0].T) for P in probs])
        p, b, d, infos, jA, jL, jJ = s.solve_batched_ragged(J, np.stack([P[1] for P in probs]), At, cxb, tk)
        print(f"{c['id']}: route {sorted(s.route())}", flush=True)
        # a ragged launch is planned for its smallest and its largest t_k and runs every member with the launch's kernels: bit for
        # bit where the member's own single solve takes the J-side route of both
        m, n, ts = c["m"], c["n"], c["t_list"]
        same_j = [_j_side(1, m, n, t) == _j_side(c["batch"], m, n, min(ts)) == _j_side(c["batch"], m, n, max(ts)) for t in ts]
        for k, t in enumerate(c["t_list"]):
            (Jk, rxk, Ak, cxk), ref = sc.solved(c, k)
            if t:
                assert np.array_equal(jA[k, :t], ref.jpvtA), (c["id"], k, "jpvtA")
                sc.check_bounds(s.factor(fi.FACTOR_A, k), p[k], Ak, cxk, ref, c["kindA"])
        _check_batch(s, c, p, b, d, infos, jA, jJ, same_j)
        check_health(s, c)
    finally:
        s.close()
