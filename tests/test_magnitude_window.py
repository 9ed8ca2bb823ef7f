"""The magnitude contract (include/enlsip_gn.h, "Magnitudes") between the band edge and the overflow of the largest column norm,
and at the small-magnitude threshold.

Inputs with entries of about 2^400 to 2^511 keep the largest column norm squared finite, so the first diagonals of F_A.R and
F_J2.R — what the detection looks at (gn_rescale.hpp) — are finite, while other plain sums of squares in the kernels need not be:
the column norms of L11 = R_A' are the ROW norms of R_A (up to sqrt(t) |R_A[0,0]|), and ||rx||^2 may exceed every column norm of J.
The cases at 2^+-600 elsewhere in the suite overflow R[0] itself and say nothing about this window.

CPU part (not marked gpu): the oracle alone shows that every constructed input has the property that makes it discriminating, so
that the GPU cases cannot drift out of the window unnoticed.  GPU part: enlsip_gn_solve and every entry point that reaches the
constraint kernels against the oracle (real LAPACK) on the SAME scaled inputs, and — power-of-two scaling being exact — bit for
bit against the same handle's solve of the ordinary problem."""
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import magnitude_window as mw                      # noqa: E402
from oracle import gn_oracle as go                 # noqa: E402

gpu = pytest.mark.gpu
SMALL = (300, 40, 6)
TOL_P = 1e-11            # p and b, as tests/test_gpu_parity.py::test_extreme_magnitudes_match_lapack
TOL_R = 1e-10            # R

# The near-parallel case is moderately conditioned (cond(R_A) = 119 / 385 / 2363 at the three shapes): its limit for p is
# max(1e-11, 10 x the oracle's own distance to the extended-precision solution of the ordinary problem).  Measured
# (test_near_parallel_oracle_distance recomputes them): 4.33e-15 at (300,40,6), 1.23e-14 at (700,130,20), 4.14e-14 at
# (300,200,90), 2.88e-15 at (300,40,5).  The factor 10 covers the different reduction orders of kernel and LAPACK.
ORACLE_DISTANCE = {(300, 40, 6): 4.4e-15, (700, 130, 20): 1.3e-14, (300, 200, 90): 4.2e-14, (300, 40, 5): 2.9e-15}


def near_parallel_limit(shape):
    return max(TOL_P, 10.0 * ORACLE_DISTANCE[shape])


def rel(a, b):
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


def same(a, b):
    """bit for bit"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@lru_cache(maxsize=None)
def oracle_random(m, n, t, eJ, eA):
    sc, base = mw.window_random(m, n, t, eJ, eA)
    return sc, go.gn_subproblem(*sc)


@lru_cache(maxsize=None)
def oracle_base(m, n, t):
    return go.gn_subproblem(*mw.base_problem(m, n, t))


@lru_cache(maxsize=None)
def oracle_near_parallel(m, n, t):
    sc, base, e = mw.near_parallel_rows(m, n, t)
    return sc, base, e, go.gn_subproblem(*sc), go.gn_subproblem(*base)


@lru_cache(maxsize=None)
def oracle_rx_dominant(m, n, t):
    sc, base, eJ = mw.window_rx_dominant(m, n, t)
    return sc, base, eJ, go.gn_subproblem(*sc), go.gn_subproblem(*base)


def same_decisions_and_p(ref, ref0):
    assert (ref.rankA, ref.rankJ2, ref.code) == (ref0.rankA, ref0.rankJ2, ref0.code)
    assert np.array_equal(ref.jpvtA, ref0.jpvtA) and np.array_equal(ref.jpvtL, ref0.jpvtL) and np.array_equal(ref.jpvtJ2, ref0.jpvtJ2)
    assert np.all(np.isfinite(ref.p)) and np.array_equal(ref.p, ref0.p)


# ---- CPU part: the oracle alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,t", mw.SHAPES + [(300, 40, 5)])
def test_near_parallel_rows_overflow_a_row_norm_but_not_the_first_diagonal(m, n, t):
    sc, base, e, ref, ref0 = oracle_near_parallel(m, n, t)
    R = ref.F_A.R
    assert 1022.0 <= mw.log2_sumsq(R[0, 0]) < 1024.0           # R_A[0,0]^2 finite
    assert mw.log2_sumsq(R[0]) > 1024.0                        # the first row of R_A = the first column of L11: its square is not
    assert np.all(np.isfinite(sc[2])) and np.all(np.isfinite(ref.b))
    assert (ref.rankA, ref.code) == (t, 1)
    same_decisions_and_p(ref, ref0)


@pytest.mark.parametrize("m,n,t", mw.SHAPES)
def test_rx_dominant_overflows_rx_but_no_column_of_J(m, n, t):
    sc, base, eJ, ref, ref0 = oracle_rx_dominant(m, n, t)
    assert mw.log2_sumsq(sc[0], axis=0).max() < 1024.0 and np.log2(abs(ref.F_J2.R[0, 0])) < 512.0
    assert mw.log2_sumsq(sc[1]) > 1024.0 and np.all(np.isfinite(sc[1]))
    same_decisions_and_p(ref, ref0)


@pytest.mark.parametrize("m,n,t", mw.SHAPES)
def test_random_window_cases_stay_in_the_window(m, n, t):
    """every kept (eJ, eA): both first diagonals finite and LAPACK's answer that of the ordinary problem; every dropped one
    overflows R[0] itself (the not-finite nomination that the 2^+-600 cases cover)"""
    cases = mw.random_window_cases(m, n, t)
    ref0 = oracle_base(m, n, t)
    J, rx, A, cx = mw.base_problem(m, n, t)
    for e in mw.EXPONENTS:
        for eJ, eA in ((e, 0), (0, e), (e, e)):
            if (eJ, eA) in cases:
                sc, ref = oracle_random(m, n, t, eJ, eA)
                assert np.log2(abs(ref.F_A.R[0, 0])) < 512.0 and np.log2(abs(ref.F_J2.R[0, 0])) < 512.0
                assert max(np.log2(abs(ref.F_A.R[0, 0])) if eA else 0.0, np.log2(abs(ref.F_J2.R[0, 0])) if eJ else 0.0) > 440.0
                same_decisions_and_p(ref, ref0)
            else:
                over = [l + 2 * x for l, x in ((mw.log2_sumsq(J, axis=0).max(), eJ), (mw.log2_sumsq(A, axis=1).max(), eA)) if x]
                assert max(over) >= 1024.0
    assert {c for c in cases if 495 in c} and {c for c in cases if 505 in c}         # the window is not empty


@pytest.mark.parametrize("side", ["above", "below"])
def test_lower_edge_is_on_the_stated_side(side):
    sc, base, e = mw.lower_edge_graded(*SMALL, side)
    ref = go.gn_subproblem(*sc)
    f = abs(ref.F_J2.R[0, 0]) * 2.0 ** 440                      # the largest column norm of J2 in units of the threshold
    assert (1.001 < f < 1.999) if side == "above" else (0.5005 < f < 0.9995)
    assert np.abs(sc[0]).max() < 2.0 ** -400                    # far outside the band: a nominated one is rescaled
    assert (ref.rankA, ref.rankJ2, ref.code) == (SMALL[2], 0, 1)   # pseudo_rank's absolute first test
    assert np.array_equal(ref.jpvtJ2, go.gn_subproblem(*base).jpvtJ2)


@pytest.mark.parametrize("m,n,t", mw.SHAPES + [(300, 40, 5)])
def test_near_parallel_oracle_distance(m, n, t):
    """the figures beside ORACLE_DISTANCE: the oracle's p on the ordinary near-parallel problem against the extended-precision one"""
    sc, base, e, ref, ref0 = oracle_near_parallel(m, n, t)
    p_mp, last = mw.extended_precision_p(*base)
    assert last < 1e-25
    dist = rel(ref0.p, p_mp)
    print(f"near-parallel {(m, n, t)}: oracle to extended precision {dist:.3e}")
    assert dist <= ORACLE_DISTANCE[(m, n, t)] and near_parallel_limit((m, n, t)) == TOL_P


# ---- GPU part ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def factors_of(solver, prob=0):
    from enlsip_gn import FACTOR_A, FACTOR_L11, FACTOR_J2
    return {w: (solver.factor(w, prob).R, solver.factor(w, prob).diagR(), solver.factor(w, prob).p) for w in (FACTOR_A, FACTOR_L11, FACTOR_J2)}


def check_decisions(got, ref, tag):
    """got: (rankA, rankJ2, code, status, jpvtA, jpvtL, jpvtJ2)"""
    rankA, rankJ2, code, status, jA, jL, jJ = got
    assert (rankA, rankJ2, code, status) == (ref.rankA, ref.rankJ2, ref.code, 0), (tag, got[:4])
    assert np.array_equal(jA, ref.jpvtA) and np.array_equal(jL, ref.jpvtL), tag
    assert np.array_equal(jJ[:ref.rankJ2], ref.jpvtJ2[:ref.rankJ2]), tag


def check_factor(fv, F, e, kk, tag, full=True):
    """|diag R|, |R| after ldexp back, pivots and a Q Q' round trip of one resident factorisation against the oracle's"""
    if kk == 0:
        return
    dg, dgr = np.ldexp(np.abs(fv.diagR()[:kk]), -e), np.ldexp(np.abs(F.diagR()[:kk]), -e)
    assert np.abs(dg - dgr).max() <= 1e-11 * dgr.max(), tag
    if full:
        assert rel(np.ldexp(np.abs(fv.R), -e), np.ldexp(np.abs(F.R), -e)) <= TOL_R, tag
    v = np.linspace(-1.0, 1.0, F.rows)
    assert rel(fv.Q_mul(fv.Qt_mul(v)), v) <= 1e-12, tag


def check_against_oracle(solver, out, ref, prob, eJ, eA, tag, tol_p=TOL_P):
    """what test_extreme_magnitudes_match_lapack checks, on the same scaled inputs"""
    from enlsip_gn import FACTOR_A, FACTOR_L11, FACTOR_J2
    J, rx, A, cx = prob
    m, n = J.shape
    t = A.shape[0]
    check_decisions((out.rankA, out.rankJ2, out.code, out.status, out.jpvtA, out.jpvtL, out.jpvtJ2), ref, tag)
    err = rel(out.p, ref.p)
    print(f"{tag}: rel p {err:.3e}")
    assert np.all(np.isfinite(out.p)) and err <= tol_p, (tag, err)
    assert rel(np.ldexp(out.b, -eA), np.ldexp(ref.b, -eA)) <= TOL_P, tag
    nd = np.linalg.norm(np.ldexp(ref.d, -eJ))
    assert abs(np.linalg.norm(np.ldexp(out.d, -eJ)) - nd) <= 1e-12 * nd, tag
    r = ref.rankJ2
    for which, F, e in ((FACTOR_A, ref.F_A, eA), (FACTOR_L11, ref.F_L11, eA), (FACTOR_J2, ref.F_J2, eJ)):
        kk = r if which == FACTOR_J2 else min(F.R.shape)
        check_factor(solver.factor(which), F, e, kk, (tag, which), full=(which != FACTOR_J2 or r == min(F.R.shape)))
    assert rel(np.ldexp(solver.JQ1(m, n), -eJ), np.ldexp(ref.F_A.rmul_Q(J), -eJ)) <= 1e-12, tag
    if ref.rankA and ref.rankJ2 > 1:
        dimA, dimJ2 = ref.rankA - 1, ref.rankJ2 // 2
        JQ1 = ref.F_A.rmul_Q(J)
        p_ref, b_ref, d_ref = go.sub_search_direction(JQ1[:, :ref.rankA], rx, cx, ref.F_A, ref.F_L11, ref.F_J2, n, t, ref.rankA, dimA, dimJ2, -1)
        p2, b2, d2 = solver.resolve(m, n, t, dimA, dimJ2, -1)
        assert rel(p2, p_ref) <= 1e-9 and rel(np.ldexp(b2, -eA), np.ldexp(b_ref, -eA)) <= 1e-10, tag


def check_first_lagrange(solver, prob, ref, eA, tag):
    """first_lagrange_mult_estimate! with grad_fx = J' rx against the oracle's, after ldexp by the scale of A.  Two triangular
    solves with R_A: forward error <= c eps cond(R_A)^2 with cond from the ORACLE's R; c = 100 covers t and the reduction orders."""
    J, rx, A, cx = prob
    t = A.shape[0]
    it = go.IterationRecord()
    lam_ref = go.first_lagrange_mult_estimate(A, J.T @ rx, cx, False, None, ref.F_A, it, go.SQRT_EPS)
    lam, gres = solver.first_lagrange(t, J.T @ rx, None)
    cond = np.linalg.cond(np.ldexp(ref.F_A.R[:, :ref.rankA], -eA))
    tol = max(TOL_P, 100.0 * np.finfo(float).eps * cond ** 2)
    err = rel(np.ldexp(lam, eA), np.ldexp(lam_ref, eA))
    print(f"{tag}: multipliers rel {err:.3e} (limit {tol:.1e})")
    assert np.all(np.isfinite(lam)) and err <= tol, (tag, err, tol)
    assert abs(gres - it.grad_res) <= 1e-11 * it.grad_res, tag


def ordinary_solve_is_ordinary(solver, m, n, t):
    out = solver.solve(*mw.base_problem(m, n, t))
    assert "rescaled" not in solver.route() and out.status == 0
    assert rel(out.p, oracle_base(m, n, t).p) <= TOL_P
    return out


@gpu
@pytest.mark.parametrize("m,n,t", mw.SHAPES)
def test_random_window_matches_lapack_and_the_ordinary_solve_bit_for_bit(m, n, t, solver):
    from enlsip_gn import FACTOR_A, FACTOR_L11, FACTOR_J2
    out0 = solver.solve(*mw.base_problem(m, n, t))
    assert "rescaled" not in solver.route()
    fac0 = factors_of(solver)
    for eJ, eA in mw.random_window_cases(m, n, t):
        prob, ref = oracle_random(m, n, t, eJ, eA)
        tag = (m, n, t, eJ, eA)
        out = solver.solve(*prob)
        check_against_oracle(solver, out, ref, prob, eJ, eA, tag)
        if eJ == 0:
            check_first_lagrange(solver, prob, ref, eA, tag)
        # exactness: a power-of-two scaling changes no mantissa (nothing here comes near the denormal range)
        assert same(out.p, out0.p), (tag, rel(out.p, out0.p))
        assert same(np.ldexp(out.b, -eA), out0.b) and same(np.ldexp(out.d, -eJ), out0.d), tag
        assert np.array_equal(out.jpvtJ2, out0.jpvtJ2), tag
        fac = factors_of(solver)
        for w, e in ((FACTOR_A, eA), (FACTOR_L11, eA), (FACTOR_J2, eJ)):
            assert same(np.ldexp(fac[w][0], -e), fac0[w][0]) and same(np.ldexp(fac[w][1], -e), fac0[w][1]), (tag, w)
            assert np.array_equal(fac[w][2], fac0[w][2]), (tag, w)
    ordinary_solve_is_ordinary(solver, m, n, t)


@gpu
@pytest.mark.parametrize("m,n,t", mw.SHAPES)
def test_rx_dominant_matches_lapack(m, n, t, solver):
    prob, base, eJ, ref, ref0 = oracle_rx_dominant(m, n, t)
    out = solver.solve(*prob)
    check_against_oracle(solver, out, ref, prob, eJ, 0, ("rx", m, n, t))
    out0 = solver.solve(*base)
    assert "rescaled" not in solver.route()
    assert same(out.p, out0.p) and same(np.ldexp(out.d, -eJ), out0.d)
    ordinary_solve_is_ordinary(solver, m, n, t)


@gpu
@pytest.mark.parametrize("m,n,t", mw.SHAPES)
def test_near_parallel_rows_match_lapack(m, n, t, solver):
    """R_A[0,0] is finite, so only the nomination above 2^440 has this input solved again; without it F_L11 comes from a column
    norm of L11 = R_A' whose plain sum of squares overflowed (make_reflector: rsq(inf) = 0, nrm = inf * 0 = NaN), in a factor
    the detection does not look at."""
    prob, base, e, ref, ref0 = oracle_near_parallel(m, n, t)
    out = solver.solve(*prob)
    check_against_oracle(solver, out, ref, prob, 0, e, ("near-parallel", m, n, t), tol_p=near_parallel_limit((m, n, t)))
    check_first_lagrange(solver, prob, ref, e, ("near-parallel", m, n, t))
    out0 = solver.solve(*base)
    assert "rescaled" not in solver.route()
    assert same(out.p, out0.p) and same(np.ldexp(out.b, -e), out0.b)
    ordinary_solve_is_ordinary(solver, m, n, t)


@gpu
def test_near_parallel_rows_in_the_factored_flow(solver):
    from enlsip_gn import FACTOR_A, FACTOR_L11
    m, n, t = SMALL
    prob, base, e, ref, ref0 = oracle_near_parallel(m, n, t)
    J, rx, A, cx = prob
    rankA, code, dimA = solver.factor_constraints(m, A, cx)
    assert (rankA, code, dimA) == (ref.rankA, ref.code, ref.rankA)
    for which, F in ((FACTOR_A, ref.F_A), (FACTOR_L11, ref.F_L11)):
        fv = solver.factor(which)
        assert np.array_equal(fv.p, F.p), which
        check_factor(fv, F, e, min(F.R.shape), ("factor_constraints", which))
    out = solver.solve_factored(J, rx, t)
    check_against_oracle(solver, out, ref, prob, 0, e, "solve_factored", tol_p=near_parallel_limit(SMALL))
    ordinary_solve_is_ordinary(solver, m, n, t)


def batch_of(m, n, ts, window_at, seed=64000):
    """ordinary problems with their own t_k, the near-parallel one (with t = ts[window_at]) at slot `window_at`"""
    from oracle import synth
    probs = [synth.make_problem(seed + k, m, n, tk) for k, tk in enumerate(ts)]
    wprob, _, e, wref, _ = oracle_near_parallel(m, n, ts[window_at])
    probs[window_at] = wprob
    refs = [wref if k == window_at else go.gn_subproblem(*P) for k, P in enumerate(probs)]
    return probs, refs, e


def packed(probs, t_max):
    from test_gpu_factored_batched import pack
    n = probs[0][0].shape[1]
    return pack([P[0] for P in probs], [P[1] for P in probs], [P[2] if P[2].size else np.zeros((0, n)) for P in probs],
                [P[3] for P in probs], t_max)


def check_batch_slot(solver, res, k, tk, ref, e, tag, tol_p=TOL_P, factors=True):
    """slot k of a batched result (and the accessors routed to problem k) against the oracle; e: the scale of A', cx of the slot"""
    from enlsip_gn import FACTOR_A, FACTOR_L11
    p, b, d, infos, jA, jL, jJ = res
    n = p.shape[1]
    kA = min(n, tk)
    check_decisions((infos[k][0], infos[k][1], infos[k][2], infos[k][5], jA[k, :tk], jL[k, :kA], jJ[k, :n - ref.rankA]), ref, (tag, k))
    err = rel(p[k], ref.p)
    print(f"{tag} slot {k}: rel p {err:.3e}")
    assert np.all(np.isfinite(p[k])) and err <= tol_p, (tag, k, err)
    if tk:
        assert rel(np.ldexp(b[k, :tk], -e), np.ldexp(ref.b, -e)) <= TOL_P, (tag, k)
    assert np.all(b[k, tk:] == 0.0), (tag, k)
    nd = np.linalg.norm(ref.d)
    assert abs(np.linalg.norm(d[k]) - nd) <= 1e-12 * nd, (tag, k)
    if factors and tk:
        for which, F in ((FACTOR_A, ref.F_A), (FACTOR_L11, ref.F_L11)):
            fv = solver.factor(which, k)
            assert np.array_equal(fv.p, F.p), (tag, k, which)
            check_factor(fv, F, e, min(F.R.shape), (tag, k, which))


@gpu
def test_near_parallel_member_of_a_uniform_batch(solver):
    m, n, t = SMALL
    B, w = 5, 2
    probs, refs, e = batch_of(m, n, [t] * B, w)
    J, rx, At, cx, tv = packed(probs, t)
    res = solver.solve_batched(J, rx, At, cx)
    for k in range(B):
        check_batch_slot(solver, res, k, t, refs[k], e if k == w else 0, "solve_batched", near_parallel_limit(SMALL) if k == w else TOL_P)
    ordinary_solve_is_ordinary(solver, m, n, t)


@gpu
def test_near_parallel_member_of_a_ragged_batch(solver):
    m, n, t_max = SMALL
    ts, w = [6, 3, 0, 6, 5], 4                      # the window member has t = 5 < t_max
    probs, refs, e = batch_of(m, n, ts, w)
    J, rx, At, cx, tv = packed(probs, t_max)
    res = solver.solve_batched_ragged(J, rx, At, cx, tv)
    for k, tk in enumerate(ts):
        check_batch_slot(solver, res, k, tk, refs[k], e if k == w else 0, "solve_batched_ragged",
                         near_parallel_limit((m, n, tk)) if k == w else TOL_P)
    ordinary_solve_is_ordinary(solver, m, n, t_max)


@gpu
def test_near_parallel_member_refactored_in_the_batched_factored_flow(solver):
    """factor_constraints_batched on ordinary working sets, then solve_factored_batched with only the member flagged whose rows
    became the near-parallel ones"""
    m, n, t = SMALL
    B, w = 5, 1
    probs, refs, e = batch_of(m, n, [t] * B, w)
    start = [list(P) for P in probs]
    start[w][2], start[w][3] = mw.base_problem(m, n, t)[2], mw.base_problem(m, n, t)[3]
    _, _, At0, cx0, _ = packed(start, t)
    J, rx, At, cx, tv = packed(probs, t)
    infos = solver.factor_constraints_batched(m, At0, cx0)
    assert all(i[0] == t and i[1] == 1 for i in infos)
    flags = np.zeros(B, dtype=np.int64)
    flags[w] = 1
    res = solver.solve_factored_batched(J, rx, At, cx, None, flags)
    for k in range(B):
        check_batch_slot(solver, res, k, t, refs[k], e if k == w else 0, "solve_factored_batched", near_parallel_limit(SMALL) if k == w else TOL_P)
    ordinary_solve_is_ordinary(solver, m, n, t)


@gpu
def test_near_parallel_rows_arrive_through_the_changed_problems_solve(solver):
    """the changed problem's new A is the window one; the slots and the factors of the others stay bit for bit as they were"""
    from test_gpu_solve_changed_batched import assert_snapshot, snapshot
    m, n, t_max = SMALL
    ts, w = [6, 3, 0, 6, 5], 3
    probs, refs, e = batch_of(m, n, ts, w)
    start = [list(P) for P in probs]
    start[w][2], start[w][3] = mw.base_problem(m, n, ts[w])[2], mw.base_problem(m, n, ts[w])[3]
    J, rx, At0, cx0, tv = packed(start, t_max)
    first = solver.solve_batched_ragged(J, rx, At0, cx0, tv)
    assert "rescaled" not in solver.route()
    keep = [k for k in range(len(ts)) if k != w]
    snap = snapshot(solver, keep)
    _, _, At, cx, _ = packed(probs, t_max)
    flags = np.zeros(len(ts), dtype=np.int64)
    flags[w] = 1
    At[flags == 0] = np.nan                         # rows of the unflagged problems are not read
    cx[flags == 0] = np.nan
    got = solver.solve_changed_batched(At, cx, tv, flags)
    assert solver.jacobian_resolved() == 1
    for k in keep:
        assert all(np.isnan(got[i][k]).all() for i in (0, 1, 2)), k
        assert not any(got[i][k].any() for i in (4, 5, 6)) and got[3][k] == (0, 0, 0, 0, 0, 0), k
    assert_snapshot(solver, snap)
    check_batch_slot(solver, got, w, ts[w], refs[w], e, "solve_changed_batched", near_parallel_limit((m, n, ts[w])))
    for k in keep:
        check_batch_slot(solver, first, k, ts[k], refs[k], 0, "solve_changed_batched (untouched)")
    ordinary_solve_is_ordinary(solver, m, n, t_max)


@gpu
@pytest.mark.parametrize("side", ["above", "below"])
def test_lower_edge_on_both_sides_of_the_threshold(side, solver):
    """graded J whose largest J2 column norm is just above 2^-440 (not nominated: the plain kernels carry it) and just below
    (nominated, rescaled): ranks and the leading pivots — those whose diagonal is within 1e-3 of the first — are LAPACK's"""
    m, n, t = SMALL
    prob, base, e = mw.lower_edge_graded(m, n, t, side)
    ref = go.gn_subproblem(*prob)
    out = solver.solve(*prob)
    assert ("rescaled" in solver.route()) == (side == "below"), solver.route()
    assert (out.rankA, out.rankJ2, out.code, out.status) == (ref.rankA, ref.rankJ2, ref.code, 0)
    assert np.array_equal(out.jpvtA, ref.jpvtA) and np.array_equal(out.jpvtL, ref.jpvtL)
    dg = np.abs(ref.F_J2.diagR())
    lead = int(np.sum(dg >= 1e-3 * dg[0]))
    assert lead >= 8 and np.array_equal(out.jpvtJ2[:lead], ref.jpvtJ2[:lead]), (lead, out.jpvtJ2[:lead], ref.jpvtJ2[:lead])
    assert rel(out.p, ref.p) <= TOL_P
    ordinary_solve_is_ordinary(solver, m, n, t)


@gpu
def test_forced_dimension_on_a_tiny_J_leaves_no_stale_status(solver):
    """solve(dimJ2 = n - t) with J, rx times 2^-600: on the unscaled data the first pass divides by diagonals that underflowed to
    zero and raises status bit 0; the rescaled pass divides by the non-zero diagonals LAPACK has.  The caller must see that
    pass's status: the constraint stage is not run again for a J-only rescale, so the bit has to be taken back before that pass."""
    m, n, t = SMALL
    prob, base = mw.window_random(m, n, t, -600, 0)
    J, rx, A, cx = prob
    ref = go.gn_subproblem(*prob)
    assert ref.rankJ2 == 0 and np.all(ref.F_J2.diagR() != 0.0)
    J1 = ref.F_A.rmul_Q(J)[:, :ref.rankA]
    p_ref, b_ref, d_ref = go.sub_search_direction(J1, rx, cx, ref.F_A, ref.F_L11, ref.F_J2, n, t, ref.rankA, ref.rankA, n - t, 1)
    out = solver.solve(J, rx, A, cx, dimJ2=n - t)
    assert "rescaled" in solver.route()
    assert (out.rankA, out.rankJ2, out.code) == (ref.rankA, 0, 1)
    assert np.all(np.isfinite(out.p)) and rel(out.p, p_ref) <= TOL_P, rel(out.p, p_ref)
    assert out.status == 0
    ordinary_solve_is_ordinary(solver, m, n, t)
