"""The high-precision references of tests/consumer_reference.py, on the CPU: before they judge a kernel they must judge the FP64
oracle (LAPACK dgeqp3 + two triangular solves, oracle/gn_oracle.py) correct with room to spare, agree with it on which multipliers
are zero, and the consumer grid must sit on both sides of the wave-form thresholds that the library's source names."""
import math
from fractions import Fraction

import numpy as np
import pytest

import consumer_reference as cr
from oracle import gn_oracle as go, synth

EPS = go.SQRT_EPS


def test_exact_products_are_correctly_rounded():
    rng = np.random.default_rng(3)
    for k in (1, 2, 63, 65, 513):
        M = rng.standard_normal((7, k))
        x = rng.standard_normal(k)
        x0 = rng.standard_normal(7)
        y, bound = cr.exact_matvec(M, x, x0)
        for i in range(7):
            exact = sum((Fraction(a) * Fraction(b) for a, b in zip(M[i], x)), Fraction(x0[i]))
            assert y[i] == float(exact)
        naive = x0 + M @ x
        assert np.all(np.abs(naive - y) <= bound)


def test_near_dependent_rows_straddle_the_tolerance():
    """the maker puts the last |R_ii| 2x above / below |R_00| sqrt(kA) eps_rank; pseudo_rank then keeps kA / kA - 1"""
    for name, m, n, t, eps, side in cr.STRADDLE_GRID:
        A = cr.near_dependent_A(11, n, t, eps, side)
        tol, d = cr.pivot_tolerance(A, eps)
        kA = min(n, t)
        assert abs(abs(d[-1]) / tol / side - 1) < 0.02, name
        assert go.pseudo_rank(d, eps) == (kA if side > 1 else kA - 1), name
        if t >= 16 * n:      # a kernel that used sqrt(t) for sqrt(kA) would drop the last constraint of the "above" case
            assert abs(d[-1]) < abs(d[0]) * math.sqrt(t) * eps, name


def _oracle_errors(ci):
    """[(label, err, bound)] of the FP64 oracle on the sampled problems of grid case ci, with the zero pattern checked against S
    on the way"""
    name, m, n, t_max, ts, kap, _ = cr.ESTIMATE_GRID[ci]
    diag = cr.random_diag(100 + ci, len(ts), t_max)
    prand = synth.normal_stream(200 + ci, 6, len(ts) * n).reshape(len(ts), n)
    out = []
    for k in cr.sample_of(ts):
        J, rx, A, cx = cr.grid_problem(ci, k, m, n, ts[k], kap)
        tk = ts[k]
        F = go.qr_colnorm(A.T)
        S, pr = cr.kept_set(F.p, F.diagR(), EPS)
        ref = cr.EstimateReference(A, S)
        kS = cr.kappa(A[S])
        sol = go.gn_subproblem(J, rx, A, cx)
        for ds in (None, diag[k, :tk]):
            scaled = ds is not None
            dsv = ds if scaled else np.ones(tk)
            for given in (True, False):
                g = J.T @ rx if given else cr.exact_gradient(J, rx)
                it = go.IterationRecord()
                lam_o = go.first_lagrange_mult_estimate(A, J.T @ rx, cx, scaled, dsv, F, it, EPS)
                lam_r, gres_r = ref.first(g, cx, ds)
                assert np.array_equal(np.flatnonzero(lam_o), np.sort(S)), (name, k)
                assert np.array_equal(np.flatnonzero(lam_r), np.sort(S)), (name, k)
                gam = (1.0 if given else cr.gamma_rhs(J, rx)) * ref.first_cancellation(g, cx)
                out.append((f"{name}[{k}] first ds={scaled} given={given}", cr.rel_err(lam_o, lam_r), cr.estimate_bound(kS, gam)))
                nrm = np.linalg.norm(g)
                out.append((f"{name}[{k}] grad_res", abs(it.grad_res - gres_r) / nrm, cr.estimate_bound(kS, gam)))
            for pname, p in (("p_solve", sol.p), ("p_rand", prand[k])):
                lam_o = go.second_lagrange_mult_estimate(J, F, rx, p, tk, scaled, dsv, EPS)
                lam_r = ref.second(J, rx, p, ds)
                assert np.array_equal(np.flatnonzero(lam_o), np.sort(S)), (name, k)
                out.append((f"{name}[{k}] second {pname} ds={scaled}", cr.rel_err(lam_o, lam_r),
                            cr.estimate_bound(kS, cr.gamma_rhs(J, rx, p))))
    return out


@pytest.mark.parametrize("ci", range(len(cr.ESTIMATE_GRID)), ids=[c[0] for c in cr.ESTIMATE_GRID])
def test_oracle_meets_the_estimate_bound_with_margin(ci):
    """C_EST (consumer_reference.py) is calibrated here: the FP64 oracle must sit 8x inside the bound on every sampled problem of
    every grid case, t > n, duplicated constraints (pr < kA) and diag_scale included."""
    for label, err, bound in _oracle_errors(ci):
        assert err * 8 <= bound, (label, err, bound)


def test_grid_walks_the_wave_form_thresholds_the_source_names():
    """the predicate `P.n <= N && P.t <= T` comes from gn_lagrange_batched.inc; the grid must put cases on both sides of each
    threshold, at the thresholds, and at the wave's small edges"""
    nmax, tmax = cr.wave_form_limits()
    assert (nmax, tmax) == (64, 64)
    g = cr.ESTIMATE_GRID
    ns = {c[2] for c in g}
    tms = {c[3] for c in g}
    assert {1, 2, nmax - 1, nmax, nmax + 1} <= ns
    assert {1, 2, tmax - 1, tmax, tmax + 1} <= tms
    forms = {(c[2] <= nmax, c[3] <= tmax) for c in g}
    assert forms == {(True, True), (True, False), (False, True), (False, False)}
    assert any(c[2] == nmax and c[3] == tmax for c in g)                        # all 64 lanes
    assert any(c[3] >= 16 * c[2] and c[3] <= tmax for c in g)                  # t >= 16 n in the wave form
    assert any(c[3] > c[2] and c[2] <= nmax and c[3] <= tmax for c in g)       # trapezoidal R in the wave form
    assert {1, 3, 5, 9} <= {len(c[4]) for c in g}
    assert any(len(set(c[4])) > 1 and 0 in c[4] for c in g)                     # ragged with empty members
    assert any(p0 % 4 and cnt % 4 for c in g for (p0, cnt) in c[6])
    assert {1, 65, 257, 513, 1000} <= {c[1] for c in g}
    st = cr.STRADDLE_GRID
    assert any(t >= 16 * n for _, _, n, t, _, _ in st) and any(n >= nmax and t >= tmax for _, _, n, t, _, _ in st)
    assert cr.max_launch_batch() == 32768
