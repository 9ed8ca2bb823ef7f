"""CPU checks of the case grid of tests/resolve_edges.py and of the reference tests/test_gpu_resolve_edges.py compares with.

1. The grid is the seven named cases, reaches every branch of resolve_edges.BRANCHES, and every case reaches the branches it was
   written for (OWN): removing a case fails.
2. The oracle is DETERMINED on every compared request: under a relative 1e-15 perturbation of J and A (a rounding of the inputs)
   its re-solved p, b, ||d|| and |d[:dimJ2]| move by at most a tenth of the GPU test's tolerance for that quantity.
   The GPU test also compares with the per-problem entry point at 1e-13, and another summation order is amplified by cond(R_A):
   test_constraint_factors_are_well_conditioned holds every batch to cond(R_A) <= 200, so that u cond(R_A) = 2.2e-14 leaves a
   factor 4.5 for the constants of the two summations.  Seeds 12331 (kp_zero_general, a square 70 x 70 Gaussian A: 142) and 12625
   (mixed_kp, A' of 100 x 99 and 100 x 100: 123) are there for that bound; the first seeds tried gave 257 and 1034.
3. The oracle SOLVES what it should: the solve steps of oracle.gn_oracle.sub_search_direction redone in mpmath at 50 digits on the
   oracle's float64 factors (R, reflectors, tau, pivots and J1, all taken as exact; nothing is factored in mpmath).  Worst relative
   error of the float64 oracle over every compared request of the cases with n <= 140, as a multiple of u * kappa (u = 2^-53;
   kappa = the 2-norm condition number of the triangle solved for p1 for d, the larger of that and R_J2[:dimJ2, :dimJ2]'s for p,
   1 for b):

       p 78.2, b 5.7, ||d|| 1.7, |d[:dimJ2]| 78.8

   and in absolute terms every one is below a tenth of the GPU tolerance, which is what the test asserts."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import resolve_edges as edges  # noqa: E402
import test_gpu_resolve_batched as rb  # noqa: E402  (helpers only: its tests are GPU tests)

from oracle import gn_oracle as go  # noqa: E402

CASES = edges.grid()
BATCHES = [b for c in CASES for b in c.batches]


OWN = {
    "code1_blocks": ("upper_t_1blk", "upper_t_nb64", "upper_t_multi", "upper_t_partial", "trsv_dimJ2_64", "trsv_dimJ2_65"),
    "codem1_blocks": ("trsv_dimA_64", "trsv_dimA_65", "trsv_dimJ2_64", "trsv_dimJ2_65"),
    "tail_mem": ("tail_mem",),
    "kp_zero": ("kp0",),
    "wide": ("kp_eq_m",),
    "t_gt_n": ("t_gt_n",),
    "mixed_kp": ("kp_mixed", "passenger"),
}


def test_grid_reaches_every_branch():
    assert [c.name for c in CASES] == ["code1_blocks", "codem1_blocks", "tail_mem", "kp_zero", "wide", "t_gt_n", "mixed_kp"]
    cov = {c.name: edges.covered(c) for c in CASES}
    union = set().union(*cov.values())
    assert union == set(edges.BRANCHES), (sorted(set(edges.BRANCHES) - union), sorted(union - set(edges.BRANCHES)))
    for c in CASES:          # the branches each case was written for
        assert set(OWN[c.name]) <= cov[c.name], (c.name, sorted(set(OWN[c.name]) - cov[c.name]))
    assert set().union(*OWN.values()) | {"head64", "head256", "tail_wave", "tail_reg"} == set(edges.BRANCHES)
    # the general-form cases with three panels or more are the ones that also run with forced pairs
    assert sorted(b.name for b in BATCHES if b.pair_variant) == ["code1_blocks", "codem1_blocks", "mixed_kp", "tail_mem_513", "tail_mem_600"]


def test_codem1_blocks_crosses_every_dimension_pair():
    """dimA in {0, 1, 63, 64, 65, t_k} x dimJ2 in {0, 64, 65, kp}: each of the 24 pairs is requested on some slot, with one code 0 hole"""
    b, = [c for c in CASES if c.name == "codem1_blocks"][0].batches
    seen, holes = set(), 0
    for rnd in b.rounds:
        for k, (dA, dJ, cd) in enumerate(rnd):
            if cd == 0:
                holes += 1
                continue
            assert cd == -1
            for a in [x for x in (0, 1, 63, 64, 65) if x == dA] + (["t_k"] if dA == b.ts[k] else []):
                for j in [x for x in (0, 64, 65) if x == dJ] + (["kp"] if dJ == b.kp(k) else []):
                    seen.add((a, j))
    want = {(a, j) for a in (0, 1, 63, 64, 65, "t_k") for j in (0, 64, 65, "kp")}
    assert seen == want, sorted(map(str, want - seen))
    assert holes == 1


@pytest.mark.parametrize("b", BATCHES, ids=[b.name for b in BATCHES])
def test_constraint_factors_are_well_conditioned(b):
    """cond(R_A) <= 200 on every problem with constraints: what the 1e-13 comparison of the batched re-solve with the per-problem
    entry point (another summation order in the triangular solves with R_A' or R_L, which has R_A's singular values) is amplified by"""
    _, refs = edges.problems(b)
    for k, ref in enumerate(refs):
        if b.ts[k]:
            c = float(np.linalg.cond(ref.F_A.R[:ref.rankA, :ref.rankA]))
            print(f"{b.name} problem {k}: cond(R_A) {c:.1f}")
            assert c <= 200.0, (b.name, k, c)


def quantities(b, k, prob, ref, dA, dJ, cd):
    """what check_against_oracle compares for this request: name -> (value, tolerance)"""
    p, bb, d = rb.oracle_resolve(prob, ref, dA, dJ, cd)
    q = {"p": (p, edges.TOL["p"] if ref.code == 1 else edges.TOL["p_deficient"]), "dnorm": (np.array([np.linalg.norm(d)]), edges.TOL["dnorm"])}
    if b.ts[k]:
        q["b"] = (bb, edges.TOL["b"])
    if ref.rankA == b.ts[k] and dJ:
        q["dabs"] = (np.abs(d[:dJ]), edges.TOL["dabs"])
    return q


@pytest.mark.parametrize("b", BATCHES, ids=[b.name for b in BATCHES])
def test_oracle_is_determined_on_every_case(b):
    probs, refs = edges.problems(b)
    worst = {}
    for k, (prob, ref) in enumerate(zip(probs, refs)):
        J, rx, A, cx = prob
        rng = np.random.default_rng(5)
        J2 = J * (1.0 + 1e-15 * rng.uniform(-1, 1, J.shape))
        A2 = A * (1.0 + 1e-15 * rng.uniform(-1, 1, A.shape))
        ref2 = go.gn_subproblem(J2, rx, A2, cx)
        assert (ref2.rankA, ref2.rankJ2) == (ref.rankA, ref.rankJ2)
        for rnd in b.rounds:
            dA, dJ, cd = rnd[k]
            if cd == 0:
                continue
            q1 = quantities(b, k, prob, ref, dA, dJ, cd)
            q2 = quantities(b, k, (J2, rx, A2, cx), ref2, dA, dJ, cd)
            for nm, (v, tol) in q1.items():
                moved = rb.rel(q2[nm][0], v)
                worst[nm] = max(worst.get(nm, 0.0), moved / tol)
                assert moved <= 0.1 * tol, (b.name, k, (dA, dJ, cd), nm, moved)
    print(f"{b.name}: largest move / tolerance " + ", ".join(f"{nm} {w:.1e}" for nm, w in sorted(worst.items())))


# ---- 3. the solve steps in mpmath -----------------------------------------------------------------------------------------------
class MpFactor:
    """a QRPivoted's float64 factors as exact mpmath numbers: column lists, tau, 0-based pivots"""

    def __init__(self, F, mp):
        self.rows, self.cols, self.k = F.rows, F.cols, F.k
        self.col = [[mp.mpf(float(x)) for x in F.factors[:, j]] for j in range(F.cols)]
        self.tau = [mp.mpf(float(x)) for x in F.tau]
        self.piv = [int(x) - 1 for x in F.jpvt]

    def reflect(self, x, mp, transpose):
        """Q' x (H_0 first) or Q x (H_{k-1} first) by the explicit reflectors H_j = I - tau_j v_j v_j'"""
        x = list(x)
        for j in (range(self.k) if transpose else range(self.k - 1, -1, -1)):
            if self.tau[j] == 0:
                continue
            v = self.col[j]
            w = (x[j] + mp.fdot(v[j + 1:], x[j + 1:])) * self.tau[j]
            x[j] -= w
            for r in range(j + 1, self.rows):
                x[r] -= w * v[r]
        return x

    def R(self, i, j):
        return self.col[j][i]


def mp_upper_solve(F, dim, y, mp):
    """U(R[:dim, :dim]) \\ y"""
    x = [mp.mpf(0)] * dim
    for i in range(dim - 1, -1, -1):
        x[i] = (y[i] - mp.fdot([F.R(i, c) for c in range(i + 1, dim)], x[i + 1:dim])) / F.R(i, i)
    return x


def mp_lower_t_solve(F, dim, y, mp):
    """L(R[:dim, :dim]') \\ y"""
    x = []
    for i in range(dim):
        x.append((y[i] - mp.fdot(F.col[i][:i], x)) / F.R(i, i))
    return x


def invperm(piv):
    inv = [0] * len(piv)
    for i, pj in enumerate(piv):
        inv[pj] = i
    return inv


class MpProblem:
    """sub_search_direction on one problem in mpmath; the stages up to d are kept per (code, dimA)"""

    def __init__(self, prob, ref, mp):
        J, rx, A, cx = prob
        self.mp, self.ref = mp, ref
        self.n, self.t, self.rankA = J.shape[1], (A.shape[0] if A.size else 0), ref.rankA
        J1 = (ref.F_A.rmul_Q(J) if self.t else J)[:, :ref.rankA]
        self.J1rows = [[mp.mpf(float(x)) for x in row] for row in J1]
        self.rx = [mp.mpf(float(x)) for x in rx]
        self.cx = [mp.mpf(float(x)) for x in cx]
        self.FA, self.FL, self.FJ = MpFactor(ref.F_A, mp), MpFactor(ref.F_L11, mp), MpFactor(ref.F_J2, mp)
        self.head = {}

    def upto_d(self, dA, cd):
        mp, t = self.mp, self.t
        if (dA, cd) not in self.head:
            bbuf = [-self.cx[pj] for pj in self.FA.piv]                                  # the permutation of cx
            if cd == 1:
                b = bbuf
                p1 = mp_lower_t_solve(self.FA, t, b, mp)                                 # R_A' p1 = b
            else:
                b = self.FL.reflect(bbuf, mp, True) if t else []
                full = mp_upper_solve(self.FL, dA, b, mp) + [mp.mpf(0)] * (t - dA)       # R_L[:dimA, :dimA] dp1 = b[:dimA]
                p1 = [full[i] for i in invperm(self.FL.piv)][:self.rankA]
            dtemp = [-mp.fdot(row, p1) - r for row, r in zip(self.J1rows, self.rx)]      # d_temp
            d = self.FJ.reflect(dtemp, mp, True) if self.FJ.k else dtemp                 # Q' by explicit reflectors
            self.head[(dA, cd)] = (b, p1, d)
        return self.head[(dA, cd)]

    def resolve(self, dA, dJ, cd):
        mp = self.mp
        b, p1, d = self.upto_d(dA, cd)
        n2 = self.n - (self.t if cd == 1 else self.rankA)
        full = mp_upper_solve(self.FJ, dJ, d, mp) + [mp.mpf(0)] * (n2 - dJ)               # R_J2[:dimJ2, :dimJ2] dp2 = d[:dimJ2]
        p2 = [full[i] for i in invperm(self.FJ.piv)]                                     # the scatter
        p = self.FA.reflect(p1 + p2, mp, False) if self.FA.k else p1 + p2                # F_A.Q
        return p, b, d


def mp_rel(x64, x, mp):
    """|| x64 - x || / || x ||, the difference taken in mpmath"""
    num = mp.sqrt(sum((mp.mpf(float(a)) - y) ** 2 for a, y in zip(x64, x)))
    den = mp.sqrt(mp.fdot(x, x))
    return float(num / (den if den > 0 else 1))


def cond_of(T):
    return float(np.linalg.cond(T)) if T.size else 1.0


def test_oracle_solves_against_high_precision():
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    u = 2.0 ** -53
    worst_mult, worst_abs = {}, {}
    for b in (b for b in BATCHES if b.n <= 140):
        probs, refs = edges.problems(b)
        for k, (prob, ref) in enumerate(zip(probs, refs)):
            P = MpProblem(prob, ref, mp)
            for rnd in b.rounds:
                dA, dJ, cd = rnd[k]
                if cd == 0:
                    continue
                p, bb, d = P.resolve(dA, dJ, cd)
                p64, b64, d64 = rb.oracle_resolve(prob, ref, dA, dJ, cd)
                kA = cond_of(ref.F_A.R[:b.ts[k], :b.ts[k]]) if cd == 1 else cond_of(ref.F_L11.R[:dA, :dA])
                kJ = cond_of(ref.F_J2.R[:dJ, :dJ])
                nd = mp.sqrt(mp.fdot(d, d))
                errs = {"p": (mp_rel(p64, p, mp), max(kA, kJ), edges.TOL["p"] if ref.code == 1 else edges.TOL["p_deficient"]),
                        "dnorm": (float(abs(mp.mpf(float(np.linalg.norm(d64))) - nd) / nd), kA, edges.TOL["dnorm"])}
                if b.ts[k]:
                    errs["b"] = (mp_rel(b64, bb, mp), 1.0, edges.TOL["b"])
                if ref.rankA == b.ts[k] and dJ:
                    errs["dabs"] = (mp_rel(np.abs(d64[:dJ]), [abs(x) for x in d[:dJ]], mp), kA, edges.TOL["dabs"])
                for nm, (e, kappa, tol) in errs.items():
                    worst_mult[nm] = max(worst_mult.get(nm, 0.0), e / (u * kappa))
                    worst_abs[nm] = max(worst_abs.get(nm, 0.0), e / tol)
                    assert e <= 0.1 * tol, (b.name, k, (dA, dJ, cd), nm, e)
    print("float64 oracle against mpmath, worst relative error / (u kappa): " + ", ".join(f"{nm} {w:.2f}" for nm, w in sorted(worst_mult.items())))
    print("                                 worst relative error / tolerance: " + ", ".join(f"{nm} {w:.1e}" for nm, w in sorted(worst_abs.items())))
    assert set(worst_mult) == {"p", "b", "dnorm", "dabs"} and all(math.isfinite(w) for w in worst_mult.values())
