"""Cases for the Newton direction on a row-sharded J (enlsip_gn_tsqr_newton_direction), shared by tests/test_tsqr_newton_host.py and
tests/test_gpu_tsqr_newton.py.  Test infrastructure, CPU only (NumPy, mpmath, the oracle); seeded; not a test module.

A case is (m, n, t, G, row heights, kind): J, rx, A, cx from oracle.synth as tests/test_gpu_newton_batched.py builds them, a Gamma of
its kind, the expected p of tests/newton_reference.py on the WHOLE matrix and cond(sW22) for newton_reference.newton_bound.

Shapes: n2 = n - rankA sits on the cuts of the device-wide Cholesky (gn_kernels_newton_wide.hpp: panels of 32, strips and syrk blocks
of 64): 1; 31, 32, 33 (one panel short, exact, and one plus a 1-row strip); 64, 65 (a full 64 x 64 block, then a second strip); 97
(four panels, the last 1 wide); 257 (more strips than waves).  Each is reached with t = 0 and with t > 0, rankA = t; G is 1 or 3, the
heights uneven with one below n where m allows.

Kinds:
  pd          newton_reference.make_gammas: sW22 positive definite, cond <= 1e8
  zero        Gamma = 0: the step is the Gauss-Newton direction
  rankdefJ    synth.make_rank_deficient_J (rankJ2 = n2 - 3), Gamma positive definite on the null space (make_gammas' shift)
  indef_first t = 0: Gamma[0, 0] lowered until sW22[0, 0] = -1
  indef_late  t = 0, n2 = 97: Gamma[39, 39] lowered until the Schur complement of the leading 39 x 39 block (positive definite) in
              entry 39 is negative: dpotrf's verdict falls on pivot 39, the 40th, in the SECOND panel, and the panels after it must see it
  full_A      rankA == n: p1 as it is
  wide_A      rank-deficient working set with t > n > rankA: E[F_L11.p, F_L11.p]
  short_A     rank-deficient working set with t < n: the reference is undefined there (error -8)

The reference is newton_reference.NewtonReference (mpmath) for n <= 40 and m <= 300 and NewtonReferenceLD, its line-for-line
restatement in pairs of np.longdouble, beyond (the rule of tests/newton_cases.py: mpmath needs minutes from n = 64 on;
tests/test_newton_cases_host.py holds the two to each other at 1e-17).  Where np.longdouble is no wider than a double, mpmath is the
reference of every case."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import newton_reference as nr
from oracle import gn_oracle as go, synth

LATE_PIVOT = 39


@dataclass(frozen=True)
class Case:
    name: str
    m: int
    n: int
    t: int
    heights: tuple
    kind: str
    seed: int

    @property
    def G(self):
        return len(self.heights)


def _c(name, m, n, t, heights, kind):
    assert sum(heights) == m and 150 <= m <= 1300, (name, m, heights)
    return Case(name, m, n, t, tuple(heights), kind, 31000 + 7 * len(_ALL))


_ALL: list = []
for args in [
    ("pd_n1", 150, 1, 0, (150,), "pd"),
    ("pd_n31_G3", 150, 31, 0, (70, 20, 60), "pd"),
    ("pd_n32", 150, 32, 0, (150,), "pd"),
    ("pd_n33_G3", 160, 33, 0, (100, 30, 30), "pd"),
    ("pd_n64", 200, 64, 0, (200,), "pd"),
    ("pd_n65_G3", 200, 65, 0, (120, 40, 40), "pd"),
    ("pd_n97_G3", 300, 97, 0, (150, 60, 90), "pd"),
    ("pd_n257_G3", 600, 257, 0, (300, 200, 100), "pd"),
    ("pd_n2_t1_G3", 150, 2, 1, (100, 1, 49), "pd"),
    ("pd_n37_t5", 150, 37, 5, (150,), "pd"),
    ("pd_n40_t7_G3", 200, 40, 7, (100, 30, 70), "pd"),
    ("pd_n70_t5", 250, 70, 5, (250,), "pd"),
    ("pd_n100_t3_G3", 300, 100, 3, (150, 60, 90), "pd"),
    ("pd_n260_t3", 600, 260, 3, (600,), "pd"),
    ("zero_n33_G3", 160, 33, 0, (100, 30, 30), "zero"),
    ("zero_n40_t7", 200, 40, 7, (200,), "zero"),
    ("zero_n97", 300, 97, 0, (300,), "zero"),
    ("rankdefJ_n40_t6_G3", 300, 40, 6, (150, 30, 120), "rankdefJ"),
    ("rankdefJ_n100_t3", 300, 100, 3, (300,), "rankdefJ"),
    ("indef_first_n33", 160, 33, 0, (160,), "indef_first"),
    ("indef_first_n97_G3", 300, 97, 0, (150, 60, 90), "indef_first"),
    ("indef_late_n97", 300, 97, 0, (300,), "indef_late"),
    ("indef_late_n97_G3", 300, 97, 0, (150, 60, 90), "indef_late"),
    ("full_A_n9_G3", 150, 9, 9, (100, 5, 45), "full_A"),
    ("wide_A_n10_t12_G3", 150, 10, 12, (100, 5, 45), "wide_A"),
    # appended (a case's seed is its position): n2 = 31 and n2 = 64 with t > 0
    ("pd_n36_t5_G3", 150, 36, 5, (70, 20, 60), "pd"),
    ("pd_n70_t6_G3", 250, 70, 6, (120, 40, 90), "pd"),
]:
    _ALL.append(_c(*args))

CASES = {c.name: c for c in _ALL}
SHORT_A = Case("short_A_n20_t13", 150, 20, 13, (150,), "short_A", 31990)       # error -8 only
BIG = Case("pd_n1024_t16_G2", 2048, 1024, 16, (1024, 1024), "pd", 31995)        # the size the device-wide form exists for; GPU only

POSDEF_KINDS = ("pd", "zero", "rankdefJ", "wide_A")
INDEFINITE_KINDS = ("indef_first", "indef_late")


def _sym_W(J, A, ref, Gam):
    return nr._sW22_oracle(J, A, ref, Gam)


@functools.lru_cache(maxsize=None)
def build(name):
    """(J, rx, A (t x n), cx, Gamma, oracle result) of a case"""
    c = SHORT_A if name == SHORT_A.name else BIG if name == BIG.name else CASES[name]
    if c.kind == "rankdefJ":
        J, rx, A, cx = synth.make_rank_deficient_J(c.seed, c.m, c.n, c.t)
    elif c.kind == "wide_A":
        J, rx, A, cx = nr.make_wide_rankdef_A(c.seed, c.m, c.n, c.t)
    elif c.kind == "short_A":
        J, rx, A, cx = synth.make_rank_deficient_A(c.seed, c.m, c.n, c.t)
    else:
        J, rx, A, cx = synth.make_problem(c.seed, c.m, c.n, c.t)
    A = np.asarray(A, dtype=np.float64).reshape(-1, c.n)
    cx = np.asarray(cx, dtype=np.float64)
    ref = go.gn_subproblem(J, rx, A, cx)
    Gam, _ = nr.make_gammas(c.seed + 1, J, A, ref, scale=0.01 if c.kind == "wide_A" else 0.3)
    if c.kind == "zero":
        Gam = np.zeros((c.n, c.n))
    elif c.kind == "indef_first":
        Gam = Gam.copy()
        Gam[0, 0] -= _sym_W(J, A, ref, Gam)[0, 0] + 1.0
    elif c.kind == "indef_late":
        Gam = Gam.copy()
        S = _sym_W(J, A, ref, Gam)
        k = LATE_PIVOT
        L = np.linalg.cholesky(S[:k, :k])
        w = np.linalg.solve(L, S[:k, k])
        schur = S[k, k] - w @ w
        assert schur > 0
        Gam[k, k] -= schur + 0.05 * np.abs(S).max()
    for x in (J, rx, A, cx, Gam):
        x.setflags(write=False)
    return J, rx, A, cx, Gam, ref


def uses_mpmath(c):
    return (c.n <= 40 and c.m <= 300) or not nr.LD_OK


@functools.lru_cache(maxsize=None)
def reference(name):
    """the high-precision reference of a case: members p, error, fail_index, cond, undefined, sW"""
    c = SHORT_A if name == SHORT_A.name else CASES[name]
    J, rx, A, cx, Gam, ref = build(name)
    return (nr.NewtonReference if uses_mpmath(c) else nr.NewtonReferenceLD)(J, rx, A, cx, Gam, ref)


def offsets(heights):
    return [int(x) for x in np.concatenate([[0], np.cumsum(heights)[:-1]])]


def sharded_restatement(J, rx, A, cx, Gam, ref, heights, drop=None):
    """The sharded formulation in NumPy: per shard the unpivoted QR of [J2_g | d_temp_g], the pivoted QR of the stacked triangles
    (R, Pi, d), then E = F_A.Q' Gamma F_A.Q, sW22 = sym(E22) + Pi R'R Pi', rhs = -E21 p1 + Pi R' d[1:kp], numpy.linalg.cholesky and
    the two solves.  drop: the shard whose triangle is left out of the stack (negative control).  Returns (p, sW22); raises
    numpy.linalg.LinAlgError when sW22 is not positive definite."""
    n = J.shape[1]
    t = A.shape[0]
    r = ref.rankA
    n2 = n - r
    Q1 = ref.F_A.Q_mul(np.eye(n)) if t else np.eye(n)
    p1 = (Q1.T @ ref.p)[:r]                      # p_gn = F_A.Q [p1; p2]
    if n2 == 0:
        return p1.copy(), np.zeros((0, 0))
    blocks, zs = [], []
    for g, (lo, h) in enumerate(zip(offsets(heights), heights)):
        if g == drop:
            continue
        JQ = J[lo:lo + h] @ Q1
        dt = -(rx[lo:lo + h] + JQ[:, :r] @ p1)
        Rg = np.linalg.qr(np.column_stack([JQ[:, r:], dt]), mode="r")
        T = np.zeros((n2, n2 + 1))
        k = min(Rg.shape[0], n2)
        T[:k] = Rg[:k]
        blocks.append(np.triu(T[:, :n2]))
        zs.append(T[:, n2])
    if blocks:
        F = go.qr_colnorm(np.vstack(blocks))
        kp = min(F.R.shape[0], n2)
        R = np.triu(F.R[:kp, :n2])
        d = F.Qt_mul(np.concatenate(zs))[:kp]
        pj = F.p - 1
        G2 = np.zeros((n2, n2))
        G2[np.ix_(pj, pj)] = R.T @ R
        g2 = np.zeros(n2)
        g2[pj] = R.T @ d
    else:
        G2, g2 = np.zeros((n2, n2)), np.zeros(n2)
    E = Q1.T @ Gam @ Q1
    if t > r:
        vp = ref.F_L11.p - 1
        E = E[np.ix_(vp, vp)]
    sW = 0.5 * (E[r:, r:] + E[r:, r:].T) + G2
    rhs = g2 - E[r:, :r] @ p1
    L = np.linalg.cholesky(sW)
    p2 = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    return Q1 @ np.concatenate([p1, p2]), sW


def rel(p, q):
    return float(np.linalg.norm(np.asarray(p) - q) / max(np.linalg.norm(q), np.finfo(float).tiny))
