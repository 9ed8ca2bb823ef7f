"""High-precision reference for the Newton direction (test infrastructure, CPU only).

newton_search_direction (src/enlsip_functions.jl:371-421) after its Hessian sums, evaluated in mpmath at DPS digits from the
exact binary inputs and the pivots / ranks of the FP64 oracle — by definition: F_A.Q (and F_L11.Q) are rebuilt in mpmath by
Householder reflectors with LAPACK's sign convention in the oracle's pivot order, J*F_A.Q is formed from J, and J2'J2, J2'J1,
J2'rx are sums over the m rows.  Nothing here goes through the R factor of J2, which is the route the batched kernels take.

Problem makers: Gamma = symmetric part + a small non-symmetric part (r_mat - c_mat need not be symmetric), shifted so that the
FP64 oracle's sW22 is positive definite with cond <= 1e8, and an indefinite partner Gamma - c I whose smallest eigenvalue of sW22
lies below -1e-3 ||sW22||, so that the verdict does not hang on rounding.

The form predicate of the batched Newton direction is parsed from gn_newton_batched.inc."""
import re
from pathlib import Path

import mpmath as mp
import numpy as np

from oracle import gn_oracle as go, synth

U = np.finfo(np.float64).eps / 2          # unit roundoff
DPS = 32                                   # digits of the mpmath reference

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "enlsip.jl_amd" / "csrc"

# rel(p, p_mp) <= C_NEWTON * u * cond(sW22).  Measured by tests/test_newton_reference.py: over every case of GRID below the FP64
# restatement of the reference's lines (tests/test_gpu_parity.py::_newton_reference) has its worst error at 14.67 u cond(sW22)
# (case rankdefA_t_ge_n, cond(sW22) ~ 1: there the error is that of p1, which comes through the two factorisations of the
# rank-deficient working set, and cond(sW22) does not see it; the next are n1_t0 at 4.67 and n2_t1 at 2.45, a few roundings on
# a result of one or two entries).  Times 8, the margin C_EST has in consumer_reference.py for the same reason (another
# summation order: here R'R instead of J2'J2, and the blocked factorisation): 117.4, rounded up.
C_NEWTON = 118.0


def newton_bound(cond_sW22):
    return C_NEWTON * U * max(cond_sW22, 1.0)


def newton_form_limit():
    """n_max of `small = P.n <= N` in gn_newton_batched.inc"""
    txt = (CSRC / "gn_newton_batched.inc").read_text()
    mt = re.search(r"const bool small\s*=\s*P\.n\s*<=\s*([0-9]+)\s*;", txt)
    assert mt, "wave-form predicate not found in gn_newton_batched.inc"
    return int(mt.group(1))


def expected_newton_form(n):
    return 1 if n <= newton_form_limit() else 0


# ---- mpmath linear algebra on lists of lists -----------------------------------------------------------------------------------
def _mpm(M):
    return [[mp.mpf(float(x)) for x in row] for row in np.atleast_2d(M)]


def _householder(cols, k):
    """LAPACK's dgeqr2 on the given columns (lists of length rows), k reflectors: returns (vs, taus, R columns)."""
    cols = [c[:] for c in cols]
    rows = len(cols[0]) if cols else 0
    vs, taus = [], []
    for j in range(k):
        x = cols[j]
        alpha = x[j]
        xn2 = mp.fsum(v * v for v in x[j + 1:])
        if xn2 == 0:
            vs.append([mp.mpf(0)] * rows)
            taus.append(mp.mpf(0))
            continue
        nrm = mp.sqrt(alpha * alpha + xn2)
        beta = -nrm if alpha >= 0 else nrm
        tau = (beta - alpha) / beta
        sc = 1 / (alpha - beta)
        v = [mp.mpf(0)] * j + [mp.mpf(1)] + [e * sc for e in x[j + 1:]]
        vs.append(v)
        taus.append(tau)
        for c in range(j, len(cols)):
            col = cols[c]
            dot = mp.fsum(v[r] * col[r] for r in range(j, rows)) * tau
            for r in range(j, rows):
                col[r] -= dot * v[r]
    return vs, taus, cols


def _apply_qt(vs, taus, x):
    x = x[:]
    for v, tau in zip(vs, taus):
        if tau == 0:
            continue
        dot = mp.fsum(a * b for a, b in zip(v, x)) * tau
        x = [b - dot * a for a, b in zip(v, x)]
    return x


def _apply_q(vs, taus, x):
    x = x[:]
    for v, tau in zip(reversed(vs), reversed(taus)):
        if tau == 0:
            continue
        dot = mp.fsum(a * b for a, b in zip(v, x)) * tau
        x = [b - dot * a for a, b in zip(v, x)]
    return x


def _cholesky_solve(S, d):
    """(L, x) with S = L L', S x = d; None when a pivot is <= 0 (dpotrf's verdict)."""
    k = len(S)
    L = [[mp.mpf(0)] * k for _ in range(k)]
    for j in range(k):
        s = S[j][j] - mp.fsum(L[j][c] * L[j][c] for c in range(j))
        if not s > 0:
            return None
        L[j][j] = mp.sqrt(s)
        for i in range(j + 1, k):
            L[i][j] = (S[i][j] - mp.fsum(L[i][c] * L[j][c] for c in range(j))) / L[j][j]
    y = [mp.mpf(0)] * k
    for i in range(k):
        y[i] = (d[i] - mp.fsum(L[i][c] * y[c] for c in range(i))) / L[i][i]
    x = [mp.mpf(0)] * k
    for i in reversed(range(k)):
        x[i] = (y[i] - mp.fsum(L[c][i] * x[c] for c in range(i + 1, k))) / L[i][i]
    return x


class NewtonReference:
    """p, error of src/enlsip_functions.jl:371-421 in mpmath, cond(sW22) (2-norm, from the FP64 oracle's sW22), and `undefined`
    for a rank-deficient working set with t < n (the reference indexes out of bounds; the library's status 2)."""

    def __init__(self, J, rx, A, cx, Gam, ref=None):
        with mp.workdps(DPS):
            self._run(J, rx, A, cx, Gam, ref or go.gn_subproblem(J, rx, A, cx))

    def _run(self, J, rx, A, cx, Gam, ref):
        m, n = J.shape
        t = A.shape[0] if A.size else 0
        r = ref.rankA
        self.rankA, self.undefined, self.error, self.p, self.cond = r, False, False, None, 1.0
        if t != r and t < n:
            self.undefined = True
            return
        kA = min(n, t)
        pA = (ref.F_A.p - 1) if t else np.zeros(0, dtype=int)
        At = _mpm(A.T) if t else []                                     # n x t
        colsA = [[At[i][c] for i in range(n)] for c in pA]              # A' P, column by column
        vA, tauA, RA = _householder(colsA, kA)
        bb = [-mp.mpf(float(cx[c])) for c in pA]
        if r == t:                                                       # p1 = LowerTriangular(R_A') \ b
            p1 = [mp.mpf(0)] * t
            for i in range(t):
                p1[i] = (bb[i] - mp.fsum(RA[i][c] * p1[c] for c in range(i))) / RA[i][i]
        else:                                                            # :371-373 through F_L11 (pivots of the oracle)
            pL = ref.F_L11.p - 1
            colsL = [[RA[i][c] if c <= i else mp.mpf(0) for i in range(t)] for c in pL]    # L11 = R_A' (t x kA), columns permuted
            vL, tauL, RL = _householder(colsL, min(t, kA))
            b = _apply_qt(vL, tauL, bb)
            dp1 = [mp.mpf(0)] * r
            for i in reversed(range(r)):
                dp1[i] = (b[i] - mp.fsum(RL[c][i] * dp1[c] for c in range(i + 1, r))) / RL[i][i]
            full = [mp.mpf(0)] * kA
            for i in range(r):
                full[pL[i]] = dp1[i]
            p1 = full[:r]
        if r == n:
            self.p = np.array([float(x) for x in p1])
            return
        n2 = n - r
        Q = [_apply_q(vA, tauA, [mp.mpf(1 if i == c else 0) for i in range(n)]) for c in range(n)]     # Q[c] = column c
        Jm, Gm = _mpm(J), _mpm(Gam)
        JQ = [[mp.fsum(Jm[i][k] * Q[c][k] for k in range(n)) for i in range(m)] for c in range(n)]       # columns of J Q
        GQ = [[mp.fsum(Gm[i][k] * Q[c][k] for k in range(n)) for i in range(n)] for c in range(n)]
        E = [[mp.fsum(Q[i][k] * GQ[c][k] for k in range(n)) for c in range(n)] for i in range(n)]
        if t > r:                                                        # :396-399
            vp = ref.F_L11.p - 1
            E = [[E[vp[i]][vp[c]] for c in range(n)] for i in range(n)]
        rxm = [mp.mpf(float(x)) for x in rx]
        W22 = [[E[r + i][r + c] + mp.fsum(a * b for a, b in zip(JQ[r + i], JQ[r + c])) for c in range(n2)] for i in range(n2)]
        d = []
        for i in range(n2):
            w21p = mp.fsum((E[r + i][c] + mp.fsum(a * b for a, b in zip(JQ[r + i], JQ[c]))) * p1[c] for c in range(r))
            d.append(-w21p - mp.fsum(a * b for a, b in zip(JQ[r + i], rxm)))
        sW = [[(W22[i][c] + W22[c][i]) / 2 for c in range(n2)] for i in range(n2)]
        sWf = np.array([[float(x) for x in row] for row in sW])
        ev = np.linalg.eigvalsh(sWf)
        self.lam_min, self.norm = float(ev[0]), float(np.abs(ev).max())
        p2 = _cholesky_solve(sW, d)
        if p2 is None:
            self.error = True
            self.p = np.zeros(n)
            return
        self.cond = float(ev[-1] / ev[0])
        self.p = np.array([float(x) for x in _apply_q(vA, tauA, p1 + p2)])


# ---- problem makers ------------------------------------------------------------------------------------------------------------
def _sW22_oracle(J, A, ref, Gam):
    n = J.shape[1]
    t = A.shape[0] if A.size else 0
    r = ref.rankA
    Q1 = ref.F_A.Q_mul(np.eye(n)) if t else np.eye(n)
    E = Q1.T @ Gam @ Q1
    if t > r:
        vp = ref.F_L11.p - 1
        E = E[np.ix_(vp, vp)]
    J2 = (J @ Q1)[:, r:]
    W22 = E[r:, r:] + J2.T @ J2
    return 0.5 * (W22 + W22.T)


def make_gammas(seed, J, A, ref, scale=0.3):
    """(Gamma, Gamma_indefinite) for one problem: the first with the oracle's sW22 positive definite and cond <= 1e8, the second
    = Gamma - c I with lambda_min(sW22) < -1e-3 ||sW22||.  With n2 = 0 both are the plain random matrix."""
    n = J.shape[1]
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n, n))
    Gam = scale * (S + S.T) + 0.1 * scale * rng.standard_normal((n, n))
    if ref.rankA == n or (ref.rankA != (A.shape[0] if A.size else 0) and (A.shape[0] if A.size else 0) < n):
        return Gam, Gam
    ev = np.linalg.eigvalsh(_sW22_oracle(J, A, ref, Gam))
    floor = max(abs(ev[-1]), 1.0) * 1e-6
    if ev[0] < floor:                       # shift: E22 moves by the same multiple of I (Q is orthogonal, a permutation keeps I)
        Gam = Gam + (floor - ev[0]) * np.eye(n)
    ev = np.linalg.eigvalsh(_sW22_oracle(J, A, ref, Gam))
    assert ev[0] > 0 and ev[-1] / ev[0] <= 1e8, (ev[0], ev[-1])
    c = ev[0] + 0.05 * max(abs(ev[-1]), 1.0)
    Gbad = Gam - c * np.eye(n)
    evb = np.linalg.eigvalsh(_sW22_oracle(J, A, ref, Gbad))
    assert evb[0] < -1e-3 * np.abs(evb).max(), evb[[0, -1]]
    return Gam, Gbad


def make_wide_rankdef_A(seed, m, n, t):
    """t >= n constraints of rank n - 2: the rank-deficient working set the reference's E[F_L11.p, F_L11.p] branch is defined for"""
    J, rx, _, _ = synth.make_problem(seed, m, n, 1)
    B = synth.normal_stream(seed, 7, t * (n - 2)).reshape(t, n - 2)
    C = synth.normal_stream(seed, 8, (n - 2) * n).reshape(n - 2, n)
    A = B @ C
    cx = synth.normal_stream(seed, 9, t)
    return J, rx, A, cx


# name, m, n, t, maker — small enough for mpmath; the GPU grid (tests/test_gpu_newton_batched.py) samples its problems from these
# shapes and adds the large ones, which are held to the per-problem entry point only
GRID = [
    ("n1_t0", 20, 1, 0, "plain"),
    ("n2_t1", 30, 2, 1, "plain"),
    ("t3_60x12", 60, 12, 3, "plain"),
    ("t0_300x40", 300, 40, 0, "plain"),
    ("t_eq_n_40x9", 40, 9, 9, "plain"),
    ("wide_m_lt_n2", 10, 24, 4, "plain"),
    ("rankdefJ_300x40_t6", 300, 40, 6, "rankdefJ"),
    ("rankdefA_t_lt_n", 54, 20, 13, "rankdefA"),
    ("rankdefA_t_ge_n", 50, 10, 12, "wide_rankdefA"),
    ("n33_t5", 120, 33, 5, "plain"),
]


def make_case(name, k=0):
    _, m, n, t, kind = next(g for g in GRID if g[0] == name)
    seed = 12000 + 97 * [g[0] for g in GRID].index(name) + k
    if kind == "plain":
        return synth.make_problem(seed, m, n, t)
    if kind == "rankdefJ":
        return synth.make_rank_deficient_J(seed, m, n, t)
    if kind == "rankdefA":
        return synth.make_rank_deficient_A(seed, m, n, t)
    return make_wide_rankdef_A(seed, m, n, t)
