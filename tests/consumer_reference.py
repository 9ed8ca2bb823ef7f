"""High-precision references for the batched consumers of a solve (test infrastructure, CPU only).

The multiplier estimates by their definition, free of the pivot order.  With S = jpvtA[:pr] - 1 the constraints that the pivoted
QR of A' keeps (pr = pseudo_rank of diag R), A'P[:, :pr] = Q[:, :pr] R11 gives

    first : lambda_S = (A_S A_S')^{-1} (A_S g - c_S),        lambda_j = 0 for j not in S
            grad_res = || g - A_S' (A_S A_S')^{-1} A_S g ||  (0 when pr = n)
    second: lambda_S = (A_S A_S')^{-1} A_S J' (rx + J p),    lambda_j = 0 for j not in S

then lambda * diag_scale entry by entry.  They are evaluated in mpmath at DPS digits from the exact binary inputs, so they share
no arithmetic with the QR-and-two-triangular-solves of the kernels or of the FP64 oracle.  The products J' rx, J p and A p are
correctly rounded sums of exact products (Dekker's two-product + math.fsum).  Problem makers: constraints with prescribed singular
values, and near-dependent constraints whose last |R_ii| sits a factor 2 above or below the pseudo-rank tolerance.

The wave-form predicate of the estimates is parsed from gn_lagrange_batched.inc, so the grid below cannot drift from the library."""
import math
import re
from pathlib import Path

import mpmath as mp
import numpy as np

from oracle import gn_oracle as go, synth

U = np.finfo(np.float64).eps / 2          # unit roundoff
DPS = 32                                   # digits of the mpmath references

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "enlsip.jl_amd" / "csrc"


def wave_form_limits():
    """(n_max, t_max) of `small = h->lagrange_small && P.n <= N && P.t <= T` in gn_lagrange_batched.inc"""
    txt = (CSRC / "gn_lagrange_batched.inc").read_text()
    mt = re.search(r"lagrange_small\s*&&\s*P\.n\s*<=\s*([0-9]+)\s*&&\s*P\.t\s*<=\s*([0-9]+)", txt)
    assert mt, "wave-form predicate not found in gn_lagrange_batched.inc"
    return int(mt.group(1)), int(mt.group(2))


def max_launch_batch():
    mt = re.search(r"constexpr\s+long long\s+GN_MAX_LAUNCH_BATCH\s*=\s*([0-9]+)", (CSRC / "enlsip_gn.hip").read_text())
    return int(mt.group(1))


def expected_form(n, t_max, small_enabled=True):
    nmax, tmax = wave_form_limits()
    return 1 if small_enabled and n <= nmax and t_max <= tmax else 0


# ---- the accuracy bound of the estimates ---------------------------------------------------------------------------------------
# rel_err <= C_EST * u * kappa(A_S)^2 * gamma.  kappa(A_S)^2 is the condition of the normal equations the closed forms solve (the
# QR route does not square it for the least-squares part, but the c_S part does).  gamma >= 1 is the cancellation the result
# inherits: in the right-hand side that the kernel forms itself, || |J'| (|rx| + |J| |p|) || / || J' (rx + J p) || (second
# estimate, and a gradient formed from the resident J, rx), times, for the first estimate, the cancellation between its
# least-squares part and its c_S part (EstimateReference.first_cancellation).
# C_EST = 128: on the sampled problems of every case of the consumer grid (tests/test_consumer_reference.py) the FP64 oracle's worst
# error is 10.4 u kappa^2 gamma (n12_t6_dup and n7_t1, kappa(A_S) ~ 1: a few roundings of the two triangular solves); 128 keeps the
# oracle 12x inside the bound, above the 8x that the test requires.  The bound is loose for kappa = 1e4 (the QR route loses about
# u kappa there, not u kappa^2), which is why the GPU tests also hold each kernel to 8x the oracle's own error.
C_EST = 128.0


def estimate_bound(kappa_S, gamma=1.0):
    return C_EST * U * kappa_S ** 2 * max(1.0, gamma)


def kappa(M):
    M = np.atleast_2d(M)
    if M.size == 0:
        return 1.0
    s = np.linalg.svd(M, compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else math.inf


def gamma_rhs(J, rx, p=None):
    """|| |J'| (|rx| + |J| |p|) || / || J' (rx + J p) || (p = None: the gradient J' rx), from the exact products"""
    r = rx if p is None else exact_matvec(J, p, x0=rx)[0]
    num = np.abs(J).T @ (np.abs(rx) + (0.0 if p is None else np.abs(J) @ np.abs(p)))
    den = np.linalg.norm(exact_matvec(J.T, r)[0])
    return float(np.linalg.norm(num) / den) if den > 0 else math.inf


def rel_err(x, ref):
    nr = np.linalg.norm(ref)
    return float(np.linalg.norm(np.asarray(x) - ref) / nr) if nr > 0 else float(np.linalg.norm(x))


# ---- exact products --------------------------------------------------------------------------------------------------------------
_SPLIT = 134217729.0        # 2^27 + 1


def _two_product(a, b):
    """p + e == a * b exactly (Dekker; no overflow / underflow in the data these tests use)"""
    p = a * b
    c = _SPLIT * a
    ah = c - (c - a)
    al = a - ah
    c = _SPLIT * b
    bh = c - (c - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_matvec(M, x, x0=None):
    """(y, bound): y[i] = x0[i] + sum_c M[i, c] x[c] correctly rounded; bound[i] = 2 k u (|x0[i]| + sum |M[i, c]| |x[c]|), k the
    length of the sum, which bounds the error of the same sum evaluated in any order in FP64."""
    M = np.atleast_2d(np.asarray(M, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    P, E = _two_product(M, x[None, :])
    rows, k = M.shape
    y = np.empty(rows)
    for i in range(rows):
        terms = [P[i], E[i]] if x0 is None else [P[i], E[i], [x0[i]]]
        y[i] = math.fsum(np.concatenate(terms))
    mag = np.abs(M) @ np.abs(x) + (0.0 if x0 is None else np.abs(x0))
    return y, 2.0 * (k + (x0 is not None)) * U * mag


def exact_gradient(J, rx):
    """J' rx correctly rounded (the reference gradient when the kernel forms it from the resident J, rx)"""
    return exact_matvec(np.asarray(J).T, rx)[0]


# ---- the estimates by their definition --------------------------------------------------------------------------------------------
def _mpf(v):
    return [mp.mpf(float(x)) for x in np.asarray(v, dtype=np.float64).ravel()]


def _mprows(M):
    return [_mpf(r) for r in np.atleast_2d(np.asarray(M, dtype=np.float64))]


class EstimateReference:
    """The closed forms for one A (t x n) and one kept set S: the Gram matrix A_S A_S' from exact products and its Cholesky factor,
    formed once for every right-hand side (mpmath.fdot throughout: about 0.25 s for a 64 x 64 A_S).  Results before diag_scale
    are kept per right-hand side, so a call that only changes diag_scale costs nothing."""

    def __init__(self, A, S, dps=DPS):
        self.A = np.asarray(A, dtype=np.float64)
        self.S = [int(i) for i in S]
        self.dps = dps
        self.t, self.n = self.A.shape
        self._memo = {}
        k = len(self.S)
        with mp.workdps(dps):
            self.AS = _mprows(self.A[self.S]) if k else []
            self.ASt = [list(col) for col in zip(*self.AS)]
            L = [[mp.mpf(0)] * k for _ in range(k)]
            for i in range(k):
                for j in range(i + 1):
                    s = mp.fdot(self.AS[i], self.AS[j]) - mp.fdot(L[i][:j], L[j][:j])
                    L[i][j] = mp.sqrt(s) if i == j else s / L[j][j]
            self.L = L

    def _gram_solve(self, b):
        """(A_S A_S')^{-1} b"""
        L, k = self.L, len(self.S)
        y = [None] * k
        for i in range(k):
            y[i] = (b[i] - mp.fdot(L[i][:i], y[:i])) / L[i][i]
        x = [None] * k
        for i in reversed(range(k)):
            x[i] = (y[i] - mp.fdot([L[j][i] for j in range(i + 1, k)], x[i + 1:])) / L[i][i]
        return x

    def _lam(self, lamS, diag):
        lam = np.zeros(self.t)
        with mp.workdps(self.dps):
            for i, j in enumerate(self.S):
                lam[j] = float(lamS[i] * mp.mpf(float(diag[j]))) if diag is not None else float(lamS[i])
        return lam

    @staticmethod
    def _key(*arrays):
        return tuple(np.asarray(a, dtype=np.float64).tobytes() for a in arrays)

    def first(self, g, cx, diag=None):
        """(lambda (t,), grad_res) for the gradient g (exact binary values) and constraint values cx"""
        key = ("first",) + self._key(g, cx)
        if key not in self._memo:
            with mp.workdps(self.dps):
                gm = _mpf(g)
                if not self.S:
                    self._memo[key] = ([], float(mp.sqrt(mp.fdot(gm, gm))), 1.0)
                else:
                    ASg = [mp.fdot(r, gm) for r in self.AS]
                    w = self._gram_solve(ASg)
                    wc = self._gram_solve([mp.mpf(float(cx[j])) for j in self.S])
                    lamS = [a - b for a, b in zip(w, wc)]
                    if len(self.S) == self.n:
                        gres = 0.0
                    else:
                        res = [gm[c] - mp.fdot(self.ASt[c], w) for c in range(self.n)]
                        gres = float(mp.sqrt(mp.fdot(res, res)))
                    nrm = lambda v: mp.sqrt(mp.fdot(v, v))
                    nl = nrm(lamS)
                    canc = float((nrm(w) + nrm(wc)) / nl) if nl > 0 else math.inf
                    self._memo[key] = (lamS, gres, canc)
        lamS, gres, _ = self._memo[key]
        return self._lam(lamS, diag), gres

    def first_cancellation(self, g, cx):
        """(||lambda_g|| + ||lambda_c||) / ||lambda|| of the first estimate's two parts, lambda_g = (A_S A_S')^{-1} A_S g and
        lambda_c = (A_S A_S')^{-1} c_S: each part carries its own rounding, the difference only their sum"""
        self.first(g, cx)
        return self._memo[("first",) + self._key(g, cx)][2]

    def second(self, J, rx, p, diag=None):
        """lambda (t,) of the second estimate: (A_S A_S')^{-1} A_S J' (rx + J p)"""
        key = ("second",) + self._key(J, rx, p)
        if key not in self._memo:
            lamS = []
            if self.S:
                with mp.workdps(self.dps):
                    Jr = _mprows(J)
                    pm, rxm = _mpf(p), _mpf(rx)
                    r = [rxm[i] + mp.fdot(Jr[i], pm) for i in range(len(Jr))]
                    Jtr = [mp.fdot(col, r) for col in zip(*Jr)]
                    lamS = self._gram_solve([mp.fdot(row, Jtr) for row in self.AS])
            self._memo[key] = lamS
        return self._lam(self._memo[key], diag)


def kept_set(jpvt, diagR, eps_rank):
    """(S, pr): the constraints that pseudo_rank keeps, 0-based, in pivot order"""
    pr = go.pseudo_rank(np.asarray(diagR), eps_rank)
    return [int(v) - 1 for v in np.asarray(jpvt)[:pr]], pr


# ---- problem makers ----------------------------------------------------------------------------------------------------------------
def _orth(seed, stream, rows, k):
    Z = synth.normal_stream(seed, stream, rows * k).reshape((rows, k), order="F")
    Q, R = np.linalg.qr(Z)
    return Q * np.sign(np.diag(R))[None, :]


def conditioned_A(seed, n, t, kappa_A, sigmas=None):
    """A (t x n) = U diag(s) V' from synth.normal_stream draws, s geometric from 1 to 1/kappa_A (or `sigmas`), scaled so that
    its entries are O(1)"""
    k = min(n, t)
    if k == 0:
        return np.zeros((t, n))
    s = np.geomspace(1.0, 1.0 / kappa_A, k) if sigmas is None else np.asarray(sigmas, dtype=np.float64)
    Uo, Vo = _orth(seed, 12, t, k), _orth(seed, 13, n, k)
    return math.sqrt(max(n, t)) * (Uo * s[None, :]) @ Vo.T


def make_problem(seed, m, n, t, kappa_A=1.0):
    """(J m x n, rx m, A t x n, cx t): J, rx, cx as synth.make_problem, A with kappa(A) = kappa_A; kappa_A = "dup": a well
    conditioned A whose last row repeats row 0 (rank t - 1, the kept duplicate decided by the pivot order)"""
    J, rx, _, cx = synth.make_problem(seed, m, n, t)
    A = conditioned_A(seed, n, t, 1.0 if kappa_A == "dup" else kappa_A)
    if kappa_A == "dup" and t >= 2:
        A[-1] = A[0]
    return J, rx, A, cx


def pivot_tolerance(A, eps_rank):
    """(|R_00| sqrt(kA) eps_rank, diag R) of the FP64 pivoted QR of A'"""
    d = go.qr_colnorm(np.asarray(A).T).diagR()
    return abs(d[0]) * math.sqrt(d.size) * eps_rank, d


def near_dependent_A(seed, n, t, eps_rank, side):
    """A (t x n, min(n, t) >= 2) whose last |R_ii| (pivoted QR of A') lands `side` (2 or 0.5) times the pseudo-rank tolerance.
    t <= n: A[-1] = A[0] + delta w.  t > n: every row near one (n-1)-dimensional subspace (singular values 1, ..., 1, delta), since
    moving one row cannot lower the rank of n generic rows.  delta is refined on the FP64 factorisation (|R_last| is linear in
    delta) until the ratio is within 2 % of `side`."""
    k = min(n, t)
    assert k >= 2
    if t <= n:
        base = conditioned_A(seed, n, t, 1.0)
        w = synth.normal_stream(seed, 14, n)

        def build(delta):
            A = base.copy()
            A[-1] = A[0] + delta * w
            return A
    else:
        def build(delta):
            return conditioned_A(seed, n, t, 1.0, sigmas=[1.0] * (k - 1) + [delta])
    delta, ratio = 1e-6, None
    for _ in range(8):
        A = build(delta)
        tol, d = pivot_tolerance(A, eps_rank)
        ratio = abs(d[-1]) / tol
        if abs(ratio / side - 1.0) < 0.02:
            return A
        delta *= side / ratio
    raise AssertionError(f"near_dependent_A did not converge: ratio {ratio} for side {side}")


def random_diag(seed, count, t_max):
    w = max(t_max, 1)
    return (1.0 + 0.25 * np.abs(synth.normal_stream(seed, 5, count * w))).reshape(count, w)[:, :t_max].copy()


# ---- the consumer grid ----------------------------------------------------------------------------------------------------------------
# (name, m, n, t_max, t_k per problem, kappa(A), query ranges (prob0, count)).  The wave form's edges (n, t_max in {1, 2, 63, 64}),
# t > n (kA = n, trapezoidal R), both sides of the switch (65), m from 1 to 1000, batches of 1, 3, 5 and 9, ragged t_k with zeros,
# and query ranges whose prob0 and count are not multiples of 4.  Not a cross product: the estimate kernels see m only through
# the gemv that forms their right-hand side.
ESTIMATE_GRID = [
    ("n1_t1", 65, 1, 1, [1, 1, 1], 1.0, [(0, 3), (1, 2)]),
    ("n1_t3", 65, 1, 3, [3, 3, 3, 3, 3], 1.0, [(0, 5), (1, 3)]),
    ("n2_t2_m1", 1, 2, 2, [2, 2, 2, 2, 2], 1e2, [(0, 5), (3, 2)]),
    ("n2_t64", 257, 2, 64, [64, 64, 64], 1e2, [(0, 3), (1, 1)]),
    ("n7_t15_ragged", 513, 7, 15, [15, 0, 7, 15, 3, 12, 1, 15, 9], 1e2, [(0, 9), (3, 5)]),
    ("n8_t64", 257, 8, 64, [64, 64, 64], 1e4, [(0, 3)]),
    ("n7_t1", 1000, 7, 1, [1] * 9, 1.0, [(0, 9), (1, 7)]),
    ("n63_t2_ragged", 65, 63, 2, [2, 0, 2, 1, 2], 1e4, [(0, 5), (1, 3)]),
    ("n63_t63", 1000, 63, 63, [63, 63, 63], 1e4, [(0, 3), (1, 2)]),
    ("n64_t64", 257, 64, 64, [64, 64, 64], 1e2, [(0, 3), (1, 1)]),
    ("n64_t15_ragged", 65, 64, 15, [15, 0, 11, 15, 15, 4, 15, 2, 15], 1e4, [(0, 9), (5, 3)]),
    ("n64_t65_ragged", 513, 64, 65, [65, 64, 65], 1e2, [(0, 3), (1, 2)]),
    ("n65_t64", 1000, 65, 64, [64, 64, 64], 1.0, [(0, 3), (1, 2)]),
    ("n65_t65", 257, 65, 65, [65], 1e4, [(0, 1)]),
    ("n65_t2_m1", 1, 65, 2, [2, 2, 2, 2, 2], 1e2, [(0, 5), (1, 3)]),
    ("n2_t65", 65, 2, 65, [65, 65, 65], 1e2, [(0, 3), (1, 2)]),
    ("n12_t6_dup", 300, 12, 6, [6, 6, 6, 6, 6], "dup", [(0, 5), (1, 3)]),
    ("n65_t9_dup_ragged", 200, 65, 9, [9, 5, 0], "dup", [(0, 3), (1, 1)]),
]


def sample_of(ts):
    """the problems of a case whose estimates are checked against the mpmath reference (every problem gets the exact checks):
    all with t_k > 0 on small shapes, the first and the last on t_max >= 32 (a 64 x 64 reference takes about a second)"""
    idx = [k for k in range(len(ts)) if ts[k] > 0]
    if max(ts) >= 32 and len(idx) > 1:
        idx = [idx[0], idx[-1]]
    return idx


def grid_problem(ci, k, m, n, tk, kappa_A):
    return make_problem(9000 + 100 * ci + k, m, n, tk, kappa_A)


# pseudo-rank straddle: (name, m, n, t, eps_rank, side).  The small diagonal is the last pivot (kA - 1); t = 64 >= 16 n at n = 2
# makes sqrt(kA) and sqrt(t) differ by 5.7x.
STRADDLE_GRID = [
    (f"{name}_{'below' if side < 1 else 'above'}_{'sqrteps' if eps == go.SQRT_EPS else '1e-14'}", m, n, t, eps, side)
    for (name, m, n, t) in (("n12_t6", 60, 12, 6), ("n2_t64", 80, 2, 64), ("n64_t64", 100, 64, 64), ("n40_t70", 120, 40, 70))
    for eps in (go.SQRT_EPS, 1e-14) for side in (0.5, 2.0)
]
