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


def _cholesky_solve(S, d, report=False):
    """x with S = L L', S x = d; None when a pivot is <= 0 (dpotrf's verdict).  report = True: (x, index of that pivot or -1)."""
    k = len(S)
    L = [[mp.mpf(0)] * k for _ in range(k)]
    for j in range(k):
        s = S[j][j] - mp.fsum(L[j][c] * L[j][c] for c in range(j))
        if not s > 0:
            return (None, j) if report else None
        L[j][j] = mp.sqrt(s)
        for i in range(j + 1, k):
            L[i][j] = (S[i][j] - mp.fsum(L[i][c] * L[j][c] for c in range(j))) / L[j][j]
    y = [mp.mpf(0)] * k
    for i in range(k):
        y[i] = (d[i] - mp.fsum(L[i][c] * y[c] for c in range(i))) / L[i][i]
    x = [mp.mpf(0)] * k
    for i in reversed(range(k)):
        x[i] = (y[i] - mp.fsum(L[c][i] * x[c] for c in range(i + 1, k))) / L[i][i]
    return (x, -1) if report else x


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
        self.fail_index, self.sW = -1, None      # the pivot dpotrf's verdict fell on; sW22 rounded to FP64
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
        self.sW = sWf
        p2, self.fail_index = _cholesky_solve(sW, d, report=True)
        if p2 is None:
            self.error = True
            self.p = np.zeros(n)
            return
        self.cond = float(ev[-1] / ev[0])
        self.p = np.array([float(x) for x in _apply_q(vA, tauA, p1 + p2)])


# ---- the same lines in np.longdouble -------------------------------------------------------------------------------------------
# One longdouble carries u_ld = 5.4e-20, and a system of condition kappa returns u_ld kappa of it: 1e-10 at kappa = 4e9.  So every
# value here is an unevaluated sum (hi, lo) of two longdoubles ("pair"), with the error-free sum and product of Knuth and Dekker;
# a pair carries about 2^-126.  Arrays of pairs are tuples of two longdouble arrays of one shape.
LD = np.longdouble
LD_OK = float(np.finfo(np.longdouble).eps) <= 1.1e-19          # the x87 extended format (64-bit significand) or better
_SPLIT = LD(2 ** 32 + 1)                                        # Dekker's splitter for a 64-bit significand


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _quick(a, b):
    s = a + b
    return s, b - (s - a)


def _halves(a):
    c = _SPLIT * a
    h = c - (c - a)
    return h, a - h


def _two_prod(a, b):
    p = a * b
    ah, al = _halves(a)
    bh, bl = _halves(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def pr(x):
    """the pair of an FP64 or longdouble array"""
    x = np.asarray(x, dtype=LD)
    return x, np.zeros_like(x)


def pr_zeros(*shape):
    return np.zeros(shape, dtype=LD), np.zeros(shape, dtype=LD)


def pr_add(x, y):
    s, e = _two_sum(x[0], y[0])
    t, f = _two_sum(x[1], y[1])
    s, e = _quick(s, e + t)
    return _quick(s, e + f)


def pr_neg(x):
    return -x[0], -x[1]


def pr_sub(x, y):
    return pr_add(x, pr_neg(y))


def pr_mul(x, y):
    p, e = _two_prod(x[0], y[0])
    return _quick(p, e + (x[0] * y[1] + x[1] * y[0]))


def pr_div(x, y):
    q1 = x[0] / y[0]
    r = pr_sub(x, pr_mul(y, (q1, 0 * q1)))
    q2 = r[0] / y[0]
    r = pr_sub(r, pr_mul(y, (q2, 0 * q2)))
    q3 = r[0] / y[0]
    return pr_add(_quick(q1, q2), (q3, 0 * q3))


def pr_sqrt(x):
    s = np.sqrt(x[0])
    r = pr_sub(x, pr_mul((s, 0 * s), (s, 0 * s)))
    return pr_add((s, 0 * s), (r[0] / (2 * s), 0 * s))


def pr_get(x, idx):
    return x[0][idx], x[1][idx]


def pr_set(x, idx, y):
    x[0][idx], x[1][idx] = y[0], y[1]


def pr_T(x):
    return x[0].T, x[1].T


def pr_sum(x, axis=0):
    """pairwise sum along an axis"""
    h, l = np.moveaxis(x[0], axis, 0), np.moveaxis(x[1], axis, 0)
    if h.shape[0] == 0:
        return pr_zeros(*h.shape[1:])
    while h.shape[0] > 1:
        k = h.shape[0] // 2
        top = (h[:k], l[:k])
        top = pr_add(top, (h[k:2 * k], l[k:2 * k]))
        h, l = np.concatenate([top[0], h[2 * k:]]), np.concatenate([top[1], l[2 * k:]])
    return h[0], l[0]


def pr_dot(x, y, axis=0):
    return pr_sum(pr_mul(x, y), axis)


def pr_outer(x, y):
    return pr_mul((x[0][:, None], x[1][:, None]), (y[0][None, :], y[1][None, :]))


def pr_gram(X, Y):
    """X'Y, the sum over the rows of the outer products"""
    acc = pr_zeros(X[0].shape[1], Y[0].shape[1])
    for i in range(X[0].shape[0]):
        acc = pr_add(acc, pr_outer(pr_get(X, i), pr_get(Y, i)))
    return acc


def pr_matvec(M, x):
    return pr_dot(M, (x[0][None, :], x[1][None, :]), axis=1)


def pr_float(x):
    return (x[0] + x[1]).astype(np.float64)


def _householder_pr(M, k):
    """_householder on the columns of the pair matrix M (rows x cols): (V rows x k, tau, R = the reduced M)."""
    M = (M[0].copy(), M[1].copy())
    rows = M[0].shape[0]
    V, tau = pr_zeros(rows, k), pr_zeros(k)
    for j in range(k):
        x = pr_get(M, (slice(None), j))
        alpha, tail = pr_get(x, j), pr_get(x, slice(j + 1, None))
        xn2 = pr_dot(tail, tail)
        if xn2[0] == 0:
            continue
        nrm = pr_sqrt(pr_add(pr_mul(alpha, alpha), xn2))
        beta = pr_neg(nrm) if alpha[0] >= 0 else nrm
        pr_set(tau, j, pr_div(pr_sub(beta, alpha), beta))
        V[0][j, j] = 1
        den = pr_sub(alpha, beta)
        pr_set(V, (slice(j + 1, None), j), pr_div(tail, (np.broadcast_to(den[0], tail[0].shape), np.broadcast_to(den[1], tail[0].shape))))
        v = pr_get(V, (slice(j, None), j))
        sub = pr_get(M, (slice(j, None), slice(j, None)))
        w = pr_dot((v[0][:, None], v[1][:, None]), sub, axis=0)
        w = pr_mul(w, (np.broadcast_to(tau[0][j], w[0].shape), np.broadcast_to(tau[1][j], w[0].shape)))
        pr_set(M, (slice(j, None), slice(j, None)), pr_sub(sub, pr_outer(v, w)))
    return V, tau, M


def _apply_q_pr(V, tau, X, transpose=False):
    """Q X (or Q' X) for the reflectors (V, tau), X a pair vector or matrix (the reflectors act on its first axis)"""
    X = (X[0].copy(), X[1].copy())
    vec = X[0].ndim == 1
    if vec:
        X = (X[0][:, None], X[1][:, None])
    order = range(V[0].shape[1]) if transpose else reversed(range(V[0].shape[1]))
    for j in order:
        if tau[0][j] == 0:
            continue
        v = pr_get(V, (slice(None), j))
        w = pr_dot((v[0][:, None], v[1][:, None]), X, axis=0)
        w = pr_mul(w, (np.broadcast_to(tau[0][j], w[0].shape), np.broadcast_to(tau[1][j], w[0].shape)))
        X = pr_sub(X, pr_outer(v, w))
    return (X[0][:, 0], X[1][:, 0]) if vec else X


def cholesky_fail_index(S):
    """index of the first pivot that is not > 0 in a left-looking Cholesky of S in S's own precision, -1 when there is none;
    also returns L"""
    S = np.array(S)
    k = S.shape[0]
    L = np.zeros_like(S)
    for j in range(k):
        s = S[j, j] - L[j, :j] @ L[j, :j]
        if not s > 0:
            return j, L
        L[j, j] = np.sqrt(s)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return -1, L


def _cholesky_pr(S):
    """cholesky_fail_index on a pair matrix"""
    k = S[0].shape[0]
    L = pr_zeros(k, k)
    for j in range(k):
        row = pr_get(L, (j, slice(0, j)))
        s = pr_sub(pr_get(S, (j, j)), pr_dot(row, row))
        if not s[0] > 0:
            return j, L
        d = pr_sqrt(s)
        pr_set(L, (j, j), d)
        if j + 1 < k:
            col = pr_sub(pr_get(S, (slice(j + 1, None), j)), pr_matvec(pr_get(L, (slice(j + 1, None), slice(0, j))), row))
            pr_set(L, (slice(j + 1, None), j), pr_div(col, (np.broadcast_to(d[0], col[0].shape), np.broadcast_to(d[1], col[0].shape))))
    return -1, L


def _trsv_pr(T, b, lower):
    """T x = b for a triangular pair matrix"""
    k = b[0].shape[0]
    x = pr_zeros(k)
    for i in (range(k) if lower else reversed(range(k))):
        done = slice(0, i) if lower else slice(i + 1, k)
        s = pr_sub(pr_get(b, i), pr_dot(pr_get(T, (i, done)), pr_get(x, done)))
        pr_set(x, i, pr_div(s, pr_get(T, (i, i))))
    return x


class NewtonReferenceLD:
    """NewtonReference line for line in pairs of np.longdouble (for the shapes mpmath is too slow for): the same members (p,
    error, fail_index, undefined, cond, lam_min, norm, sW), F_A.Q and F_L11.Q rebuilt from A in the oracle's pivot order, J F_A.Q
    from J, J2'J2, J2'J1 and J2'rx sums over the m rows, nothing through R."""

    def __init__(self, J, rx, A, cx, Gam, ref=None):
        ref = ref or go.gn_subproblem(J, rx, A, cx)
        m, n = J.shape
        t = A.shape[0] if A.size else 0
        r = ref.rankA
        self.rankA, self.undefined, self.error, self.p, self.cond = r, False, False, None, 1.0
        self.fail_index, self.sW = -1, None
        if t != r and t < n:
            self.undefined = True
            return
        kA = min(n, t)
        pA = (ref.F_A.p - 1) if t else np.zeros(0, dtype=int)
        vA, tauA, RA = _householder_pr(pr(np.asarray(A).T[:, pA] if t else np.zeros((n, 0))), kA)
        bb = pr(-np.asarray(cx)[pA] if t else np.zeros(0))
        if r == t:                                                       # p1 = LowerTriangular(R_A') \ b
            p1 = _trsv_pr(pr_T(pr_get(RA, (slice(0, t), slice(0, t)))), bb, lower=True)
        else:                                                            # :371-373 through F_L11 (pivots of the oracle)
            pL = ref.F_L11.p - 1
            L11 = pr_T((np.triu(RA[0][:kA, :]), np.triu(RA[1][:kA, :])))          # t x kA
            vL, tauL, RL = _householder_pr(pr_get(L11, (slice(None), pL)), min(t, kA))
            b = _apply_q_pr(vL, tauL, bb, transpose=True)
            dp1 = _trsv_pr(pr_get(RL, (slice(0, r), slice(0, r))), pr_get(b, slice(0, r)), lower=False)
            full = pr_zeros(kA)
            pr_set(full, pL[:r], dp1)
            p1 = pr_get(full, slice(0, r))
        if r == n:
            self.p = pr_float(p1)
            return
        # J Q = (Q' J')' and E = Q' Gamma Q = (Q' (Q' Gamma)')': the reflectors applied, Q never formed (kA = 0: plain copies)
        JQ = pr_T(_apply_q_pr(vA, tauA, pr(np.asarray(J).T), transpose=True))
        E = pr_T(_apply_q_pr(vA, tauA, pr_T(_apply_q_pr(vA, tauA, pr(Gam), transpose=True)), transpose=True))
        if t > r:
            vp = ref.F_L11.p - 1
            E = pr_get(E, np.ix_(vp, vp))
        J1, J2 = pr_get(JQ, (slice(None), slice(0, r))), pr_get(JQ, (slice(None), slice(r, None)))
        W22 = pr_add(pr_get(E, (slice(r, None), slice(r, None))), pr_gram(J2, J2))
        W21 = pr_add(pr_get(E, (slice(r, None), slice(0, r))), pr_gram(J2, J1))
        d = pr_neg(pr_add(pr_matvec(W21, p1), pr_matvec(pr_T(J2), pr(rx))))
        sW = pr_add(W22, pr_T(W22))
        sW = (sW[0] / 2, sW[1] / 2)
        self.sW = pr_float(sW)
        if np.all(np.isfinite(self.sW)):
            ev = np.linalg.eigvalsh(self.sW)
            self.lam_min, self.norm = float(ev[0]), float(np.abs(ev).max())
        else:
            self.lam_min, self.norm = float("nan"), float("nan")
        self.fail_index, L = _cholesky_pr(sW)
        if self.fail_index >= 0:
            self.error = True
            self.p = np.zeros(n)
            return
        self.cond = float(ev[-1] / ev[0])
        p2 = _trsv_pr(pr_T(L), _trsv_pr(L, d, lower=True), lower=False)
        both = (np.concatenate([p1[0], p2[0]]), np.concatenate([p1[1], p2[1]]))
        self.p = pr_float(_apply_q_pr(vA, tauA, both))


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


def make_wide_rankdef_A(seed, m, n, t, defect=2):
    """t >= n constraints of rank n - defect: the rank-deficient working set the reference's E[F_L11.p, F_L11.p] branch is defined
    for"""
    J, rx, _, _ = synth.make_problem(seed, m, n, 1)
    B = synth.normal_stream(seed, 7, t * (n - defect)).reshape(t, n - defect)
    C = synth.normal_stream(seed, 8, (n - defect) * n).reshape(n - defect, n)
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
