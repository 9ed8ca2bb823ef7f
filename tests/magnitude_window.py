"""Inputs for the magnitude contract between the band edge and the overflow of the largest column norm (entries of about 2^400 to
2^511), and at the small-magnitude threshold 2^-440 — built from oracle/synth.py, shared by the CPU and the GPU part of
tests/test_magnitude_window.py.  Every construction returns the scaled problem AND the ordinary problem it is an exact
power-of-two multiple of, so that a test can compare the two.  Norms of the scaled data are taken in exponent-shifted arithmetic
(log2_sumsq): a plain sum of squares of such data overflows in NumPy as it does in a kernel."""
from functools import lru_cache

import numpy as np

from oracle import gn_oracle as go, synth

SEED = 7
SHAPES = [(300, 40, 6), (700, 130, 20), (300, 200, 90)]      # one-wave forms, workgroup forms, distributed constraint stage (t > 64)
EXPONENTS = (495, 505, 511)
TINY_LOG2 = -440                                              # the small-magnitude nomination threshold (gn_rescale.hpp)


def log2_sumsq(x, axis=None):
    """log2 of sum(x^2) over `axis`, for data whose squares leave the exponent range: the data are shifted to magnitude 1 first"""
    x = np.asarray(x, dtype=np.float64)
    amax = np.abs(x).max()
    if not amax > 0:
        return -np.inf if axis is None else np.full(np.delete(x.shape, axis), -np.inf)
    e = int(np.frexp(amax)[1])
    s = np.ldexp(x, -e)
    with np.errstate(divide="ignore"):
        return np.log2((s * s).sum(axis=axis)) + 2.0 * e


def scaled(prob, eJ, eA):
    J, rx, A, cx = prob
    return np.ldexp(J, eJ), np.ldexp(rx, eJ), np.ldexp(A, eA), np.ldexp(cx, eA)


@lru_cache(maxsize=None)
def base_problem(m, n, t):
    return synth.make_problem(SEED, m, n, t)


def window_random(m, n, t, eJ, eA):
    """(scaled problem, ordinary problem): make_problem with J, rx times 2^eJ and A, cx times 2^eA"""
    base = base_problem(m, n, t)
    return scaled(base, eJ, eA), base


def first_diagonal_overflows(m, n, t, eJ, eA):
    """True when the largest column norm squared of the scaled J or A' is not finite.  dgeqp3 takes the column of largest norm
    first and a reflector keeps the norm, so this is R[0]^2 of F_A; J2 = (J Q1)[:, rankA:] has columns no longer than
    ||J||_F, and a J whose LARGEST column overflows has (for these random inputs, t << n) an overflowing largest J2 column too.
    Such a problem is nominated by the not-finite test that the cases at 2^+-600 cover."""
    J, rx, A, cx = base_problem(m, n, t)
    return bool((eJ and log2_sumsq(J, axis=0).max() + 2 * eJ >= 1024) or (eA and log2_sumsq(A, axis=1).max() + 2 * eA >= 1024))


def random_window_cases(m, n, t):
    """(eJ, eA) of the random cases: every exponent on J only, on A only and on both, without those whose R[0] itself overflows"""
    cases = []
    for e in EXPONENTS:
        for eJ, eA in ((e, 0), (0, e), (e, e)):
            if not first_diagonal_overflows(m, n, t, eJ, eA):
                cases.append((eJ, eA))
    return cases


def window_rx_dominant(m, n, t, eJ=505):
    """rx carries 2^4 more than J: ||rx||^2 is above 2^1024 while every column norm squared of J is finite.  A, cx ordinary."""
    J, rx, A, cx = base_problem(m, n, t)
    base = (J, np.ldexp(rx, 4), A, cx)
    return scaled(base, eJ, 0), base, eJ


def near_parallel_rows(m, n, t, top=1024):
    """Constraint rows a_j = u + 0.05 noise_j / sqrt(n) (u: the first row of make_problem's A, normalised), times the power of two
    that puts the largest row norm squared — R_A[0,0]^2 — into [2^(top-2), 2^top).  The rows of R_A then have norms up to
    sqrt(t) |R_A[0,0]|: with top = 1024 the first one's square is beyond the exponent range while R_A[0,0]^2 is finite.
    Returns (scaled problem, ordinary problem, e); J, rx are ordinary."""
    J, rx, A, cx = base_problem(m, n, t)
    u = A[0] / np.linalg.norm(A[0])
    A2 = u[None, :] + 0.05 * A / np.sqrt(n)
    l2 = log2_sumsq(A2, axis=1).max()                       # log2 of the largest row norm squared, ordinary magnitude
    e = int(np.floor((top - l2) / 2.0))                     # largest e with l2 + 2e <= top
    if l2 + 2 * e >= top:
        e -= 1
    base = (J, rx, A2, cx)
    return scaled(base, 0, e), base, e


@lru_cache(maxsize=None)
def _graded_base(m, n, t):
    prob = synth.make_graded_J(SEED, m, n, t, log10_cond=6.0)
    return prob, go.gn_subproblem(*prob)


def lower_edge_graded(m, n, t, side):
    """Graded J (log10_cond 6), J and rx times the power of two that puts the largest column norm of J2 — |F_J2.R[0,0]| — into
    [2^-440, 2^-439) (side "above": not nominated) or into [2^-441, 2^-440) (side "below": nominated; its entries are far
    outside the band, so it is rescaled).  Returns (scaled problem, ordinary problem, e)."""
    prob, ref = _graded_base(m, n, t)
    r00 = abs(ref.F_J2.R[0, 0])
    e = TINY_LOG2 - int(np.floor(np.log2(r00))) - (0 if side == "above" else 1)
    return scaled(prob, e, 0), prob, e


def extended_precision_p(J, rx, A, cx, dps=40, sweeps=6):
    """The minimiser of ||J p + rx|| subject to A p + cx = 0 (A of full row rank, J of full rank on its null space) to about
    `dps` digits: the KKT system [J'J A'; A 0] [p; lam] = [-J'rx; -cx], solved by iterative refinement whose residuals are
    evaluated in mpmath from the exact binary inputs and whose corrections come from the FP64 factorisation of the system.
    Each sweep gains 16 - log10(cond) digits; the last correction (returned, relative to p) shows where it stopped."""
    import mpmath as mp
    from scipy.linalg import lu_factor, lu_solve
    m, n = J.shape
    t = A.shape[0]
    K = np.block([[J.T @ J, A.T], [A, np.zeros((t, t))]])
    lu = lu_factor(K)
    with mp.workdps(dps):
        toM = lambda M: np.array([[mp.mpf(float(x)) for x in row] for row in np.atleast_2d(M)], dtype=object)
        tov = lambda v: np.array([mp.mpf(float(x)) for x in v], dtype=object)
        Jm, Am, rxm, cxm = toM(J), toM(A), tov(rx), tov(cx)
        x = tov(lu_solve(lu, np.concatenate([-J.T @ rx, -cx])))
        last = None
        for _ in range(sweeps):
            p, lam = x[:n], x[n:]
            r = np.concatenate([Jm.T @ (Jm @ p + rxm) + Am.T @ lam, Am @ p + cxm])
            dx = lu_solve(lu, -np.array([float(v) for v in r]))
            x = x + tov(dx)
            last = float(np.linalg.norm(dx[:n]) / np.linalg.norm(np.array([float(v) for v in x[:n]])))
            if last < 1e-25:
                break
        return np.array([float(v) for v in x[:n]]), last
