"""Cases of the finite-difference Hessian sums (src/enlsip_functions.jl:243-328) shared by tests/test_hessian_sums_host.py and
tests/test_gpu_hessian_sums_batched.py: the special entries of x, a restatement in Python of the documented summation order and of
the per-pair arithmetic (the product is compared with it byte for byte), callbacks that record the points the reference's loops
hand out and replay stored evaluations to them, and random data of one problem.

The sums are contractions of whatever the evaluations hold, so the random problems draw F and G directly; only the end-to-end
problems of tests/direction_cases.py evaluate real functions."""
import math
from fractions import Fraction

import numpy as np

from oracle import enlsip_outer as eo

U = 2.0 ** -53
EPS1 = eo.EPS ** (1.0 / 3.0)


def step(xk):
    return max(abs(xk), 1.0) * EPS1


def find_roundtrip(start=0.3, n_try=200):
    """the first x of the walk start, start / 2, start / 4, ... with (x - eps) + eps != x: the diagonal's f2 is not x there.
    Inside one binade of x the two roundings cancel (x - eps is x - eps + d with |d| <= ulp(x) / 2, and x + d rounds back to x
    except on a double tie), so the walk goes down: once ulp(x) is below the rounding error of x - eps, about 2^-70, the way
    back misses x."""
    x = start
    for _ in range(n_try):
        e = step(x)
        if (x - e) + e != x:
            return x
        x = x / 2
    raise AssertionError("no x with (x - eps) + eps != x on the walk")


# found by find_roundtrip() on the CPU and kept: tests/test_hessian_sums_host.py asserts the property and that the walk still
# finds this value
X_ROUNDTRIP = float.fromhex("0x1.3333333333333p-20")      # 0.3 / 2^18 = 1.1444091796875e-06

# 0.0, -0.0, below and above 1 in magnitude, negative, 2^60 (a step of 2^60 eps1: the step is relative, x +- eps != x at every
# magnitude), and the round-trip value
X_SPECIAL = (0.0, -0.0, 0.3, -0.75, 5.5, -12.25, 2.0 ** 60, X_ROUNDTRIP)


def special_x(n, shift=0):
    return np.array([X_SPECIAL[(i + shift) % len(X_SPECIAL)] for i in range(n)])


def pairs(n):
    return [(k, j) for k in range(n) for j in range(k + 1)]


def ordered(terms):
    """the documented order: partial s adds the terms s, s + 64, ... ascending from +0.0, then the butterfly"""
    x = np.zeros(64)
    for j, v in enumerate(terms):
        x[j & 63] = x[j & 63] + v
    for mk in (1, 2, 7, 15, 16, 32):
        y = x.copy()
        for s in range(64):
            y[s] = x[s] + x[s ^ mk] if s < (s ^ mk) else x[s ^ mk] + x[s]
        x = y
    return float(x[0])


def terms(rows, w, idx=None):
    """(((f1 - f2) - f3) + f4) * w per entry, every operation rounded on its own; rows: (4, width); idx: 0-based rows to gather,
    -1 for a padding entry (term 0.0)"""
    f1, f2, f3, f4 = (np.asarray(r, dtype=np.float64) for r in rows)
    with np.errstate(invalid="ignore", over="ignore"):
        if idx is None:
            return (((f1 - f2) - f3) + f4) * w
        out = np.zeros(len(idx))
        for i, a in enumerate(idx):
            if a >= 0:
                out[i] = (((f1[a] - f2[a]) - f3[a]) + f4[a]) * w[i]
        return out


def restated(x, F, rx, G, lam, active, t, pair0=0):
    """per pair of the range: dict(k, j, u, v, s_r, s_c, r, c, gamma, div_r, div_c) by the documented arithmetic"""
    n = len(x)
    out = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for q in range(F.shape[0]):
            k, j = pairs(n)[pair0 + q]
            ek, ej = np.float64(step(x[k])), np.float64(step(x[j]))
            u = terms(F[q], rx)
            s_r = ordered(u)
            div_r = (4 * ej) * ek
            r = np.float64(s_r) / div_r
            v = np.zeros(0)
            s_c, c, div_c = 0.0, np.float64(0.0), (4.0 * ek) * ej
            if t > 0:
                v = terms(G[q], lam, [int(a) - 1 for a in active[:t]])
                s_c = ordered(v)
                c = np.float64(s_c) / div_c
            out.append(dict(k=k, j=j, u=u, v=v, s_r=s_r, s_c=s_c, r=float(r), c=float(c), gamma=float(r - c), div_r=float(div_r),
                            div_c=float(div_c)))
    return out


def restated_gamma(x, F, rx, G, lam, active, t, pair0=0, Gamma=None):
    n = len(x)
    Gamma = np.zeros((n, n)) if Gamma is None else Gamma
    for e in restated(x, F, rx, G, lam, active, t, pair0):
        Gamma[e["k"], e["j"]] = Gamma[e["j"], e["k"]] = e["gamma"]
    return Gamma


def entry_bound(e, m, t):
    """the issue's per-entry tolerance between two summation orders of the same rounded terms"""
    su, sv = float(np.abs(e["u"]).sum()), float(np.abs(e["v"]).sum())
    return 2 * m * U * su / e["div_r"] + 2 * t * U * sv / e["div_c"] + 4 * U * (abs(e["r"]) + abs(e["c"]))


def exact(values):
    return sum((Fraction(float(v)) for v in values), Fraction(0))


class Recorder:
    """an evaluation callback for the reference's loops: records every point it is handed and answers with the stored rows
    (``rows``: (calls, width)) in call order, or with zeros"""

    def __init__(self, width, rows=None):
        self.width, self.rows, self.points = width, rows, []

    def __call__(self, x):
        i = len(self.points)
        self.points.append(np.array(x, dtype=np.float64, copy=True))
        return np.zeros(self.width) if self.rows is None else self.rows[i]

    def fn(self):
        return eo.EvalFunction(self, None)


def reference_points(x):
    """(pairs, 4, n): what hessian_res hands to its callback, in call order"""
    n = len(x)
    rec = Recorder(1)
    eo.hessian_res(rec.fn(), np.array(x, dtype=np.float64), np.zeros(1), n, 1)
    return np.array(rec.points).reshape(len(pairs(n)), 4, n)


def reference_gamma(x, F, rx, G, lam, active, t):
    """hessian_res - hessian_cons of the reference on the stored evaluations of ALL pairs (F: (pairs, 4, m), G: (pairs, 4, l))"""
    n, m, l = len(x), F.shape[2], G.shape[2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r_mat = eo.hessian_res(Recorder(m, F.reshape(F.shape[0] * 4, m)).fn(), np.array(x), rx, n, m)
        c_mat = eo.hessian_cons(Recorder(l, G.reshape(G.shape[0] * 4, l)).fn(), np.array(x), lam, active, n, l, t)
        return r_mat - c_mat


def random_problem(rng, m, n, l, t, npairs=None, x=None, pad=True):
    """x, rx, lam, a shuffled active list with a padding 0 inside its used part (when t > 1 and pad), and evaluations of npairs
    pairs whose second differences are of mixed magnitude"""
    npairs = n * (n + 1) // 2 if npairs is None else npairs
    x = special_x(n, int(rng.integers(0, 8))) if x is None else np.asarray(x, dtype=np.float64)
    base = rng.standard_normal((npairs, 1, m))
    F = base + 1e-4 * rng.standard_normal((npairs, 4, m)) * 10.0 ** rng.integers(-3, 2, size=(npairs, 1, m))
    gbase = rng.standard_normal((npairs, 1, l))
    G = gbase + 1e-4 * rng.standard_normal((npairs, 4, l))
    rx = rng.standard_normal(m) * 10.0 ** rng.integers(-2, 2, size=m)
    lam = rng.standard_normal(t) * 10.0 ** rng.integers(-3, 2, size=t)
    active = np.zeros(l, dtype=np.int64)
    active[:t] = (rng.permutation(l) + 1)[:t]
    if pad and t > 1:
        active[int(rng.integers(0, t))] = 0
    return dict(x=x, F=np.ascontiguousarray(F), rx=rx, G=np.ascontiguousarray(G), lam=lam, active=active, t=t, m=m, n=n, l=l)
