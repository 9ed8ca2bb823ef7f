"""Cases of the line-search set-up shared by tests/test_steplength_bound_host.py and tests/test_gpu_linesearch_setup_batched.py:
upper_bound_steplength (src/enlsip_functions.jl:2149-2178) on an Ap that is given, the oracle's answer on the same Ap, random
batches for the device call and named edges whose Ap is exact in any summation order (small integers)."""
import math
from types import SimpleNamespace

import numpy as np

from oracle import enlsip_outer as eo

U = np.finfo(np.float64).eps / 2
GAP = 1e-9          # the input conditions of the device cases: see gap_report


def oracle_bound(Ap, cx, inactive, n_inactive, index_del):
    """oracle/enlsip_outer.py::upper_bound_steplength on a given Ap: the oracle forms dot(A[j, :], p) itself, so it is handed the
    one-column matrix A = Ap and p = [1.0], whose row products are Ap[j] * 1.0, i.e. Ap[j] exactly."""
    Ap = np.asarray(Ap, dtype=np.float64)
    l = Ap.size
    W = SimpleNamespace(inactive=np.asarray(inactive, dtype=np.int64), t=l - int(n_inactive), l=l)
    with np.errstate(all="ignore"):
        a, idx = eo.upper_bound_steplength(Ap.reshape(l, 1), np.asarray(cx, dtype=np.float64), np.array([1.0]), W, int(index_del))
    return float(a), int(idx)


def random_case(rng, n=None, l=None, tie=False):
    """One problem: A (l x n), p, cx, inactive (l, zero padded, ascending as remove_constraint keeps it), n_inactive, index_del.
    cx has both signs and a scale that puts alpha on both sides of 3.  tie: two rows of the list with bitwise equal cx and A."""
    n = int(rng.integers(1, 12)) if n is None else n
    l = int(rng.integers(1, 40)) if l is None else l
    A = rng.standard_normal((l, n))
    p = rng.standard_normal(n)
    cx = rng.standard_normal(l) * (10.0 ** rng.uniform(-1.5, 1.5))
    ni = int(rng.integers(0, l + 1))
    rows = np.sort(rng.choice(np.arange(1, l + 1), size=ni, replace=False))
    inactive = np.zeros(l, dtype=np.int64)
    inactive[:ni] = rows
    if tie and ni >= 2:
        a, b = rng.choice(ni, size=2, replace=False)
        A[rows[b] - 1] = A[rows[a] - 1]
        cx[rows[b] - 1] = cx[rows[a] - 1]
    index_del = int(rows[rng.integers(ni)]) if ni and rng.random() < 0.3 else 0
    return dict(A=A, p=p, cx=cx, inactive=inactive, n_inactive=ni, index_del=index_del, tie=bool(tie and ni >= 2))


def random_batch(seed, B, n, l, m, n_inactive=None):
    """A batch for the device call: arrays with a leading batch axis; Jp and rx (B, m) for the sums.  No ties."""
    rng = np.random.default_rng(seed)
    cs = [random_case(rng, n, l) for _ in range(B)]
    if n_inactive is not None:      # a list of a fixed length, in a permuted order
        for c in cs:
            c["inactive"][:] = 0
            c["inactive"][:n_inactive] = rng.permutation(l)[:n_inactive] + 1
            c["n_inactive"] = n_inactive
            c["index_del"] = int(c["inactive"][rng.integers(n_inactive)]) if rng.random() < 0.3 else 0
    out = {k: np.stack([np.asarray(c[k]) for c in cs]) for k in ("A", "p", "cx", "inactive")}
    out["n_inactive"] = np.array([c["n_inactive"] for c in cs], dtype=np.int64)
    out["index_del"] = np.array([c["index_del"] for c in cs], dtype=np.int64)
    out["Jp"] = rng.standard_normal((B, m)) * 10.0 ** rng.uniform(-2, 2, (B, 1))
    out["rx"] = rng.standard_normal((B, m)) * 10.0 ** rng.uniform(-2, 2, (B, 1))
    return out


def gap_report(A, p, cx, inactive, n_inactive, index_del):
    """(gap, margin, cond) of one problem, from float64 products alone.  gap: relative distance of the two smallest qualifying
    alpha_j (inf with fewer than two).  margin: min over the looked-at rows with cx_j > 0 of |Ap_j| / sum_c |a_jc| |p_c| (inf
    without one).  With gap > GAP and margin > GAP neither the sign of an Ap_j nor the order of two alpha_j can depend on how a dot
    product of up to 1024 terms was summed (its error is below 2 n u sum |a||p| < 3e-13 sum |a||p|).  cond: sum |a||p| / |Ap| of
    the winning row when its alpha is below the cap (0 otherwise): two evaluations of that dot product, each within n u sum |a||p|
    to first order, give alpha_upp values that differ by at most 4 n u cond relative, which the device test holds to 1e-12."""
    Ap = A @ p
    mag = np.abs(A) @ np.abs(p)
    alphas, margin = [], math.inf
    for i in range(int(n_inactive)):
        j = int(inactive[i])
        if j == 0 or j == index_del or not cx[j - 1] > 0:
            continue
        margin = min(margin, abs(Ap[j - 1]) / mag[j - 1]) if mag[j - 1] > 0 else 0.0
        if Ap[j - 1] < 0:
            alphas.append((-cx[j - 1] / Ap[j - 1], j))
    alphas.sort()
    gap = (alphas[1][0] - alphas[0][0]) / alphas[1][0] if len(alphas) >= 2 else math.inf
    cond = mag[alphas[0][1] - 1] / abs(Ap[alphas[0][1] - 1]) if alphas and alphas[0][0] < 3.0 else 0.0
    return gap, margin, cond


# the device test's random batches: (name, seed, B, n, l, m, n_inactive or None).  The seeds are those whose batches meet the input
# conditions of gap_report (tests/test_steplength_bound_host.py checks them): (63, 63) and gen_l257 needed another one.
GPU_SHAPES = (
    [(f"wave_n{n}_l{l}", 100 + 7 * n + l + (1000 if (n, l) == (63, 63) else 0), 5, n, l, 33, None)
     for n in (1, 2, 63, 64) for l in (1, 2, 63, 64)]
    + [("outside_n65_l64", 201, 5, 65, 64, 7, None), ("outside_n64_l65", 202, 5, 64, 65, 7, None),
       ("gen_l255", 203, 5, 130, 255, 255, None), ("gen_l256", 204, 5, 1, 256, 256, None), ("gen_l257", 1205, 5, 130, 257, 257, None),
       ("gen_l600_list590", 206, 5, 130, 600, 5000, 590), ("gen_n1_l600", 207, 1, 1, 600, 1, 590),
       ("wave_m1", 208, 1, 2, 3, 1, None), ("wave_m255", 209, 5, 2, 3, 255, None), ("wave_m256", 210, 5, 2, 3, 256, None),
       ("wave_m257", 211, 5, 2, 3, 257, None), ("wave_m5000", 212, 5, 2, 3, 5000, None), ("gen_m1", 213, 5, 65, 3, 1, None)])


def gpu_batches():
    return {name: random_batch(seed, B, n, l, m, ni) for name, seed, B, n, l, m, ni in GPU_SHAPES}


# ---- named edges on a given (cx, Ap) ---------------------------------------------------------------------------------------------
def edge_cases(l=8):
    """(name, cx, Ap, inactive, n_inactive, index_del, want) with l >= 8; want = (alpha_upp, index) where the issue states it, else
    None (the oracle decides).  Every finite value is a small integer or a power of two, so a device product that realises Ap is
    exact.  Rows are 1-based; the rows past 8 never qualify (cx = -1)."""
    nan, inf = np.nan, np.inf
    full = lambda: np.arange(1, l + 1)

    def mk(name, cx8, Ap8, inactive=None, n_inactive=None, index_del=0, want=None):
        cx, Ap = np.full(l, -1.0), np.full(l, -1.0)
        cx[:8], Ap[:8] = cx8, Ap8
        lst = np.zeros(l, dtype=np.int64)
        src = full() if inactive is None else np.asarray(inactive, dtype=np.int64)
        lst[:src.size] = src
        return (name, cx, Ap, lst, src.size if n_inactive is None else n_inactive, index_del, want)

    base_cx = [1.0, 1.0, 4.0, -1.0, 2.0, 1.0, 0.0, 1.0]
    base_Ap = [-1.0, -2.0, -2.0, -1.0, -4.0, 1.0, -1.0, -1.0]      # alpha: 1, .5, 2, -, .5, -, -, 1: rows 2 and 5 tie at 0.5
    perm = np.concatenate([[5, 8, 2, 1, 3, 4, 6, 7], np.arange(9, l + 1)]).astype(np.int64)
    far = np.concatenate([np.arange(9, l + 1), [5, 2, 1, 3, 4, 6, 7, 8]]).astype(np.int64)     # the tie at the list's far end
    return [
        mk("n_inactive_0", base_cx, base_Ap, n_inactive=0, want=(3.0, 0)),
        mk("all_zero_list", base_cx, base_Ap, inactive=np.zeros(l, dtype=np.int64), want=(3.0, 0)),
        mk("zero_inside_list", base_cx, base_Ap, inactive=[1, 0, 2, 0, 3], want=(0.5, 2)),
        mk("tie_ascending_first_wins", base_cx, base_Ap, want=(0.5, 2)),
        mk("tie_permuted_first_wins", base_cx, base_Ap, inactive=perm, want=(0.5, 5)),
        mk("tie_far_end_first_wins", base_cx, base_Ap, inactive=far, want=(0.5, 5)),
        mk("index_del_on_winner", base_cx, base_Ap, index_del=2, want=(0.5, 5)),
        mk("index_del_on_both", [1.0, 1.0, 4.0, -1.0, -2.0, 1.0, 0.0, 1.0], base_Ap, index_del=2, want=(1.0, 1)),
        mk("cx_zero_and_negative", [0.0, -1.0, -0.0, -2.0, 0.0, -1.0, 0.0, -4.0], [-1.0] * 8, want=(3.0, 0)),
        mk("Ap_zero_and_positive", [1.0] * 8, [0.0, -0.0, 1.0, 2.0, 0.0, -0.0, 4.0, 0.0], want=(3.0, 0)),
        mk("all_alpha_above_3", [8.0, 4.0, 16.0, 8.0, 32.0, 8.0, 8.0, 8.0], [-1.0, -1.0, -2.0, -2.0, -2.0, -1.0, -1.0, -2.0],
           want=(3.0, 2)),
        mk("alpha_exactly_3", [3.0, 6.0, 8.0, 8.0, 8.0, 8.0, 8.0, 8.0], [-1.0, -2.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0], want=(3.0, 1)),
        mk("nan_in_cx", [nan, 1.0, nan, 1.0, 1.0, 1.0, 1.0, 1.0], [-8.0, -1.0, -8.0, -2.0, -1.0, -1.0, -1.0, -1.0], want=(0.5, 4)),
        mk("nan_in_Ap", [1.0] * 8, [nan, -1.0, nan, -4.0, -1.0, nan, -1.0, -1.0], want=(0.25, 4)),
        mk("all_nan", [nan] * 8, [nan] * 8, want=(3.0, 0)),
        mk("inf_in_cx", [inf, 1.0, -inf, 1.0, 1.0, 1.0, 1.0, 1.0], [-1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0], want=(1.0, 2)),
        mk("inf_cx_alone", [inf, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0], [-1.0] * 8, want=(3.0, 0)),
        mk("inf_in_Ap", [1.0] * 8, [-inf, inf, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0], want=(0.0, 1)),
        mk("inf_over_inf", [inf, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], [-inf, -2.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0], want=(0.5, 2)),
    ]


def realise(Ap, n, rng):
    """(A, p) with A @ p == Ap exactly in any summation order and in FMA or plain arithmetic: p = (1, 1, -1, 0, ...)[:n], the other
    columns small integers, and a row whose Ap is not finite carries it alone in column 0."""
    l = Ap.size
    p = np.zeros(n)
    p[:3] = [1.0, 1.0, -1.0][:min(n, 3)]
    A = rng.integers(-4, 5, size=(l, n)).astype(np.float64)
    fin = np.isfinite(Ap)
    A[~fin, :] = 0.0
    rest = A[:, 1:] @ p[1:] if n > 1 else np.zeros(l)
    A[:, 0] = np.where(fin, np.where(fin, Ap, 0.0) - rest, Ap)
    return A, p
