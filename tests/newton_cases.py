"""Cases for the batched Newton direction at the cuts of its own kernels (test infrastructure, CPU only: NumPy, mpmath, the oracle).

gn_kernels_newton_batched.hpp cuts the work by the Cholesky order n2 = n - rankA (panels of 32, 16 x 16 MFMA tiles), by
kp = min(m, n2) (the depth of R'R, clipped per tile row) and by kA (the reflector loops start at (k & ~63) + lane).  The table below
puts n2, kp and kA on those cuts, and designed Hessians put dpotrf's verdict on chosen pivots.

Designed sW22.  With Q1 = F_A.Q and J2 = (J Q1)[:, rankA:] of the oracle,

    Gamma = Q1 (blockdiag(0, T - J2'J2) + 0.03 M) Q1',   M = Q1' N Q1 with its [rankA:, rankA:] block zeroed, N Gaussian

so that the oracle's sW22 is T up to rounding of size u ||J2||^2 (with t >= n > rankA the block sits on the rows and columns
F_L11.p[rankA:], where the reference reads it).  J and rx are first scaled by a power of two so that ||J2||_2^2 <= 2 ||T||_2:
otherwise the cancellation E22 + J2'J2 costs a factor ||J2||^2 / ||T||.  The library scatters sW22 back through jpvtJ before it
factors it, so a designed pivot index is the index the kernel sees.

T = L D L', L unit lower triangular with Gaussian entries 0.2 / sqrt(n2) below the diagonal:
  fail(k)        D = 1 except D[k] = -0.05: every pivot before k is 1, pivot k is -0.05
  graded(c, 0|1) D = logspace(0, -log10 c), in order or permuted
and beside them
  plain          newton_reference.make_gammas
  graded_J       synth.make_graded_J(log10_cond = GRADED_J_DECADES) with Gamma = GRADED_J_DELTA I: the ill-conditioning comes through R'R
  nan(i, j)      a plain Gamma with Gamma[i, j] = NaN, t = 0 (E = Gamma), i > j: pivot i of sW22 is the first NaN one

tests/test_newton_cases_host.py certifies every premise on the CPU before tests/test_gpu_newton_edges.py uses the cases.

The bound: rel(p, p_ref) <= C_EDGE u kappa, kappa = (||J2||_2^2 + ||sym E22||_2) / lambda_min(sW22), which is cond(sW22) up to
a factor 2 where nothing cancels and, unlike it, sees a cancellation between E22 and J2'J2."""
from __future__ import annotations

import functools

import numpy as np

import newton_reference as nr
from oracle import gn_oracle as go, synth

U = nr.U
GRADED_J_DECADES = 4.0
GRADED_J_DELTA = 1e-9
PERM_SCALE = 0.01            # scale of Gamma on the wide rank-deficient working sets: ||sym Gamma|| <= lambda_min(J2'J2) / 4 (certified)
NB, TILE = 32, 16            # the cuts of k_newton_chol_batched (NWB_NB) and of its MFMA tiles

# rel(p, p_ref) <= C_EDGE u kappa.  Measured by tests/test_newton_cases_host.py::test_constant over every positive-definite member
# of CASES: the FP64 restatement of the reference's lines (tests/test_gpu_parity.py::_newton_reference) against the
# high-precision reference has its worst error at WORST_MULTIPLE u kappa on WORST_CASE.  Times 8, the project's margin for another
# summation order, this stays below newton_reference.C_NEWTON = 118: the old constant covers the new cases under kappa and is kept.
# (kappa does not see cond(A): a nearly square working set such as 88 x 90 puts the error of p1 at 154 u kappa with kappa ~ 1,
# and the kA >= 65 shapes of the table stay away from it.)
WORST_MULTIPLE = 4.801
WORST_CASE = "edge-n96-t84[0]"
C_EDGE = nr.C_NEWTON
MAX_BOUND = 1e-4              # a compared member has C_EDGE u kappa <= MAX_BOUND: beyond it a case checks nothing

# seeds that missed a margin of the host test and were advanced: {(case id, member): seeds skipped}
ADVANCED_SEEDS: dict = {}


def bound(kappa):
    return C_EDGE * U * max(kappa, 1.0)


# ---- kinds ------------------------------------------------------------------------------------------------------------------------
def _t_matrix(seed, n2, kind):
    """T = L D L' of a designed kind"""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.standard_normal((n2, n2)) * (0.2 / np.sqrt(n2)), -1) + np.eye(n2)
    if kind[0] == "fail":
        D = np.ones(n2)
        D[kind[1]] = -0.05
    else:
        D = np.logspace(0.0, -np.log10(kind[1]), n2)
        if kind[2]:
            D = D[rng.permutation(n2)]
    return (L * D) @ L.T


def _q1(n, t, ref):
    return ref.F_A.Q_mul(np.eye(n)) if t else np.eye(n)


def designed(seed, prob, kind):
    """((J, rx, A, cx) with J and rx scaled, its oracle result, Gamma) for a `fail` or `graded` kind"""
    J, rx, A, cx = prob
    n = J.shape[1]
    t = A.shape[0] if A.size else 0
    ref = go.gn_subproblem(J, rx, A, cx)
    r = ref.rankA
    assert r < n and (t == r or t >= n), "designed kinds need a defined Newton step with n2 > 0"
    Q1 = _q1(n, t, ref)
    T = _t_matrix(seed, n - r, kind)
    ratio = 2.0 * np.linalg.norm(T, 2) / np.linalg.norm((J @ Q1)[:, r:], 2) ** 2
    s = 2.0 ** min(0, int(np.floor(0.5 * np.log2(ratio))))
    J, rx = J * s, rx * s
    ref = go.gn_subproblem(J, rx, A, cx)
    assert ref.rankA == r
    Q1 = _q1(n, t, ref)
    J2 = (J @ Q1)[:, r:]
    idx = (ref.F_L11.p - 1)[r:] if t > r else np.arange(r, n)
    M = Q1.T @ np.random.default_rng(seed + 1).standard_normal((n, n)) @ Q1
    M[np.ix_(idx, idx)] = 0.0
    E = 0.03 * M
    E[np.ix_(idx, idx)] = T - J2.T @ J2
    return (J, rx, A, cx), ref, Q1 @ E @ Q1.T


# ---- the table ---------------------------------------------------------------------------------------------------------------------
PLAIN, G6 = ("plain",), ("graded", 1e6, 0)
# the upper grading is 1e9, not 1e10: graded(1e10) has kappa = 1.6e10 on (33, 0), and C_EDGE u kappa <= MAX_BOUND admits
# kappa <= 7.6e9, so 1e9 (kappa = 4.2e9) is the largest power of ten the constant allows
GRADES = [("graded", 1e6, 0), ("graded", 1e6, 1), ("graded", 1e9, 0), ("graded", 1e9, 1)]


def _mem(t, kind=PLAIN, maker="plain", defect=0, take=1):
    return dict(t=t, kind=kind, maker=maker, defect=defect, take=take)


def _case(cid, n, members, m=None, ranges=None, note=""):
    B = len(members)
    return dict(id=cid, n=n, m=n + 8 if m is None else m, members=members, form=nr.expected_newton_form(n),
                ranges=ranges or [(0, B), (1, B - 2 if B > 3 else B - 1)], note=note)


# kA >= 65 with n t > 8192 goes through the distributed constraint stage, after which the batched Newton direction is refused
# (return code -7, gn_newton_batched.inc); the GPU test holds the library to that on these shapes
REFUSED_SHAPES = [(140, 70), (134, 130), (200, 129)]


def _fail_indices(n2):
    return [k for k in (0, 15, 16, 31, 32, 33, 63, 64, 65) if k < n2 - 1] + [n2 - 1]


@functools.lru_cache(maxsize=None)
def _cases() -> tuple:
    out = []
    # tile and panel edges, nv = 1 / odd n, kA >= 65: two plain members around a graded one
    shapes = [(15, 0), (16, 0), (17, 0), (21, 5), (22, 5),                                        # tiles, wave form
              (31, 0), (32, 0), (33, 0), (38, 5), (47, 0), (48, 0), (49, 0), (63, 0), (64, 0), (64, 16),     # panels, wave form
              (65, 0), (70, 5), (101, 5), (102, 5), (133, 5), (134, 5),                           # panels, general form
              (73, 9),                                                                            # odd n, last workgroup of one vector
              (100, 70), (120, 68), (96, 84)]          # kA >= 65: reflector loops start past 0 (n t <= 8192: see REFUSED_SHAPES)
    for n, t in shapes:
        out.append(_case(f"edge-n{n}-t{t}", n, [_mem(t), _mem(t, G6), _mem(t)]))
    # sW22 ill-conditioned by design
    for n, t in [(33, 0), (64, 0), (70, 5), (134, 5)]:
        out.append(_case(f"graded-n{n}-t{t}", n, [_mem(t, g) for g in GRADES] + [_mem(t)]))
    for n, t in [(38, 5), (102, 5)]:
        out.append(_case(f"gradedJ-n{n}-t{t}", n, [_mem(t, ("graded_J",), "graded_J"), _mem(t), _mem(t, ("graded_J",), "graded_J")]))
    # dpotrf's verdict on a designed pivot, one failing member between positive-definite ones
    for n, t in [(64, 0), (65, 0), (134, 5)]:
        ks = _fail_indices(n - t)
        for i in range(0, len(ks), 2):
            pair = ks[i:i + 2]
            mem = [_mem(t)]
            for k in pair:
                mem += [_mem(t, ("fail", k)), _mem(t, G6 if k == pair[0] else PLAIN)]
            out.append(_case(f"fail-n{n}-t{t}-k" + "_".join(map(str, pair)), n, mem, ranges=[(0, len(mem)), (1, 2)]))
    out.append(_case("fail-take-n134-t5", 134, [_mem(5), _mem(5, ("fail", 15)), _mem(5, take=0), _mem(5, ("fail", 65)), _mem(5, G6)],
                     ranges=[(0, 5), (1, 3)]))
    out.append(_case("nan-n70-t0", 70, [_mem(0), _mem(0, ("nan", 66, 10)), _mem(0)], ranges=[(0, 3), (1, 2)]))
    # E[F_L11.p, F_L11.p] beyond one tile: wide rank-deficient working sets (no high-precision reference: see has_reference)
    for n, t, rank in [(40, 44, 23), (40, 44, 7), (70, 72, 37)]:
        w = dict(maker="wide_rankdefA", defect=n - rank)
        out.append(_case(f"perm-n{n}-t{t}-rank{rank}", n, [_mem(t, **w), _mem(t, **w), _mem(t, **w)]))
    # kp < n2 at a tile edge
    for m in (16, 17, 33):
        out.append(_case(f"kp{m}-n40-t0", 40, [_mem(0), _mem(0, G6), _mem(0)], m=m))
    out.append(_case("kp33-n70-t5", 70, [_mem(5), _mem(5, G6), _mem(5)], m=33))
    # one ragged batch over the wave form's panel and tile edges
    out.append(_case("ragged-n40", 40, [_mem(0), _mem(7), _mem(8, G6), _mem(23), _mem(24)], ranges=[(0, 5), (1, 3)]))
    ids = [c["id"] for c in out]
    assert len(ids) == len(set(ids)), ids
    return tuple(out)


def cases() -> list:
    return list(_cases())


def case(cid):
    return next(c for c in _cases() if c["id"] == cid)


def t_max(c):
    return max(mb["t"] for mb in c["members"])


def ragged(c):
    return len({mb["t"] for mb in c["members"]}) > 1


def has_reference(c):
    """False for the wide rank-deficient working sets.  With a rank defect above 2 the reflectors k >= rankA of F_A and the order
    F_L11.p[rankA:] come from rounding noise, and E22 re-indexed by that order is no similarity of the basis J2'J2 is written in:
    the step of the reference's lines then moves by 2e-2 to 7e-1 under a perturbation of A of 1e-15 relative, and the mpmath,
    longdouble and FP64 evaluations differ by 1e-4 to 1e-3.  What is defined is the step ON GIVEN FACTORS: the GPU test holds the
    batched call to enlsip_gn_newton_direction on a second handle with the same resident factors, and the host test holds the
    restated kernels to the reference's lines on the oracle's factors; only the high-precision comparison is skipped."""
    return all(mb["maker"] != "wide_rankdefA" for mb in c["members"])


def literal(c, k):
    """(rankA, n2, kp) the table means for member k"""
    mb = c["members"][k]
    rankA = c["n"] - mb["defect"] if mb["maker"] == "wide_rankdefA" else mb["t"]
    return rankA, c["n"] - rankA, min(c["m"], c["n"] - rankA)


def _hash(s: str) -> int:
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def seed_of(c, k):
    mb = c["members"][k]
    # members of one shape and kind share their problem across cases (their references are computed once)
    base = 61000 + 11 * (_hash(f"{c['n']}-{c['m']}-{mb['t']}-{mb['maker']}-{mb['defect']}") % 20000)
    return base + 3 * k * (mb["kind"] == PLAIN) + _hash(repr(mb["kind"])) % 1000 + ADVANCED_SEEDS.get((c["id"], k), 0)


@functools.lru_cache(maxsize=None)
def _member(n, m, t, maker, defect, kind, seed):
    if maker == "wide_rankdefA":
        prob = nr.make_wide_rankdef_A(seed, m, n, t, defect)
    elif maker == "graded_J":
        prob = synth.make_graded_J(seed, m, n, t, GRADED_J_DECADES)
    else:
        prob = synth.make_problem(seed, m, n, t)
    if kind[0] in ("fail", "graded"):
        prob, ref, Gam = designed(seed, prob, kind)
    else:
        ref = go.gn_subproblem(*prob)
        if kind[0] == "graded_J":
            Gam = GRADED_J_DELTA * np.eye(n)
        else:
            Gam = nr.make_gammas(seed, prob[0], prob[2], ref, scale=PERM_SCALE if maker == "wide_rankdefA" else 0.3)[0]
            if kind[0] == "nan":
                Gam = Gam.copy()
                Gam[kind[1], kind[2]] = np.nan
    for a in prob + (Gam,):
        a.setflags(write=False)
    return prob, ref, Gam


def member(c, k):
    """((J, rx, A, cx), oracle result, Gamma) of member k; read-only and shared"""
    mb = c["members"][k]
    return _member(c["n"], c["m"], mb["t"], mb["maker"], mb["defect"], mb["kind"], seed_of(c, k))


def partner_gamma(c, k):
    """a positive-definite Gamma for the problem of a failing member: the `plain` one of its (scaled) problem"""
    prob, ref, _ = member(c, k)
    return nr.make_gammas(seed_of(c, k) + 5, prob[0], prob[2], ref)[0]


# ---- references --------------------------------------------------------------------------------------------------------------------
def uses_mpmath(c):
    return (c["n"] <= 40 and c["m"] <= 300) or not nr.LD_OK


@functools.lru_cache(maxsize=None)
def _reference(n, m, t, maker, defect, kind, seed, mpm):
    prob, ref, Gam = _member(n, m, t, maker, defect, kind, seed)
    return (nr.NewtonReference if mpm else nr.NewtonReferenceLD)(*prob, Gam, ref)


def reference(c, k, mpm=None):
    """the high-precision reference of member k: mpmath where n <= 40 and m <= 300, the longdouble restatement beyond"""
    mb = c["members"][k]
    return _reference(c["n"], c["m"], mb["t"], mb["maker"], mb["defect"], mb["kind"], seed_of(c, k), uses_mpmath(c) if mpm is None else mpm)


def parts(prob, ref, Gam):
    """FP64 pieces of the reference's lines on the oracle's factors: Q1, p1, E (re-indexed where t > rankA), J1, J2"""
    J, rx, A, cx = prob
    n = J.shape[1]
    t = A.shape[0] if A.size else 0
    r = ref.rankA
    Q1 = _q1(n, t, ref)
    if r == t:
        p1 = np.linalg.solve(np.triu(ref.F_A.R)[:t, :t].T, -cx[ref.F_A.p - 1]) if t else np.zeros(0)
    else:
        b = ref.F_L11.Qt_mul(-cx[ref.F_A.p - 1])
        p1 = ref.F_L11.P[:r, :r] @ np.linalg.solve(np.triu(ref.F_L11.R)[:r, :r], b[:r])
    JQ1 = J @ Q1
    E0 = Q1.T @ Gam @ Q1 if t else np.array(Gam)          # no reflector, no product: a NaN entry of Gamma stays one entry
    vp = (ref.F_L11.p - 1) if t > r else np.arange(n)
    return dict(Q1=Q1, p1=p1, E0=E0, vp=vp, E=E0[np.ix_(vp, vp)], J1=JQ1[:, :r], J2=JQ1[:, r:], r=r)


@functools.lru_cache(maxsize=None)
def _certificate(n, m, t, maker, defect, kind, seed):
    prob, ref, Gam = _member(n, m, t, maker, defect, kind, seed)
    P = parts(prob, ref, Gam)
    r = P["r"]
    E22 = 0.5 * (P["E"][r:, r:] + P["E"][r:, r:].T)
    sW = E22 + P["J2"].T @ P["J2"]
    out = dict(sW=sW, nJ2=float(np.linalg.norm(P["J2"], 2) ** 2))
    if np.all(np.isfinite(sW)):
        ev = np.linalg.eigvalsh(sW)
        out.update(nE22=float(np.linalg.norm(E22, 2)), lam_min=float(ev[0]), norm=float(np.abs(ev).max()))
        out["kappa"] = (out["nJ2"] + out["nE22"]) / out["lam_min"] if ev[0] > 0 else float("inf")
    else:
        out.update(nE22=float("nan"), lam_min=float("nan"), norm=float("nan"), kappa=float("inf"))
    if maker == "wide_rankdefA":
        # figures that hold in ANY orthonormal basis of null(A) and any order of it (the device has its own): sW22 there is
        # P'Q2' sym(Gamma) Q2 P + Q2'J'J Q2, so lambda_min >= lambda_min(J2'J2) - ||sym Gamma||, and kappa is bounded likewise
        out["nG"] = float(np.linalg.norm(0.5 * (Gam + Gam.T), 2))
        out["lamJ"] = float(np.linalg.eigvalsh(P["J2"].T @ P["J2"])[0])
        out["kappa"] = (out["nJ2"] + out["nG"]) / (out["lamJ"] - out["nG"]) if out["lamJ"] > out["nG"] else float("inf")
    out["fail_index"] = nr.cholesky_fail_index(sW)[0]
    return out


def certificate(c, k):
    """FP64 figures of member k: sW22 of the oracle, ||J2||^2, ||sym E22||, lambda_min, kappa, the left-looking verdict"""
    mb = c["members"][k]
    return _certificate(c["n"], c["m"], mb["t"], mb["maker"], mb["defect"], mb["kind"], seed_of(c, k))


def expected_fail_index(c, k):
    kind = c["members"][k]["kind"]
    return kind[1] if kind[0] in ("fail", "nan") else -1


def expected_status(c, k):
    return 1 if expected_fail_index(c, k) >= 0 else 0


# ---- the kernels' decomposition, restated in FP64 with switchable defects --------------------------------------------------------
def right_looking(S, mutate=None):
    """(L, fail index) of the blocked right-looking Cholesky of k_newton_chol_batched: panels of NB, the trailing matrix updated
    by TILE x TILE tiles of its lower triangle.  mutate: "tile_row" skips the last partial tile row of every trailing update,
    "late_pivot" ignores a pivot that is not > 0 in a panel after the first."""
    A = np.array(S, dtype=np.float64)
    n2 = A.shape[0]
    for j0 in range(0, n2, NB):
        nb = min(NB, n2 - j0)
        for k in range(j0, j0 + nb):
            akk = A[k, k]
            if not akk > 0.0:
                if not (mutate == "late_pivot" and j0 > 0):
                    return A, k
            with np.errstate(invalid="ignore"):
                A[k, k] = np.sqrt(akk)
            A[k + 1:, k] /= A[k, k]
            c1 = j0 + nb
            A[k + 1:, k + 1:c1] -= np.outer(A[k + 1:, k], A[k + 1:c1, k])
        t0 = j0 + nb
        rem = n2 - t0
        nrt = rem // TILE if mutate == "tile_row" else (rem + TILE - 1) // TILE
        hi = min(n2, t0 + TILE * nrt)
        P = A[t0:hi, j0:t0]
        A[t0:hi, t0:hi] -= P @ P.T
    return np.tril(A), -1


def kernel_model(prob, ref, Gam, mutate=None):
    """(p, status) as the batched kernels cut the work: R'R tile by tile with the depth clip kmax = min(kp, 16 I + 16), scattered
    through jpvtJ, the blocked Cholesky, p = F_A.Q [p1; p2].  mutate: one of "tile_row", "kmax4" (kmax rounded down to a multiple of
    4), "late_pivot", "no_perm" (E read without F_L11.p)."""
    P = parts(prob, ref, Gam)
    r, n = P["r"], prob[0].shape[1]
    n2, kp = n - r, min(prob[0].shape[0], n - r)
    E = P["E0"] if mutate == "no_perm" else P["E"]
    R = np.triu(ref.F_J2.R)[:kp, :n2]
    pj = ref.F_J2.p - 1
    G = np.zeros((n2, n2))
    for I in range((n2 + TILE - 1) // TILE):
        kmax = min(kp, TILE * I + TILE)
        if mutate == "kmax4":
            kmax &= ~3
        rows = slice(TILE * I, min(n2, TILE * I + TILE))
        G[rows, TILE * I:] = R[:kmax, rows].T @ R[:kmax, TILE * I:]
    G = np.triu(G) + np.triu(G, 1).T
    sW = np.zeros((n2, n2))
    sW[np.ix_(pj, pj)] = G
    sW += 0.5 * (E[r:, r:] + E[r:, r:].T)
    d = -(E[r:, :r] + P["J2"].T @ P["J1"]) @ P["p1"] - P["J2"].T @ prob[1]
    L, fail = right_looking(sW, mutate)
    if fail >= 0:
        return np.zeros(n), 1
    p2 = np.linalg.solve(L.T, np.linalg.solve(L, d))
    return P["Q1"] @ np.concatenate([P["p1"], p2]), 0
