"""The resident factors by their DEFINING identities, on every route (test infrastructure: nothing here is on the product path,
nothing here touches a GPU by itself).

A solve leaves F_A, F_L11 and F_J2 resident and every consumer reads them through the accessors.  A pivoted QR has a definition
that needs neither the oracle nor a sign convention:

    Q [R; 0] = M P        checked column by column in BOTH directions, over the full length (the tail of Q'(M P e_j) must vanish),
    R'R = (M P)'(M P)     on every column,

with M the matrix the factor is DEFINED on: A' for F_A, F_A.R' for F_L11 (oracle/gn_oracle.py: qr_colnorm(F_A.R.T)) and
(J Q_A)[:, rankA:] for F_J2, Q_A formed from the library's own F_A.Q_mul.  `check_factor_identity` evaluates them for anything with
R, p, Qt_mul, Q_mul (the oracle's QRPivoted, the library's FactorView); `check_solve_identities` runs the whole chain of one solved
problem, including the J1 columns the routed J*Q1 kernel left in W, get_JQ1, and out.d over its full length with its sign;
`cases()` picks, BY RULE from tests/dispatch_grid.py, the shapes that reach every route bit below the size cap, every kind that is
not `full`, the forced variants the library offers and the problem-index cases.

Tolerances = the reference floor (the worst residual of the SAME checker on the oracle's LAPACK factors over every case, measured
by tests/test_factor_identities_host.py, which also asserts that the floors below still hold) times a margin for the reduction
orders LAPACK does not have (tree QR, MFMA accumulation, rsq / rcp + Newton reflector scalars), under a cap that keeps the 1e-9
mutations of the host test failing.  The figures are repeated in DESIGN.md §2."""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

import dispatch_grid as dg

FACTOR_A, FACTOR_L11, FACTOR_J2 = 0, 1, 2          # include/enlsip_gn.h: ENLSIP_GN_FACTOR_*
EPS = float(np.finfo(np.float64).eps)

# ---- tolerances --------------------------------------------------------------------------------------------------------------------
# Reference floors: worst residual over cases() with the oracle's factors on the CPU (test_reference_floor_over_every_case prints
# and bounds them).  Measured: column identities 1.2e-15 (both directions; F_L11 at 448 x 384, t = 64), orthogonality of the explicit
# Q_A 1.9e-15 (n = 600), W / get_JQ1 against the long-double product 5.9e-16, Gram 1.5e-15, d 2.3e-15 (kinds full, rankdefA,
# rankdefJ); the graded kind's d 6.8e-11, 0.43 of its conditioning term eps ||J1||_2 ||p|| / ||d||.
FLOOR_COL = 2.5e-15
FLOOR_GRAM = 2.0e-15
FLOOR_D = 3.0e-15
D_COND_PASSES = 4.0                  # graded d: see assert_within
MARGIN = 20.0                        # tree QR, MFMA accumulation order, fast reflector scalars: none of them in LAPACK
CAP_COL, CAP_GRAM_D = 1e-13, 1e-12   # beyond these the 1e-9 mutations of the host test would stop failing
TOL_COL = min(MARGIN * FLOOR_COL, CAP_COL)          # 5e-14: Q'(MP e_j) = [R e_j; 0], Q [R e_j; 0] = MP e_j, Q_A'Q_A = I, W, get_JQ1
TOL_GRAM = min(MARGIN * FLOOR_GRAM, CAP_GRAM_D)     # 4e-14
TOL_D = min(MARGIN * FLOOR_D, CAP_GRAM_D)           # 6e-14
# MI355X maxima over every case of tests/test_gpu_factor_identities.py: columns 1.4e-15, orthogonality 2.1e-15 (n = 512), W / get_JQ1
# 9.5e-16, Gram 1.6e-15, d 2.2e-15, graded d 4.8e-11 (0.29 of its term): the device needs 1.1 times the floor.

SIZE_CAP = 600000            # m * n of a case
BATCH_CAP = 8
NEED_LARGE_BATCH = {"pipeline_split", "sweep_pairs", "chunked"}     # pipeline from 128 problems, pairs by size from 8192 far
                                                                    # workgroups, chunks above the launch limit


def sample_columns(ncols: int, seed: int = 0) -> np.ndarray:
    """All columns up to 96; beyond: j mod 32 in {0, 1, 31} (both edges of every panel), the last one and 16 seeded ones."""
    if ncols <= 96:
        return np.arange(ncols)
    j = np.arange(ncols)
    pick = set(j[np.isin(j % 32, (0, 1, 31))].tolist()) | {ncols - 1}
    pick |= set(np.random.default_rng(1000 + seed).choice(ncols, size=16, replace=False).tolist())
    return np.array(sorted(pick))


def _norm2(M) -> float:
    return float(np.linalg.norm(M, 2)) if M.size else 0.0


def check_factor_identity(F, M, *, rows_defined=None, cols=None, gram=True):
    """(res_qt, res_q, res_gram) of the factorisation F of M: the worst column of |Q'(MP e_j) - [R e_j; 0]| and of
    |Q [R e_j; 0] - MP e_j| over the checked columns, relative to ||M||_2, and the worst column of |R'R - (MP)'(MP)| over EVERY
    column, relative to ||M||_2^2.  rows_defined = r: a factorisation that stopped after r steps — columns j < r in full, columns
    j >= r on the first r rows of the Q' direction only, the Gram identity on the leading r x r block.  cols: the columns to check
    (default: sample_columns).  gram = False: no Gram identity (returned as 0)."""
    M = np.asarray(M, dtype=np.float64)
    rows, nc = M.shape
    R = np.asarray(F.R)
    p = np.asarray(F.p)
    k = R.shape[0]
    assert R.shape == (min(rows, nc), nc), (R.shape, M.shape)
    assert p.shape == (nc,) and np.array_equal(np.sort(p), np.arange(1, nc + 1)), "jpvt is not a permutation"
    if rows == 0 or nc == 0:
        return 0.0, 0.0, 0.0
    assert np.array_equal(np.tril(R, -1), np.zeros_like(R)), "R is not upper triangular"
    nrm = _norm2(M)
    nrm = nrm if nrm > 0 else 1.0
    Mp = M[:, p - 1]
    r = k if rows_defined is None else min(int(rows_defined), k)
    res_qt = res_q = 0.0
    for j in (sample_columns(nc) if cols is None else np.asarray(cols)):
        j = int(j)
        want = np.zeros(rows)
        want[:k] = R[:, j]
        got = np.asarray(F.Qt_mul(Mp[:, j]))
        assert got.shape == (rows,)
        if j < r or rows_defined is None:
            res_qt = max(res_qt, float(np.linalg.norm(got - want)) / nrm)          # the tail beyond k must vanish
            back = np.asarray(F.Q_mul(want))
            res_q = max(res_q, float(np.linalg.norm(back - Mp[:, j])) / nrm)
        else:
            res_qt = max(res_qt, float(np.linalg.norm(got[:r] - want[:r])) / nrm)
    res_gram = 0.0
    if gram:
        Rr, Mr = (R, Mp) if rows_defined is None else (R[:r, :r], Mp[:, :r])
        G = Rr.T @ Rr - Mr.T @ Mr
        res_gram = float(np.sqrt((G * G).sum(axis=0)).max()) / nrm ** 2 if G.size else 0.0
    return res_qt, res_q, res_gram


# ---- access to one solved problem ------------------------------------------------------------------------------------------------
class SolverAccess:
    """Problem `prob` of the batch a GNSolver holds resident, through its accessors only."""

    def __init__(self, solver, m: int, n: int, prob: int = 0):
        self.s, self.m, self.n, self.prob = solver, m, n, prob

    def factor(self, which: int):
        return self.s.factor(which, self.prob)

    def JQ1(self) -> np.ndarray:
        return self.s.JQ1(self.m, self.n, self.prob)

    def W(self):
        """The working matrix [J Q_A | d] after the sweep (m x (n + 1)), or None for a problem of the second pipeline half:
        enlsip_gn_debug_copy_W reads the handle it is given, and that half lives on the child handle."""
        split = self.s.launch_plan()[0]
        if split > 0 and self.prob >= split:
            return None
        ldw = C.c_int64(0)
        self.s._lib.enlsip_gn_debug_copy_W(self.s._h, self.prob, None, C.byref(ldw), 0)        # -3: only reports ldw
        cap = int(ldw.value) * (self.n + 1)
        assert cap >= self.m * (self.n + 1)
        buf = np.zeros(cap)
        rc = self.s._lib.enlsip_gn_debug_copy_W(self.s._h, self.prob, buf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ldw), cap)
        assert rc == 0, rc
        return buf.reshape(self.n + 1, int(ldw.value)).T[:self.m, :]


class OracleAccess:
    """The same interface over the oracle's solution of (J, rx, A, cx): the reference floor of every identity."""

    def __init__(self, ref, J):
        self.ref, self.J = ref, np.asarray(J, dtype=np.float64)

    def factor(self, which: int):
        return (self.ref.F_A, self.ref.F_L11, self.ref.F_J2)[which]

    def JQ1(self) -> np.ndarray:
        return self.ref.F_A.rmul_Q(self.J)

    def W(self):
        return self.JQ1()                 # LAPACK leaves no sweep behind: the J1 columns are those of J * F_A.Q


def _col_err(X, Y, nrm) -> float:
    D = np.asarray(X, dtype=np.float64) - np.asarray(Y, dtype=np.float64)
    return float(np.sqrt((D * D).sum(axis=0)).max()) / nrm if D.size else 0.0


def check_solve_identities(acc, J, rx, A, cx, out, *, kind="full", cols=None, rows_defined=None, cols_J2=None) -> dict:
    """Every identity of one solved problem, from `acc` alone (SolverAccess / OracleAccess); out: its p, d, rankA (GNResult,
    GNSolution or anything with those fields).  Exact properties (shapes, diagonals, permutations) are asserted here; the residuals
    come back in a dict for assert_within — keys orth, A.qt / A.q / A.gram, L11.*, J2.*, W, JQ1, d and d_cond (the conditioning
    term of the d bound, eps ||J1||_2 ||p|| / ||d||, see assert_within).  cols_J2: the columns of F_J2 to check where they are
    not those of `cols` (tests/test_gpu_sweep_edges.py: every column of F_J2, the sampled ones of the small factors)."""
    J = np.asarray(J, dtype=np.float64)
    m, n = J.shape
    A = np.asarray(A, dtype=np.float64).reshape(-1, n)
    t = A.shape[0]
    kA = min(n, t)
    rankA = int(out.rankA)
    res = {}
    FA, FL, FJ = acc.factor(FACTOR_A), acc.factor(FACTOR_L11), acc.factor(FACTOR_J2)
    # factor_shape, diagR() and R.diagonal() agree exactly; shapes are those of the definition
    for F, shp in ((FA, (kA, t)), (FL, (min(t, kA), kA)), (FJ, (min(m, n - rankA), n - rankA))):
        R = np.asarray(F.R)
        assert R.shape == shp, (R.shape, shp)
        if hasattr(F, "shape"):
            assert tuple(F.shape) == shp
        assert np.array_equal(np.asarray(F.diagR()), R.diagonal()), "diagR() differs from diag(R)"
    # Q_A explicitly: n applications of F_A.Q_mul to unit vectors
    if t:
        QA = np.empty((n, n))
        I = np.eye(n)
        for j in range(n):
            QA[:, j] = FA.Q_mul(I[:, j])
    else:
        QA = np.eye(n)
    res["orth"] = _norm2(QA.T @ QA - np.eye(n))
    res["A.qt"], res["A.q"], res["A.gram"] = check_factor_identity(FA, A.T, cols=cols)
    res["L11.qt"], res["L11.q"], res["L11.gram"] = check_factor_identity(FL, np.asarray(FA.R).T, cols=cols)
    # J Q_A on the host in long double, rounded once
    JQ = np.asarray(J.astype(np.longdouble) @ QA.astype(np.longdouble), dtype=np.float64)
    nJ = _norm2(J)
    J1, J2 = JQ[:, :rankA], JQ[:, rankA:]
    res["J2.qt"], res["J2.q"], res["J2.gram"] = check_factor_identity(FJ, J2, cols=cols if cols_J2 is None else cols_J2, rows_defined=rows_defined,
                                                                      gram=kind != "graded")
    # the J1 columns the routed J*Q1 kernel wrote (the sweep starts at column rankA: k_caqr_update_refl's col0; the re-solve reads
    # them there: k_dtemp_batched), and get_JQ1
    W = acc.W()
    res["W"] = _col_err(W[:, :rankA], J1, nJ) if W is not None and rankA else 0.0
    res["JQ1"] = _col_err(acc.JQ1(), JQ, nJ)
    # d over its full length, with its sign: the carried right-hand side of the sweep against the accessor path
    p = np.asarray(out.p, dtype=np.float64)
    d = np.asarray(out.d, dtype=np.float64)
    assert d.shape == (m,) and np.all(np.isfinite(d)) and np.all(np.isfinite(p))
    p1 = np.asarray(FA.Qt_mul(p))[:rankA] if t else np.zeros(0)
    dref = np.asarray(FJ.Qt_mul(-(J1 @ p1) - np.asarray(rx, dtype=np.float64)))
    nd = float(np.linalg.norm(dref))
    res["d"] = float(np.linalg.norm(d - dref)) / (nd if nd > 0 else 1.0)
    res["d_cond"] = EPS * _norm2(J1) * float(np.linalg.norm(p)) / (nd if nd > 0 else 1.0)
    return res


def assert_within(res: dict, kind: str, tag=None):
    """The tolerances of the module head.  kind `graded`: d carries the conditioning term eps ||J1||_2 ||p|| / ||d|| — p1 is
    recovered from p, and p has gone through Q_A twice (p = Q_A [p1; p2] where it was made, Q_A'p here); each pass loses a small
    multiple of eps ||p||, which J1 carries into a d that is small beside J1 p1: not a rounding of d itself.  D_COND_PASSES = 4:
    two passes, a factor 2 each (LAPACK's own two passes measure 0.43 of the term in all)."""
    bad = {}
    for key, v in res.items():
        if key == "d_cond":
            continue
        if key == "d":
            tol = TOL_D + (D_COND_PASSES * res["d_cond"] if kind == "graded" else 0.0)
        elif key.endswith(".gram"):
            tol = TOL_GRAM
        else:
            tol = TOL_COL
        if not v <= tol:
            bad[key] = (v, tol)
    assert not bad, (tag, bad)


# ---- the case list ---------------------------------------------------------------------------------------------------------------
def _pool():
    return [c for c in dg.grid() if c["batch"] <= BATCH_CAP and c["m"] * c["n"] <= SIZE_CAP]


def _route(c, **kw):
    return dg.expected_route(c["batch"], c["m"], c["n"], c["t"], c["kind"] == "rankdefA", **kw)


def reachable_bits() -> set:
    """Route bits some grid case reaches below the size cap."""
    out = set()
    for c in _pool():
        out |= _route(c)
    return out


def _kp(c):
    return min(c["m"], c["n"] - min(c["n"], c["t"]))


def _npan(c):
    return (_kp(c) + dg.PB - 1) // dg.PB


@contextlib.contextmanager
def _pairs_forced():
    """expected_route as ENLSIP_GN_PAIR=1 makes it: pairs for every shape with three panels or more, whatever the far workgroups"""
    old = dg.PAIR_MIN_WGS
    dg.PAIR_MIN_WGS = 0
    try:
        yield
    finally:
        dg.PAIR_MIN_WGS = old


def _case(c, tag, *, want=None, env=None, flags=0, tile_rows=0, probs=None, t_list=None):
    batch = c["batch"]
    return dict(id=f"{tag}-b{batch}-{c['m']}x{c['n']}-t{c['t']}-{c['kind']}", batch=batch, m=c["m"], n=c["n"], t=c["t"], kind=c["kind"],
                want=_route(c) if want is None else want, env=env or {}, flags=flags, tile_rows=tile_rows,
                probs=probs if probs is not None else sorted({0, batch - 1}), t_list=t_list)


def cases() -> list:
    """Dicts: id, batch, m, n, t, kind, want (route bits the solve must report), env / flags / tile_rows (of the handle), probs
    (the problems whose factors are checked), t_list (a ragged batch's own t_k) — see the module head for the rules."""
    pool = _pool()
    out = []
    # greedy cover of the reachable route bits by the `full` and `rankdefA` cases (the only kinds that change the route)
    todo = reachable_bits()
    while todo:
        best = max(pool, key=lambda c: (len(_route(c) & todo), -c["m"] * c["n"] * c["batch"]))
        gain = _route(best) & todo
        assert gain
        out.append(_case(best, "cover"))
        todo -= gain
    have = {(c["batch"], c["m"], c["n"], c["t"], c["kind"]) for c in out}
    for c in pool:
        if c["kind"] != "full" and (c["batch"], c["m"], c["n"], c["t"], c["kind"]) not in have:
            out.append(_case(c, "kind"))
    # forced variants, each on a handle of its own
    one = [c for c in pool if c["batch"] == 1 and c["kind"] == "full"]
    by_size = sorted(one, key=lambda c: c["m"] * c["n"])
    with _pairs_forced():
        for odd in (1, 0):       # ENLSIP_GN_PAIR=1: the smallest shapes with >= 3 panels, an odd and an even count, more than one tile
            c = next(c for c in by_size if _npan(c) >= 3 and _npan(c) % 2 == odd and c["m"] > 512)
            out.append(_case(c, "pairs", env={"ENLSIP_GN_PAIR": "1"}))
            assert "sweep_pairs" in out[-1]["want"]
    c = next(c for c in by_size if c["m"] > 512 and _npan(c) >= 2)
    out.append(_case(c, "tile256", want=_route(c, tile_rows=256), tile_rows=256))
    sweep_or_jq1 = {b for b in dg.header_route_names() if b.startswith("jq1_")}
    out.append(_case(c, "reflectors", want=(_route(c) - sweep_or_jq1) | {"jq1_plain", "sweep_reflectors"}, flags=2))   # FLAG_UPDATE_REFLECTORS
    c = next(c for c in by_size if _kp(c) > 512)
    blocks = {b for b in dg.header_route_names() if b.startswith("pivot_blocks") or b == "pivot_hybrid"}
    out.append(_case(c, "steps", want=(_route(c) - blocks) | {"pivot_steps"}, env={"ENLSIP_GN_QRCP_HYBRID": "0"}))
    c = dict(batch=1, m=256, n=32, t=4, kind="full")
    assert "jq1_fused_small" in _route(c)
    unfused = _route(dict(c, m=257)) - {"sweep_tile512"} | {"sweep_tile256"}       # one row more is the same route without the fusion, but for the tile
    out.append(_case(c, "unfused", want=unfused, env={"ENLSIP_GN_FUSE_SMALL": "0"}))
    # problem indices: a batch of 5, both pipeline halves of 128, a ragged batch with its own leading dimension of F_L11
    c = max((c for c in pool if c["batch"] == 5 and c["kind"] == "full"), key=_npan)
    out.append(_case(c, "index", probs=[0, 4]))
    c = dict(batch=128, m=300, n=66, t=5, kind="full")
    assert c in dg.grid()
    out.append(_case(c, "halves", probs=[0, 63, 64, 127]))
    c = dict(batch=3, m=300, n=40, t=6, kind="full")
    out.append(_case(c, "ragged", want=set(), probs=[0, 2], t_list=[0, 3, 6]))
    ids = [c["id"] for c in out]
    assert len(ids) == len(set(ids)), ids
    return out


def covered_bits(cs=None) -> set:
    out = set()
    for c in (cases() if cs is None else cs):
        out |= c["want"]
    return out


def problem(c, k: int):
    """(J, rx, A, cx) of problem k of case c (a ragged case: its own t_k rows of A)."""
    from oracle import synth
    gens = {"full": synth.make_problem, "rankdefA": synth.make_rank_deficient_A, "rankdefJ": synth.make_rank_deficient_J,
            "graded": synth.make_graded_J}
    seed = 77000 + 131 * (hash_id(c["id"]) % 1000) + k
    t = c["t_list"][k] if c["t_list"] else c["t"]
    return gens[c["kind"]](seed, c["m"], c["n"], t)


def hash_id(s: str) -> int:
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % 1000003
    return h


@contextlib.contextmanager
def handle_env(env: dict):
    """The environment of a forced variant, set only around the creation of its handle (the library reads it there)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
