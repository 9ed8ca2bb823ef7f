"""Structurally sparse Jacobians and bound constraints, on every route (test infrastructure, CPU only: NumPy, the oracle's seeded
streams, tests/dispatch_grid.py and tests/factor_identities.py; nothing here touches a GPU).

Every other generator of the suite is dense.  Exact zeros reach branches a dense matrix reaches by rounding accident or never: the
identity reflector of make_reflector (gn_device_utils.hpp: xnorm2 == 0 or alpha^2 + xnorm2 < GN_TINY_NORM2), a reflector that starts
on alpha == 0, partial column norms that are exactly zero in every form of the pivoted QR, and exact ties of the pivot search.

Kinds of J (m x n, t = 0 unless the case says otherwise; G is the Gaussian draw of oracle.synth.make_problem):
* upper        triu(G) + s I with s = max(4, ceil(sqrt(n))): every Householder step of every row partition meets a zero tail, so
               every reflector of the sweep is the identity.  (With s = 4 the triangle loses rank from n ~ 500 on, cond 1e10 at
               n = 513: the shift grows with sqrt(n) and keeps cond(J) below 10.)
* tileblock    column block c (PB = 32 columns) is non-zero only in row tile c mod tiles, the tile height being the one of the case's
               route: whole tiles of a panel are zero, tree nodes combine a zero triangle with a live one, panels start on alpha == 0.
* banded       G where |i n // m - j| <= 3.
* zerocols     G with columns 0, 31, 32 and n - 1 exactly zero (variant `panel`: the whole panel 32 .. 63).
* lastrows     only the last max(n + 5, 40) rows are non-zero (variant `short`: m = 512 k + that many, the live rows are a short
               last tile of their own).
* mixed_scale  G with three columns times 2^-480 among unit columns: alpha^2 + xnorm2 falls below GN_TINY_NORM2 on them while the
               matrix as a whole stays in the magnitude window (no rescale).
Kinds of A (t x n), each beside a dense and a banded J:
* bounds       rows a_k e_{i_k}', distinct i_k, a_k = +-(1 + k / 64): tie-free pivots in the order of descending |a_k|.
* bounds_tied  a_k = +-1: every pivot is an exact tie, LAPACK's idamax rule (lowest position) decides all of them.
* bounds_dup   bounds with row t - 1 on the column of row 0 (cx consistent): rankA = t - 1, a second attempt, and the column of row 0 is
               exactly zero after the first step.

Shapes come by rule: for every J kind the smallest shape of every distinct set of sweep_* bits and of every distinct set of pivot_*
bits among the t = 0 shapes of dispatch_grid.grid() below factor_identities.SIZE_CAP (and a small lattice beside them, LATTICE, for
the sets a kind's structure needs more rows for), the forced variants of factor_identities.cases(), the constraint forms of
constraint_cases.form_shapes() and one shape per J*Q1 form.  tests/test_sparse_cases_host.py certifies every case on the CPU
before tests/test_gpu_sparse_jacobians.py runs it."""
from __future__ import annotations

import functools
import math
import re

import numpy as np

import constraint_cases as cc
import dispatch_grid as dg
import factor_identities as fi
from oracle import gn_oracle as go, synth

KINDS_J = ("upper", "tileblock", "banded", "zerocols", "lastrows", "mixed_scale")
KINDS_A = ("bounds", "bounds_tied", "bounds_dup")
BAND = 3
TINY_EXP = -480                                  # mixed_scale: the three columns are G * 2^TINY_EXP
GN_TINY_NORM2 = float(re.search(r"constexpr double GN_TINY_NORM2 = ([0-9.e+-]+);",
                                (dg.CSRC / "gn_device_utils.hpp").read_text()).group(1))
LATTICE = ((1024, 512), (1024, 513))             # two full tiles: tileblock keeps its rank there on 16 and 17 column blocks
# cases whose first seed leaves a pivot of F_J2 within LEAD_FLOOR = 2e-7 of its runner-up (measured by the host test: 1.4e-8 and
# 1.1e-7) and which are the only ones of their kind on their pivot form: the next seed that certifies them
SEED_SHIFT = {"tileblock-grid-b1-1024x513-t0": 1, "mixed_scale-grid-b1-551x512-t0": 1}
HEALTH_SHAPE = (300, 40, 6)                      # the Gaussian problem a handle solves after its case; other cases use (71, 32, 4)
HEALTH_SHAPE_2 = (71, 32, 4)


def sweep_bits(route) -> frozenset:
    return frozenset(b for b in route if b.startswith("sweep_"))


def pivot_bits(route) -> frozenset:
    return frozenset(b for b in route if b.startswith("pivot_"))


def tile_height(m, route) -> int:
    """the row-tile height the route reports (make_plan: 256 rows up to m = 256 and where the handle asks for it)"""
    if "sweep_tile512" in route:
        return 512
    return 256


# ---- builders ------------------------------------------------------------------------------------------------------------------
def upper_shift(n) -> float:
    return float(max(4, math.ceil(math.sqrt(n))))


def zero_columns(n, variant=None) -> list:
    if variant == "panel":
        return list(range(32, 64))
    return sorted({c for c in (0, 31, 32, n - 1) if c < n})


def tiny_columns(n) -> list:
    return sorted({1, n // 2, n - 2})


def live_rows(n) -> int:
    return max(n + 5, 40)


def _tile_blocks(m, n, tile):
    """(rows of every tile, column blocks of every tile) of the tileblock kind"""
    tiles = (m + tile - 1) // tile
    rows = [min(tile, m - r * tile) for r in range(tiles)]
    nblk = (n + dg.PB - 1) // dg.PB
    blocks = [[c for c in range(nblk) if c % tiles == r] for r in range(tiles)]
    return rows, blocks


def applies(kind, m, n, tile) -> bool:
    """whether the structure of a kind exists at a shape (a tileblock on one tile is dense, a wide J has no last rows to keep)"""
    if kind == "banded":
        return m >= n
    if kind == "lastrows":
        return m > live_rows(n)
    if kind == "tileblock":
        rows, blocks = _tile_blocks(m, n, tile)
        width = lambda cs: sum(min(dg.PB, n - c * dg.PB) for c in cs)
        return len(rows) >= 2 and n > dg.PB and all(r >= width(cs) + 8 for r, cs in zip(rows, blocks))
    return True


def build_J(kind, seed, m, n, tile=512, variant=None) -> np.ndarray:
    G = synth.normal_stream(seed, 0, m * n).reshape((m, n), order="F")
    i, j = np.arange(m)[:, None], np.arange(n)[None, :]
    if kind == "dense":
        return G
    if kind == "upper":
        return np.triu(G) + upper_shift(n) * np.eye(m, n)
    if kind == "tileblock":
        tiles = (m + tile - 1) // tile
        return np.where((j // dg.PB) % tiles == i // tile, G, 0.0)
    if kind == "banded":
        return np.where(np.abs(i * n // m - j) <= BAND, G, 0.0)
    if kind == "zerocols":
        J = G.copy()
        J[:, zero_columns(n, variant)] = 0.0
        return J
    if kind == "lastrows":
        return np.where(i >= m - live_rows(n), G, 0.0)
    if kind == "mixed_scale":
        J = G.copy()
        J[:, tiny_columns(n)] = np.ldexp(J[:, tiny_columns(n)], TINY_EXP)
        return J
    raise ValueError(kind)


def build_A(kind, seed, n, t):
    """(A, cx, columns i_k, a_k) of a bounds kind"""
    assert 2 <= t <= n
    cols = np.argsort(synth.normal_stream(seed, 21, n), kind="stable")[:t].copy()
    sign = np.where(synth.normal_stream(seed, 22, t) < 0.0, -1.0, 1.0)
    a = sign * (np.ones(t) if kind == "bounds_tied" else 1.0 + np.arange(t) / 64.0)
    if kind == "bounds_dup":
        cols[t - 1] = cols[0]
    A = np.zeros((t, n))
    A[np.arange(t), cols] = a
    cx = synth.normal_stream(seed, 3, t)
    if kind == "bounds_dup":
        cx[0] = cx[t - 1] * a[0] / a[t - 1]
    return A, cx, cols, a


def build(c, k=0):
    """(J, rx, A, cx) of problem k of a case"""
    m, n = c["m"], c["n"]
    t = c["t_list"][k] if c["t_list"] else c["t"]
    seed = c["seed"] + k
    kindJ = c["kinds"][k] if c["kinds"] else c["kindJ"]
    J = build_J(kindJ, seed, m, n, c["tile"], c["variant"])
    rx = synth.normal_stream(seed, 1, m)
    if c["kindA"] and t:
        A, cx, _, _ = build_A(c["kindA"], seed, n, t)
    elif t:
        _, _, A, cx = synth.make_problem(seed, m, n, t)
    else:
        A, cx = np.zeros((0, n)), np.zeros(0)
    return J, rx, A, cx


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_pool() -> tuple:
    """the t = 0 shapes of the dispatch grid below the size cap, and LATTICE, by size"""
    pool = {(c["m"], c["n"]) for c in dg.grid() if c["batch"] == 1 and c["kind"] == "full" and c["t"] == 0}
    pool |= set(LATTICE)
    return tuple(sorted((s for s in pool if s[0] * s[1] <= fi.SIZE_CAP), key=lambda s: (s[0] * s[1], s[1])))


@functools.lru_cache(maxsize=None)
def shapes_of(kind) -> tuple:
    """the smallest shape of every distinct set of sweep_* bits and of every distinct set of pivot_* bits the kind applies at"""
    first = {}
    for (m, n) in shape_pool():
        r = dg.expected_route(1, m, n, 0)
        if not applies(kind, m, n, tile_height(m, r)):
            continue
        first.setdefault(("sweep", sweep_bits(r)), (m, n))
        first.setdefault(("pivot", pivot_bits(r)), (m, n))
    return tuple(sorted(set(first.values()), key=lambda s: (s[0] * s[1], s[1])))


def _hash(s: str) -> int:
    return fi.hash_id(s)


def _case(tag, kindJ, m, n, t=0, *, kindA=None, want=None, env=None, flags=0, tile_rows=0, variant=None, batch=1, kinds=None,
          t_list=None, rank_deficient=False):
    route = dg.expected_route(batch, m, n, t, rank_deficient, tile_rows=tile_rows or 512) if want is None else set(want)
    tile = 256 if (tile_rows == 256 or m <= 256) else 512
    name = kindJ + (f".{variant}" if variant else "") + (f"+{kindA}" if kindA else "")
    cid = f"{name}-{tag}-b{batch}-{m}x{n}-t{t}"
    return dict(id=cid, tag=tag, kindJ=kindJ, kindA=kindA, variant=variant, batch=batch, m=m, n=n, t=t, want=route, env=env or {},
                flags=flags, tile_rows=tile_rows, tile=tile, seed=61000 + 7 * (_hash(cid) % 20000) + SEED_SHIFT.get(cid, 0), kinds=kinds, t_list=t_list)


def forced_variants() -> list:
    """(tag, (m, n), keyword arguments of _case): the forced variants of factor_identities.cases(), on the t = 0 pool"""
    pool = [dict(batch=1, m=m, n=n, t=0, kind="full") for (m, n) in shape_pool()]
    out = []
    with fi._pairs_forced():
        for odd in (1, 0):
            c = next(c for c in pool if fi._npan(c) >= 3 and fi._npan(c) % 2 == odd and c["m"] > 512)
            out.append(("pairs_odd" if odd else "pairs_even", (c["m"], c["n"]), dict(want=fi._route(c), env={"ENLSIP_GN_PAIR": "1"})))
            assert "sweep_pairs" in out[-1][2]["want"]
    c = next(c for c in pool if c["m"] > 512 and fi._npan(c) >= 2)
    out.append(("tile256", (c["m"], c["n"]), dict(want=fi._route(c, tile_rows=256), tile_rows=256)))
    jq1 = {b for b in dg.header_route_names() if b.startswith("jq1_")}
    out.append(("reflectors", (c["m"], c["n"]), dict(want=(fi._route(c) - jq1) | {"jq1_plain", "sweep_reflectors"}, flags=2)))
    c = next(c for c in pool if fi._kp(c) > 512)
    blocks = {b for b in dg.header_route_names() if b.startswith("pivot_blocks") or b == "pivot_hybrid"}
    out.append(("steps", (c["m"], c["n"]), dict(want=(fi._route(c) - blocks) | {"pivot_steps"}, env={"ENLSIP_GN_QRCP_HYBRID": "0"})))
    # the fused small kernel and its unfused partner (m <= 256, n <= 32, n2 < 32) at t = 0
    c = dict(batch=1, m=256, n=24, t=0, kind="full")
    assert "jq1_fused_small" in fi._route(c)
    out.append(("fused", (256, 24), dict(want=fi._route(c))))
    unfused = fi._route(dict(c, m=257)) - {"sweep_tile512"} | {"sweep_tile256"}
    out.append(("unfused", (256, 24), dict(want=unfused, env={"ENLSIP_GN_FUSE_SMALL": "0"})))
    return out


WIDE_VARIANTS = ("pairs_odd", "tile256", "fused", "unfused")      # every kind; the others: upper, tileblock, zerocols
BATCH_SHAPE = (300, 24)                                           # the batch of five: one tile, pivot_wave2
BATCH_KINDS = ("upper", "banded", "zerocols", "lastrows", "mixed_scale")    # tileblock needs two tiles and two column blocks
RAGGED = dict(m=300, n=40, t_list=(0, 3, 6))


@functools.lru_cache(maxsize=None)
def a_shapes() -> tuple:
    """((m, n, t, with a banded J too), ...): the smallest (n, t) of every constraint form, and one shape per J*Q1 form"""
    out = [(cc.rows_of(n), n, t) for (n, t) in cc.form_shapes().values()]
    jq1 = {"jq1_fused_small": None, "jq1_rows32": (300, 24, 8), "jq1_rows2": None, "jq1_mfma": None, "jq1_v2_n128": (192, 128, 64)}
    for (m, n, t) in sorted(out, key=lambda s: s[1] * s[2]):
        for b in jq1:
            if jq1[b] is None and b in dg.expected_route(1, m, n, t):
                jq1[b] = (m, n, t)
    assert all(jq1.values()), jq1
    for b, s in jq1.items():
        assert b in dg.expected_route(1, *s), (b, s)
        if s not in out:
            out.append(s)
    banded = set(jq1.values())
    return tuple((m, n, t, (m, n, t) in banded) for (m, n, t) in out)


@functools.lru_cache(maxsize=None)
def _cases() -> tuple:
    out = []
    for kind in KINDS_J:
        for (m, n) in shapes_of(kind):
            out.append(_case("grid", kind, m, n))
    for (m, n) in [s for s in shapes_of("zerocols") if s[1] > 64][:2]:     # a whole zero panel: the two smallest shapes that have one
        out.append(_case("grid", "zerocols", m, n, variant="panel"))
    for k in (1, 2):                                              # the live rows are the short last tile, k zero tiles above it
        out.append(_case("grid", "lastrows", 512 * k + live_rows(24), 24, variant="short"))
    for tag, (m, n), kw in forced_variants():
        for kind in KINDS_J:
            tile = 256 if (kw.get("tile_rows") == 256 or m <= 256) else 512
            if applies(kind, m, n, tile) and (tag in WIDE_VARIANTS or kind in ("upper", "tileblock", "zerocols")):
                out.append(_case(tag, kind, m, n, **kw))
    for (m, n, t, with_banded) in a_shapes():
        for kindA in KINDS_A:
            for kindJ in ("dense", "banded") if with_banded else ("dense",):
                dup = kindA == "bounds_dup"
                out.append(_case("form", kindJ, m, n, t, kindA=kindA, rank_deficient=dup))
    ids = [c["id"] for c in out]
    assert len(ids) == len(set(ids)), ids
    return tuple(out)


def cases() -> list:
    return list(_cases())


def batch_case():
    m, n = BATCH_SHAPE
    return _case("five", "mixed", m, n, batch=len(BATCH_KINDS), kinds=BATCH_KINDS)


def ragged_case():
    # a ragged launch is planned for its smallest t_k: no route is claimed (tests/factor_identities.py: the `ragged` case)
    return _case("ragged", "dense", RAGGED["m"], RAGGED["n"], max(RAGGED["t_list"]), kindA="bounds", batch=len(RAGGED["t_list"]),
                 t_list=RAGGED["t_list"], want=set())


# ---- references, computed once and shared ----------------------------------------------------------------------------------------
_solved = {}


def solved(c, k=0):
    """((J, rx, A, cx), the oracle's solution) of problem k of a case"""
    key = (c["id"], k)
    if key not in _solved:
        P = build(c, k)
        _solved[key] = (P, go.gn_subproblem(*P))
    return _solved[key]


@functools.lru_cache(maxsize=None)
def health_problem(shape):
    P = synth.make_problem(4242, *shape)
    return P, go.gn_subproblem(*P)


def structural_drop(c, k=0) -> list:
    """0-based columns of J2 the rank decision must drop by structure (t = 0 cases: J2 = J)"""
    kind = c["kinds"][k] if c["kinds"] else c["kindJ"]
    if kind == "zerocols":
        return zero_columns(c["n"], c["variant"])
    if kind == "mixed_scale":
        return tiny_columns(c["n"])
    return []


def J2_of(ref, J):
    return ref.F_A.rmul_Q(J)[:, ref.rankA:] if ref.rankA else np.asarray(J)


def cond_kept(ref, J) -> float:
    """condition of the columns of J2 the rank decision kept"""
    keep = ref.jpvtJ2[:ref.rankJ2] - 1
    M = J2_of(ref, J)[:, keep]
    if M.size == 0:
        return 1.0
    s = np.linalg.svd(M, compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else math.inf


# ---- the exact checks, shared by the host test (on the oracle's factors, clean and mutated) and the GPU test ----------------------
def check_zero_columns(F, p, rankJ2, zero_cols, n2):
    """zerocols, t = 0: the rank is the number of non-zero columns, the dropped positions hold exactly the zero columns with
    diag R == 0.0, and p is exactly 0.0 on them"""
    z = sorted(zero_cols)
    assert rankJ2 == n2 - len(z), ("rankJ2", rankJ2, n2 - len(z))
    jp = np.asarray(F.p)
    assert sorted((jp[rankJ2:] - 1).tolist()) == z, ("dropped columns", sorted((jp[rankJ2:] - 1).tolist()), z)
    dR = np.asarray(F.diagR())
    assert np.all(dR[rankJ2:] == 0.0), ("diag R on the dropped positions", dR[rankJ2:])
    assert np.all(np.asarray(p)[z] == 0.0), ("p on the zero columns", np.asarray(p)[z])


def check_pass_through(F, d, rx, kp, seed):
    """upper, t = 0: every reflector of the sweep is the identity (tau = 0 makes T = 0 and each update C - V 0), and the pivoted QR
    of R0 works on rows 0 .. kp-1 only: rows kp .. m-1 go through Q' and Q unchanged, bit for bit, and |d| = |rx| there"""
    m = np.asarray(rx).size
    v = synth.normal_stream(seed, 23, m)
    qt, q = np.asarray(F.Qt_mul(v)), np.asarray(F.Q_mul(v))
    bad_t, bad_q = int((qt[kp:] != v[kp:]).sum()), int((q[kp:] != v[kp:]).sum())
    bad_d = int((np.abs(np.asarray(d)[kp:]) != np.abs(np.asarray(rx)[kp:])).sum())
    print(f"pass-through rows {kp}..{m - 1}: Q'v differs on {bad_t}, Qv on {bad_q}, |d| from |rx| on {bad_d}", flush=True)
    assert bad_t == 0 and bad_q == 0 and bad_d == 0, (bad_t, bad_q, bad_d)


def zero_tile_rows(J, tile) -> list:
    """the first and last row of every row tile of J that is zero in every column"""
    m = J.shape[0]
    out = []
    for r0 in range(0, m, tile):
        r1 = min(r0 + tile, m)
        if not J[r0:r1].any():
            out += sorted({r0, r1 - 1})
    return out


def check_bounds(F_A, p, A, cx, ref, kindA):
    """bounds, bounds_tied: LAPACK's pivots (the idamax rule where they tie), the explicit Q_A against LAPACK's entries in
    {0, +-1}, feasibility, and the bound itself.  Returns (worst |Q_A - LAPACK's|, feasibility, worst relative error of p[i_k])."""
    t, n = A.shape
    jp = np.asarray(F_A.p)
    assert np.array_equal(jp, ref.jpvtA), ("jpvtA", jp, ref.jpvtA)
    I = np.eye(n)
    QA = np.column_stack([F_A.Q_mul(I[:, j]) for j in range(n)])
    QL = ref.F_A.Q_mul(I)
    # dlarfg scales x by fl(1 / (alpha - beta)): a fl(1 / a) is 1 or 1 - 2^-53, so LAPACK's own entries sit within one ulp of {0, +-1}
    assert float(np.abs(QL - np.round(QL)).max()) <= fi.EPS and np.array_equal(np.abs(np.round(QL)).sum(axis=0), np.ones(n)), \
        "LAPACK's Q_A is not a signed permutation"
    dq = float(np.abs(QA - QL).max())
    p = np.asarray(p)
    feas = float(np.linalg.norm(A @ p + cx) / (np.linalg.norm(A, 2) * np.linalg.norm(p) + np.linalg.norm(cx)))
    cols = np.abs(A).argmax(axis=1)
    a = A[np.arange(t), cols]
    want = -cx / a
    # relative to the largest bound value: H = I - v v' forms x_j + s x_i and subtracts, so an entry of 1e-5 beside entries of order 1
    # carries eps of THOSE — LAPACK's own p reaches 9.0e-13 entry by entry (|cx_k| = 2.7e-5, host test) and 1.5e-16 in this measure
    ep = float(np.abs(p[cols] - want).max() / np.abs(want).max())
    ent = float((np.abs(p[cols] - want) / np.abs(want)).max())
    print(f"{kindA}: |Q_A - LAPACK's| {dq:.2e}, feasibility {feas:.2e}, p[i_k] against -cx_k / a_k {ep:.2e} of the largest "
          f"(entry by entry {ent:.2e})", flush=True)
    assert dq <= fi.TOL_COL and feas <= 1e-13 and ep <= 1e-13, (dq, feas, ep)
    return dq, feas, ep
