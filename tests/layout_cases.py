"""Padded and misaligned layouts of the caller's J and A' (test infrastructure, CPU only).

The library never copies the caller's device buffers: a device-form solve keeps (J, ldj, strideJ, rx, At, ldat, strideAt, cx) and
every later consumer reads the caller's memory through those numbers.  This module builds such buffers:

- `Layout(pad_j, pad_at, gap_j, gap_at, off_j, off_at)`: extra rows of the leading dimensions, extra doubles between problems,
  offset in doubles of the first problem from a 256-byte-aligned allocation;
- `place(problems, layout)` lays a batch out: every double that is not data is the quiet NaN `FILL` (rows m..ldj, the gaps, the
  doubles in front, a guard behind, and the constraint columns t_k..t_max of a ragged slot, which the header of
  enlsip_gn_solve_batched_ragged leaves unread); `unplace` inverts it;
- `v2_layout_ok` restates the layout guard of launch_jq1_v2 from its source line (a regex that fails loudly when the line
  changes); tests/dispatch_grid.py's expected_route takes it as its optional layout argument;
- `JQ1_CASES`, `BATCH_CASES`, `RAGGED_CASES`, `HOST_CASE`, `CONSUMER_CASES`: the smallest shapes that reach each reader."""
from __future__ import annotations

import functools
import re
from collections import namedtuple
from pathlib import Path

import numpy as np

import consumer_reference as cr
import dispatch_grid as dg
from oracle import synth

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "enlsip.jl_amd" / "csrc"

FILL = np.uint64(0x7FF8A5A5C3C30001)          # a quiet NaN with a payload no kernel produces
GUARD = 64                                    # doubles behind the last problem
ALLOC_ALIGN = 256                             # bytes: what the offsets count from

Layout = namedtuple("Layout", "pad_j pad_at gap_j gap_at off_j off_at")

# name -> (layout, meets the layout guard of launch_jq1_v2 for even m).  The parity of gap_j is the parity the table claims for
# strideJ: place() adds one double to a stride whose ldj * n would turn it round.
LAYOUTS = {
    "tight": (Layout(0, 0, 0, 0, 0, 0), True),
    "even": (Layout(8, 3, 10, 5, 0, 1), True),
    "odd_ld": (Layout(7, 3, 11, 5, 0, 1), False),          # ldj odd for even m
    "odd_stride": (Layout(8, 3, 11, 5, 0, 1), False),      # ldj even, strideJ odd
    "offset": (Layout(8, 3, 10, 5, 1, 1), False),          # J & 15 == 8
    "offset2": (Layout(8, 3, 10, 5, 2, 1), True),          # 16-byte aligned again, not 256
}
ALL_LAYOUTS = tuple(LAYOUTS)
CONSUMER_LAYOUTS = ("even", "odd_ld", "offset")


# ---- the builder ---------------------------------------------------------------------------------------------------------------
Placed = namedtuple("Placed", "J At rx cx ts B m n t_max ldj strideJ ldat strideAt off_j off_at")


def strides(layout: Layout, m: int, n: int, t_max: int):
    """(ldj, strideJ, ldat, strideAt) of a batch of m x n problems with up to t_max constraints"""
    ldj, ldat = m + layout.pad_j, max(n, 1) + layout.pad_at
    sJ = ldj * n + layout.gap_j
    if (sJ & 1) != (layout.gap_j & 1):
        sJ += 1
    return ldj, sJ, ldat, ldat * t_max + layout.gap_at


def _filled(count: int) -> np.ndarray:
    return np.full(count, FILL, dtype=np.uint64).view(np.float64)


def _view(buf, off, B, stride, cols, ld, rows):
    """(B, cols, rows) window: problem k's column c starts at entry off + k * stride + c * ld of the flat array"""
    w = buf.itemsize
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(B, cols, rows), strides=(stride * w, ld * w, w))


def place(problems, layout: Layout, t_max: int = None) -> Placed:
    """problems: [(J m x n, rx m, A t_k x n, cx t_k)], one (m, n).  Flat host arrays for J (column-major m x n per problem) and A'
    (column-major n x t_max per problem, columns t_k.. FILL) in `layout`, the tight rx (B, m) and cx (B, t_max; FILL past t_k)."""
    B = len(problems)
    m, n = problems[0][0].shape
    ts = np.array([P[2].shape[0] if P[2].size else 0 for P in problems], dtype=np.int64)
    t_max = int(ts.max()) if t_max is None else t_max
    ldj, sJ, ldat, sAt = strides(layout, m, n, t_max)
    Jb = _filled(layout.off_j + B * sJ + GUARD)
    Ab = _filled(layout.off_at + B * sAt + GUARD)
    cx = _filled(B * max(t_max, 1)).reshape(B, max(t_max, 1))[:, :t_max].copy()
    _view(Jb, layout.off_j, B, sJ, n, ldj, m)[...] = np.stack([np.asarray(P[0], dtype=np.float64).T for P in problems])
    Av = _view(Ab, layout.off_at, B, sAt, t_max, ldat, n)
    for k, P in enumerate(problems):
        if ts[k]:
            Av[k, :ts[k]] = P[2]
            cx[k, :ts[k]] = P[3]
    rx = np.stack([np.asarray(P[1], dtype=np.float64) for P in problems])
    return Placed(Jb, Ab, rx, cx, ts, B, m, n, t_max, ldj, sJ, ldat, sAt, layout.off_j, layout.off_at)


def unplace(pl: Placed):
    """the problems `place` was given"""
    Jv = _view(pl.J, pl.off_j, pl.B, pl.strideJ, pl.n, pl.ldj, pl.m)
    Av = _view(pl.At, pl.off_at, pl.B, pl.strideAt, pl.t_max, pl.ldat, pl.n)
    return [(Jv[k].T.copy(), pl.rx[k].copy(), Av[k, :pl.ts[k]].copy(), pl.cx[k, :pl.ts[k]].copy()) for k in range(pl.B)]


def data_mask(pl: Placed):
    """(mask over pl.J, mask over pl.At): True where a double is data"""
    mj, ma = np.zeros(pl.J.size, bool), np.zeros(pl.At.size, bool)
    _view(mj, pl.off_j, pl.B, pl.strideJ, pl.n, pl.ldj, pl.m)[...] = True
    for k in range(pl.B):
        for c in range(pl.ts[k]):
            o = pl.off_at + k * pl.strideAt + c * pl.ldat
            ma[o:o + pl.n] = True
    return mj, ma


# ---- the layout guard of the fast J*Q1 kernel, restated from its source -------------------------------------------------------------
_GUARD_RE = re.compile(r"if \(\(a\.ldj & (\d+)\) \|\| \(a\.strideJ & (\d+)\) \|\| \(\(size_t\)a\.J & (\d+)\)\) return false;")


def v2_guard_source() -> str:
    """the guard line of launch_jq1_v2, as written"""
    txt = (CSRC / "gn_kernels_q1_v2.hpp").read_text()
    body = txt[txt.index("inline bool launch_jq1_v2"):]
    found = _GUARD_RE.findall(body)
    assert len(found) == 1, "the layout guard of launch_jq1_v2 changed: restate it in tests/layout_cases.py"
    return _GUARD_RE.search(body).group(0)


def _guard_masks():
    return tuple(int(x) for x in _GUARD_RE.search(v2_guard_source()).groups())


def v2_layout_ok(ldj: int, strideJ: int, addr: int) -> bool:
    """True when launch_jq1_v2 accepts this layout of J (addr: the address in bytes of the first problem of the launch)"""
    a, b, c = _guard_masks()
    return not ((ldj & a) or (strideJ & b) or (addr & c))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# kind: "synth" -> synth.make_problem, "cr" -> consumer_reference.make_problem with kappa(A) = 10 (kappa 1 makes every row of A
# the same length, and the pivot order of A' a matter of rounding).  pipeline: the handles are created
# with ENLSIP_GN_PIPELINE=1, which splits the small uniform shapes (n <= 64, m <= 512) too.
Case = namedtuple("Case", "name B m n t_max ts layouts route kind seed pipeline")


def _case(name, B, m, n, t, layouts, route=(), ts=None, kind="synth", seed=0, pipeline=False):
    return Case(name, B, m, n, t, tuple(ts) if ts is not None else (t,) * B, tuple(layouts), frozenset(route), kind, seed, pipeline)


JQ1_CASES = [
    _case("v2_n128", 3, 256, 128, 64, ALL_LAYOUTS, {"jq1_v2_n128"}, seed=61000),
    _case("v2_n256", 3, 288, 256, 64, ALL_LAYOUTS, {"jq1_v2_n256"}, seed=61010),          # m % 64 != 0
    _case("v2_n384", 3, 416, 384, 64, ALL_LAYOUTS, {"jq1_v2_n384"}, seed=61020),
    _case("v2_n512", 3, 544, 512, 64, ALL_LAYOUTS, {"jq1_v2_n512"}, seed=61030),          # not a multiple of the 512-row tile
    _case("rows32", 3, 300, 20, 3, ALL_LAYOUTS, {"jq1_rows32"}, seed=61040),
    _case("rows2", 3, 300, 40, 6, ALL_LAYOUTS, {"jq1_rows2"}, seed=61050),
    _case("fused_small", 3, 256, 32, 4, ALL_LAYOUTS, {"jq1_fused_small"}, seed=61060),
    _case("mfma", 3, 700, 300, 100, ALL_LAYOUTS, {"jq1_mfma"}, seed=61070),               # general, t > 64
]
BATCH_CASES = [
    # 130 problems: the second pipeline half starts at J + 65 * strideJ.  (300, 40, 6) is a small uniform shape, which the library
    # splits only on a handle created with ENLSIP_GN_PIPELINE=1
    _case("split_rows2", 130, 300, 40, 6, CONSUMER_LAYOUTS, {"pipeline_split", "jq1_rows2"}, seed=62000, pipeline=True),
    _case("split_v2_n128", 130, 256, 128, 64, CONSUMER_LAYOUTS, {"pipeline_split"}, seed=62200),
    _case("chunked", dg.MAX_LAUNCH_BATCH + 1, 8, 4, 2, CONSUMER_LAYOUTS, {"chunked"}, seed=63000),
]
RAGGED_CASES = [
    _case("ragged", 5, 300, 40, 6, ("even", "odd_ld"), {"jq1_rows2"}, ts=[6, 0, 3, 1, 6], seed=64000),
]
HOST_CASE = _case("host_form", 3, 300, 40, 6, ("odd_ld",), {"jq1_rows2"}, seed=65000)
CONSUMER_CASES = [
    _case("wave", 3, 300, 40, 6, CONSUMER_LAYOUTS, {"jq1_rows2"}, kind="cr", seed=66000),
    _case("general", 3, 200, 70, 66, CONSUMER_LAYOUTS, {"jq1_mfma"}, kind="cr", seed=66010),      # the general form past 64
    _case("behind_v2", 3, 256, 128, 64, CONSUMER_LAYOUTS, {"jq1_v2_n128"}, kind="cr", seed=66020),
]
SOLVE_CASES = JQ1_CASES + BATCH_CASES + RAGGED_CASES
ALL_CASES = SOLVE_CASES + [HOST_CASE] + CONSUMER_CASES


@functools.lru_cache(maxsize=None)
def problems(case: Case):
    """the case's problems, made once and shared (treat as read-only)"""
    gen = functools.partial(cr.make_problem, kappa_A=10.0) if case.kind == "cr" else synth.make_problem
    out = []
    for k in range(case.B):
        J, rx, A, cx = gen(case.seed + k, case.m, case.n, case.ts[k])
        out.append((J, rx, A if case.ts[k] else np.zeros((0, case.n)), cx))
    return out


def seams(case: Case):
    """problems on both sides of the case's pipeline or chunk seam ([] when it has none)"""
    B = case.B
    if B > dg.MAX_LAUNCH_BATCH:
        nch = (B + dg.MAX_LAUNCH_BATCH - 1) // dg.MAX_LAUNCH_BATCH
        per = (B + nch - 1) // nch
        return [per - 1, per]
    if "pipeline_split" in case.route:
        return [(B + 1) // 2 - 1, (B + 1) // 2]
    return []


def resident_from(case: Case) -> int:
    """first problem of the chunk that stays resident"""
    return seams(case)[1] if case.B > dg.MAX_LAUNCH_BATCH else 0


def sample(case: Case):
    """the problems compared with the oracle: cr.sample_of the batch, and always the first, the last and both sides of a seam"""
    s = set(cr.sample_of(list(case.ts))) if case.B <= 8 else set()
    return sorted(s | {0, case.B - 1} | set(seams(case)))


def launch_bases(case: Case, pl: Placed, base_addr: int):
    """byte address of the first problem of every launch set of the solve: the batch, each pipeline half, each chunk"""
    starts = [0] + seams(case)[1:]
    return [base_addr + 8 * (pl.off_j + k * pl.strideJ) for k in starts]


def expected_route(case: Case, pl: Placed, base_addr: int) -> set:
    """dispatch_grid.expected_route under this layout.  A ragged batch picks its Jacobian-side kernels by its smallest t_k and its
    constraint kernels by t_max: only the J*Q1 bits on which the two agree are expected of it."""
    lay = (pl.ldj, pl.strideJ, launch_bases(case, pl, base_addr)[0])     # every launch set shares its answer (host test)
    if len(set(case.ts)) > 1:
        both = dg.expected_route(case.B, case.m, case.n, max(case.ts), layout=lay) & dg.expected_route(case.B, case.m, case.n, min(case.ts), layout=lay)
        return {b for b in both if b.startswith("jq1_")}
    r = dg.expected_route(case.B, case.m, case.n, case.t_max, layout=lay)
    if case.pipeline:
        r.add("pipeline_split")
    return r
