"""The degenerate-rank, short-shard and in-place cases of the row-sharded TSQR, shared by tests/test_tsqr_edges_host.py (which proves
each case's premise from the oracle and NumPy alone), tests/test_gpu_tsqr_edges.py (which runs them on the device) and
tests/tsqr_rank_worker.py (TSQR_CASES=edges: the message path with real ranks).  Not a test module.

A case is a seeded problem of oracle/synth.py at the smallest shape at which its branch of gn_tsqr.inc exists, the row blocks it is
sharded into, the rank threshold, and what the oracle (real LAPACK, unsharded) is expected to find, written as literals:
(rankA, code, n2, rankJ2)."""
from dataclasses import dataclass
from typing import Callable

import numpy as np

from oracle import gn_oracle as go, synth


def _zero_shard():
    J, rx, A, cx = synth.make_problem(SEEDS["tile_edges_n40_t3"], 1025, 40, 3)
    J, rx = J.copy(), rx.copy()
    J[513:1024] = 0.0             # block 1 of (513, 511, 1)
    rx[513:1024] = 0.0
    return J, rx, A, cx


SEEDS = {
    "rankdefA_n12_t6": 91012,
    "rankdefA_n96_t8_short": 91096,
    "rankdefA_n130_t40": 91130,
    "rankdefJ_n40_t6": 92040,
    "rankdefJ_n96_t8_short": 92096,
    "t_eq_n_9": 93009,
    "all_short_n24_t4": 94024,
    "tile_edges_n40_t3": 95040,
    "gate_n128_t64": 96128,
    "rankdefA_n40_t8_panel": 91040,
}


@dataclass(frozen=True)
class Case:
    name: str
    make: Callable             # () -> (J m x n, rx m, A t x n, cx t)
    blocks: tuple              # heights of the row blocks
    eps_rank: float
    expected: tuple            # (rankA, code, n2, rankJ2) of the oracle's unsharded solve
    in_place: bool = False     # also run with the shards as views J + lo, ldj = m
    branch: str = ""           # what of gn_tsqr.inc the case reaches


def _c(name, maker, shape, blocks, expected, in_place=False, branch=""):
    make = maker if shape is None else (lambda: maker(SEEDS[name], *shape))
    return Case(name, make, tuple(blocks), go.SQRT_EPS, tuple(expected), in_place, branch)


_ALL = [
    _c("rankdefA_n12_t6", synth.make_rank_deficient_A, (600, 12, 6), (300, 200, 100), (5, -1, 7, 7),
       branch="rankA < t: second attempt of the local pass with n2 = 7 > n - kA = 6, p1 of 5 entries through F_L11"),
    _c("rankdefA_n96_t8_short", synth.make_rank_deficient_A, (1864, 96, 8), (1100, 700, 64), (7, -1, 89, 89),
       branch="second attempt with a 64-row shard (kp = 64 < n2 = 89) and a ragged last 512-row tile"),
    _c("rankdefA_n130_t40", synth.make_rank_deficient_A, (1500, 130, 40), (700, 500, 300), (39, -1, 91, 91),
       branch="second attempt with the general F_A form (40 constraint reflectors, n > 128)"),
    # beyond the issue's table: n - kA = 32 is a whole panel of the CAQR, so n2 = 33 needs a panel more than the first attempt
    # launched.  In the three cases above both widths fall into the same panels and the first attempt's result is already right
    # (a library without the second attempt passes them); this is the smallest shape at which it is not.
    _c("rankdefA_n40_t8_panel", synth.make_rank_deficient_A, (600, 40, 8), (300, 200, 100), (7, -1, 33, 33),
       branch="second attempt that adds a CAQR panel: n2 = 33 against n - kA = 32"),
    _c("rankdefJ_n40_t6", synth.make_rank_deficient_J, (900, 40, 6), (300, 300, 300), (6, 1, 34, 31),
       branch="pivoted QR of the stack truncates (31 of 34); d splits between dlead and the combine tail"),
    _c("rankdefJ_n96_t8_short", synth.make_rank_deficient_J, (1864, 96, 8), (1100, 700, 64), (8, 1, 88, 85), in_place=True,
       branch="truncation of a stack whose last block has 64 rows of 88; in place at offsets 1100, 1800"),
    _c("t_eq_n_9", synth.make_problem, (400, 9, 9), (200, 150, 50), (9, 1, 0, 0),
       branch="n2 == 0: no stack, no sub-handle solve, d_norm from the local tails with kp = 0"),
    _c("all_short_n24_t4", synth.make_problem, (15, 24, 4), (5, 5, 5), (4, 1, 20, 15),
       branch="every shard shorter than n2 and m < n2: rankJ2 = m, zero fill of rows >= kp in every block"),
    _c("tile_edges_n40_t3", synth.make_problem, (1025, 40, 3), (513, 511, 1), (3, 1, 37, 37), in_place=True,
       branch="513, 511 and 1 rows: either side of the 512-row tile, a one-row shard; in place at offsets 513 (odd), 1024"),
    _c("zero_shard_n40_t3", _zero_shard, None, (513, 511, 1), (3, 1, 37, 37),
       branch="a shard of zeros: its triangle, z and tail are zero"),
]

# Beyond the issue's table: the one shape at which an in-place shard changes the J*Q1 kernel.  n = 128 and kA = 64 satisfy the
# shape part of launch_jq1_v2's gate; block 1 (64 rows) starts at row 33, so its base is 8-byte but not 16-byte aligned in place
# and 16-byte aligned as a contiguous copy.  In place only (the contiguous run is its partner).
GATE = _c("gate_n128_t64", synth.make_problem, (128, 128, 64), (33, 64, 31), (64, 1, 64, 64), in_place=True,
          branch="launch_jq1_v2's alignment gate: block 1 is 64 rows at an odd offset")

CASES = {c.name: c for c in _ALL}
IN_PLACE = [c.name for c in _ALL if c.in_place]
RANK_WORKER = ["rankdefA_n12_t6", "t_eq_n_9", "all_short_n24_t4", "rankdefJ_n40_t6"]       # tests/tsqr_rank_worker.py, TSQR_CASES=edges
REUSE_ORDER = ["rankdefA_n96_t8_short", "t_eq_n_9", "tile_edges_n40_t3", "rankdefA_n96_t8_short"]


def get(name: str) -> Case:
    return GATE if name == GATE.name else CASES[name]


def build(name: str):
    """(J, rx, A (t x n), cx) of a case."""
    J, rx, A, cx = get(name).make()
    n = J.shape[1]
    return J, rx, np.asarray(A, dtype=np.float64).reshape(-1, n), np.asarray(cx, dtype=np.float64)


def offsets(blocks):
    """First row of every block."""
    return [int(x) for x in np.concatenate([[0], np.cumsum(blocks)[:-1]])]


def comparable(ref):
    """What of the oracle's unsharded solve the inputs determine, as keywords of tsqr_magnitude_cases.check_against_oracle (the
    ranks, the code, p and d_norm always are).

    * A of full rank and J2 of full column rank: everything (all n2 entries of dlead, every pivot).
    * The pivoted QR of J2 truncates, or J2 has fewer rows than columns: the leading rankJ2 pivots and entries of dlead.  The later
      reflectors are built from rounding dust and the entries of Q'd there belong to an arbitrary basis: the NumPy restatement of
      the sharded algorithm itself differs from the unsharded oracle by 7e-2 (rankdefJ_n40_t6) and 5e-2 (rankdefJ_n96_t8_short) of
      the largest entry there, and the unsharded d of all_short_n24_t4 has 15 entries, not n2 = 20.
    * A rank deficient (code -1): neither pivots nor entries of dlead.  F_A.Q takes all min(n, t) reflectors, those of the dropped
      columns too, and these are built from rounding dust: J2 = (J F_A.Q)[:, rankA:] is defined up to an orthogonal factor on
      its right, which changes the pivot order and Q'd but neither p nor ||d|| (tests/test_gpu_parity.py compares the same way:
      "full-rank A: J2 is well defined, so are the leading pivots"; tests/test_tsqr_edges_host.py shows it on these cases)."""
    n2 = ref.p.size - ref.rankA
    if ref.code != 1:
        return {"lead_rows": 0, "pivots": False}
    return {"lead_rows": None if ref.rankJ2 == n2 else int(ref.rankJ2), "pivots": True}
