"""The magnitude cases of the row-sharded TSQR, shared by tests/test_tsqr_scaled_host.py (which proves each case's premise from the
oracle alone) and tests/test_gpu_tsqr_magnitudes.py (which runs them on the device).  Not a test module.

A case is a seeded ordinary problem whose inputs are multiplied by exact powers of two; `build` returns the scaled inputs, the rank
threshold, the row blocks and what the oracle (real LAPACK) is expected to find."""
from dataclasses import dataclass

import numpy as np

from oracle import gn_oracle as go, synth

# name -> (n, t, row blocks).  n = 96: several 512-row tiles with a ragged last one in the whole matrix and in block 0, and a block
# shorter than n2 (kp = m_loc = 64 < n2); n = 40 with 300-row blocks: the one-tile local stage.
SHAPES = {
    "n96_t0": (96, 0, (1100, 700, 64)),
    "n96_t8": (96, 8, (1100, 700, 64)),
    "n40_t0": (40, 0, (300, 300, 300)),
}

# name -> needs constraints
CASES = {
    "all_up_600": False,             # 1. (J, rx) 2^600
    "all_down_600": False,           # 2. (J, rx) 2^-600, default eps_rank: the absolute test makes rankJ2 = 0
    "all_down_600_small_eps": False,  # 3. (J, rx) 2^-600, eps_rank = 2^-700: full rank
    "J_up_600": False,               # 4. J 2^600, rx ordinary
    "window_505": False,             # 5. (J, rx) 2^505: above the nomination threshold 2^440, R still finite
    "A_up_600": True,                # 6a. (A', cx) 2^600, J ordinary
    "A_and_J_up_600": True,          # 6b. both
    "mixed_shards": False,           # 7. the rows of block 0 times 2^600, the other blocks ordinary
}
BITWISE = {"all_up_600": 600, "all_down_600_small_eps": -600, "window_505": 505}     # case -> power of two of (J, rx)


def case_ids():
    return [(s, c) for s in SHAPES for c, needs_t in CASES.items() if SHAPES[s][1] > 0 or not needs_t]


@dataclass
class Case:
    J: np.ndarray
    rx: np.ndarray
    A: np.ndarray
    cx: np.ndarray
    eps_rank: float
    blocks: tuple
    rankJ2_full: bool        # the oracle is expected to find J2 of full rank (else rank 0)
    probe: np.ndarray        # a column of ONE shard whose plain sum of squares leaves the range
    premise: str             # "inf", "zero", or "nominated" (finite, but the column norm is above 2^440)
    base: tuple              # the unscaled J, rx, A, cx


def build(shape: str, case: str) -> Case:
    n, t, blocks = SHAPES[shape]
    m = sum(blocks)
    J0, rx0, A0, cx0 = synth.make_problem(88000 + 7 * n + t, m, n, t)
    A0 = np.asarray(A0, dtype=np.float64).reshape(t, n)
    J, rx, A, cx = J0, rx0, A0, cx0
    eps, full, premise = go.SQRT_EPS, True, "inf"
    b0 = blocks[0]
    if case == "all_up_600":
        J, rx = np.ldexp(J0, 600), np.ldexp(rx0, 600)
    elif case == "all_down_600":
        J, rx, full, premise = np.ldexp(J0, -600), np.ldexp(rx0, -600), False, "zero"
    elif case == "all_down_600_small_eps":
        J, rx, eps, premise = np.ldexp(J0, -600), np.ldexp(rx0, -600), 2.0 ** -700, "zero"
    elif case == "J_up_600":
        J = np.ldexp(J0, 600)
    elif case == "window_505":
        J, rx, premise = np.ldexp(J0, 505), np.ldexp(rx0, 505), "nominated"
    elif case == "A_up_600":
        A, cx = np.ldexp(A0, 600), np.ldexp(cx0, 600)
    elif case == "A_and_J_up_600":
        A, cx, J, rx = np.ldexp(A0, 600), np.ldexp(cx0, 600), np.ldexp(J0, 600), np.ldexp(rx0, 600)
    elif case == "mixed_shards":
        J, rx = J0.copy(), rx0.copy()
        J[:b0], rx[:b0] = np.ldexp(J0[:b0], 600), np.ldexp(rx0[:b0], 600)
    else:
        raise KeyError(case)
    probe = A[0] if case == "A_up_600" else J[:b0, 0]           # a column of A' (replicated) / of block 0 of J
    return Case(J, rx, A, cx, eps, blocks, full, probe, premise, (J0, rx0, A0, cx0))


def safe_norm(x):
    """||x||_2 as (mantissa part, exponent): the norm of x 2^-k with k the exponent of the largest entry, and k — NumPy's own norm
    squares plainly and overflows at these magnitudes."""
    x = np.asarray(x, dtype=np.float64)
    big = np.abs(x).max() if x.size else 0.0
    if not big > 0.0:
        return 0.0, 0
    k = int(np.frexp(big)[1])
    return float(np.linalg.norm(np.ldexp(x, -k))), k


def check_against_oracle(out, ref, tag, lead_rows=None, pivots=True):
    """ranks, code, pivots on the leading rankJ2 positions, p to 1e-11, |dlead| to 1e-10 of its largest entry, d_norm to 1e-12
    (the tolerances of tests/test_gpu_parity.py); `out`: a TSQRResult.  `lead_rows`: compare only that many leading entries of
    dlead (default: all n2) — for a J2 whose pivoted QR truncates (tests/tsqr_edge_cases.py): beyond rankJ2 the reflectors are built
    from rounding dust, so the entries of Q'd there belong to an arbitrary basis and only their norm (inside d_norm) is defined.
    `pivots=False`: do not compare jpvtJ2 — for a rank-deficient A (code -1), where J2 itself is defined only up to an orthogonal
    factor on its right (tsqr_edge_cases.comparable)."""
    n2 = ref.p.size - ref.rankA
    nl = n2 if lead_rows is None else int(lead_rows)
    assert (out.rankA, out.rankJ2, out.code) == (ref.rankA, ref.rankJ2, ref.code), tag
    r = ref.rankJ2
    if pivots:
        assert np.array_equal(np.asarray(out.jpvtJ2)[:r], ref.jpvtJ2[:r]), tag
    else:
        assert sorted(np.asarray(out.jpvtJ2).tolist()) == list(range(1, n2 + 1)), tag
    assert np.all(np.isfinite(out.p)), tag
    np_ref = np.linalg.norm(ref.p)
    err_p = float(np.linalg.norm(out.p - ref.p) / (np_ref if np_ref > 0 else 1.0))
    lead_ref = np.abs(ref.d[:nl])
    _, k = safe_norm(lead_ref)
    err_l = float(np.abs(np.ldexp(np.abs(out.dlead[:nl]), -k) - np.ldexp(lead_ref, -k)).max() / np.ldexp(lead_ref, -k).max()) if nl else 0.0
    nd, kd = safe_norm(ref.d)
    err_d = abs(float(np.ldexp(out.d_norm, -kd)) - nd) / nd
    print(f"{tag}: rel p {err_p:.2e}  lead {err_l:.2e}  d_norm {err_d:.2e}  ranks ({out.rankA}, {out.rankJ2})", flush=True)
    assert err_p <= 1e-11, (tag, err_p)
    assert err_l <= 1e-10, (tag, err_l)
    assert err_d <= 1e-12, (tag, err_d)
