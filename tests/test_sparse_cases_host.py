"""CPU premises of tests/test_gpu_sparse_jacobians.py (cases: tests/sparse_cases.py), from NumPy, SciPy's LAPACK and the oracle
alone, so that a failure on the GPU means a kernel is wrong and not the case:

* oracle identities: the oracle solves every case, and factor_identities.check_solve_identities on its LAPACK factors stays within
  FLOOR_COL / FLOOR_GRAM / FLOOR_D — the floors behind the GPU tolerances hold on structural inputs too;
* the premises of the exact assertions, on LAPACK's own factors: an unpivoted dgeqrf of `upper` has tau == 0 everywhere and the
  oracle's F_J2 passes rows n.. through bit for bit; `zerocols` has rankJ2 = the number of non-zero columns, the zero columns in
  the last pivot positions with diag R == 0.0 and p == 0.0 there; `mixed_scale` squares below GN_TINY_NORM2 on its three columns,
  stays inside the magnitude window and drops exactly those columns; `bounds` / `bounds_tied` have an explicit Q_A with entries in
  {0, +-1}, jpvtA in the order of descending |a_k| / LAPACK's own, the same under a second call; `bounds_dup` has rank t - 1;
* tie freedom: the smallest relative lead of a chosen pivot of F_J2 over its runner-up (test_constraint_cases_host.smallest_lead);
  cases with leads >= LEAD_FLOOR = 2e-7 are `pivots_certified` and have jpvtJ2 compared on the device, and every kind keeps a
  certified case on every pivot form it reaches;
* teeth: on the oracle's factors an identity reflector replaced by tau = 2, a zero column's p entry set to 1e-9 and two tied pivots
  of bounds_tied exchanged each fail the checks the GPU test runs.

Measured here (pytest -s prints them; test_oracle_floors_over_every_case those of the current run): worst identity residual of the
oracle over the 153 cases 1.1e-15 columns (FLOOR_COL 2.5e-15) / 9.5e-16 Gram (FLOOR_GRAM 2.0e-15) / 6.4e-16 d (FLOOR_D 3.0e-15); two
cases needed their next seed to lead by 2e-7 (sparse_cases.SEED_SHIFT); LAPACK's Q_A of the bounds kinds is a signed permutation to
one ulp (a fl(1 / a) is 1 or 1 - 2^-53); LAPACK's p[i_k] is -cx_k / a_k within 1.5e-16 of the largest bound value and within 9.0e-13
entry by entry (|cx_k| = 2.7e-5 beside entries of order 1)."""
import math

import numpy as np
import pytest
import scipy.linalg

from oracle import gn_oracle as go

import dispatch_grid as dg
import factor_identities as fi
import sparse_cases as sc
import test_constraint_cases_host as cch

CASES = sc.cases()
IDS = [c["id"] for c in CASES]
LEAD_FLOOR = cch.LEAD_FLOOR
_res = {}


def identities(c) -> dict:
    """check_solve_identities on the oracle's factors of a case, computed once"""
    if c["id"] not in _res:
        (J, rx, A, cx), ref = sc.solved(c)
        _res[c["id"]] = fi.check_solve_identities(fi.OracleAccess(ref, J), J, rx, A, cx, ref)
    return _res[c["id"]]


def lead_of(c, k=0):
    (J, rx, A, cx), ref = sc.solved(c, k)
    if ref.rankJ2 == 0:
        return math.inf
    return cch.smallest_lead(sc.J2_of(ref, J), ref.jpvtJ2, ref.rankJ2)


_lead = {}


def pivots_certified(c, k=0) -> bool:
    """jpvtJ2 is compared with the oracle's on the device: every chosen pivot of F_J2 leads its runner-up by LEAD_FLOOR"""
    key = (c["id"], k)
    if key not in _lead:
        _lead[key] = lead_of(c, k)
    # a rank-deficient A leaves the columns of Q_A beyond rankA to rounding, and J2 with them: bounds_dup's
    # duplicate is exactly zero in LAPACK and a residue of 1e-16 where fl(1 / a) a != 1, so its last reflector is I or not
    return sc.solved(c, k)[1].code == 1 and _lead[key] >= LEAD_FLOOR


# ---- 1. the oracle's identities, the leads, the route premises ----------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_oracle_identities_and_leads(c):
    (J, rx, A, cx), ref = sc.solved(c)
    m, n, t = c["m"], c["n"], c["t"]
    assert m * n <= fi.SIZE_CAP and J.shape == (m, n) and A.shape == (t, n)
    res = identities(c)
    fi.assert_within(res, "full", c["id"])
    cert = pivots_certified(c)
    print(f"{c['id']}: rankA {ref.rankA} rankJ2 {ref.rankJ2} code {ref.code} lead {_lead[(c['id'], 0)]:.2e} certified {cert} "
          + " ".join(f"{k}={v:.1e}" for k, v in sorted(res.items())), flush=True)
    col = max(v for k, v in res.items() if k.endswith((".qt", ".q")) or k in ("orth", "W", "JQ1"))
    gram = max(v for k, v in res.items() if k.endswith(".gram"))
    assert col <= fi.FLOOR_COL and gram <= fi.FLOOR_GRAM and res["d"] <= fi.FLOOR_D, (c["id"], col, gram, res["d"])
    assert "rescaled" not in c["want"] and c["want"] <= set(dg.header_route_names())
    drop = sc.structural_drop(c)
    if t == 0:
        assert ref.rankJ2 == min(m, n) - len(drop), (c["id"], ref.rankJ2)
        assert sorted((ref.jpvtJ2[ref.rankJ2:] - 1).tolist()) == drop
    else:
        assert ref.rankJ2 == n - ref.rankA
    if c["kindA"]:
        assert (ref.rankA, ref.code) == ((t - 1, -1) if c["kindA"] == "bounds_dup" else (t, 1))
        assert ("second_attempt" in c["want"]) == (c["kindA"] == "bounds_dup")
    tile = sc.tile_height(m, c["want"])
    if c["kindJ"] == "tileblock":
        assert tile == c["tile"] and sc.applies("tileblock", m, n, tile)


def test_oracle_floors_over_every_case():
    WORST = {}
    for c in CASES:
        for key, v in identities(c).items():
            if v > WORST.get(key, (-1.0, None))[0]:
                WORST[key] = (v, c["id"])
    for key in sorted(WORST):
        print(f"oracle floor on structural inputs {key:9s} {WORST[key][0]:.2e}  ({WORST[key][1]})", flush=True)
    col = max(WORST[k][0] for k in WORST if k.endswith((".qt", ".q")) or k in ("orth", "W", "JQ1"))
    gram = max(WORST[k][0] for k in WORST if k.endswith(".gram"))
    print(f"floors: columns {col:.2e} (FLOOR_COL {fi.FLOOR_COL:.1e}), Gram {gram:.2e} ({fi.FLOOR_GRAM:.1e}), d {WORST['d'][0]:.2e} "
          f"({fi.FLOOR_D:.1e})", flush=True)
    assert col <= fi.FLOOR_COL and gram <= fi.FLOOR_GRAM and WORST["d"][0] <= fi.FLOOR_D


def test_case_list_follows_its_rules():
    names = set(dg.header_route_names())
    pool_sweeps = {sc.sweep_bits(dg.expected_route(1, m, n, 0)) for (m, n) in sc.shape_pool()}
    pool_pivots = {sc.pivot_bits(dg.expected_route(1, m, n, 0)) for (m, n) in sc.shape_pool()}
    for kind in ("upper", "zerocols", "mixed_scale"):             # the kinds that apply everywhere reach every set of the pool
        got = [c for c in CASES if c["kindJ"] == kind and c["tag"] == "grid" and not c["variant"]]
        assert {sc.sweep_bits(c["want"]) for c in got} == pool_sweeps and {sc.pivot_bits(c["want"]) for c in got} == pool_pivots, kind
    for kind in sc.KINDS_J:
        got = [c for c in CASES if c["kindJ"] == kind and c["tag"] == "grid" and not c["variant"]]
        assert [(c["m"], c["n"]) for c in got] == list(sc.shapes_of(kind)) and got, kind
        for c in got:
            assert sc.applies(kind, c["m"], c["n"], sc.tile_height(c["m"], c["want"])), c["id"]
        # every pivot form the kind reaches keeps a case whose pivots are compared with the oracle's
        for bits in {sc.pivot_bits(c["want"]) for c in got}:
            assert any(pivots_certified(c) for c in got if sc.pivot_bits(c["want"]) == bits), (kind, sorted(bits))
    tags = {c["tag"] for c in CASES}
    assert tags == {"grid", "pairs_odd", "pairs_even", "tile256", "reflectors", "steps", "fused", "unfused", "form"}
    for tag in tags - {"grid", "form"}:
        assert any(c["kindJ"] == "upper" for c in CASES if c["tag"] == tag), tag
    pairs = {c["tag"]: fi._npan(c) for c in CASES if c["tag"].startswith("pairs")}
    assert pairs["pairs_odd"] % 2 == 1 and pairs["pairs_even"] % 2 == 0 and min(pairs.values()) >= 3
    # zero columns on every pivot form of the issue: the one-wave forms, the LDS form, the register blocks, the launch-per-step form
    zc = [c for c in CASES if c["kindJ"] == "zerocols"]
    for bit in ("pivot_wave32", "pivot_wave64", "pivot_lds_r2", "pivot_blocks_128", "pivot_blocks_256", "pivot_hybrid", "pivot_steps"):
        assert any(bit in c["want"] for c in zc), bit
    assert "pivot_wave2" in dg.expected_route(len(sc.BATCH_KINDS), *sc.BATCH_SHAPE, 0) and "zerocols" in sc.BATCH_KINDS
    # the A kinds: every constraint form and every J*Q1 form, each with a dense J; a banded J on the J*Q1 shapes
    forms = [c for c in CASES if c["tag"] == "form"]
    for kindA in sc.KINDS_A:
        got = [c for c in forms if c["kindA"] == kindA]
        for f in cc_forms():
            assert any(f in c["want"] and c["kindJ"] == "dense" for c in got), (kindA, f)
        for b in ("jq1_fused_small", "jq1_rows32", "jq1_rows2", "jq1_mfma", "jq1_v2_n128"):
            assert any(b in c["want"] and c["kindJ"] == k for c in got for k in ("banded",)), (kindA, b)
            assert any(b in c["want"] and c["kindJ"] == "dense" for c in got), (kindA, b)
    assert all(c["want"] <= names for c in CASES)


def cc_forms():
    return sc.cc.FORMS


# ---- 2. the premises of the exact assertions ----------------------------------------------------------------------------------------
UPPER = [c for c in CASES if c["kindJ"] == "upper"]


@pytest.mark.parametrize("c", UPPER, ids=[c["id"] for c in UPPER])
def test_upper_has_identity_reflectors_in_lapack(c):
    (J, rx, A, cx), ref = sc.solved(c)
    m, n = J.shape
    (qr, tau), _ = scipy.linalg.qr(J, mode="raw")
    assert np.all(tau == 0.0) and np.array_equal(np.triu(qr)[:min(m, n)], J[:min(m, n)]), c["id"]
    s = np.linalg.svd(J, compute_uv=False)
    assert s[0] / s[-1] <= 10.0, (c["id"], s[0] / s[-1])
    kp = min(m, n)
    sc.check_pass_through(ref.F_J2, ref.d, rx, kp, c["seed"])


ZERO = [c for c in CASES if c["kindJ"] == "zerocols"]


@pytest.mark.parametrize("c", ZERO, ids=[c["id"] for c in ZERO])
def test_zero_columns_in_lapack(c):
    (J, rx, A, cx), ref = sc.solved(c)
    z = sc.zero_columns(c["n"], c["variant"])
    assert not J[:, z].any() and np.all(np.abs(np.delete(J, z, axis=1)).sum(axis=0) > 0)
    sc.check_zero_columns(ref.F_J2, ref.p, ref.rankJ2, z, c["n"])


MIXED = [c for c in CASES if c["kindJ"] == "mixed_scale"]


@pytest.mark.parametrize("c", MIXED, ids=[c["id"] for c in MIXED])
def test_mixed_scale_sits_below_the_reflector_threshold(c):
    (J, rx, A, cx), ref = sc.solved(c)
    tiny = sc.tiny_columns(c["n"])
    sq = (J[:, tiny] ** 2).sum(axis=0)
    assert np.all(sq > 0) and np.all(sq < sc.GN_TINY_NORM2), (c["id"], sq)
    amax = np.abs(J).max()
    assert 2.0 ** -400 <= amax <= 2.0 ** 400 and abs(ref.F_J2.R[0, 0]) >= 2.0 ** -440     # gn_rescale.hpp: never nominated
    assert ref.rankJ2 == c["n"] - len(tiny) and np.all(ref.p[tiny] == 0.0)


BOUNDS = [c for c in CASES if c["kindA"]]


@pytest.mark.parametrize("c", BOUNDS, ids=[c["id"] for c in BOUNDS])
def test_bounds_in_lapack(c):
    (J, rx, A, cx), ref = sc.solved(c)
    t, n = A.shape
    _, _, cols, a = sc.build_A(c["kindA"], c["seed"], n, t)
    assert np.count_nonzero(A) == t and np.array_equal(np.abs(A).argmax(axis=1), cols)
    if c["kindA"] == "bounds_dup":
        assert cols[t - 1] == cols[0] and len(set(cols.tolist())) == t - 1
        assert (ref.rankA, ref.code) == (t - 1, -1) and ref.F_A.diagR()[t - 1] == 0.0
        assert ref.jpvtA[0] == t and ref.jpvtA[t - 1] == 1            # the largest row first, its duplicate (zero after step one) last
        assert cch.smallest_lead(A.T, ref.jpvtA, t - 1) >= LEAD_FLOOR
        return
    assert len(set(cols.tolist())) == t
    QA = ref.F_A.Q_mul(np.eye(n))
    # entries in {0, +-1} to one ulp: dlarfg scales by fl(1 / (alpha - beta)), and a fl(1 / a) is 1 or 1 - 2^-53
    assert np.abs(QA - np.round(QA)).max() <= fi.EPS and np.array_equal(np.abs(np.round(QA)).sum(axis=0), np.ones(n))
    again = go.qr_colnorm(A.T)
    assert np.array_equal(again.jpvt, ref.jpvtA) and np.array_equal(again.factors, ref.F_A.factors)
    if c["kindA"] == "bounds":
        assert np.array_equal(ref.jpvtA, t - np.arange(t)), (c["id"], ref.jpvtA)          # descending |a_k|
        assert cch.smallest_lead(A.T, ref.jpvtA, t) >= LEAD_FLOOR
    else:
        assert np.array_equal(ref.jpvtA, np.arange(1, t + 1)), (c["id"], ref.jpvtA)        # idamax: the lowest position of a tie
        assert np.all(np.abs(ref.F_A.diagR()) == 1.0)
    # the bound itself, on the oracle: relative to the largest bound value (entry by entry LAPACK's own p is off by up to 9.0e-13
    # where |cx_k| = 2.7e-5 sits beside entries of order 1: H = I - v v' forms x_j + s x_i and subtracts)
    want = -cx / a
    print(f"{c['id']}: oracle p[i_k] against -cx_k / a_k: {np.abs(ref.p[cols] - want).max() / np.abs(want).max():.2e} of the largest, "
          f"{(np.abs(ref.p[cols] - want) / np.abs(want)).max():.2e} entry by entry", flush=True)
    assert np.abs(ref.p[cols] - want).max() <= 1e-13 * np.abs(want).max()


def test_batches_are_certified():
    for c in (sc.batch_case(), sc.ragged_case()):
        worst = {}
        for k in range(c["batch"]):
            (J, rx, A, cx), ref = sc.solved(c, k)
            res = fi.check_solve_identities(fi.OracleAccess(ref, J), J, rx, A, cx, ref)
            for key, v in res.items():
                worst[key] = max(worst.get(key, 0.0), v)
            assert pivots_certified(c, k), (c["id"], k)
            assert ref.rankJ2 == c["n"] - ref.rankA - len(sc.structural_drop(c, k))
        print(c["id"], {k: f"{v:.1e}" for k, v in sorted(worst.items())}, flush=True)
        assert max(v for k, v in worst.items() if k not in ("d", "d_cond") and not k.endswith(".gram")) <= fi.FLOOR_COL
        assert worst["d"] <= fi.FLOOR_D


# ---- 3. the tests have teeth ----------------------------------------------------------------------------------------------------------
def _first(pred):
    return next(c for c in CASES if pred(c))


def test_identity_reflector_replaced_by_a_sign_flip_fails():
    """LAPACK's unpivoted factors of `upper` (tau == 0 everywhere) seen as a factorisation with jpvt = identity: the identities hold;
    with one tau = 2 (H = I - 2 e e': the sign of that row flips) they fail, and the same mutation beyond kp breaks the pass-through."""
    c = _first(lambda c: c["kindJ"] == "upper" and c["tag"] == "grid" and c["m"] > c["n"] + 8 and pivots_certified(c))
    (J, rx, A, cx), ref = sc.solved(c)
    m, n = J.shape
    (qr, tau), _ = scipy.linalg.qr(J, mode="raw")
    F = go.QRPivoted(np.asfortranarray(qr), tau.copy(), np.arange(1, n + 1, dtype=np.int64))
    assert max(fi.check_factor_identity(F, J)) <= fi.FLOOR_COL
    sc.check_pass_through(F, F.Qt_mul(-rx), rx, 0, c["seed"])            # Q = I: every row passes through
    bad = tau.copy()
    bad[n // 2] = 2.0
    G = go.QRPivoted(np.asfortranarray(qr), bad, F.jpvt)
    res = fi.check_factor_identity(G, J)
    print(c["id"], "tau = 2 on an identity reflector:", res, flush=True)
    assert max(res[0], res[1]) > fi.TOL_COL
    with pytest.raises(AssertionError):
        sc.check_pass_through(G, G.Qt_mul(-rx), rx, 0, c["seed"])


def test_a_zero_column_with_a_small_p_fails():
    c = _first(lambda c: c["kindJ"] == "zerocols" and c["tag"] == "grid" and pivots_certified(c))
    (J, rx, A, cx), ref = sc.solved(c)
    z = sc.zero_columns(c["n"], c["variant"])
    sc.check_zero_columns(ref.F_J2, ref.p, ref.rankJ2, z, c["n"])
    p = ref.p.copy()
    p[z[0]] = 1e-9
    with pytest.raises(AssertionError):
        sc.check_zero_columns(ref.F_J2, p, ref.rankJ2, z, c["n"])


class _Swapped:
    """F_A with two pivots exchanged"""

    def __init__(self, F):
        self.F = F
        self.R, self.Q_mul, self.Qt_mul, self.diagR = F.R, F.Q_mul, F.Qt_mul, F.diagR
        self.p = F.p.copy()
        self.p[[2, 3]] = self.p[[3, 2]]


def test_two_tied_pivots_exchanged_fail():
    c = _first(lambda c: c["kindA"] == "bounds_tied" and c["kindJ"] == "dense" and pivots_certified(c) and c["t"] >= 8)
    (J, rx, A, cx), ref = sc.solved(c)
    sc.check_bounds(ref.F_A, ref.p, A, cx, ref, c["kindA"])
    with pytest.raises(AssertionError):
        sc.check_bounds(_Swapped(ref.F_A), ref.p, A, cx, ref, c["kindA"])
    assert max(fi.check_factor_identity(_Swapped(ref.F_A), A.T)) > fi.TOL_COL      # the identities see it too
