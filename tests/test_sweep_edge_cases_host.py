"""tests/sweep_edge_cases.py on the CPU: the table's traces contain every edge value its families name and no case can be removed
without losing one; every case stays within the size limits; the full-column checker passes on the oracle's LAPACK factors of
every case under the floors of tests/factor_identities.py (the reference floor behind the tolerances of
tests/test_gpu_sweep_edges.py); and it FAILS for a column of R inside a partial 32-column block off by 1e-9 — a column the sampled
checker never looks at — and for the last 32 rows of d off by 1e-9."""
import functools
import time

import numpy as np
import pytest

import factor_identities as fi
import sweep_edge_cases as se
from oracle import gn_oracle as go

CASES = se.cases()


def test_constants_come_from_the_sources():
    assert (se.PB, se.CW, se.XMAP_MAX_BATCH, se.XMAP_MIN_TILES, se.NEAR_PAIR, se.NEAR_PLAIN, se.PAIR_MIN_WGS) == (32, 32, 8, 16, 2, 1, 8192)


def test_every_named_edge_is_in_some_trace_and_no_case_is_idle():
    req = se.required_edges()
    per_case = [se.edges(c, se.trace_of(c)) for c in CASES]
    have = set().union(*per_case)
    assert not req - have, sorted(req - have)
    for i, c in enumerate(CASES):
        rest = set().union(*(e for j, e in enumerate(per_case) if j != i))
        assert req - rest, f"{c['id']} covers nothing the other cases do not"
    assert len(CASES) <= 45
    assert {c["family"] for c in CASES} == set("ABCDE")


def test_traces_say_what_the_issue_lists():
    """Spot checks of the restated sweep against figures worked out by hand from run_caqr."""
    by = {c["id"]: se.trace_of(c) for c in CASES}
    # n2 = 128 on 600 rows, look-ahead forced: the first pair's far window of 65 columns is 64 near columns (two full blocks) and
    # the right-hand side alone on the second stream: 0 column blocks plus its own block
    tr = by["D-pairs-b1-600x131-t3"]
    assert [(L["window"], L["stream"], L["ncb"], L["ny"], L["skip_rhs"]) for L in tr[:2]] == [
        ((0, 64, 64, False), "A", 2, 2, False), ((64, 0, 1, True), "B", 0, 1, True)]
    assert tr[0]["problems"][0]["forms"] == ["full", "full"]
    # n2 = 97 (even count, second panel of the last pair one column wide): 34 far columns = a full block and a two-column block
    tr = by["A-r33-b1-1024x100-t3"]
    assert (tr[0]["nfar"], tr[0]["skip_rhs"], tr[0]["problems"][0]["forms"]) == (34, False, ["full", "le16"])
    assert (tr[1]["nfar"], tr[1]["bwb"], tr[1]["skip_rhs"], tr[1]["ncb"]) == (1, 1, True, 0)
    # 17 tiles: one tile into the third octet, 7 padding workgroups per column block
    tr = by["C-octet-b2-8193x103-t3"]
    assert (tr[0]["tiles"], tr[0]["xmap"], tr[0]["xpad"], tr[0]["nvu_last"]) == (17, 17, 7, 1)
    assert by["C-octet-b9-8192x99-t3"][0]["xmap"] == 0 and by["C-octet-b1-7680x83-t3"][0]["xmap"] == 0
    # mixed: the companion launch serves the problem whose J2 ends with the first panel, the pair kernel the two others
    tr = by["E-mixed-b3-400x100-t4.40.68"]
    assert [L["kind"] for L in tr] == ["pair", "companion", "single"] and tr[0]["ny"] == tr[1]["ny"] == (65 - 1) // 32 + 1     # ntrail = 65
    assert [P["n2"] for P in tr[0]["problems"]] == [96, 60] and [P["n2"] for P in tr[1]["problems"]] == [32]


def test_size_limits_and_build_time(record_property):
    t0 = time.perf_counter()
    for c in CASES:
        assert c["m"] * c["n"] <= se.SIZE_CAP and c["batch"] <= se.BATCH_CAP, c["id"]
        for k in range(c["batch"]):
            _solved(c["id"], k)
    dt = time.perf_counter() - t0
    record_property("build_and_oracle_seconds", round(dt, 1))
    print(f"{len(CASES)} cases, {sum(c['batch'] for c in CASES)} problems: built and solved by the oracle in {dt:.1f} s")


@functools.lru_cache(maxsize=None)
def _solved(cid: str, k: int):
    c = next(c for c in CASES if c["id"] == cid)
    P = se.problem(c, k)
    return P, go.gn_subproblem(*P)


def _probs(c):
    """Every problem of a mixed batch (each has its own width), the first and the last of a uniform one."""
    return range(c["batch"]) if c["t_list"] else sorted({0, c["batch"] - 1})


def test_reference_floors_hold_over_every_column():
    worst = {}
    for c in CASES:
        for k in _probs(c):
            (J, rx, A, cx), ref = _solved(c["id"], k)
            res = fi.check_solve_identities(fi.OracleAccess(ref, J), J, rx, A, cx, ref, cols_J2=np.arange(c["n"] - ref.rankA))
            for key, v in res.items():
                if v > worst.get(key, (-1.0, None))[0]:
                    worst[key] = (v, c["id"])
    for key in sorted(worst):
        print(f"reference floor {key:9s} {worst[key][0]:.2e}  ({worst[key][1]})")
    col = max(worst[k][0] for k in worst if k.endswith((".qt", ".q")) or k in ("orth", "W", "JQ1"))
    gram = max(worst[k][0] for k in worst if k.endswith(".gram"))
    print(f"floors over the sweep edge table: columns {col:.2e}, Gram {gram:.2e}, d {worst['d'][0]:.2e}")
    assert col <= fi.FLOOR_COL, (col, fi.FLOOR_COL)
    assert gram <= fi.FLOOR_GRAM, (gram, fi.FLOOR_GRAM)
    assert worst["d"][0] <= fi.FLOOR_D, (worst["d"], fi.FLOOR_D)


# ---- checker mutations ----------------------------------------------------------------------------------------------------------
class _RColumnOff:
    """F_J2 with column j of R off by a relative 1e-9."""

    def __init__(self, F, j):
        self.F, self.j = F, j

    @property
    def R(self):
        R = np.array(self.F.R, copy=True)
        R[:, self.j] *= 1.0 + 1e-9
        return R

    def diagR(self):
        return self.R.diagonal().copy()

    @property
    def p(self):
        return self.F.p

    def Qt_mul(self, v):
        return self.F.Qt_mul(v)

    def Q_mul(self, v):
        return self.F.Q_mul(v)


class _Access(fi.OracleAccess):
    def __init__(self, ref, J, j):
        super().__init__(ref, J)
        self.j = j

    def factor(self, which):
        F = super().factor(which)
        return _RColumnOff(F, self.j) if which == fi.FACTOR_J2 else F


class _Out:
    def __init__(self, ref, d):
        self.p, self.d, self.rankA = ref.p, d, ref.rankA


def _mutation_case(family):
    """The family's case with the widest J2 (a column 32 b + 16 beyond the 96 the sampled checker walks in full)."""
    return max((c for c in CASES if c["family"] == family), key=lambda c: (c["n"] - min(c["t_list"] or [c["t"]]), -c["m"]))


@pytest.mark.parametrize("family", "ABCDE")
def test_full_column_checker_fails_where_the_sampled_one_is_blind(family):
    c = _mutation_case(family)
    (J, rx, A, cx), ref = _solved(c["id"], 0)
    n2 = c["n"] - ref.rankA
    assert n2 > 96, c["id"]
    sampled = set(fi.sample_columns(n2).tolist())
    inside = [j for j in range(16, n2, 32) if j not in sampled]
    assert inside, (c["id"], "every column 32 b + 16 is sampled")
    j = inside[-1]
    every = np.arange(n2)
    clean = fi.check_solve_identities(fi.OracleAccess(ref, J), J, rx, A, cx, ref, cols_J2=every)
    fi.assert_within(clean, "full")
    res = fi.check_solve_identities(_Access(ref, J, j), J, rx, A, cx, ref, cols_J2=every)
    print(c["id"], "column", j, {k: f"{v:.1e}" for k, v in res.items() if k.startswith("J2")})
    assert res["J2.qt"] > fi.TOL_COL and res["J2.q"] > fi.TOL_COL and res["J2.gram"] > fi.TOL_GRAM
    with pytest.raises(AssertionError):
        fi.assert_within(res, "full")
    # the sampled checker skips column j: its two column identities pass (the Gram identity, which needs no Q, walks every column)
    blind = fi.check_solve_identities(_Access(ref, J, j), J, rx, A, cx, ref)
    assert j not in sampled and blind["J2.qt"] <= fi.TOL_COL and blind["J2.q"] <= fi.TOL_COL
    # the last 32 rows of d off by 1e-9
    d = np.array(ref.d, copy=True)
    d[-32:] *= 1.0 + 1e-9
    res = fi.check_solve_identities(fi.OracleAccess(ref, J), J, rx, A, cx, _Out(ref, d), cols_J2=[])
    print(c["id"], "d tail", f"{res['d']:.1e}")
    assert res["d"] > fi.TOL_D
    with pytest.raises(AssertionError):
        fi.assert_within(res, "full")
