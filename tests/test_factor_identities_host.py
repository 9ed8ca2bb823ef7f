"""tests/factor_identities.py on the CPU: the case list reaches every route bit it can, the checker passes on the oracle's LAPACK
factors of every case (the reference floor behind the GPU tolerances), and it FAILS for each way an accessor could be subtly
wrong — a negated row of R (which the magnitude comparisons of the older tests let through), a tau or an entry of R off by 1e-9, two
pivots swapped, a reflector beyond column 32 dropped, the entries of Q'v beyond k zeroed."""
import numpy as np
import pytest

import dispatch_grid as dg
import factor_identities as fi
from oracle import gn_oracle as go


def test_case_list_covers_every_reachable_route_bit():
    names = set(dg.header_route_names())
    cs = fi.cases()
    by_rule = [c for c in cs if c["id"].startswith(("cover", "kind"))]
    assert all(c["batch"] <= fi.BATCH_CAP and c["m"] * c["n"] <= fi.SIZE_CAP for c in by_rule)
    assert fi.covered_bits(by_rule) == fi.reachable_bits()
    # below the size cap, on default handles: everything but the bits another test asserts and the bits that need a large batch
    assert names - fi.covered_bits(by_rule) == set(dg.COVERED_ELSEWHERE) | fi.NEED_LARGE_BATCH == {
        "jq1_rows64", "jq1_plain", "sweep_reflectors", "sweep_lookahead", "sweep_xmap", "sweep_upper_input", "pivot_steps", "chunked",
        "rescaled", "pipeline_split", "sweep_pairs"}
    # with the forced variants and the batch of 128: what no case of this list reaches at all
    assert fi.covered_bits(cs) <= names
    assert names - fi.covered_bits(cs) == {"jq1_rows64", "sweep_lookahead", "sweep_xmap", "sweep_upper_input", "chunked", "rescaled"}
    # every kind of the grid that fits, every forced variant, the index cases
    pool_kinds = {(c["batch"], c["m"], c["n"], c["t"], c["kind"]) for c in dg.grid()
                  if c["kind"] != "full" and c["batch"] <= fi.BATCH_CAP and c["m"] * c["n"] <= fi.SIZE_CAP}
    assert pool_kinds <= {(c["batch"], c["m"], c["n"], c["t"], c["kind"]) for c in by_rule}
    tags = [c["id"].split("-")[0] for c in cs]
    for tag, cnt in (("pairs", 2), ("tile256", 1), ("reflectors", 1), ("steps", 1), ("unfused", 1), ("index", 1), ("halves", 1), ("ragged", 1)):
        assert tags.count(tag) == cnt, tag
    pairs = [c for c in cs if c["id"].startswith("pairs")]
    assert sorted(fi._npan(c) % 2 for c in pairs) == [0, 1] and all(fi._npan(c) >= 3 for c in pairs)
    assert any(c["t"] == 0 for c in cs) and any(c["m"] < c["n"] - c["t"] for c in cs) and any(c["t"] > 64 for c in cs)
    assert any((c["m"], c["n"], c["t"]) == (1100, 513, 0) or fi._kp(c) > 512 for c in cs)


def _solve_oracle(c, k):
    J, rx, A, cx = fi.problem(c, k)
    return (J, rx, A, cx), go.gn_subproblem(J, rx, A, cx)


def test_reference_floor_over_every_case():
    """The checker on the oracle's factors, every case and checked problem: the worst residual of each identity is the reference
    floor.  It must stay below the floors the GPU tolerances are built from (factor_identities.FLOOR_*)."""
    worst = {}
    for c in fi.cases():
        for k in c["probs"]:
            (J, rx, A, cx), ref = _solve_oracle(c, k)
            res = fi.check_solve_identities(fi.OracleAccess(ref, J), J, rx, A, cx, ref, kind=c["kind"])
            fi.assert_within(res, c["kind"], (c["id"], k))
            for key, v in res.items():
                if v > worst.get(key, (-1.0, None))[0]:
                    worst[key] = (v, c["id"])
    for key in sorted(worst):
        print(f"reference floor {key:9s} {worst[key][0]:.2e}  ({worst[key][1]})")
    col = max(worst[k][0] for k in worst if k.endswith((".qt", ".q")) or k in ("orth", "W", "JQ1"))
    gram = max(worst[k][0] for k in worst if k.endswith(".gram"))
    print(f"floors: columns {col:.2e}, Gram {gram:.2e}, d {worst['d'][0]:.2e}")
    assert col <= fi.FLOOR_COL and gram <= fi.FLOOR_GRAM
    # d: the graded kind is bounded with its conditioning term (assert_within above); the floor is that of the other kinds
    assert fi.TOL_COL <= fi.CAP_COL and fi.TOL_GRAM <= fi.CAP_GRAM_D and fi.TOL_D <= fi.CAP_GRAM_D


def test_reference_floor_of_d_without_the_graded_kind():
    worst = 0.0
    for c in fi.cases():
        if c["kind"] == "graded":
            continue
        k = c["probs"][-1]
        (J, rx, A, cx), ref = _solve_oracle(c, k)
        acc = fi.OracleAccess(ref, J)
        # only the d chain (cols=[]: no column of a factor is walked again)
        res = fi.check_solve_identities(acc, J, rx, A, cx, ref, kind=c["kind"], cols=[])
        worst = max(worst, res["d"])
    print(f"reference floor of d, kinds full / rankdefA / rankdefJ: {worst:.2e}")
    assert worst <= fi.FLOOR_D


# ---- mutations -------------------------------------------------------------------------------------------------------------------
class Mutated:
    """A QRPivoted seen through one wrong accessor."""

    def __init__(self, F, what):
        self.F, self.what = F, what
        self.tau = F.tau.copy()
        k = F.k
        if what == "tau":
            self.tau[min(5, k - 1)] *= 1.0 + 1e-9
        if what == "drop":
            assert k > 40 and self.tau[40] != 0.0
            self.tau[40] = 0.0                       # H_41 = I in dormqr: the reflector is skipped in both directions
        self.G = go.QRPivoted(F.factors, self.tau, F.jpvt)

    @property
    def R(self):
        R = self.F.R.copy()
        if self.what == "row":
            R[min(3, R.shape[0] - 1), :] *= -1.0
        if self.what == "entry":
            off = np.abs(np.triu(R, 1))
            i, j = np.unravel_index(np.argmax(off), off.shape)
            R[i, j] *= 1.0 + 1e-9
        return R

    def diagR(self):
        return self.R.diagonal().copy()

    @property
    def p(self):
        p = self.F.p.copy()
        if self.what == "pivots":
            p[[0, 1]] = p[[1, 0]]
        return p

    def Qt_mul(self, v):
        out = self.G.Qt_mul(v)
        if self.what == "tail":
            out[self.F.k:] = 0.0
        return out

    def Q_mul(self, v):
        return self.G.Q_mul(v)


class MutatedAccess(fi.OracleAccess):
    def __init__(self, ref, J, what, which=fi.FACTOR_J2):
        super().__init__(ref, J)
        self.what, self.which = what, which

    def factor(self, which):
        F = super().factor(which)
        return Mutated(F, self.what) if which == self.which else F


def _mutation_cases():
    """By rule from the grid: the smallest two-panel-sized tall case with a reflector beyond column 40 (32 < kp <= 64 <= m) and
    the smallest wide one (m < n2) with kp > 40."""
    one = sorted((c for c in dg.grid() if c["batch"] == 1 and c["kind"] == "full"), key=lambda c: c["m"] * c["n"])
    tall = next(c for c in one if 40 < fi._kp(c) <= 64 and c["m"] >= c["n"] - c["t"] + 8)
    wide = next(c for c in one if c["m"] < c["n"] - c["t"] and fi._kp(c) > 40)
    return [fi._case(tall, "tall"), fi._case(wide, "wide")]


@pytest.mark.parametrize("what", ["row", "tau", "entry", "pivots", "drop", "tail"])
@pytest.mark.parametrize("shape", [0, 1], ids=["two_panels", "wide"])
def test_checker_fails_for_each_mutation(what, shape):
    """Each mutation on F_J2, through the whole chain.  `tail` on the wide case: F_J2 has m = k rows there, nothing lies beyond
    k and the mutation is the identity — it is asserted to be exactly that (no case can see it), the tall case carries it."""
    c = _mutation_cases()[shape]
    (J, rx, A, cx), ref = _solve_oracle(c, 0)
    clean = fi.check_solve_identities(fi.OracleAccess(ref, J), J, rx, A, cx, ref)
    fi.assert_within(clean, "full")
    if what == "tail" and shape == 1:
        assert ref.F_J2.rows == ref.F_J2.k
        v = np.arange(1.0, ref.F_J2.rows + 1)
        assert np.array_equal(Mutated(ref.F_J2, "tail").Qt_mul(v), ref.F_J2.Qt_mul(v))
        return
    res = fi.check_solve_identities(MutatedAccess(ref, J, what), J, rx, A, cx, ref)
    with pytest.raises(AssertionError):
        fi.assert_within(res, "full")
    seen = {k for k, v in res.items() if k != "d_cond" and v > 10 * max(clean[k], 1e-15)}
    print(what, c["id"], {k: f"{res[k]:.1e}" for k in sorted(seen)})
    expect = {"row": {"J2.qt", "J2.q"}, "tau": {"J2.qt", "J2.q"}, "entry": {"J2.gram"}, "pivots": {"J2.qt", "J2.q", "J2.gram"},
              "drop": {"J2.qt", "J2.q"}, "tail": {"d"}}[what]
    assert expect <= seen, (expect, seen)
    # the older magnitude comparison (|R| against |R_ref|, ||Q'v|| = ||v||) lets the negated row through
    if what == "row":
        assert np.array_equal(np.abs(Mutated(ref.F_J2, "row").R), np.abs(ref.F_J2.R))


def test_truncated_factorisation_form_of_the_checker():
    """rows_defined: a factorisation stopped after r steps (R rows and reflectors beyond r undefined) passes with rows_defined = r
    and fails without it."""
    c = _mutation_cases()[0]
    (J, rx, A, cx), ref = _solve_oracle(c, 0)
    F = ref.F_J2
    r = F.k - 7
    tau = F.tau.copy()
    tau[r:] = 0.0
    fac = F.factors.copy(order="F")
    fac[r:, r:] = 1.0                                     # never reduced
    T = go.QRPivoted(fac, tau, F.jpvt)
    J2 = ref.F_A.rmul_Q(J)[:, ref.rankA:]
    assert max(fi.check_factor_identity(T, J2, rows_defined=r)) <= fi.TOL_COL
    assert max(fi.check_factor_identity(T, J2)) > 1e-3
