"""The premises of tests/newton_cases.py, certified on the CPU; every assertion is about the inputs and the references, never about
the library.  Per case: the oracle finds the literal (rankA, n2, kp) of the table; the verdict of every member has its margin in
FP64 and in the high-precision sW22 (a `fail(k)` member fails at exactly k in a right-looking, a left-looking and the
high-precision Cholesky); the longdouble restatement is held to mpmath where both run; the constant of the bound is measured; the
FP64 restatement of the kernels' decomposition meets the bound and four defects of it miss it on a named case.  Run with -s to see
the margins, kappa, the reference used and the measured constant of every case."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import newton_cases as nc  # noqa: E402
import newton_reference as nr  # noqa: E402
from test_gpu_parity import _newton_reference  # noqa: E402  (a plain function; importing the module needs no GPU)

CASES = nc.cases()
IDS = [c["id"] for c in CASES]


def rel(a, b):
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


def pivots(S):
    """the pivots of an unblocked right-looking Cholesky in natural order, up to and including the first that is not > 0"""
    A = np.array(S, dtype=np.float64)
    out = []
    for k in range(A.shape[0]):
        out.append(A[k, k])
        if not A[k, k] > 0.0:
            break
        A[k + 1:, k] /= np.sqrt(A[k, k])
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k])
    return out


def test_the_table_reaches_its_cuts():
    n2s = {nc.literal(c, k)[1] for c in CASES for k in range(len(c["members"]))}
    assert {15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 97, 128, 129} <= n2s
    assert any(c["form"] == 1 and nc.literal(c, 0)[1] == 64 for c in CASES)              # two full panels on one wave
    assert any(c["form"] == 0 and min(c["n"], nc.t_max(c)) >= 65 for c in CASES)         # reflector loops that start past 0
    assert any(c["form"] == 0 and c["n"] % 8 == 1 for c in CASES)                        # a last workgroup of one vector
    kps = {nc.literal(c, 0)[2] for c in CASES if nc.literal(c, 0)[2] < nc.literal(c, 0)[1]}
    assert kps == {16, 17, 33}
    for n, t in [(64, 0), (65, 0), (134, 5)]:
        got = {mb["kind"][1] for c in CASES if c["n"] == n for mb in c["members"] if mb["kind"][0] == "fail" and mb["t"] == t}
        assert got == {k for k in (0, 15, 16, 31, 32, 33, 63, 64, 65, n - t - 1) if k < n - t}, (n, t, got)
    assert not nc.ADVANCED_SEEDS or all(v > 0 for v in nc.ADVANCED_SEEDS.values())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_premises(c):
    if not nr.LD_OK:
        print("np.longdouble is narrower than the x87 extended format here: mpmath is the reference of every case")
    assert c["form"] == nr.expected_newton_form(c["n"])
    for k, mb in enumerate(c["members"]):
        prob, ref, Gam = nc.member(c, k)
        rankA, n2, kp = nc.literal(c, k)
        assert (ref.rankA, c["n"] - ref.rankA, min(c["m"], c["n"] - ref.rankA)) == (rankA, n2, kp), (c["id"], k, ref.rankA)
        if mb["maker"] == "wide_rankdefA":
            assert mb["t"] >= c["n"] > ref.rankA
        cert = nc.certificate(c, k)
        want = nc.expected_fail_index(c, k)
        if not nc.has_reference(c):
            # no high-precision reference (newton_cases.has_reference): the verdict is certified in every basis of null(A) instead
            left = cert["fail_index"]
            print(f"{c['id']}[{k}] {mb['kind']}: reference none  n2 {n2} kp {kp}  lam_min(J2'J2) {cert['lamJ']:.3e}  "
                  f"||sym Gamma|| {cert['nG']:.3e}  ||J2||^2 {cert['nJ2']:.3e}  kappa (any basis) <= {cert['kappa']:.3e}")
            assert want == -1 == left == nc.right_looking(cert["sW"])[1]
            assert cert["lamJ"] >= 4.0 * cert["nG"] and cert["lam_min"] >= cert["lamJ"] - cert["nG"] - 1e-9 * cert["nJ2"]
            assert nc.bound(cert["kappa"]) <= nc.MAX_BOUND
            continue
        hi = nc.reference(c, k)
        piv = pivots(cert["sW"])
        right = len(piv) - 1 if not piv[-1] > 0.0 else -1
        blocked = nc.right_looking(cert["sW"])[1]
        print(f"{c['id']}[{k}] {mb['kind']}: reference {'mpmath' if nc.uses_mpmath(c) else 'longdouble'}  n2 {n2} kp {kp}  "
              f"lam_min {cert['lam_min']:.3e}  ||J2||^2 {cert['nJ2']:.3e}  ||sym E22|| {cert['nE22']:.3e}  kappa {cert['kappa']:.3e}  "
              f"verdict index {right}")
        assert right == blocked == cert["fail_index"] == hi.fail_index == want, (c["id"], k, right, blocked, cert["fail_index"], hi.fail_index)
        assert hi.error == (want >= 0) and not hi.undefined
        if want < 0:
            floor = 1e4 * nc.U * (cert["nJ2"] + cert["nE22"])
            assert cert["lam_min"] >= floor and hi.lam_min >= floor, (c["id"], k, cert["lam_min"], hi.lam_min, floor)
            assert nc.bound(cert["kappa"]) <= nc.MAX_BOUND, (c["id"], k, cert["kappa"])
        elif mb["kind"][0] == "fail":
            assert piv[-1] <= -1e-3 * cert["norm"] and min(piv[:-1], default=1.0) >= 0.5, (c["id"], k, piv[-1], min(piv[:-1], default=1.0))
            assert abs(piv[-1] + 0.05) <= 1e-9 and max(abs(x - 1.0) for x in piv[:-1] + [1.0]) <= 1e-9
        else:
            assert np.isnan(piv[-1]) and np.all(np.isfinite(piv[:-1]))


SMALL = [c for c in CASES if c["n"] <= 40 and c["m"] <= 300 and nc.has_reference(c)]


@pytest.mark.skipif(not nr.LD_OK, reason="np.longdouble is narrower than the x87 extended format: mpmath is the only reference here")
def test_longdouble_restatement_against_mpmath():
    """The longdouble restatement held to mpmath at 1e-17 relative, on every member small enough for both.  (One longdouble per
    value returns u_ld kappa, 1.03e-10 on graded-n33-t0[2] at kappa 4.2e9; the restatement therefore carries pairs of
    longdoubles, and the two references round to the same FP64 p on every member.)"""
    worst = (0.0, "")
    for c in SMALL:
        for k in range(len(c["members"])):
            a, b = nc.reference(c, k, mpm=False), nc.reference(c, k, mpm=True)
            assert a.error == b.error and a.fail_index == b.fail_index
            e = rel(a.p, b.p)
            kap = nc.certificate(c, k)["kappa"]
            print(f"{c['id']}[{k}]: longdouble against mpmath {e:.2e}  kappa {kap:.2e}")
            worst = max(worst, (e, f"{c['id']}[{k}]"))
    print("worst:", worst)
    assert worst[0] <= 1e-17, worst


def test_constant():
    """the FP64 restatement of the reference's lines against the high-precision reference, in units of u kappa"""
    worst = (0.0, "")
    for c in CASES:
        for k in range(len(c["members"])):
            if nc.expected_status(c, k) or not nc.has_reference(c):
                continue
            prob, ref, Gam = nc.member(c, k)
            p64, e64 = _newton_reference(*prob, Gam)
            hi = nc.reference(c, k)
            assert not e64 and not hi.error
            kap = nc.certificate(c, k)["kappa"]
            mult = rel(p64, hi.p) / (nc.U * max(kap, 1.0))
            print(f"{c['id']}[{k}]: rel {rel(p64, hi.p):.3e}  kappa {kap:.3e}  multiple of u kappa {mult:.3f}")
            worst = max(worst, (mult, f"{c['id']}[{k}]"))
    print(f"worst multiple {worst[0]:.3f} on {worst[1]}; times 8: {8 * worst[0]:.1f}; C_EDGE {nc.C_EDGE}")
    assert 8.0 * worst[0] <= nc.C_EDGE, worst
    assert worst[0] <= 2.0 * nc.WORST_MULTIPLE, worst        # the recorded figure; another BLAS moves it by a few roundings


def reference_p(c, k):
    """the high-precision p; without one (newton_cases.has_reference), the reference's lines in FP64 on the same oracle factors"""
    if nc.has_reference(c):
        return nc.reference(c, k).p
    prob, ref, Gam = nc.member(c, k)
    p, err = _newton_reference(*prob, Gam)
    assert not err
    return p


def model_misses(c, mutate):
    """the members of a case on which the restated kernels (with a defect) give another status or miss the bound"""
    out = []
    for k in range(len(c["members"])):
        prob, ref, Gam = nc.member(c, k)
        with np.errstate(invalid="ignore"):
            p, st = nc.kernel_model(prob, ref, Gam, mutate)
        if st != nc.expected_status(c, k):
            out.append(k)
        elif st == 0 and not rel(p, reference_p(c, k)) <= nc.bound(nc.certificate(c, k)["kappa"]):
            out.append(k)
        elif st == 1 and p.any():
            out.append(k)
    return out


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restated_kernels_meet_the_bound(c):
    assert model_misses(c, None) == []


MUTATIONS = [
    ("tile_row", ["edge-n33-t0", "edge-n49-t0", "edge-n38-t5", "edge-n102-t5", "edge-n134-t5"]),
    ("kmax4", ["kp17-n40-t0", "kp33-n40-t0", "kp33-n70-t5"]),
    ("late_pivot", ["fail-n64-t0-k32_33", "fail-n65-t0-k63_64", "fail-n134-t5-k65_128"]),
    ("no_perm", ["perm-n40-t44-rank23", "perm-n40-t44-rank7", "perm-n70-t72-rank37"]),
]


@pytest.mark.parametrize("mutate,named", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_defect_of_the_restated_kernels_misses_a_named_case(mutate, named):
    for cid in named:
        missed = model_misses(nc.case(cid), mutate)
        print(f"{mutate}: {cid} members {missed}")
        assert missed, (mutate, cid)
