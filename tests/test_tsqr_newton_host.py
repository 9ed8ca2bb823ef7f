"""Host certification of tests/tsqr_newton_cases.py (no GPU): for every case a NumPy restatement of the SHARDED formulation of the
Newton direction — R, Pi and d from a pivoted QR of the stacked per-shard triangles, then E, Pi R'R Pi', -E21 p1 + Pi R' d[1:kp],
Cholesky and the solves — meets the high-precision reference on the whole matrix within newton_reference.newton_bound(cond), the bound
tests/test_gpu_tsqr_newton.py holds the library to.  The labelled kinds hold (numpy.linalg.cholesky raises exactly on the indefinite
cases, the late-pivot construction fails at the intended pivot), and leaving one shard's triangle out of the stack leaves the bound
on every positive-definite case (negative control)."""
import numpy as np
import pytest

import newton_reference as nr
import tsqr_newton_cases as tc

NAMES = list(tc.CASES)


def test_the_entry_point_is_declared_and_wrapped():
    """the C ABI, the ctypes table and the Python wrappers name the call"""
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    hdr = (root / "include" / "enlsip_gn.h").read_text()
    assert "int enlsip_gn_tsqr_newton_direction(" in hdr and "int enlsip_gn_tsqr_newton_direction_dev(" in hdr
    import sys
    sys.path.insert(0, str(root / "enlsip.jl_amd" / "python"))
    from enlsip_gn import _lib, tsqr
    assert "enlsip_gn_tsqr_newton_direction" in _lib.PROTOTYPES and "enlsip_gn_tsqr_newton_direction_dev" in _lib.PROTOTYPES
    assert callable(tsqr.tsqr_newton_direction_lib) and callable(tsqr.tsqr_newton_direction_dev)


def test_shapes_cover_the_cuts():
    from enlsip_gn import tsqr
    assert callable(tsqr.tsqr_newton_direction_lib)
    for with_t in (False, True):
        got = {c.n - c.t for c in tc.CASES.values() if c.kind == "pd" and (c.t > 0) == with_t}
        assert got >= {1, 31, 32, 33, 64, 65, 97, 257}, (with_t, got)
    assert {c.G for c in tc.CASES.values()} == {1, 3}
    for c in tc.CASES.values():
        if c.G > 1:
            assert len(set(c.heights)) > 1 and (c.n == 1 or min(c.heights) < c.n or c.n <= 2), c.name


@pytest.mark.parametrize("name", NAMES)
def test_restatement_meets_the_reference(name):
    from enlsip_gn import tsqr
    assert callable(tsqr.tsqr_newton_direction_lib)
    c = tc.CASES[name]
    J, rx, A, cx, Gam, ref = tc.build(name)
    R = tc.reference(name)
    assert not R.undefined
    assert ref.rankA == (c.n if c.kind == "full_A" else c.n - 2 if c.kind == "wide_A" else c.t)
    if c.kind == "rankdefJ":
        assert ref.rankJ2 == c.n - c.t - 3
    if c.kind in tc.INDEFINITE_KINDS:
        assert R.error and np.all(R.p == 0.0)
        want = 0 if c.kind == "indef_first" else tc.LATE_PIVOT
        assert R.fail_index == want, (R.fail_index, want)
        # the construction in FP64: the leading block is positive definite and the next pivot is not
        k, S = nr.cholesky_fail_index(R.sW)
        assert k == want
        if want:
            np.linalg.cholesky(R.sW[:want, :want])
            assert want >= 32, "the verdict must fall behind the first panel"
        with pytest.raises(np.linalg.LinAlgError):
            tc.sharded_restatement(J, rx, A, cx, Gam, ref, c.heights)
        return
    assert not R.error
    p, sW = tc.sharded_restatement(J, rx, A, cx, Gam, ref, c.heights)
    err, bound = tc.rel(p, R.p), nr.newton_bound(R.cond)
    print(f"{name}: rel {err:.3e} bound {bound:.3e} cond {R.cond:.3e}")
    assert bound <= 1e-4, "a bound this wide checks nothing"
    assert err <= bound, (name, err, bound)
    if c.kind == "full_A":
        assert np.array_equal(p, (ref.F_A.Q_mul(np.eye(c.n)).T @ ref.p)[:c.n])
    if c.kind == "zero":       # the Gauss-Newton direction
        assert tc.rel(ref.p, R.p) <= bound, (tc.rel(ref.p, R.p), bound)


@pytest.mark.parametrize("name", [n for n in NAMES if tc.CASES[n].kind in tc.POSDEF_KINDS])
def test_a_dropped_shard_leaves_the_bound(name):
    from enlsip_gn import tsqr
    assert callable(tsqr.tsqr_newton_direction_lib)
    c = tc.CASES[name]
    J, rx, A, cx, Gam, ref = tc.build(name)
    R = tc.reference(name)
    bound = nr.newton_bound(R.cond)
    with_p = 0
    for g in range(c.G):
        try:
            p, _ = tc.sharded_restatement(J, rx, A, cx, Gam, ref, c.heights, drop=g)
        except np.linalg.LinAlgError:
            left = True               # what is left of sW22 is not positive definite: no p at all
        else:
            with_p += 1
            left = tc.rel(p, R.p) > bound
        assert left, (name, g, tc.rel(p, R.p), bound)
    if c.G > 1:                       # with shards left in the stack the control must have compared a p, not only caught a raise
        assert with_p >= 1, name
