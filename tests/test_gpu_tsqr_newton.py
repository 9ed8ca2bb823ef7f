"""GPU tests of the Newton direction on a row-sharded J (enlsip_gn_tsqr_newton_direction, _dev) on the cases of
tests/tsqr_newton_cases.py, which tests/test_tsqr_newton_host.py certifies on the CPU.  Every case runs on a handle created with
ENLSIP_GN_NEWTON_WIDE=0 (the one-workgroup factorisation) and on one created with =1 (the device-wide one), and the form the library
reports is asserted for each.

1. agreement: within newton_reference.newton_bound(cond) of the high-precision reference on the whole matrix, the two forms within
   twice that of each other and of enlsip_gn_newton_direction after enlsip_gn_solve on the whole matrix; the verdict and p == 0 exact
   on the indefinite kinds, p == p1 exact for rankA == n.
2. repeatability: the call twice, the _dev form, and ldg > n give the same bits.
3. nothing disturbed: the enlsip_gn_tsqr_products family, the scale and the exchange record answer the same bits before and after,
   and a following enlsip_gn_solve_tsqr gives the bits of a fresh handle.
4. the refusals, each with nothing written to p.
5. one n2 = 1008 case under the device-wide form."""
import ctypes as C

import numpy as np
import pytest

import newton_reference as nr
import tsqr_newton_cases as tc
from oracle import gn_oracle as go

pytestmark = pytest.mark.gpu
EPS = go.SQRT_EPS
SENT = -7.25e77


def same(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def dev(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda:0")


def fp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture
def handle(monkeypatch):
    """handle(wide) -> a GNSolver created under ENLSIP_GN_NEWTON_WIDE=wide; all of them are closed after the test"""
    from enlsip_gn import GNSolver
    made = []

    def make(wide=None):
        if wide is None:
            monkeypatch.delenv("ENLSIP_GN_NEWTON_WIDE", raising=False)
        else:
            monkeypatch.setenv("ENLSIP_GN_NEWTON_WIDE", str(wide))       # read at handle creation
        s = GNSolver(device=0)
        made.append(s)
        return s
    yield make
    for s in made:
        s.close()


def expected_form(wide, n, n2=1):
    """2 where the device-wide factorisation ran; a call with n2 == 0 factors nothing and never reports it"""
    return 2 if (wide and n2 > 0) else (1 if n <= 64 else 0)


def sharded(s, name):
    from enlsip_gn.tsqr import tsqr_solve_shards
    c = tc.SHORT_A if name == tc.SHORT_A.name else tc.BIG if name == tc.BIG.name else tc.CASES[name]
    J, rx, A, cx, Gam, ref = tc.build(name)
    return tsqr_solve_shards(s, J, rx, A, cx, c.G, EPS, row_blocks=list(c.heights))


def raw_call(s, Gam_cm, ldg, p, bad=None):
    """the host form on a column-major image of Gamma with leading dimension ldg; returns the return code"""
    return s._lib.enlsip_gn_tsqr_newton_direction(s._h, fp(Gam_cm) if Gam_cm is not None else None, ldg,
                                                  fp(p) if p is not None else None, C.byref(bad) if bad is not None else None)


# ---- 1. agreement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.CASES))
def test_agreement_with_the_reference(handle, name):
    from enlsip_gn.tsqr import tsqr_newton_direction_lib
    c = tc.CASES[name]
    J, rx, A, cx, Gam, ref = tc.build(name)
    R = tc.reference(name)
    bound = nr.newton_bound(R.cond)
    whole = handle()
    whole.solve(J, rx, A, cx, EPS)
    p_whole, bad_whole = whole.newton_direction(Gam)
    got = {}
    for wide in (0, 1):
        s = handle(wide)
        out = sharded(s, name)
        assert out.rankA == ref.rankA and out.rankJ2 == ref.rankJ2, (out.rankA, out.rankJ2)
        p, bad = tsqr_newton_direction_lib(s, c.n, Gam)
        assert s.newton_form() == expected_form(wide, c.n, out.n2), (wide, s.newton_form())
        got[wide] = p
        if c.kind in tc.INDEFINITE_KINDS:
            assert bad and np.all(p == 0.0) and not np.any(np.signbit(p)), (name, wide)
            assert bad_whole
            continue
        assert not bad and not bad_whole
        err = tc.rel(p, R.p)
        print(f"{name} wide={wide}: rel {err:.3e} bound {bound:.3e}; to the whole-matrix call {tc.rel(p, p_whole):.3e}")
        assert err <= bound, (name, wide, err, bound)
        assert tc.rel(p, p_whole) <= 2 * bound, (name, wide, tc.rel(p, p_whole), 2 * bound)
        if c.kind == "zero":       # the Gauss-Newton direction of the sharded solve
            assert tc.rel(p, out.p) <= bound, (name, wide, tc.rel(p, out.p), bound)
        if c.kind == "full_A":
            # p1 as it is (:379-381), NOT F_A.Q p1: the sharded solve's own p is F_A.Q p1, so p is held to F_A.Q' of it within the
            # bound, and bit for bit to what the whole-matrix call copies out of the same constraint stage's p1
            assert out.n2 == 0 and same(p, p_whole)
            assert tc.rel(p, ref.F_A.Q_mul(np.eye(c.n)).T @ out.p) <= bound
    if c.kind not in tc.INDEFINITE_KINDS:
        assert tc.rel(got[0], got[1]) <= 2 * bound, (name, tc.rel(got[0], got[1]), 2 * bound)


def wide_threshold():
    """TSQR_NEWTON_WIDE_MIN_N2 of gn_tsqr_newton.inc"""
    import re
    mt = re.search(r"constexpr int TSQR_NEWTON_WIDE_MIN_N2\s*=\s*([0-9]+)\s*;", (nr.CSRC / "gn_tsqr_newton.inc").read_text())
    assert mt, "the default threshold was not found in gn_tsqr_newton.inc"
    return int(mt.group(1))


@pytest.mark.parametrize("name", ["pd_n33_G3", "pd_n37_t5", "pd_n64", "pd_n70_t5", "pd_n100_t3_G3"])
def test_default_form_follows_the_threshold(handle, name):
    """a handle created without the switch: the device-wide form from the measured n2 threshold on, inside the same bound"""
    from enlsip_gn.tsqr import tsqr_newton_direction_lib
    c = tc.CASES[name]
    s = handle()
    out = sharded(s, name)
    p, bad = tsqr_newton_direction_lib(s, c.n, tc.build(name)[4])
    assert s.newton_form() == expected_form(out.n2 >= wide_threshold(), c.n), (out.n2, s.newton_form())
    R = tc.reference(name)
    assert not bad and tc.rel(p, R.p) <= nr.newton_bound(R.cond)


# ---- 2. repeatability -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("name", ["pd_n33_G3", "pd_n40_t7_G3", "pd_n65_G3", "pd_n100_t3_G3", "indef_late_n97_G3", "full_A_n9_G3"])
def test_repeatability(handle, name, wide):
    import torch
    from enlsip_gn.tsqr import tsqr_newton_direction_lib, tsqr_newton_direction_dev
    c = tc.CASES[name]
    n = c.n
    Gam = tc.build(name)[4]
    s = handle(wide)
    n2 = sharded(s, name).n2
    p0, bad0 = tsqr_newton_direction_lib(s, n, Gam)
    p1, bad1 = tsqr_newton_direction_lib(s, n, Gam)
    assert same(p0, p1) and bad0 == bad1
    # the device form
    pd, st = tsqr_newton_direction_dev(s, n, dev(Gam.T))
    assert same(pd.cpu().numpy(), p0) and int(st.cpu()[0]) == int(bad0)
    assert s.newton_form() == expected_form(wide, n, n2)
    # ldg > n, both forms, the padding rows filled with a sentinel
    ldg = n + 3
    Gp = np.full((n, ldg), SENT)
    Gp[:, :n] = Gam.T                     # row c of the C-order image = column c of the column-major matrix
    p2, bad2 = np.full(n, SENT), C.c_int64(-1)
    assert raw_call(s, Gp, ldg, p2, bad2) == 0
    assert same(p2, p0) and bool(bad2.value) == bad0
    pd3 = torch.full((n,), SENT, dtype=torch.float64, device="cuda:0")
    tsqr_newton_direction_dev(s, n, dev(Gp), p_d=pd3, ldg=ldg)
    assert same(pd3.cpu().numpy(), p0)


# ---- 3. nothing disturbed ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("name", ["pd_n40_t7_G3", "pd_n100_t3_G3"])
def test_nothing_resident_is_disturbed(handle, name, wide):
    import torch
    from enlsip_gn.tsqr import (tsqr_solve_lib, tsqr_products_lib, tsqr_first_lagrange_lib, tsqr_second_lagrange_lib,
                                tsqr_newton_direction_lib, tsqr_scale, tsqr_exchange)
    c = tc.CASES[name]
    J, rx, A, cx, Gam, ref = tc.build(name)
    n, t = c.n, c.t
    Jd, rxd, Atd, cxd = dev(J.T), dev(rx), dev(A), dev(cx)       # the shard stays alive: the products read it
    torch.cuda.synchronize()

    def solve(s):
        out = tsqr_solve_lib(s, Jd, rxd, Atd, cxd, EPS)
        return [out.p, out.dlead, np.array([out.d_norm]), out.jpvtJ2.astype(np.float64), np.array([out.rankA, out.rankJ2, out.code], float)]

    def answers(s, p_gn):
        pr = tsqr_products_lib(s, n, t, p=p_gn)
        lam1, gres = tsqr_first_lagrange_lib(s, n, t)
        lam2 = tsqr_second_lagrange_lib(s, n, t, p_gn)
        ex = tsqr_exchange(s)
        return [pr.grad, pr.sums, pr.Ap, lam1, np.array([gres]), lam2, np.array(tsqr_scale(s), dtype=np.float64),
                np.array([ex["ranks"], ex["rank_tags_seen"]], dtype=np.float64)], ex["transport"]

    s = handle(wide)
    first = solve(s)
    before, tr0 = answers(s, first[0])
    p, bad = tsqr_newton_direction_lib(s, n, Gam)
    assert not bad and s.newton_form() == expected_form(wide, n)
    after, tr1 = answers(s, first[0])
    assert tr0 == tr1 and all(same(a, b) for a, b in zip(before, after))
    # the step can be taken again and gives the same bits: p1, the factors and the carried d are what they were
    p_again, _ = tsqr_newton_direction_lib(s, n, Gam)
    assert same(p, p_again)
    again = solve(s)
    fresh = solve(handle(wide))
    assert all(same(a, b) for a, b in zip(again, fresh)) and all(same(a, b) for a, b in zip(again, first))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [0, 1])
def test_refusals_write_nothing(handle, wide):
    from enlsip_gn.tsqr import tsqr_solve_shards, hip_local_stage
    import torch
    name = "pd_n40_t7_G3"
    c = tc.CASES[name]
    J, rx, A, cx, Gam, ref = tc.build(name)
    n = c.n
    G = np.ascontiguousarray(Gam.T)

    def refused(s, code, Gcm=G, ldg=n, with_p=True):
        p, bad = np.full(n, SENT), C.c_int64(-5)
        rc = raw_call(s, Gcm, ldg, p if with_p else None, bad)
        assert rc == code, (rc, code, s._lib.enlsip_gn_last_error(s._h))
        assert np.all(p == SENT) and bad.value == -5

    s = handle(wide)
    assert s._lib.enlsip_gn_tsqr_newton_direction(None, fp(G), n, fp(np.zeros(n)), None) == -1
    refused(s, -7)                                   # a fresh handle
    s.solve(J, rx, A, cx, EPS)
    refused(s, -7)                                   # after enlsip_gn_solve
    refused(s, -7, ldg=n - 1)                        # ... whatever ldg is: n belongs to a resident sharded solve only
    sharded(s, name)
    s.solve(J, rx, A, cx, EPS)
    refused(s, -7)                                   # ... which withdraws a sharded solve
    # a local stage without a combine
    Jd, rxd, Atd, cxd = dev(J.T), dev(rx), dev(A), dev(cx)
    Rl, zl = torch.empty(n * n, dtype=torch.float64, device="cuda:0"), torch.empty(n, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    hip_local_stage(s, c.m, n, c.t, Jd.data_ptr(), c.m, rxd.data_ptr(), Atd.data_ptr(), cxd.data_ptr(), Rl.data_ptr(), zl.data_ptr(), EPS)
    refused(s, -7)
    # argument errors on a resident sharded solve
    sharded(s, name)
    refused(s, -3, Gcm=None)
    refused(s, -4, ldg=n - 1)
    refused(s, -5, with_p=False)
    pd = torch.full((n,), SENT, dtype=torch.float64, device="cuda:0")
    st = torch.full((1,), -5, dtype=torch.int32, device="cuda:0")
    Gd = dev(G)
    torch.cuda.synchronize()
    lib = s._lib.enlsip_gn_tsqr_newton_direction_dev
    assert lib(s._h, None, n, C.c_void_p(pd.data_ptr()), C.c_void_p(st.data_ptr())) == -3
    assert lib(s._h, C.c_void_p(Gd.data_ptr()), n - 1, C.c_void_p(pd.data_ptr()), C.c_void_p(st.data_ptr())) == -4
    assert lib(s._h, C.c_void_p(Gd.data_ptr()), n, None, C.c_void_p(st.data_ptr())) == -5
    assert np.all(pd.cpu().numpy() == SENT) and int(st.cpu()[0]) == -5
    # a rescaled sharded solve
    tsqr_solve_shards(s, J * 2.0 ** 600, rx, A, cx, c.G, EPS, scaled=True, row_blocks=list(c.heights))
    refused(s, -15)
    # the rank-deficient working set with t < n
    sa = tc.SHORT_A
    assert tc.reference(sa.name).undefined
    out = sharded(s, sa.name)
    assert out.rankA == sa.t - 1 and out.code == -1
    Gs = np.ascontiguousarray(tc.build(sa.name)[4].T)
    p, bad = np.full(sa.n, SENT), C.c_int64(-5)
    assert raw_call(s, Gs, sa.n, p, bad) == -8
    assert np.all(p == SENT) and bad.value == -5
    # and the handle still answers a legal call
    sharded(s, name)
    p, bad = np.full(n, SENT), C.c_int64(-5)
    assert raw_call(s, G, n, p, bad) == 0 and bad.value == 0
    assert tc.rel(p, tc.reference(name).p) <= nr.newton_bound(tc.reference(name).cond)


# ---- 5. the size the device-wide form exists for ----------------------------------------------------------------------------------
def test_n2_1008_under_the_device_wide_form(handle):
    from enlsip_gn.tsqr import tsqr_newton_direction_lib
    c = tc.BIG
    J, rx, A, cx, Gam, ref = tc.build(c.name)
    ev = np.linalg.eigvalsh(nr._sW22_oracle(J, A, ref, Gam))
    assert ev[0] > 0
    bound = nr.newton_bound(float(ev[-1] / ev[0]))
    whole = handle()
    whole.solve(J, rx, A, cx, EPS)
    p_whole, bad_whole = whole.newton_direction(Gam)
    assert not bad_whole
    s = handle(1)
    out = sharded(s, c.name)
    assert out.rankA == c.t and out.n2 == 1008
    p, bad = tsqr_newton_direction_lib(s, c.n, Gam)
    assert not bad and s.newton_form() == 2
    err = tc.rel(p, p_whole)
    print(f"n2 = 1008: to the whole-matrix call {err:.3e}, 2 x bound {2 * bound:.3e}")
    assert err <= 2 * bound, (err, 2 * bound)
