"""Every reader of the caller's J and A' on padded and misaligned layouts (tests/layout_cases.py).

A device-form solve keeps the caller's (J, ldj, strideJ, At, ldat, strideAt) and every later call reads the caller's memory through
them.  Each case is solved on buffers laid out by layout_cases.place (fill NaN in every double that is not data) and, on a fresh
handle, on tight buffers:

- the reported route contains dispatch_grid.expected_route under the layout: the fast J*Q1 kernel on the layouts that pass the guard
  of launch_jq1_v2, the general kernel and no V2 bit on the others;
- where both runs report the same route set, every output of every problem is bitwise the tight run's (a layout changes addresses,
  not the order of any sum); the constraint-stage outputs, which no J*Q1 kernel touches, always are;
- a sample (first, last, both sides of a pipeline or chunk seam) against the oracle with test_gpu_parity.compare at its TOL_P;
- the placed buffers are bytewise what was uploaded after all calls.

Then the consumers of the resident padded state: the batched products and multiplier estimates, the single-problem accessors at
the last slot, the changed-problems solve on slots rewritten in place, and the factored flow with a mixed refactor mask."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import consumer_reference as cr
import layout_cases as lc
import test_gpu_consumer_edges as ce
import test_gpu_parity as par
from oracle import gn_oracle as go, synth

pytestmark = pytest.mark.gpu
EPS = go.SQRT_EPS
DEV = "cuda:0"


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def make_handle(case):
    """a fresh handle; a `pipeline` case: one that splits the small uniform shapes too (read at creation)"""
    from enlsip_gn import GNSolver
    old = os.environ.get("ENLSIP_GN_PIPELINE")
    if case.pipeline:
        os.environ["ENLSIP_GN_PIPELINE"] = "1"
    try:
        return GNSolver(device=0)
    finally:
        if case.pipeline:
            if old is None:
                del os.environ["ENLSIP_GN_PIPELINE"]
            else:
                os.environ["ENLSIP_GN_PIPELINE"] = old


class Buffers:
    """a Placed batch on the device, and output buffers in the strides of the batched solves"""

    def __init__(self, pl):
        self.pl = pl
        self.J, self.At = torch.from_numpy(pl.J).to(DEV), torch.from_numpy(pl.At).to(DEV)
        self.rx, self.cx = torch.from_numpy(pl.rx).to(DEV), torch.from_numpy(np.ascontiguousarray(pl.cx)).to(DEV)
        assert self.J.data_ptr() % lc.ALLOC_ALIGN == 0 and self.At.data_ptr() % lc.ALLOC_ALIGN == 0
        self.want_J, self.want_At = pl.J.copy(), pl.At.copy()          # what the device buffers must still hold at the end
        B, m, n, t = pl.B, pl.m, pl.n, pl.t_max
        f = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=DEV)
        z = lambda *s: torch.zeros(s, dtype=torch.int64, device=DEV)
        self.out = dict(p=f(B, n), b=f(B, t), d=f(B, m), info=torch.full((B, 6), -7, dtype=torch.int64, device=DEV), jA=z(B, t),
                        jL=z(B, min(n, t)), jJ=z(B, n))

    @property
    def jptr(self):
        return self.J.data_ptr() + 8 * self.pl.off_j

    @property
    def aptr(self):
        return self.At.data_ptr() + 8 * self.pl.off_at if self.pl.t_max else 0

    def in_args(self):
        pl = self.pl
        return (self.jptr, pl.ldj, pl.strideJ, self.rx.data_ptr(), self.aptr, pl.ldat, pl.strideAt, self.cx.data_ptr() if pl.t_max else 0)

    def a_args(self):
        pl = self.pl
        return (self.aptr, pl.ldat, pl.strideAt, self.cx.data_ptr() if pl.t_max else 0)

    def out_args(self):
        o = self.out
        return dict(dp=o["p"].data_ptr(), db=o["b"].data_ptr(), dd=o["d"].data_ptr(), dinfo=o["info"].data_ptr(),
                    djA=o["jA"].data_ptr(), djL=o["jL"].data_ptr(), djJ=o["jJ"].data_ptr())

    def results(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def rewrite_slot(self, k, A, cx):
        """a new A (t_k x n) and cx for slot k, in place: the data entries only, the fill of the slot stays"""
        pl = self.pl
        for c in range(pl.ts[k]):
            o = pl.off_at + k * pl.strideAt + c * pl.ldat
            self.At[o:o + pl.n] = torch.from_numpy(np.ascontiguousarray(A[c])).to(DEV)
            self.want_At[o:o + pl.n] = A[c]
        self.cx[k, :pl.ts[k]] = torch.from_numpy(np.ascontiguousarray(cx)).to(DEV)

    def assert_inputs_untouched(self, tag):
        torch.cuda.synchronize()
        assert same(self.J.cpu().numpy(), self.want_J), (tag, "J")
        assert same(self.At.cpu().numpy(), self.want_At), (tag, "At")
        pl = self.pl
        gj, ga = self.J.cpu().numpy().view(np.uint64), self.At.cpu().numpy().view(np.uint64)
        assert np.all(gj[:pl.off_j] == lc.FILL) and np.all(gj[-lc.GUARD:] == lc.FILL) and np.all(ga[:pl.off_at] == lc.FILL)
        assert np.all(ga[-lc.GUARD:] == lc.FILL), tag


def solve(s, case, buf):
    """a device-form solve of the whole batch: ragged when the case is, (results, route)"""
    pl = buf.pl
    if len(set(case.ts)) > 1:
        s.solve_batched_ragged_dev(pl.B, pl.m, pl.n, pl.t_max, np.array(case.ts), *buf.in_args(), EPS, **buf.out_args())
    else:
        s.solve_batched_dev(pl.B, pl.m, pl.n, pl.t_max, *buf.in_args(), EPS, **buf.out_args())
    return buf.results(), s.route()


def diags(s, case):
    """diag R of the three factors of every resident problem"""
    from enlsip_gn import FACTOR_A, FACTOR_L11, FACTOR_J2
    r0 = lc.resident_from(case)
    return {w: s.diagR_batched(w, max(case.n, case.t_max), r0, case.B - r0) for w in (FACTOR_A, FACTOR_L11, FACTOR_J2)}


@functools.lru_cache(maxsize=None)
def oracle(case, k):
    return go.gn_subproblem(*lc.problems(case)[k])


@functools.lru_cache(maxsize=None)
def tight_run(case):
    """the case on tight buffers and a fresh handle, once for all its layouts: (results, route, diag R)"""
    s = make_handle(case)
    try:
        buf = Buffers(lc.place(lc.problems(case), lc.LAYOUTS["tight"][0], case.t_max))
        res, route = solve(s, case, buf)
        return res, route, diags(s, case)
    finally:
        s.close()


def result_of(res, case, k, tk=None):
    from enlsip_gn import GNResult
    tk = case.ts[k] if tk is None else tk
    i = [int(x) for x in res["info"][k]]
    return GNResult(res["p"][k], res["b"][k, :tk], res["d"][k], i[0], i[1], i[2], i[3], i[4], i[5], res["jA"][k, :tk],
                    res["jL"][k, :min(case.n, tk)], res["jJ"][k, :case.n - i[0]])


def written_pivots(jJ, info):
    """jpvtJ2 with the entries the library leaves unwritten (past n2 = n - rankA) set to zero"""
    out = np.array(jJ, copy=True)
    n2 = out.shape[1] - np.asarray(info)[:, 0]
    out[np.arange(out.shape[1])[None, :] >= n2[:, None]] = 0
    return out


def assert_same_results(got, want, keys, tag, rows=None):
    for key in keys:
        a, b = got[key], want[key]
        if key == "jJ":
            a, b = written_pivots(a, got["info"]), written_pivots(b, want["info"])
        if rows is not None:
            a, b = a[rows], b[rows]
        if not same(a, b):
            bad = sorted({int(i) for i in np.argwhere(np.atleast_2d(a.view(np.int64) != b.view(np.int64)))[:, 0]})
            raise AssertionError((tag, key, "differs from the tight run in problems", bad[:8], len(bad)))


ALL_KEYS = ("p", "b", "d", "info", "jA", "jL", "jJ")
CONSTRAINT_KEYS = ("b", "jA", "jL")           # written by the constraint stage, which no J*Q1 kernel feeds


def check_route(case, ln, buf, got, jq1_only=False):
    want = lc.expected_route(case, buf.pl, buf.J.data_ptr())
    if jq1_only:          # a uniform batch through the ragged entry: the constraint stage runs its ragged forms
        want = {b for b in want if b.startswith("jq1_")}
    assert want <= got, (case.name, ln, sorted(want - got), sorted(got))
    assert case.route - {b for b in case.route if b.startswith("jq1_v2_")} <= got, (case.name, ln, sorted(got))
    v2 = {b for b in got if b.startswith("jq1_v2_")}
    fast = f"jq1_v2_n{case.n}"
    if fast in tight_expected(case):
        if lc.LAYOUTS[ln][1]:
            assert v2 == {fast} and "jq1_mfma" not in got, (case.name, ln, sorted(got))
        else:
            assert not v2 and "jq1_mfma" in got, (case.name, ln, sorted(got))
    else:
        assert not v2, (case.name, ln, sorted(got))


def tight_expected(case):
    """route of the case's shape on a tight buffer ({} for a ragged batch, which expected_route does not model)"""
    import dispatch_grid as dg
    return dg.expected_route(case.B, case.m, case.n, case.t_max) if len(set(case.ts)) == 1 else set()


# ---- 1. the solve itself, every reader of the Jacobian side ---------------------------------------------------------------------------
SOLVE_PAIRS = [(c, ln) for c in lc.SOLVE_CASES for ln in c.layouts]


@pytest.mark.parametrize("case,ln", SOLVE_PAIRS, ids=[f"{c.name}-{ln}" for c, ln in SOLVE_PAIRS])
def test_solve_on_a_layout(case, ln):
    from enlsip_gn import FACTOR_A, FACTOR_L11
    tag = (case.name, ln)
    t_res, t_route, t_diag = tight_run(case)
    buf = Buffers(lc.place(lc.problems(case), lc.LAYOUTS[ln][0], case.t_max))
    s = make_handle(case)
    try:
        res, route = solve(s, case, buf)
        dg_ = diags(s, case)
    finally:
        s.close()
    print(tag, "route", sorted(route ^ t_route))
    check_route(case, ln, buf, route)
    assert np.all(np.isfinite(res["p"])) and np.all(np.isfinite(res["d"])), tag          # no fill was read as data
    # same route, same bytes
    assert_same_results(res, t_res, CONSTRAINT_KEYS, tag)
    assert same(dg_[FACTOR_A], t_diag[FACTOR_A]) and same(dg_[FACTOR_L11], t_diag[FACTOR_L11]), tag
    if route == t_route:
        assert_same_results(res, t_res, ALL_KEYS, tag)
        for w in dg_:
            assert same(dg_[w], t_diag[w]), (tag, "diag R", w)
    # against the oracle
    for k in lc.sample(case):
        out, ref = result_of(res, case, k), oracle(case, k)
        print(tag, k, "rel p", par.rel(out.p, ref.p), "rel b", par.rel(out.b, ref.b) if ref.b.size else 0.0)
        par.compare(out, ref, case.m, case.n)
    buf.assert_inputs_untouched(tag)


def test_host_form_stages_a_padded_layout():
    """enlsip_gn_solve_batched on HOST arrays laid out by place(odd_ld): the staging copies read ldj, strideJ, ldat, strideAt"""
    import enlsip_gn._lib as L
    case, ln = lc.HOST_CASE, lc.HOST_CASE.layouts[0]
    probs = lc.problems(case)
    pl = lc.place(probs, lc.LAYOUTS[ln][0], case.t_max)
    keepJ, keepA = pl.J.copy(), pl.At.copy()
    B, m, n, t = case.B, case.m, case.n, case.t_max
    p, b, d = np.full((B, n), np.nan), np.full((B, t), np.nan), np.full((B, m), np.nan)
    jA, jL, jJ = np.zeros((B, t), np.int64), np.zeros((B, min(n, t)), np.int64), np.zeros((B, n), np.int64)
    info = (L.Info * B)()
    fp = lambda a, off=0: C.c_void_p(a.ctypes.data + 8 * off)
    s, w = make_handle(case), make_handle(case)
    try:
        rc = s._lib.enlsip_gn_solve_batched(s._h, B, m, n, t, fp(pl.J, pl.off_j), pl.ldj, pl.strideJ, fp(pl.rx), fp(pl.At, pl.off_at),
                                            pl.ldat, pl.strideAt, fp(np.ascontiguousarray(pl.cx)), EPS, fp(p), fp(b), fp(d),
                                            C.cast(info, C.c_void_p), fp(jA), fp(jL), fp(jJ))
        assert rc == 0, s._lib.enlsip_gn_last_error(s._h)
        route = s.route()
        tp, tb, td, tinfo, tjA, tjL, tjJ = w.solve_batched(np.stack([np.ascontiguousarray(P[0].T) for P in probs]),
                                                            np.stack([P[1] for P in probs]), np.stack([P[2] for P in probs]),
                                                            np.stack([P[3] for P in probs]))
        assert case.route <= route and route == w.route(), (sorted(route), sorted(w.route()))
    finally:
        s.close()
        w.close()
    infos = [(int(i.rankA), int(i.rankJ2), int(i.code), int(i.dimA), int(i.dimJ2), int(i.status)) for i in info]
    assert same(p, tp) and same(b, tb) and same(d, td) and same(jA, tjA) and same(jL, tjL) and infos == tinfo
    assert same(written_pivots(jJ, infos), written_pivots(tjJ, tinfo))
    res = dict(p=p, b=b, d=d, info=np.array(infos), jA=jA, jL=jL, jJ=jJ)
    for k in range(B):
        par.compare(result_of(res, case, k), oracle(case, k), m, n)
    assert same(pl.J, keepJ) and same(pl.At, keepA)


# ---- 2. consumers on the resident padded state -------------------------------------------------------------------------------------------
CONSUMER_PAIRS = [(c, ln) for c in lc.CONSUMER_CASES for ln in c.layouts]


@functools.lru_cache(maxsize=None)
def checker(case):
    """estimate references of the case (mpmath), made once for its layouts"""
    probs = lc.problems(case)
    chk = ce.Checker(lambda k: probs[k], list(case.ts), case.n, case.t_max, None, case.name)
    chk.form = cr.expected_form(case.n, case.t_max)
    return chk


def nanbuf(*shape):
    return ce._nan_buffer(*shape)


def within(got, ref_bound, tag):
    ref, bound = ref_bound
    err = np.abs(got - ref)
    assert np.all(err <= bound), (tag, float(np.max(err - bound)))


def ragged_solve(s, case, buf):
    pl = buf.pl
    s.solve_batched_ragged_dev(pl.B, pl.m, pl.n, pl.t_max, np.array(case.ts), *buf.in_args(), EPS, **buf.out_args())
    return buf.results(), s.route()


def batched_consumers(s, case, prand):
    """the four batched device forms over the whole resident batch"""
    B, m, n, t = case.B, case.m, case.n, case.t_max
    dG, dJp, dAp, dl1, dgr, dl2 = nanbuf(B, n), nanbuf(B, m), nanbuf(B, t), nanbuf(B, t), nanbuf(B), nanbuf(B, t)
    st1, st2 = (torch.full((B,), ce.ST_SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
    dp = torch.from_numpy(prand).to(DEV)
    torch.cuda.synchronize()
    assert s.gradient_batched_dev(0, B, dG.data_ptr()) == 0
    assert s.jacobian_times_batched_dev(0, B, dp.data_ptr(), dJp.data_ptr(), dAp.data_ptr()) == 0
    assert s.first_lagrange_batched_dev(0, B, dl1.data_ptr(), dgrad_res=dgr.data_ptr(), dstatus=st1.data_ptr()) == 0
    assert s.consumer_form() == cr.expected_form(n, t)
    assert s.second_lagrange_batched_dev(0, B, dp.data_ptr(), dl2.data_ptr(), dstatus=st2.data_ptr()) == 0
    torch.cuda.synchronize()
    return dict(grad=dG.cpu().numpy(), Jp=dJp.cpu().numpy(), Ap=dAp.cpu().numpy(), lam1=dl1.cpu().numpy(), gres=dgr.cpu().numpy(),
                lam2=dl2.cpu().numpy(), st1=st1.cpu().numpy(), st2=st2.cpu().numpy())


def single_consumers(s, case, k, prand, Gam):
    """the single-problem forms at slot k, in an order that leaves the truncated re-solve before the factor reads and the Newton step"""
    from enlsip_gn import FACTOR_A, FACTOR_L11, FACTOR_J2
    m, n, t = case.m, case.n, case.t_max
    out = dict(grad=s.gradient(n, k), JQ1=s.JQ1(m, n, k))
    out["Jp"], out["Ap"] = s.jacobian_times(m, t, prand[k], k)
    kp = min(m, n - min(n, t))
    out["dims"] = (t - 2, kp - 1)
    out["rp"], out["rb"], out["rd"] = s.resolve(m, n, t, t - 2, kp - 1, -1, k)
    for nm, w in (("RA", FACTOR_A), ("RL", FACTOR_L11), ("RJ", FACTOR_J2)):
        out[nm] = s.factor(w, k).R
    out["newton"], out["newton_err"] = s.newton_direction(Gam, k)
    return out


@pytest.mark.parametrize("case,ln", CONSUMER_PAIRS, ids=[f"{c.name}-{ln}" for c, ln in CONSUMER_PAIRS])
def test_consumers_on_a_resident_layout(case, ln):
    tag = (case.name, ln)
    B, m, n, t = case.B, case.m, case.n, case.t_max
    probs = lc.problems(case)
    prand = synth.normal_stream(case.seed + 50, 6, B * n).reshape(B, n)
    rng = np.random.default_rng(case.seed)
    S0 = rng.standard_normal((n, n))
    Gam = 0.3 * (S0 + S0.T)                                              # random symmetric
    buf = Buffers(lc.place(probs, lc.LAYOUTS[ln][0], t))
    tbuf = Buffers(lc.place(probs, lc.LAYOUTS["tight"][0], t))
    s, w = make_handle(case), make_handle(case)
    try:
        res, route = ragged_solve(s, case, buf)                          # all t_k = t_max: what the changed-problems solve needs resident
        t_res, t_route = ragged_solve(w, case, tbuf)
        check_route(case, ln, buf, route, jq1_only=True)
        same_route = route == t_route
        assert same_route == (not (f"jq1_v2_n{n}" in t_route and not lc.LAYOUTS[ln][1])), tag
        # ---- batched device forms: every problem bitwise the tight handle's, a sample against the references
        got, want = batched_consumers(s, case, prand), batched_consumers(w, case, prand)
        for key in ("grad", "Jp", "Ap", "lam1", "gres", "st1") + (("lam2", "st2") if same_route else ()):
            assert same(got[key], want[key]), (tag, key)
        assert not got["st1"].any() and not got["st2"].any(), tag
        chk = checker(case)
        for k in cr.sample_of(list(case.ts)):
            J, rx, A, cx = probs[k]
            within(got["grad"][k], cr.exact_matvec(J.T, rx), tag + (k, "grad"))
            within(got["Jp"][k], cr.exact_matvec(J, prand[k]), tag + (k, "Jp"))
            within(got["Ap"][k], cr.exact_matvec(A, prand[k]), tag + (k, "Ap"))
            Sk, pr, _ = ce.gpu_kept_set(s, k, t, EPS)
            assert pr == min(n, t), tag
            R, kS = chk.ref(k, Sk), cr.kappa(A[Sk])
            F_o, S_o = chk.factor_o(k)
            assert sorted(S_o) == sorted(Sk), tag
            g = cr.exact_gradient(J, rx)
            lam_r, gres_r = R.first(g, cx, None)
            gam = cr.gamma_rhs(J, rx) * R.first_cancellation(g, cx)
            it = go.IterationRecord()
            lam_o = go.first_lagrange_mult_estimate(A, J.T @ rx, cx, False, np.ones(t), F_o, it, EPS)
            chk.judge(f"{tag}[{k}] first", cr.rel_err(got["lam1"][k], lam_r), cr.rel_err(lam_o, lam_r), cr.estimate_bound(kS, gam), kS * gam)
            nrm = max(np.linalg.norm(g), 1e-300)
            chk.judge(f"{tag}[{k}] grad_res", abs(got["gres"][k] - gres_r) / nrm, abs(it.grad_res - gres_r) / nrm,
                      cr.estimate_bound(kS, gam), kS * gam)
            lam_r = R.second(J, rx, prand[k], None)
            lam_o = go.second_lagrange_mult_estimate(J, F_o, rx, prand[k], t, False, np.ones(t), EPS)
            gam = cr.gamma_rhs(J, rx, prand[k])
            chk.judge(f"{tag}[{k}] second", cr.rel_err(got["lam2"][k], lam_r), cr.rel_err(lam_o, lam_r), cr.estimate_bound(kS, gam), kS * gam)
        # ---- single-problem forms at the last slot
        k = B - 1
        J, rx, A, cx = probs[k]
        ref = oracle(case, k)
        g1, w1 = single_consumers(s, case, k, prand, Gam), single_consumers(w, case, k, prand, Gam)
        for key in ("grad", "Jp", "Ap", "RA", "RL") + (("JQ1", "rp", "rb", "rd", "RJ", "newton") if same_route else ()):
            assert same(g1[key], w1[key]), (tag, "single", key)
        within(g1["grad"], cr.exact_matvec(J.T, rx), tag + ("single grad",))
        within(g1["Jp"], cr.exact_matvec(J, prand[k]), tag + ("single Jp",))
        within(g1["Ap"], cr.exact_matvec(A, prand[k]), tag + ("single Ap",))
        JQ1 = ref.F_A.rmul_Q(J)
        assert par.rel(g1["JQ1"], JQ1) <= 1e-12, tag
        dimA, dimJ2 = g1["dims"]
        p_ref, b_ref, d_ref = go.sub_search_direction(JQ1[:, :ref.rankA], rx, cx, ref.F_A, ref.F_L11, ref.F_J2, n, t, ref.rankA, dimA,
                                                      dimJ2, -1)
        assert par.rel(g1["rp"], p_ref) <= 1e-11 and par.rel(g1["rb"], b_ref) <= 1e-12, tag
        assert abs(np.linalg.norm(g1["rd"]) - np.linalg.norm(d_ref)) <= 1e-12 * np.linalg.norm(d_ref), tag
        assert par.rel(np.abs(g1["rd"][:dimJ2]), np.abs(d_ref[:dimJ2])) <= 1e-10, tag
        for key, F in (("RA", ref.F_A), ("RL", ref.F_L11), ("RJ", ref.F_J2)):
            assert g1[key].shape == F.R.shape and par.rel(np.abs(g1[key]), np.abs(F.R)) <= 1e-11, (tag, key)
        pn_ref, err_ref = par._newton_reference(J, rx, A, cx, Gam)
        assert g1["newton_err"] == err_ref and not err_ref and par.rel(g1["newton"], pn_ref) <= 1e-10, tag
        # ---- the changed-problems solve: two slots of the padded A' and cx rewritten in place, their fill left where it is
        final = list(probs)
        flags = np.zeros(B, dtype=np.int64)
        for kk in (0, B - 1):
            _, _, A2, cx2 = cr.make_problem(case.seed + 100 + kk, m, n, t, kappa_A=10.0)          # tie-free pivots, as the case's own A
            buf.rewrite_slot(kk, A2, cx2)
            final[kk] = (probs[kk][0], probs[kk][1], A2, cx2)
            flags[kk] = 1
        for o in buf.out.values():
            o.fill_(float("nan") if o.dtype == torch.float64 else -7)
        s.solve_changed_batched_dev(B, m, n, t, np.array(case.ts), flags, *buf.a_args(), EPS, **buf.out_args())
        assert s.jacobian_resolved() == 2
        ch = buf.results()
        fbuf = Buffers(lc.place(final, lc.LAYOUTS["tight"][0], t))
        f = make_handle(case)
        try:
            f_res, f_route = ragged_solve(f, case, fbuf)
        finally:
            f.close()
        assert np.all(np.isnan(ch["p"][1:B - 1])) and np.all(ch["info"][1:B - 1] == -7), tag      # only the flagged slots are written
        rows = [0, B - 1]
        assert_same_results(ch, f_res, CONSTRAINT_KEYS, tag + ("changed",), rows)
        if same_route:
            assert_same_results(ch, f_res, ALL_KEYS, tag + ("changed",), rows)
        for kk in rows:
            par.compare(result_of(ch, case, kk), go.gn_subproblem(*final[kk]), m, n)
        buf.assert_inputs_untouched(tag + ("changed",))
        # ---- the factored flow on the same padded buffers: constraint stage, slot 1 rewritten, a mixed refactor mask
        s.factor_constraints_batched_dev(B, m, n, t, np.array(case.ts), *buf.a_args(), EPS)
        _, _, A3, cx3 = cr.make_problem(case.seed + 200, m, n, t, kappa_A=10.0)
        buf.rewrite_slot(1, A3, cx3)
        final[1] = (probs[1][0], probs[1][1], A3, cx3)
        refactor = np.zeros(B, dtype=np.int64)
        refactor[1] = 1
        s.solve_factored_batched_dev(B, m, n, t, np.array(case.ts), refactor, *buf.in_args(), EPS, **buf.out_args())
        assert s.constraint_refactored() == 1
        fa, fa_route = buf.results(), s.route()
        fbuf = Buffers(lc.place(final, lc.LAYOUTS["tight"][0], t))
        f = make_handle(case)
        try:
            f_res, f_route = ragged_solve(f, case, fbuf)
        finally:
            f.close()
        assert_same_results(fa, f_res, CONSTRAINT_KEYS, tag + ("factored",))
        if same_route:
            assert_same_results(fa, f_res, ALL_KEYS, tag + ("factored",))
        for kk in range(B):
            par.compare(result_of(fa, case, kk), go.gn_subproblem(*final[kk]), m, n)
        buf.assert_inputs_untouched(tag + ("factored",))
        tbuf.assert_inputs_untouched(tag + ("tight",))
    finally:
        s.close()
        w.close()
