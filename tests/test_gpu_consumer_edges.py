"""Batched consumers of a solve at their edges, against references that share no arithmetic with them (tests/consumer_reference.py):
the two multiplier estimates by their pivot-free closed forms in mpmath, the gradient and the products as correctly rounded sums.
Every case runs on a default handle and on one created with ENLSIP_GN_LAGRANGE_SMALL=0, and checks the form the library reports
against the predicate parsed from its source.

- estimate grid: n and t_max at 1, 2, 63, 64, 65, t > n, t = n = 64, m from 1 to 1000, ragged t_k, ranges off multiples of 4;
  each estimate within the bound C u kappa(A_S)^2 gamma AND within max(8 x the FP64 oracle's error, 32 u) on the same problem,
  S taken from the GPU's own factors; exact zeros outside S and past t_k, grad_res = 0 when pr = n, status 0
- pseudo-rank straddle: the last |R_ii| 2x above / below the tolerance, in both forms, eps_rank sqrt(eps) and 1e-14; status 2
- products at their tails: m, n and t_max off multiples of 4 / 64 / 512, each entry within the dot-product bound, A p past t_k 0
- routing on ragged batches: pipeline halves, chunks, a rescued member on the second half
- guard slots: the _dev forms write nothing outside [prob0, prob0 + count) of the caller's buffers"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import consumer_reference as cr
from oracle import gn_oracle as go, synth

pytestmark = pytest.mark.gpu
EPS = go.SQRT_EPS
U = cr.U
STATS = {"est_over_bound": (0.0, ""), "est_over_oracle_limit": (0.0, ""), "est_over_8x_oracle_form0": (0.0, ""),
         "est_over_8x_oracle_form1": (0.0, ""), "prod_over_bound": (0.0, "")}


def _make_solver(general=False):
    from enlsip_gn import GNSolver
    old = os.environ.get("ENLSIP_GN_LAGRANGE_SMALL")
    if general:
        os.environ["ENLSIP_GN_LAGRANGE_SMALL"] = "0"       # read at handle creation
    try:
        return GNSolver(device=0)
    finally:
        if general:
            if old is None:
                del os.environ["ENLSIP_GN_LAGRANGE_SMALL"]
            else:
                os.environ["ENLSIP_GN_LAGRANGE_SMALL"] = old


@pytest.fixture(scope="module")
def solvers():
    """(handle, wave form enabled): the default handle and one forced to the general form"""
    s0, s1 = _make_solver(), _make_solver(general=True)
    yield ((s0, True), (s1, False))
    s0.close()
    s1.close()
    out = os.environ.get("ENLSIP_CONSUMER_STATS")       # worst ratios of the module, for the record
    if out:
        with open(out, "w") as f:
            json.dump(STATS, f, indent=1)


def _note(key, ratio, label):
    if ratio > STATS[key][0]:
        STATS[key] = (float(ratio), label)


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def same(a, b):
    """bit for bit, NaN payloads included"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- solving a host batch ------------------------------------------------------------------------------------------------------
def solve(s, probs, t_max):
    """probs: [(J, rx, A (t_k x n), cx)]; uniform t_k: solve_batched, else solve_batched_ragged.  Returns (p, rankA per problem)."""
    from enlsip_gn import GNSolver
    n = probs[0][0].shape[1]
    ts = [P[2].shape[0] for P in probs]
    J = np.stack([np.asfortranarray(P[0]).T for P in probs])
    rx = np.stack([P[1] for P in probs])
    if len(set(ts)) == 1 and ts[0] == t_max:
        out = s.solve_batched(J, rx, np.stack([P[2] for P in probs]), np.stack([P[3] for P in probs]))
    else:
        At, cx, t = GNSolver.pack_ragged([P[2] if P[2].size else np.zeros((0, n)) for P in probs], [P[3] for P in probs], n=n)
        if At.shape[1] < t_max:
            At = np.concatenate([At, np.zeros((len(probs), t_max - At.shape[1], n))], axis=1)
            cx = np.concatenate([cx, np.zeros((len(probs), t_max - cx.shape[1]))], axis=1)
        out = s.solve_batched_ragged(J, rx, At, cx, t)
    return out[0], [i[0] for i in out[3]]


def gpu_kept_set(s, k, tk, eps):
    """(S, pr, diag R) from the handle's own factorisation of problem k"""
    from enlsip_gn import FACTOR_A
    if tk == 0:
        return [], 0, np.zeros(0)
    F = s.factor(FACTOR_A, k)
    d = F.diagR()
    S, pr = cr.kept_set(F.p, d, eps)
    return S, pr, d


# ---- the estimate checks of one range ----------------------------------------------------------------------------------------------
class Checker:
    """Runs both estimates over [prob0, prob0 + count) of a solved batch on one handle and checks every problem exactly and the
    sampled ones against the references (cached across handles and ranges: S is the same set on both handles)."""

    def __init__(self, problem, ts, n, t_max, diag, tag):
        self.problem, self.ts, self.n, self.t_max, self.diag, self.tag = problem, ts, n, t_max, diag, tag
        self.refs, self.oracle = {}, {}

    def ref(self, k, S):
        key = (k, tuple(sorted(S)))
        if key not in self.refs:
            self.refs[key] = cr.EstimateReference(self.problem(k)[2], S)
        return self.refs[key]

    def factor_o(self, k):
        if k not in self.oracle:
            A = self.problem(k)[2]
            F = go.qr_colnorm(A.T)
            self.oracle[k] = (F, cr.kept_set(F.p, F.diagR(), EPS)[0])
        return self.oracle[k]

    def judge(self, label, err, err_o, bound, first_order):
        """err: the kernel's error, err_o: the FP64 oracle's on the same problem.  Besides the bound, the kernel must stay within 8x
        the oracle's error, or within 32 u times the first-order amplification kappa(A_S) gamma: one rounding more or less in a
        right-hand side that cancels (or, in the second estimate, the solve's resident J Q1 in place of the oracle's dormqr) can
        move either error by more than 8x, a kernel that drops digits cannot hide in it"""
        assert err <= bound, (label, err, bound)
        limit = max(8.0 * err_o, 32.0 * U * first_order)
        assert err <= limit, (label, err, limit)
        _note("est_over_bound", err / bound, label)
        _note("est_over_oracle_limit", err / limit, label)
        _note(f"est_over_8x_oracle_form{self.form}", err / max(8.0 * err_o, 32.0 * U), label)

    def run(self, s, small, prob0, count, G, P, sample, P_names=("p_solve",), skip=()):
        n, t_max, ts = self.n, self.t_max, self.ts
        self.form = cr.expected_form(n, t_max, small)
        sl = slice(prob0, prob0 + count)
        for ds in (None, self.diag):
            dss = None if ds is None else ds[sl]
            for gfx in (G, None):
                lam, gres, st, rc = s.first_lagrange_batched(t_max, prob0, count, None if gfx is None else gfx[sl], dss)
                assert s.consumer_form() == cr.expected_form(n, t_max, small), self.tag
                assert rc == (1 if st.any() else 0)
                assert all(st[j] == 0 for j in range(count) if prob0 + j not in skip), (self.tag, st)
                for j in range(count):
                    k = prob0 + j
                    if k in skip:
                        continue
                    tk = ts[k]
                    S, pr, _ = gpu_kept_set(s, k, tk, EPS)
                    label = f"{self.tag}[{k}] first small={small} ds={ds is not None} grad_fx={gfx is not None}"
                    nz = np.zeros(t_max, bool)
                    nz[S] = True
                    assert np.all(lam[j][~nz] == 0.0) and np.all(lam[j][nz] != 0.0), (label, lam[j], S)
                    if pr == n:
                        assert gres[j] == 0.0, label
                    if k not in sample:
                        continue
                    J, rx, A, cx = self.problem(k)
                    g = gfx[k] if gfx is not None else cr.exact_gradient(J, rx)
                    R = self.ref(k, S)
                    lam_r, gres_r = R.first(g, cx, None if ds is None else ds[k, :tk])
                    gam = (1.0 if gfx is not None else cr.gamma_rhs(J, rx)) * R.first_cancellation(g, cx)
                    kS = cr.kappa(A[S])
                    F_o, S_o = self.factor_o(k)
                    it = go.IterationRecord()
                    g_o = gfx[k] if gfx is not None else J.T @ rx
                    lam_o = go.first_lagrange_mult_estimate(A, g_o, cx, ds is not None, ds[k, :tk] if ds is not None else np.ones(tk),
                                                            F_o, it, EPS)
                    R_o = R if sorted(S_o) == sorted(S) else self.ref(k, S_o)
                    lam_ro, gres_ro = R_o.first(g, cx, None if ds is None else ds[k, :tk])
                    self.judge(label, cr.rel_err(lam[j, :tk], lam_r), cr.rel_err(lam_o, lam_ro), cr.estimate_bound(kS, gam), kS * gam)
                    nrm = max(np.linalg.norm(g), 1e-300)         # grad_res: the error relative to ||grad||
                    self.judge(label + " grad_res", abs(gres[j] - gres_r) / nrm, abs(it.grad_res - gres_ro) / nrm,
                               cr.estimate_bound(kS, gam), kS * gam)
            for pname, PP in zip(P_names, P):
                lam, st, rc = s.second_lagrange_batched(t_max, PP[sl], prob0, dss)
                assert rc == (1 if st.any() else 0)
                assert all(st[j] == 0 for j in range(count) if prob0 + j not in skip), (self.tag, st)
                for j in range(count):
                    k = prob0 + j
                    if k in skip:
                        continue
                    tk = ts[k]
                    S, pr, _ = gpu_kept_set(s, k, tk, EPS)
                    label = f"{self.tag}[{k}] second {pname} small={small} ds={ds is not None}"
                    nz = np.zeros(t_max, bool)
                    nz[S] = True
                    assert np.all(lam[j][~nz] == 0.0) and np.all(lam[j][nz] != 0.0), (label, lam[j], S)
                    if k not in sample or tk == 0:
                        continue
                    J, rx, A, cx = self.problem(k)
                    R = self.ref(k, S)
                    lam_r = R.second(J, rx, PP[k], None if ds is None else ds[k, :tk])
                    F_o, S_o = self.factor_o(k)
                    dsv = ds[k, :tk] if ds is not None else np.ones(tk)
                    lam_o = go.second_lagrange_mult_estimate(J, F_o, rx, PP[k], tk, ds is not None, dsv, EPS)
                    R_o = R if sorted(S_o) == sorted(S) else self.ref(k, S_o)
                    lam_ro = R_o.second(J, rx, PP[k], None if ds is None else ds[k, :tk])
                    kS, gam = cr.kappa(A[S]), cr.gamma_rhs(J, rx, PP[k])
                    self.judge(label, cr.rel_err(lam[j, :tk], lam_r), cr.rel_err(lam_o, lam_ro), cr.estimate_bound(kS, gam),
                               kS * gam)


# ---- 1. the estimate grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(cr.ESTIMATE_GRID)), ids=[c[0] for c in cr.ESTIMATE_GRID])
def test_estimate_grid(solvers, ci):
    name, m, n, t_max, ts, kap, queries = cr.ESTIMATE_GRID[ci]
    B = len(ts)
    probs = [cr.grid_problem(ci, k, m, n, ts[k], kap) for k in range(B)]
    diag = cr.random_diag(100 + ci, B, t_max)
    prand = synth.normal_stream(200 + ci, 6, B * n).reshape(B, n)
    chk = Checker(lambda k: probs[k], ts, n, t_max, diag, name)
    sample = set(cr.sample_of(ts))
    for s, small in solvers:
        P, _ = solve(s, probs, t_max)
        G = s.gradient_batched(n, 0, B)
        for prob0, count in queries:
            chk.run(s, small, prob0, count, G, (P, prand), sample, P_names=("p_solve", "p_rand"))


# ---- 2. the pseudo-rank straddle ---------------------------------------------------------------------------------------------------
def _straddle_batch(seed, m, n, t, eps, side):
    J0, rx0, A0, cx0 = cr.make_problem(seed, m, n, t)
    J1, rx1, _, cx1 = cr.make_problem(seed + 1, m, n, t)
    J2, rx2, A2, cx2 = cr.make_problem(seed + 2, m, n, t)
    return [(J0, rx0, A0, cx0), (J1, rx1, cr.near_dependent_A(seed + 1, n, t, eps, side), cx1), (J2, rx2, A2, cx2)]


def _straddle_check(s, k, tk, eps, lam1, lam2, st2, rankA, tag):
    """pr of the zero pattern = pseudo_rank of the GPU's diag R, the kept set = its pivots; status 2 exactly when pr > rankA"""
    S, pr, _ = gpu_kept_set(s, k, tk, eps)
    assert np.count_nonzero(lam1) == pr and set(np.flatnonzero(lam1)) == set(S), (tag, k, lam1, S)
    want = 2 if pr > rankA else 0
    assert st2 == want, (tag, k, st2, pr, rankA)
    if want == 0:
        assert set(np.flatnonzero(lam2)) == set(S), (tag, k)
    return pr


@pytest.mark.parametrize("case", cr.STRADDLE_GRID, ids=[c[0] for c in cr.STRADDLE_GRID])
def test_pseudo_rank_straddle(solvers, case):
    name, m, n, t, eps, side = case
    probs = _straddle_batch(7000 + n + t, m, n, t, eps, side)
    kA = min(n, t)
    prs = []
    for s, small in solvers:
        P, rankA = solve(s, probs, t)
        lam, _, st, _ = s.first_lagrange_batched(t, 0, 3, None, None, eps_rank=eps)
        assert s.consumer_form() == cr.expected_form(n, t, small) and not st.any()
        lam2, st2, rc2 = s.second_lagrange_batched(t, P, 0, None, eps_rank=eps)
        assert rc2 == (1 if st2.any() else 0)
        pr = _straddle_check(s, 1, t, eps, lam[1], lam2[1], st2[1], rankA[1], name)
        assert pr == (kA if side > 1 else kA - 1), (name, pr)          # the GPU's factorisation straddles as LAPACK's does
        if eps < EPS and side > 1:
            assert st2[1] == 2, name                                   # the solve (sqrt(eps)) dropped the constraint, 1e-14 keeps it
        for k in (0, 2):
            _straddle_check(s, k, t, eps, lam[k], lam2[k], st2[k], rankA[k], name)
        prs.append(pr)
    assert prs[0] == prs[1], (name, prs)


def test_pseudo_rank_straddle_ragged(solvers):
    """status 2 in a ragged batch: near-dependent members above the 1e-14 tolerance (dropped by the sqrt(eps) solve) next to ones
    below it, generic and empty members"""
    m, n, t_max, eps = 90, 12, 6, 1e-14
    plan = [(6, 2.0), (0, None), (5, 0.5), (6, None), (3, 2.0), (6, 0.5), (2, None)]
    probs = []
    for k, (tk, side) in enumerate(plan):
        J, rx, A, cx = cr.make_problem(7300 + k, m, n, tk)
        if side is not None:
            A = cr.near_dependent_A(7300 + k, n, tk, eps, side)
        probs.append((J, rx, A, cx))
    ts = [tk for tk, _ in plan]
    prs = []
    for s, small in solvers:
        P, rankA = solve(s, probs, t_max)
        lam, _, st, _ = s.first_lagrange_batched(t_max, 0, len(ts), None, None, eps_rank=eps)
        assert s.consumer_form() == cr.expected_form(n, t_max, small) and not st.any()
        lam2, st2, rc2 = s.second_lagrange_batched(t_max, P, 0, None, eps_rank=eps)
        assert rc2 == 1
        got = []
        for k, (tk, side) in enumerate(plan):
            assert np.all(lam[k, tk:] == 0.0) and np.all(lam2[k, tk:] == 0.0)
            got.append(_straddle_check(s, k, tk, eps, lam[k, :tk], lam2[k, :tk], st2[k], rankA[k], "ragged"))
            if side is not None:
                assert st2[k] == (2 if side > 1 else 0), (k, st2[k])
        prs.append(got)
    assert prs[0] == prs[1]


# ---- 3. products at their tails ------------------------------------------------------------------------------------------------------
SENTINEL = np.uint64(0x7FF8DEADBEEF0001)          # a quiet NaN with a payload no kernel produces
ST_SENTINEL = 0x7EADBEEF


def _nan_buffer(*shape):
    return torch.full(shape, int(SENTINEL.astype(np.int64)), dtype=torch.int64, device="cuda:0").view(torch.float64)


PRODUCT_CASES = [(1, 1, 3, [3, 0, 2]), (63, 2, 5, [5, 1, 0, 4, 5]), (64, 3, 3, [2, 3, 0, 1]), (65, 4, 5, [5, 3, 5, 0, 2]),
                 (511, 5, 65, [65, 7, 0, 64, 33]), (512, 65, 3, [3, 0, 1]), (513, 65, 65, [65, 1, 64, 0, 17])]


@pytest.mark.parametrize("m,n,t_max,ts", PRODUCT_CASES, ids=[f"m{c[0]}_n{c[1]}_t{c[2]}" for c in PRODUCT_CASES])
def test_products_at_tails(solvers, m, n, t_max, ts):
    B = len(ts)
    probs = [cr.make_problem(7600 + 10 * n + k, m, n, ts[k]) for k in range(B)]
    p = synth.normal_stream(7700 + n, 6, B * n).reshape(B, n)
    for s, _ in solvers:
        solve(s, probs, t_max)
        dG, dJp, dAp = _nan_buffer(B, n), _nan_buffer(B, m), _nan_buffer(B, t_max)
        dp = torch.from_numpy(p).to("cuda:0")
        torch.cuda.synchronize()
        assert s.gradient_batched_dev(0, B, dG.data_ptr()) == 0
        assert s.jacobian_times_batched_dev(0, B, dp.data_ptr(), dJp.data_ptr(), dAp.data_ptr()) == 0
        G, Jp, Ap = dG.cpu().numpy(), dJp.cpu().numpy(), dAp.cpu().numpy()
        for k in range(B):
            J, rx, A, _ = probs[k]
            tk = ts[k]
            for what, got, (ref, bound) in (("grad", G[k], cr.exact_matvec(J.T, rx)), ("Jp", Jp[k], cr.exact_matvec(J, p[k])),
                                            ("Ap", Ap[k, :tk], cr.exact_matvec(A, p[k]) if tk else (np.zeros(0), np.zeros(0)))):
                err = np.abs(got - ref)
                assert np.all(err <= bound), (what, k, np.max(err - bound))
                if got.size:
                    _note("prod_over_bound", float(np.max(err / bound)), f"m{m}_n{n}_t{t_max}[{k}] {what}")
            assert np.all(Ap[k, tk:] == 0.0) and not np.signbit(Ap[k, tk:]).any(), (k, Ap[k, tk:])


# ---- 4. routing on ragged batches -------------------------------------------------------------------------------------------------
def _vector_batch(seed, B, m, n, t_max, ts, scale=None):
    """B problems from four draws (J, rx, A', cx), rows past t_k zero; scale = {k: factor of J_k, rx_k}"""
    J = synth.normal_stream(seed, 0, B * m * n).reshape(B, n, m)
    rx = synth.normal_stream(seed, 1, B * m).reshape(B, m)
    At = synth.normal_stream(seed, 2, B * t_max * n).reshape(B, t_max, n)
    cx = synth.normal_stream(seed, 3, B * t_max).reshape(B, t_max)
    for k, tk in enumerate(ts):
        At[k, tk:] = 0.0
        cx[k, tk:] = 0.0
    for k, f in (scale or {}).items():
        J[k] *= f
        rx[k] *= f

    def problem(k):
        return J[k].T, rx[k], At[k, :ts[k]], cx[k, :ts[k]]
    return J, rx, At, cx, problem


def per_first(s, k, tk, grad, ds):
    lam, gres = np.zeros(max(tk, 1)), C.c_double(0.0)
    rc = s._lib.enlsip_gn_first_lagrange(s._h, k, _fp(grad), _fp(ds), EPS, _fp(lam), C.byref(gres))
    return rc, lam[:tk], gres.value


def per_second(s, k, tk, p, ds):
    lam = np.zeros(max(tk, 1))
    rc = s._lib.enlsip_gn_second_lagrange(s._h, k, _fp(np.ascontiguousarray(p)), _fp(ds), EPS, _fp(lam))
    return rc, lam[:tk]


STATUS_OF_RC = {0: 0, 1: 1, -7: 2}


def test_ragged_pipeline_split_range(solvers):
    """m=1024, n=48, t_max=16, 192 problems with t_k from 0 to 16: pipeline-split, wave form; a range straddling the split from an
    odd prob0, on host and device buffers"""
    B, m, n, t_max = 192, 1024, 48, 16
    ts = [k % 17 for k in range(B)]
    J, rx, At, cx, problem = _vector_batch(7800, B, m, n, t_max, ts)
    diag = cr.random_diag(7801, B, t_max)
    chk = Checker(problem, ts, n, t_max, diag, "pipeline")
    for s, small in solvers:
        out = s.solve_batched_ragged(J, rx, At, cx, np.array(ts))
        P = out[0]
        split = s.pipeline_split()
        assert 0 < split < B, split
        p0 = split - 3 if (split - 3) % 2 else split - 4
        cnt = 7
        sample = {p0, split - 1, split, p0 + cnt - 1} - {k for k in range(B) if ts[k] == 0}
        G = s.gradient_batched(n, 0, B)
        chk.run(s, small, p0, cnt, G, (P,), sample)
        lam = _nan_buffer(cnt, t_max)
        st = torch.full((cnt,), ST_SENTINEL, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        assert s.first_lagrange_batched_dev(p0, cnt, lam.data_ptr(), dstatus=st.data_ptr()) == 0
        lam_h, _, st_h, _ = s.first_lagrange_batched(t_max, p0, cnt)
        assert same(lam.cpu().numpy(), lam_h) and np.array_equal(st.cpu().numpy(), st_h)


def test_ragged_chunked_range(solvers):
    """GN_MAX_LAUNCH_BATCH + 40 problems of a tiny ragged shape run in two chunks; a range inside the resident (last) chunk with
    t_k = 0 members"""
    B = cr.max_launch_batch() + 40
    m, n, t_max = 6, 3, 3
    ts = [k % 4 for k in range(B)]
    J, rx, At, cx, problem = _vector_batch(7900, B, m, n, t_max, ts)
    diag = cr.random_diag(7901, B, t_max)
    chk = Checker(problem, ts, n, t_max, diag, "chunked")
    p0, cnt = B - 37, 30
    sample = set(range(p0, p0 + cnt, 3))
    for s, small in solvers:
        out = s.solve_batched_ragged(J, rx, At, cx, np.array(ts))
        assert "chunked" in s.route()
        Gr = np.zeros((B, n))
        Gr[p0:p0 + cnt] = s.gradient_batched(n, p0, cnt)
        chk.run(s, small, p0, cnt, Gr, (out[0],), sample)
        for k in sorted(sample):
            if ts[k] == 0:
                lam, gres, st, _ = s.first_lagrange_batched(t_max, k, 1)
                g = cr.exact_gradient(*problem(k)[:2])
                assert np.all(lam == 0.0) and st[0] == 0
                assert abs(gres[0] - np.linalg.norm(g)) <= 8 * n * U * np.linalg.norm(g)


def test_ragged_pipeline_rescued_member(solvers):
    """a ragged pipelined batch with a member scaled by 2^600 on the second half: its slots are bitwise the per-problem entry
    points' (J' rx overflows to inf / NaN there, as in the reference), the other members against the references"""
    B, m, n, t_max = 192, 1024, 48, 16
    ts = [1 + k % 16 for k in range(B)]
    kr = 150
    J, rx, At, cx, problem = _vector_batch(8000, B, m, n, t_max, ts, scale={kr: 2.0 ** 600})
    diag = cr.random_diag(8001, B, t_max)
    chk = Checker(problem, ts, n, t_max, diag, "rescued")
    for s, small in solvers:
        out = s.solve_batched_ragged(J, rx, At, cx, np.array(ts))
        P = out[0]
        split = s.pipeline_split()
        assert 0 < split <= kr and "rescaled" in s.route(), (split, s.route())
        p0, cnt = kr - 5, 11
        G = s.gradient_batched(n, 0, B)
        assert same(G[kr], s.gradient(n, kr))
        Jp, Ap = s.jacobian_times_batched(m, t_max, P[p0:p0 + cnt], p0)
        jp1, ap1 = s.jacobian_times(m, ts[kr], P[kr], kr)
        assert same(Jp[kr - p0], jp1) and same(Ap[kr - p0, :ts[kr]], ap1) and np.all(Ap[kr - p0, ts[kr]:] == 0.0)
        tk = ts[kr]
        for gfx in (G, None):
            lam, gres, st, _ = s.first_lagrange_batched(t_max, p0, cnt, None if gfx is None else gfx[p0:p0 + cnt], diag[p0:p0 + cnt])
            rc1, lam1, gres1 = per_first(s, kr, tk, None if gfx is None else G[kr], np.ascontiguousarray(diag[kr, :tk]))
            assert same(lam[kr - p0, :tk], lam1) and same(gres[kr - p0], gres1) and st[kr - p0] == STATUS_OF_RC[rc1]
        lam2, st2, _ = s.second_lagrange_batched(t_max, P[p0:p0 + cnt], p0, diag[p0:p0 + cnt])
        rc1, lam1 = per_second(s, kr, tk, P[kr], np.ascontiguousarray(diag[kr, :tk]))
        assert same(lam2[kr - p0, :tk], lam1) and st2[kr - p0] == STATUS_OF_RC[rc1]
        chk.run(s, small, p0, cnt, G, (P,), {p0, kr - 1, kr + 1, p0 + cnt - 1}, skip={kr})


# ---- 5. guard slots of the _dev forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("general", [False, True], ids=["wave", "general"])
def test_dev_forms_write_only_their_range(solvers, general):
    s, small = solvers[1] if general else solvers[0]
    m, n, t_max = 100, 10, 6
    ts = [6, 3, 0, 6, 5, 6, 2]
    B, prob0, count, g = len(ts), 1, 5, 2
    probs = [cr.make_problem(8100 + k, m, n, ts[k]) for k in range(B)]
    P, _ = solve(s, probs, t_max)
    diag = cr.random_diag(8101, B, t_max)
    dp = torch.from_numpy(np.ascontiguousarray(P[prob0:prob0 + count])).to("cuda:0")
    dds = torch.from_numpy(np.ascontiguousarray(diag[prob0:prob0 + count])).to("cuda:0")
    bufs = {"grad": _nan_buffer(count + 2 * g, n), "Jp": _nan_buffer(count + 2 * g, m), "Ap": _nan_buffer(count + 2 * g, t_max),
            "lam1": _nan_buffer(count + 2 * g, t_max), "gres": _nan_buffer(count + 2 * g), "lam2": _nan_buffer(count + 2 * g, t_max)}
    sts = {k: torch.full((count + 2 * g,), ST_SENTINEL, dtype=torch.int32, device="cuda:0") for k in ("st1", "st2")}

    def base(b):
        return b.data_ptr() + g * b[0].numel() * b.element_size()
    torch.cuda.synchronize()
    assert s.gradient_batched_dev(prob0, count, base(bufs["grad"])) == 0
    assert s.jacobian_times_batched_dev(prob0, count, dp.data_ptr(), base(bufs["Jp"]), base(bufs["Ap"])) == 0
    assert s.first_lagrange_batched_dev(prob0, count, base(bufs["lam1"]), dgrad_fx=base(bufs["grad"]), ddiag_scale=dds.data_ptr(),
                                        dgrad_res=base(bufs["gres"]), dstatus=base(sts["st1"])) == 0
    assert s.second_lagrange_batched_dev(prob0, count, dp.data_ptr(), base(bufs["lam2"]), ddiag_scale=dds.data_ptr(),
                                         dstatus=base(sts["st2"])) == 0
    assert s.consumer_form() == cr.expected_form(n, t_max, small)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in bufs.items()}
    hs = {k: v.cpu().numpy() for k, v in sts.items()}
    for k, v in h.items():
        for guard in (v[:g], v[g + count:]):
            assert np.all(guard.view(np.uint64) == SENTINEL), k
    for k, v in hs.items():
        assert np.all(v[:g] == ST_SENTINEL) and np.all(v[g + count:] == ST_SENTINEL), k
        assert np.all(v[g:g + count] == 0), k
    # the range itself: bitwise the host forms, zeros past t_k
    sl = slice(prob0, prob0 + count)
    G = s.gradient_batched(n, prob0, count)
    Jp, Ap = s.jacobian_times_batched(m, t_max, P[sl], prob0)
    lam1, gres, _, _ = s.first_lagrange_batched(t_max, prob0, count, G, diag[sl])
    lam2, _, _ = s.second_lagrange_batched(t_max, P[sl], prob0, diag[sl])
    r = slice(g, g + count)
    assert same(h["grad"][r], G) and same(h["Jp"][r], Jp) and same(h["Ap"][r], Ap)
    assert same(h["lam1"][r], lam1) and same(h["gres"][r], gres) and same(h["lam2"][r], lam2)
    for j in range(count):
        tk = ts[prob0 + j]
        assert np.all(h["Ap"][g + j, tk:] == 0.0) and np.all(h["lam1"][g + j, tk:] == 0.0) and np.all(h["lam2"][g + j, tk:] == 0.0)
