"""Batched consumers of a solve (enlsip_gn_gradient_batched, _jacobian_times_batched, _first_lagrange_batched,
_second_lagrange_batched and their _dev forms): every problem of a range against the per-problem entry points (<= 1e-12, same
status) and against the oracle's first/second_lagrange_mult_estimate (src/enlsip_functions.jl:461-537); the general form bitwise
the per-problem results; ragged batches, resident-rank mismatch, pipeline halves, rescue handles, chunks and argument errors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import gn_oracle as go, synth

pytestmark = pytest.mark.gpu
EPS = go.SQRT_EPS


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
def solver():
    s = _make_solver()
    yield s
    s.close()


@pytest.fixture(scope="module")
def solver_general():
    s = _make_solver(general=True)
    yield s
    s.close()


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a)


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- problems on the host ----------------------------------------------------------------------------------------------------
def host_batch(m, n, ts, seed, deficient=(), near=(), scale=None):
    """Problems with their own t_k; `deficient`: a repeated constraint row (rank-deficient A'); `near`: a row that repeats row 0 up
    to 1e-10 (rank-deficient under SQRT_EPS, full rank under 1e-14); `scale`: {k: factor of J_k, rx_k}."""
    probs = []
    for k, tk in enumerate(ts):
        J, rx, A, cx = synth.make_problem(5000 * seed + k, m, n, int(tk))
        A = A.copy()
        if k in deficient and tk >= 2:
            A[-1] = A[0]
        if k in near and tk >= 2:
            A[-1] = A[0] + 1e-10 * synth.normal_stream(91 + k, 7, n)
        if scale and k in scale:
            J, rx = J * scale[k], rx * scale[k]
        probs.append((J, rx, A, cx))
    return probs


def solve_host(s, probs, t_max, ragged):
    from enlsip_gn import GNSolver
    n = probs[0][0].shape[1]
    J = np.stack([np.asfortranarray(P[0]).T for P in probs])
    rx = np.stack([P[1] for P in probs])
    if ragged:
        At, cx, t = GNSolver.pack_ragged([P[2] if P[2].size else np.zeros((0, n)) for P in probs], [P[3] for P in probs])
        out = s.solve_batched_ragged(J, rx, At, cx, t)
    else:
        At = np.stack([P[2] for P in probs])
        cx = np.stack([P[3] for P in probs])
        out = s.solve_batched(J, rx, At, cx)
    return out[0]          # p (batch, n)


# ---- the per-problem entry points, raw return codes -------------------------------------------------------------------------
def per_first(s, k, tk, grad, ds, eps=EPS):
    lam, gres = np.zeros(max(tk, 1)), C.c_double(0.0)
    rc = s._lib.enlsip_gn_first_lagrange(s._h, k, _fp(grad), _fp(ds), eps, _fp(lam), C.byref(gres))
    return rc, lam[:tk], gres.value


def per_second(s, k, tk, p, ds, eps=EPS):
    lam = np.zeros(max(tk, 1))
    rc = s._lib.enlsip_gn_second_lagrange(s._h, k, _fp(np.ascontiguousarray(p)), _fp(ds), eps, _fp(lam))
    return rc, lam[:tk]


STATUS_OF_RC = {0: 0, 1: 1, -7: 2}


def same(a, b):
    """bit for bit, NaN payloads included"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def close(a, b, tol):
    return np.array_equal(a, b) if tol == 0 else rel(a, b) <= tol


def check_against_per_problem(s, B, m, n, t_max, ts, P, sample, tol, diag=None):
    """Every consumer over the whole batch (one call each) against the per-problem entry points on `sample`."""
    G = s.gradient_batched(n, 0, B)
    Jp, Ap = s.jacobian_times_batched(m, t_max, P, 0)
    for k in sample:
        tk = ts[k]
        assert close(G[k], s.gradient(n, k), tol)
        jp1, ap1 = s.jacobian_times(m, tk, P[k], k)
        assert close(Jp[k], jp1, tol) and close(Ap[k, :tk], ap1, tol)
        assert np.all(Ap[k, tk:] == 0.0)
    for ds in (None, diag):
        for grad in (G, None):
            lam, gres, st, rc = s.first_lagrange_batched(t_max, 0, B, grad, ds)
            assert rc == (1 if st.any() else 0)
            for k in sample:
                tk = ts[k]
                assert np.all(lam[k, tk:] == 0.0)
                if tk == 0 and grad is None:
                    continue            # the per-problem entry point has no gradient here (checked against the oracle)
                rc1, lam1, gres1 = per_first(s, k, tk, None if grad is None else G[k],
                                             None if ds is None else np.ascontiguousarray(ds[k, :tk]))
                assert STATUS_OF_RC[rc1] == st[k], (k, rc1, st[k])
                assert close(lam[k, :tk], lam1, tol), (k, rel(lam[k, :tk], lam1))
                assert close(np.array([gres[k]]), np.array([gres1]), tol)
        lam2, st2, rc2 = s.second_lagrange_batched(t_max, P, 0, ds)
        assert rc2 == (1 if st2.any() else 0)
        for k in sample:
            tk = ts[k]
            assert np.all(lam2[k, tk:] == 0.0)
            rc1, lam1 = per_second(s, k, tk, P[k], None if ds is None else np.ascontiguousarray(ds[k, :tk]))
            assert STATUS_OF_RC[rc1] == st2[k]
            assert close(lam2[k, :tk], lam1, tol)
    return G


def check_against_oracle(s, probs, ts, t_max, P, sample, G, diag):
    for k in sample:
        J, rx, A, cx = probs[k]
        tk = ts[k]
        grad = J.T @ rx
        assert rel(G[k], grad) <= 1e-13
        if tk == 0:
            lam, gres, st, _ = s.first_lagrange_batched(t_max, k, 1, None, None)
            assert abs(gres[0] - np.linalg.norm(grad)) <= 1e-10 * np.linalg.norm(grad) and st[0] == 0
            continue
        ref = go.gn_subproblem(J, rx, A, cx)
        for scaling in (False, True):
            ds = diag[k, :tk] if scaling else np.ones(tk)
            it = go.IterationRecord()
            lam_ref = go.first_lagrange_mult_estimate(A, grad, cx, scaling, ds, ref.F_A, it, EPS)
            dsb = diag[k:k + 1] if scaling else None
            for gfx in (grad[None, :], None):
                lam, gres, st, _ = s.first_lagrange_batched(t_max, k, 1, gfx, dsb)
                assert rel(lam[0, :tk], lam_ref) <= 1e-10
                assert abs(gres[0] - it.grad_res) <= 1e-10 * max(1.0, abs(it.grad_res))
            lam2_ref = go.second_lagrange_mult_estimate(J, ref.F_A, rx, ref.p, tk, scaling, ds)
            lam2, st2, _ = s.second_lagrange_batched(t_max, P[k:k + 1], k, dsb)
            assert rel(lam2[0, :tk], lam2_ref) <= 1e-9


def random_diag(B, t_max, seed):
    return 1.0 + 0.25 * np.abs(synth.normal_stream(seed, 5, B * max(t_max, 1))).reshape(B, max(t_max, 1))[:, :t_max].copy()


# ---- 1. parity on host-generated shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,m,n,t,form", [(48, 256, 32, 4, 1), (24, 512, 64, 8, 1), (6, 300, 100, 70, 0)])
def test_parity_uniform(solver, B, m, n, t, form):
    probs = host_batch(m, n, [t] * B, seed=B + n)
    P = solve_host(solver, probs, t, ragged=False)
    diag = random_diag(B, t, 11)
    ts = [t] * B
    G = check_against_per_problem(solver, B, m, n, t, ts, P, range(B), 1e-12, diag)
    assert solver.consumer_form() == form
    check_against_oracle(solver, probs, ts, t, P, range(0, B, max(1, B // 8)), G, diag)


def test_ragged_batch(solver, solver_general):
    """t_k = 0 members and a rank-deficient A'; padded lambda and Ap slots exactly 0 (C3 shape: the wave form by default)."""
    m, n, t_max = 512, 64, 8
    ts = [8, 0, 5, 8, 3, 0, 8, 1, 7, 2]
    probs = host_batch(m, n, ts, seed=3, deficient=(3, 8))
    diag = random_diag(len(ts), t_max, 12)
    for s, form in ((solver, 1), (solver_general, 0)):
        P = solve_host(s, probs, t_max, ragged=True)
        G = check_against_per_problem(s, len(ts), m, n, t_max, ts, P, range(len(ts)), 1e-12 if form else 0, diag)
        assert s.consumer_form() == form
        check_against_oracle(s, probs, ts, t_max, P, range(len(ts)), G, diag)


# ---- 2. the general form is bitwise the per-problem path -----------------------------------------------------------------------
@pytest.mark.parametrize("B,m,n,t", [(40, 256, 32, 4), (16, 512, 64, 8)])
def test_general_form_bitwise(solver_general, B, m, n, t):
    probs = host_batch(m, n, [t] * B, seed=7 + n)
    P = solve_host(solver_general, probs, t, ragged=False)
    check_against_per_problem(solver_general, B, m, n, t, [t] * B, P, range(B), 0, random_diag(B, t, 13))
    assert solver_general.consumer_form() == 0


# ---- 3. resident-rank mismatch of the second estimate ----------------------------------------------------------------------------
def test_second_estimate_rank_mismatch(solver):
    m, n, t = 256, 32, 4
    B = 8
    probs = host_batch(m, n, [t] * B, seed=17, near=(3,))
    P = solve_host(solver, probs, t, ragged=False)
    eps = 1e-14
    lam, st, rc = solver.second_lagrange_batched(t, P, 0, None, eps_rank=eps)
    assert rc == 1 and st[3] == 2 and st.sum() == 2
    rc1, _ = per_second(solver, 3, t, P[3], None, eps)
    assert rc1 == -7
    for k in range(B):
        if k == 3:
            continue
        rc1, lam1 = per_second(solver, k, t, P[k], None, eps)
        assert rc1 == 0 and rel(lam[k], lam1) <= 1e-12
        J, rx, A, cx = probs[k]
        ref = go.gn_subproblem(J, rx, A, cx)
        assert rel(lam[k], go.second_lagrange_mult_estimate(J, ref.F_A, rx, ref.p, t, False, np.ones(t), eps)) <= 1e-9


# ---- 5. routing: pipeline halves, rescue handles, chunks ------------------------------------------------------------------------
def _solve_dev(s, J, rx, At, cx):
    B, n, m = J.shape
    t = At.shape[1]
    p = torch.empty((B, n), dtype=torch.float64, device=J.device)
    torch.cuda.synchronize()
    s.solve_batched_dev(B, m, n, t, J.data_ptr(), m, m * n, rx.data_ptr(), At.data_ptr(), n, n * t, cx.data_ptr(), EPS,
                        dp=p.data_ptr())
    s.synchronize()
    return p


def test_pipeline_split_range(solver):
    from enlsip_gn import workload as wl
    B, m, n, t = 192, 1024, 256, 32
    J, rx, At, cx = wl.make_batch(300, B, m, n, t, "cuda:0")
    p = _solve_dev(solver, J, rx, At, cx)
    split = solver.pipeline_split()
    assert 0 < split < B
    P = p.cpu().numpy()
    rng = np.random.default_rng(5)
    sample = sorted({0, split - 1, split, B - 1, *rng.choice(B, 12, replace=False).tolist()})
    diag = random_diag(B, t, 14)
    G = check_against_per_problem(solver, B, m, n, t, [t] * B, P, sample, 1e-12, diag)
    assert solver.consumer_form() == 0
    probs = {k: (np.asfortranarray(J[k].cpu().numpy().T), rx[k].cpu().numpy(), At[k].cpu().numpy().reshape(t, n),
                 cx[k].cpu().numpy()) for k in sample[:4]}
    check_against_oracle(solver, probs, {k: t for k in probs}, t, P, list(probs), G, diag)
    # a range straddling the split, device buffers
    p0, cnt = split - 3, 7
    lam = torch.full((cnt, t), 7.0, dtype=torch.float64, device="cuda:0")
    gres = torch.zeros(cnt, dtype=torch.float64, device="cuda:0")
    st = torch.full((cnt,), 9, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rc = solver.first_lagrange_batched_dev(p0, cnt, lam.data_ptr(), dgrad_res=gres.data_ptr(), dstatus=st.data_ptr())
    assert rc == 0 and int(st.abs().sum()) == 0
    lam_h, gres_h = lam.cpu().numpy(), gres.cpu().numpy()
    for j in range(cnt):
        rc1, lam1, gres1 = per_first(solver, p0 + j, t, None, None)
        assert rc1 == 0 and rel(lam_h[j], lam1) <= 1e-12 and abs(gres_h[j] - gres1) <= 1e-12 * max(1.0, gres1)
    Jp = torch.zeros((cnt, m), dtype=torch.float64, device="cuda:0")
    assert solver.jacobian_times_batched_dev(p0, cnt, p[p0:p0 + cnt].contiguous().data_ptr(), dJp=Jp.data_ptr()) == 0
    for j in range(cnt):
        assert rel(Jp[j].cpu().numpy(), solver.jacobian_times(m, t, P[p0 + j], p0 + j)[0]) <= 1e-12


def test_rescued_member(solver):
    """A problem scaled by 2^600 lives on a rescue handle: its slots are bitwise what the per-problem entry points return (J' rx
    overflows to NaN there, as in the reference: compared bit for bit)."""
    m, n, t = 256, 32, 4
    B = 8
    probs = host_batch(m, n, [t] * B, seed=23, scale={2: 2.0 ** 600})
    P = solve_host(solver, probs, t, ragged=False)
    assert "rescaled" in solver.route()
    diag = random_diag(B, t, 15)
    G = solver.gradient_batched(n, 0, B)
    assert same(G[2], solver.gradient(n, 2))
    Jp, Ap = solver.jacobian_times_batched(m, t, P, 0)
    jp1, ap1 = solver.jacobian_times(m, t, P[2], 2)
    assert same(Jp[2], jp1) and same(Ap[2], ap1)
    for grad in (G, None):
        lam, gres, st, rc = solver.first_lagrange_batched(t, 0, B, grad, diag)
        rc1, lam1, gres1 = per_first(solver, 2, t, None if grad is None else G[2], np.ascontiguousarray(diag[2]))
        assert same(lam[2], lam1) and same(gres[2], gres1) and st[2] == STATUS_OF_RC[rc1]
        for k in (0, 1, 3, B - 1):
            rc1, lam1, gres1 = per_first(solver, k, t, None if grad is None else G[k], np.ascontiguousarray(diag[k]))
            assert rel(lam[k], lam1) <= 1e-12 and st[k] == STATUS_OF_RC[rc1]
    lam2, st2, rc2 = solver.second_lagrange_batched(t, P, 0, diag)
    rc1, lam1 = per_second(solver, 2, t, P[2], np.ascontiguousarray(diag[2]))
    assert same(lam2[2], lam1) and st2[2] == STATUS_OF_RC[rc1]
    for k in (0, 1, 3, B - 1):
        rc1, lam1 = per_second(solver, k, t, P[k], np.ascontiguousarray(diag[k]))
        assert rel(lam2[k], lam1) <= 1e-12 and st2[k] == STATUS_OF_RC[rc1]


def test_chunked_batch(solver):
    """40 000 C5-shaped problems run in two chunks: a range inside the resident (last) chunk works, one reaching the first fails."""
    from enlsip_gn import workload as wl
    B, m, n, t = 40000, 256, 32, 4
    J, rx, At, cx = wl.make_batch(0, B, m, n, t, "cuda:0")
    p = _solve_dev(solver, J, rx, At, cx)
    assert "chunked" in solver.route()
    p0, cnt = 39000, 1000
    lam = torch.zeros((cnt, t), dtype=torch.float64, device="cuda:0")
    st = torch.zeros(cnt, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert solver.first_lagrange_batched_dev(p0, cnt, lam.data_ptr(), dstatus=st.data_ptr()) == 0
    lam2 = torch.zeros((cnt, t), dtype=torch.float64, device="cuda:0")
    assert solver.second_lagrange_batched_dev(p0, cnt, p[p0:].contiguous().data_ptr(), lam2.data_ptr()) == 0
    P = p.cpu().numpy()
    for j in (0, 1, 517, cnt - 1):
        _, lam1, _ = per_first(solver, p0 + j, t, None, None)
        assert rel(lam[j].cpu().numpy(), lam1) <= 1e-12
        _, lam1 = per_second(solver, p0 + j, t, P[p0 + j], None)
        assert rel(lam2[j].cpu().numpy(), lam1) <= 1e-12
    rc = solver._lib.enlsip_gn_first_lagrange_batched_dev(solver._h, 19990, 20, None, None, EPS, C.c_void_p(lam.data_ptr()),
                                                         None, None)
    assert rc == -3 and b"earlier chunk" in solver._lib.enlsip_gn_last_error(solver._h)
    del J, rx, At, cx
    torch.cuda.empty_cache()


# ---- 6. argument errors; after enlsip_gn_factor_constraints ---------------------------------------------------------------------
def test_argument_errors(solver):
    fresh = _make_solver()
    try:
        lam = np.zeros(16)
        assert fresh._lib.enlsip_gn_first_lagrange_batched(fresh._h, 0, 1, None, None, EPS, _fp(lam), None, None) == -1
        form = C.c_int(5)
        assert fresh._lib.enlsip_gn_get_consumer_form(fresh._h, C.byref(form)) == 0 and form.value == -1
    finally:
        fresh.close()
    m, n, t, B = 256, 32, 4, 4
    P = solve_host(solver, host_batch(m, n, [t] * B, seed=29), t, ragged=False)
    L, h = solver._lib, solver._h
    lam, G, Jp = np.zeros(B * t), np.zeros(B * n), np.zeros(B * m)
    pv = np.ascontiguousarray(P)
    assert L.enlsip_gn_first_lagrange_batched(h, 0, 0, None, None, EPS, _fp(lam), None, None) == -2
    assert L.enlsip_gn_gradient_batched(h, 1, B, _fp(G)) == -3
    assert L.enlsip_gn_second_lagrange_batched(h, -1, 2, _fp(pv), None, EPS, _fp(lam), None) == -3
    assert L.enlsip_gn_jacobian_times_batched(h, 0, B, _fp(pv), None, None) == -4
    assert L.enlsip_gn_jacobian_times_batched(h, 0, B, _fp(pv), _fp(Jp), None) == 0
    assert L.enlsip_gn_second_lagrange_batched(h, 0, B, None, None, EPS, _fp(lam), None) == -4
    # the single-problem handle of enlsip_gn_factor_constraints: grad_fx required, no second estimate
    J, rx, A, cx = host_batch(m, n, [t], seed=31)[0]
    solver.factor_constraints(m, A, cx)
    grad = J.T @ rx
    lam_b, gres_b, st_b, rc = solver.first_lagrange_batched(t, 0, 1, grad[None, :], None)
    lam1, gres1 = solver.first_lagrange(t, grad, None)
    assert rc == 0 and rel(lam_b[0], lam1) <= 1e-12 and abs(gres_b[0] - gres1) <= 1e-12 * max(1.0, gres1)
    assert L.enlsip_gn_first_lagrange_batched(h, 0, 1, None, None, EPS, _fp(lam), None, None) == -1
    assert L.enlsip_gn_second_lagrange_batched(h, 0, 1, _fp(grad[:n].copy()), None, EPS, _fp(lam), None) == -1


# ---- 7. no side effects ---------------------------------------------------------------------------------------------------------
def test_no_side_effects(solver):
    from enlsip_gn import FACTOR_A, FACTOR_J2
    m, n, t, B = 512, 64, 8, 12
    probs = host_batch(m, n, [t] * B, seed=37)
    P = solve_host(solver, probs, t, ragged=False)
    before = [(solver.factor(FACTOR_A, k).R, solver.factor(FACTOR_J2, k).R, per_first(solver, k, t, None, None)[1],
               per_second(solver, k, t, P[k], None)[1], solver.JQ1(m, n, k)) for k in (0, 5, B - 1)]
    solver.gradient_batched(n, 0, B)
    solver.jacobian_times_batched(m, t, P, 0)
    solver.first_lagrange_batched(t, 0, B)
    solver.second_lagrange_batched(t, P, 0)
    after = [(solver.factor(FACTOR_A, k).R, solver.factor(FACTOR_J2, k).R, per_first(solver, k, t, None, None)[1],
              per_second(solver, k, t, P[k], None)[1], solver.JQ1(m, n, k)) for k in (0, 5, B - 1)]
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(a, b)
    assert np.array_equal(solve_host(solver, probs, t, ragged=False), P)
