"""GPU tests of the consumers around the subproblem on a row-sharded J (enlsip_gn_tsqr_products*, _first_lagrange, _second_lagrange):
products against correctly rounded references within the derived allowance of tests/tsqr_product_cases.py, bitwise identities
between the forms, the multiplier estimates against the mpmath references of tests/consumer_reference.py, the refusals, and real
ranks on the device over the callback exchange (tests/tsqr_products_worker.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import consumer_reference as cr
import tsqr_product_cases as pc
from oracle import gn_oracle as go

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = go.SQRT_EPS
U = cr.U
GUARD = 8
SENT = -7.25e77


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def same(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def dev(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda:0")


def fp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_REFS = {}


def case(name, n, with_p):
    key = (name, n, with_p)
    if key not in _REFS:
        heights = pc.splits()[name]
        J, rx, p = pc.problem(pc.case_seed(name, n, with_p), sum(heights), n, with_p)
        _REFS[key] = (J, rx, p, heights, pc.Reference(J, rx, p, len(heights)))
    return _REFS[key]


# ---- 1. products of every split against the references; in place == contiguous copies -------------------------------------------
@pytest.mark.parametrize("with_p", [False, True])
@pytest.mark.parametrize("n", pc.NS)
@pytest.mark.parametrize("name", list(pc.splits()))
def test_products_of_the_shards(solver, name, n, with_p):
    from enlsip_gn.tsqr import tsqr_products_shards_dev
    J, rx, p, heights, ref = case(name, n, with_p)
    Jd, rxd = dev(J.T), dev(rx)
    out = tsqr_products_shards_dev(solver, Jd, rxd, p, len(heights), row_blocks=list(heights))
    Jp = out.Jp.cpu().numpy() if with_p else None
    bad = ref.check(out.grad, out.sums, f"{name} n={n} p={with_p}", Jp)
    assert bad is None, bad
    if not with_p:
        assert out.sums[1] == 0.0 and out.sums[2] == 0.0
    # the shards read where they lie (odd start rows, ldj = m): the same bits
    inp = tsqr_products_shards_dev(solver, Jd, rxd, p, len(heights), row_blocks=list(heights), in_place=True)
    assert same(inp.grad, out.grad) and same(inp.sums, out.sums)
    if with_p:
        assert same(inp.Jp.cpu().numpy(), Jp)


def test_in_place_shard_at_an_odd_row_with_guards(solver):
    """One shard of CH + 1 rows starting at row 3 of a taller matrix: dJp holds exactly m_loc values between untouched guard rows,
    the message exactly msg_len doubles, and a fresh handle gives the bits of the reused one."""
    import torch
    from enlsip_gn import GNSolver
    from enlsip_gn.tsqr import hip_products_local, hip_products_combine, tsqr_products_msg_len
    CH, n, lo = pc.chunk_height(), 65, 3
    ml, m = CH + 1, CH + 1 + 3 + 5
    J, rx, p = pc.problem(4242, m, n)
    Jd, rxd, pd = dev(J.T), dev(rx), dev(p)
    L = tsqr_products_msg_len(n)
    res = []
    fresh = GNSolver(device=0)
    try:
        for s in (solver, fresh, solver):
            Jp = torch.full((ml + 2 * GUARD,), SENT, dtype=torch.float64, device="cuda:0")
            msg = torch.full((L + 2 * GUARD,), SENT, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            hip_products_local(s, ml, n, Jd.data_ptr() + 8 * lo, m, rxd.data_ptr() + 8 * lo, pd.data_ptr(), Jp.data_ptr() + 8 * GUARD,
                               msg.data_ptr() + 8 * GUARD)
            Jph, msgh = Jp.cpu().numpy(), msg.cpu().numpy()
            assert np.all(Jph[:GUARD] == SENT) and np.all(Jph[-GUARD:] == SENT) and np.all(Jph[GUARD:-GUARD] != SENT)
            assert np.all(msgh[:GUARD] == SENT) and np.all(msgh[-GUARD:] == SENT) and np.all(msgh[GUARD:-GUARD] != SENT)
            assert msgh[GUARD + 2] == n and msgh[GUARD] == 0.0 and msgh[GUARD + 1] == 0.0      # no communicator: not stated
            grad, sums = hip_products_combine(s, 1, n, msg.data_ptr() + 8 * GUARD)
            res.append((Jph, msgh, grad, sums))
    finally:
        fresh.close()
    ref = pc.Reference(J[lo:lo + ml], rx[lo:lo + ml], p, 1)
    bad = ref.check(res[0][2], res[0][3], "odd row", res[0][0][GUARD:-GUARD])
    assert bad is None, bad
    for r in res[1:]:
        assert all(same(a, b) for a, b in zip(r, res[0]))


# ---- 2./3./5. the collective forms on one rank: bitwise against the stage form, estimates against the references -------------------
def sharded_solve(s, J, rx, A, cx):
    from enlsip_gn.tsqr import tsqr_solve_lib
    import torch
    t = A.shape[0]
    Jd, rxd = dev(J.T), dev(rx)
    Atd, cxd = (dev(A), dev(cx)) if t else (None, None)
    torch.cuda.synchronize()
    out = tsqr_solve_lib(s, Jd, rxd, Atd, cxd, EPS)
    return out, (Jd, rxd, Atd, cxd)      # the caller keeps the shard alive


def judge(label, err, err_o, bound, first_order):
    """the rule of tests/test_gpu_consumer_edges.py: inside the bound, and within 8x the oracle's own error (or 32 u times the
    first-order amplification, where one rounding more or less in a cancelling right-hand side moves either error)"""
    assert err <= bound, (label, err, bound)
    limit = max(8.0 * err_o, 32.0 * U * first_order)
    assert err <= limit, (label, err, limit)


@pytest.mark.parametrize("name,n,t,kap", pc.ESTIMATE_CASES)
def test_collective_forms_on_one_rank(solver, name, n, t, kap):
    import torch
    from enlsip_gn import GNSolver, FACTOR_A
    from enlsip_gn.tsqr import (tsqr_products_lib, tsqr_first_lagrange_lib, tsqr_second_lagrange_lib, tsqr_products_shards_dev,
                                tsqr_transport, tsqr_exchange)
    m = pc.chunk_height() + 65
    J, rx, A, cx = cr.make_problem(8800 + n + t, m, n, t, kap)
    A = A.reshape(t, n)
    out, keep = sharded_solve(solver, J, rx, A, cx)
    before = (tsqr_transport(solver), tsqr_exchange(solver), solver.route())
    p = out.p
    # products: p = NULL and p given, against the references and, bit for bit, against the stage form with G = 1
    for pp in (None, p):
        ref = pc.Reference(J, rx, pp, 1)
        Jpd = torch.full((m + 2 * GUARD,), SENT, dtype=torch.float64, device="cuda:0") if pp is not None else None
        grad = np.full(n + 2, SENT)
        sums = np.full(5, SENT)
        Ap = np.full(t + 2, SENT)
        torch.cuda.synchronize()
        rc = solver._lib.enlsip_gn_tsqr_products(solver._h, fp(pp), C.c_void_p(Jpd.data_ptr() + 8 * GUARD) if pp is not None else None,
                                                 C.c_void_p(grad.ctypes.data + 8), C.c_void_p(sums.ctypes.data + 8),
                                                 C.c_void_p(Ap.ctypes.data + 8) if pp is not None else None)
        assert rc == 0, solver._lib.enlsip_gn_last_error(solver._h)
        assert grad[0] == SENT and grad[-1] == SENT and sums[0] == SENT and sums[-1] == SENT and Ap[0] == SENT and Ap[-1] == SENT
        Jp = None
        if pp is not None:
            Jph = Jpd.cpu().numpy()
            assert np.all(Jph[:GUARD] == SENT) and np.all(Jph[-GUARD:] == SENT)
            Jp = Jph[GUARD:-GUARD]
            Ap_ref, Ap_bound = cr.exact_matvec(A, pp) if t else (np.zeros(0), np.zeros(0))
            assert np.all(np.abs(Ap[1:-1] - Ap_ref) <= Ap_bound), (name, Ap[1:-1], Ap_ref)
        bad = ref.check(grad[1:-1], sums[1:-1], f"{name} p={pp is not None}", Jp)
        assert bad is None, bad
        stage = tsqr_products_shards_dev(solver, keep[0], keep[1], pp, 1)
        assert same(stage.grad, grad[1:-1]) and same(stage.sums, sums[1:-1])
        if pp is not None:
            assert same(stage.Jp.cpu().numpy(), Jp)
        lib2 = tsqr_products_lib(solver, n, t, pp)
        assert same(lib2.grad, grad[1:-1]) and same(lib2.sums, sums[1:-1])
    # the extracted exchange helper left the solve's bookkeeping as it was
    assert before == (tsqr_transport(solver), tsqr_exchange(solver), solver.route())
    assert before[0] == "none"
    # estimates
    diag = cr.random_diag(31, 1, t)[0]
    g_lib = tsqr_products_lib(solver, n, t, None).grad
    first = {}
    for ds in (None, diag):
        lam0, gres0 = tsqr_first_lagrange_lib(solver, n, t, None, ds, EPS)
        lam1, gres1 = tsqr_first_lagrange_lib(solver, n, t, g_lib, ds, EPS)
        assert same(lam0, lam1) and same(gres0, gres1), name      # grad_fx given == the NULL form fed its own gradient
        lam2 = tsqr_second_lagrange_lib(solver, n, t, p, ds, EPS)
        first[ds is not None] = (lam0, gres0, lam2)
    # the one-GPU calls on the same whole matrix
    s2 = GNSolver(device=0)
    try:
        s2.solve(J, rx, A, cx, EPS)
        one = {}
        for ds in (None, diag):
            l1, g1 = s2.first_lagrange(t, None, ds, EPS)
            one[ds is not None] = (l1, g1, s2.second_lagrange(t, p, ds, EPS))
        if t:
            F = s2.factor(FACTOR_A, 0)
            S, pr = cr.kept_set(F.p, F.diagR(), EPS)
        else:
            S, pr = [], 0
    finally:
        s2.close()
    g_exact = cr.exact_gradient(J, rx)
    if t == 0:
        for k in (False, True):
            assert abs(first[k][1] - np.linalg.norm(g_exact)) <= 4 * (m + n) * U * np.linalg.norm(np.abs(J).T @ np.abs(rx))
        return
    if name.endswith("dup"):
        assert pr < t                                  # the zero multipliers and grad_res of prankA < t are reached
    R = cr.EstimateReference(A, S)
    F_o = go.qr_colnorm(A.T)
    S_o = cr.kept_set(F_o.p, F_o.diagR(), EPS)[0]
    R_o = R if sorted(S_o) == sorted(S) else cr.EstimateReference(A, S_o)
    kS = cr.kappa(A[S])
    nz = np.zeros(t, bool)
    nz[S] = True
    for k, ds in ((False, None), (True, diag)):
        lam, gres, lam2 = first[k]
        assert np.all(lam[~nz] == 0.0) and np.all(lam2[~nz] == 0.0), (name, lam, S)
        lam_r, gres_r = R.first(g_exact, cx, ds)
        gam = cr.gamma_rhs(J, rx) * R.first_cancellation(g_exact, cx)
        it = go.IterationRecord()
        lam_o = go.first_lagrange_mult_estimate(A, J.T @ rx, cx, ds is not None, ds if ds is not None else np.ones(t), F_o, it, EPS)
        lam_ro, gres_ro = R_o.first(g_exact, cx, ds)
        bound = cr.estimate_bound(kS, gam)
        nrm = max(np.linalg.norm(g_exact), 1e-300)
        for tag, (l, g) in (("sharded", (lam, gres)), ("one-GPU", one[k][:2])):
            judge(f"{name} first {tag} ds={k}", cr.rel_err(l, lam_r), cr.rel_err(lam_o, lam_ro), bound, kS * gam)
            judge(f"{name} grad_res {tag} ds={k}", abs(g - gres_r) / nrm, abs(it.grad_res - gres_ro) / nrm, bound, kS * gam)
        if pr == n:
            assert gres == 0.0
        lam2_r = R.second(J, rx, p, ds)
        gam2 = cr.gamma_rhs(J, rx, p)
        lam2_o = go.second_lagrange_mult_estimate(J, F_o, rx, p, t, ds is not None, ds, EPS)
        lam2_ro = R_o.second(J, rx, p, ds)
        for tag, l in (("sharded", lam2), ("one-GPU", one[k][2])):
            judge(f"{name} second {tag} ds={k}", cr.rel_err(l, lam2_r), cr.rel_err(lam2_o, lam2_ro), cr.estimate_bound(kS, gam2), kS * gam2)


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(solver):
    import torch
    from enlsip_gn import GNSolver
    from enlsip_gn.tsqr import tsqr_scale, tsqr_products_msg_len, hip_products_local, hip_products_combine
    lib = solver._lib
    m, n, t = 300, 6, 2
    J, rx, A, cx = cr.make_problem(99, m, n, t)
    grad, sums, lam = np.full(n, SENT), np.full(3, SENT), np.full(t, SENT)
    gres = C.c_double(SENT)

    def collective(s):
        return (lib.enlsip_gn_tsqr_products(s._h, None, None, fp(grad), fp(sums), None),
                lib.enlsip_gn_tsqr_first_lagrange(s._h, None, None, EPS, fp(lam), C.byref(gres)),
                lib.enlsip_gn_tsqr_second_lagrange(s._h, fp(np.ones(n)), None, EPS, fp(lam)))

    def untouched():
        return np.all(grad == SENT) and np.all(sums == SENT) and np.all(lam == SENT) and gres.value == SENT

    s = GNSolver(device=0)
    try:
        assert collective(s) == (-7, -7, -7) and untouched()                     # no sharded solve on the handle
        assert b"shard" in lib.enlsip_gn_last_error(s._h)
        out, keep = sharded_solve(s, J, rx, A, cx)
        assert lib.enlsip_gn_tsqr_products(s._h, None, None, fp(grad), fp(sums), None) == 0
        grad[:] = SENT
        sums[:] = SENT
        s.solve(J, rx, A, cx)                                                      # an ordinary solve withdraws the shard
        assert collective(s) == (-7, -7, -7) and untouched()
        big, keep2 = sharded_solve(s, J * 2.0 ** 600, rx, A, cx)                   # rescaled
        assert tsqr_scale(s) != (0, 0)
        assert collective(s) == (-15, -15, -15) and untouched()
        assert b"rescaled" in lib.enlsip_gn_last_error(s._h)
        # the stateless local stage still answers on in-band data, on the same handle
        L = tsqr_products_msg_len(n)
        msg = torch.zeros((L,), dtype=torch.float64, device="cuda:0")
        Jd, rxd = keep[0], keep[1]
        torch.cuda.synchronize()
        hip_products_local(s, m, n, Jd.data_ptr(), m, rxd.data_ptr(), 0, 0, msg.data_ptr())
        g, sm = hip_products_combine(s, 1, n, msg.data_ptr())
        assert pc.Reference(J, rx, None, 1).check(g, sm, "local after a rescaled solve") is None
        # argument errors, nothing written
        before = msg.cpu().numpy().copy()
        v = lambda x: C.c_void_p(x) if x else None
        loc = lambda ml, nn, pJ, ld, prx, pm: lib.enlsip_gn_tsqr_products_local_dev(s._h, ml, nn, v(pJ), ld, v(prx), None, None, v(pm))
        assert loc(m, n, Jd.data_ptr(), m - 1, rxd.data_ptr(), msg.data_ptr()) == -5          # bad ldj
        assert loc(m, n, 0, m, rxd.data_ptr(), msg.data_ptr()) == -4                           # NULL dJ
        assert loc(m, n, Jd.data_ptr(), m, 0, msg.data_ptr()) == -6
        assert loc(m, 0, Jd.data_ptr(), m, rxd.data_ptr(), msg.data_ptr()) == -3
        assert loc(-1, n, Jd.data_ptr(), m, rxd.data_ptr(), msg.data_ptr()) == -2
        assert loc(m, n, Jd.data_ptr(), m, rxd.data_ptr(), 0) == -8
        assert same(msg.cpu().numpy(), before)
        # a message stack whose header names another n / another rank count / the wrong slot
        stack = torch.stack([msg, msg]).contiguous()
        stack[:, 0] = torch.tensor([1.0, 2.0], device="cuda:0")
        stack[:, 1] = 2.0
        torch.cuda.synchronize()
        comb = lambda: lib.enlsip_gn_tsqr_products_combine_dev(s._h, 2, n, C.c_void_p(stack.data_ptr()), fp(grad), fp(sums))
        assert comb() == 0
        grad[:] = SENT
        sums[:] = SENT
        for col, val in ((2, n + 1.0), (1, 3.0), (0, 1.0)):
            old = float(stack[1, col])
            stack[1, col] = val
            torch.cuda.synchronize()
            assert comb() == -13 and untouched()
            stack[1, col] = old
        assert lib.enlsip_gn_tsqr_products_combine_dev(s._h, 2, n, None, fp(grad), fp(sums)) == -4
        assert lib.enlsip_gn_tsqr_products_combine_dev(s._h, 0, n, C.c_void_p(stack.data_ptr()), fp(grad), fp(sums)) == -2
        # m_loc = 0 is legal: a zero message
        hip_products_local(s, 0, n, 0, 0, 0, 0, 0, msg.data_ptr())
        z = msg.cpu().numpy()
        assert z[2] == n and np.all(z[3:] == 0.0)
    finally:
        s.close()


# ---- real ranks on the device ----------------------------------------------------------------------------------------------------------
def run_ranks(world, port, extra_env=None):
    """each rank a process of its own under its own timeout; the test ends at the first non-zero exit"""
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **(extra_env or {}))
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, os.path.join(ROOT, "tests", "tsqr_products_worker.py")],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    from concurrent.futures import ThreadPoolExecutor, as_completed
    outs, failed = [None] * world, None
    with ThreadPoolExecutor(world) as pool:
        waits = {pool.submit(pr.communicate): r for r, pr in enumerate(procs)}
        for fut in as_completed(waits):
            r = waits[fut]
            outs[r] = fut.result()[0]
            if procs[r].returncode != 0 and failed is None:
                failed = (r, procs[r].returncode)
                for q in procs:                       # its peers wait in the exchange: end them now
                    if q.poll() is None:
                        q.terminate()
    assert failed is None, (failed, outs[failed[0]][-3000:])
    return outs


@pytest.mark.parametrize("world", [2, 3])
def test_real_ranks_over_the_callback_exchange(solver, world, tmp_path):
    import tsqr_products_worker as wk
    from enlsip_gn.tsqr import tsqr_products_shards_dev
    res = str(tmp_path / "res")
    outs = run_ranks(world, 29560 + world, {"TSQR_PRODUCTS_OUT": res})
    assert all("FAIL" not in o and " ok" in o for o in outs), outs
    got = [np.load(f"{res}.{r}.npz") for r in range(world)]
    for key in got[0].files:
        for r in range(1, world):
            assert same(got[r][key], got[0][key]), (key, r)                       # every rank: identical bits
    # the single-GPU rehearsal on the same split gives the bits of the multi-process run
    J, rx, A, cx, heights = wk.problem(world)
    p = got[0]["p"]
    for pp, tag in ((None, "g0"), (p, "gp")):
        reh = tsqr_products_shards_dev(solver, dev(J.T), dev(rx), pp, world, row_blocks=heights)
        assert same(reh.grad, got[0][tag + "_grad"]) and same(reh.sums, got[0][tag + "_sums"]), tag


def test_one_rank_rccl_self_gather():
    import ctypes.util
    if not (os.path.exists("/opt/rocm/lib/librccl.so.1") or ctypes.util.find_library("rccl")):
        return                                                                      # no librccl on this box: nothing to exercise
    outs = run_ranks(1, 29569, {"TSQR_PRODUCTS_RCCL": "1"})
    assert "FAIL" not in outs[0] and "transport rccl" in outs[0], outs[0]
