"""The batched constraint stage (enlsip_gn_factor_constraints_batched) and the solve that goes on with it
(enlsip_gn_solve_factored_batched): per problem the pair must leave what enlsip_gn_solve_batched_ragged leaves on the final working
sets, bit for bit, while the constraint kernels run only over the problems whose working set changed."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import synth

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

ROOT = Path(__file__).resolve().parents[1]
CONSTRAINT_ROUTES = [nm.lower() for nm in
                     re.findall(r"ENLSIP_GN_ROUTE_(CONSTRAINT_\w+)", (ROOT / "include" / "enlsip_gn.h").read_text())]
CANDIDATES = [  # (m, n, t_max): tests/test_gpu_ragged_batch.py's list, copied
    (64, 16, 24), (128, 48, 40), (160, 64, 64), (192, 100, 40), (288, 200, 30), (480, 400, 16), (880, 800, 8),
    (680, 600, 20), (288, 200, 50), (480, 400, 30), (640, 512, 80), (160, 100, 120),
]
FACTORS = (0, 1, 2)     # FACTOR_A, FACTOR_L11, FACTOR_J2


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ref_solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def same(a, b):
    """bit for bit, NaN payloads included"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return a.shape == b.shape and np.array_equal(a, b)


def same_outputs(got, want):
    for name, a, b in zip(("p", "b", "d", "info", "jpvtA", "jpvtL"), got, want):
        assert (same(a, b) if isinstance(a, np.ndarray) else a == b), name
    n = got[0].shape[1]
    for k, info in enumerate(want[3]):      # jpvtJ2 has n2 = n - rankA entries per problem; the library writes no others
        assert same(got[6][k, :n - info[0]], want[6][k, :n - info[0]]), ("jpvtJ2", k)


def same_factors(s, r, probs):
    for k in probs:
        for which in FACTORS:
            assert same(s.factor(which, k).R, r.factor(which, k).R), (k, which)
            assert same(s.factor(which, k).diagR(), r.factor(which, k).diagR()), (k, which)


def pack(Js, rxs, As, cxs, t_max):
    """The padded ragged layout with a given t_max (pack_ragged takes the largest t_k)."""
    n = Js[0].shape[1]
    B = len(Js)
    At, cx, t = np.zeros((B, t_max, n)), np.zeros((B, t_max)), np.zeros(B, dtype=np.int64)
    for k in range(B):
        t[k] = As[k].shape[0] if As[k].size else 0
        if t[k]:
            At[k, :t[k]] = As[k]
            cx[k, :t[k]] = cxs[k]
    J = np.stack([np.asfortranarray(Jk).T for Jk in Js])
    return J, np.stack(rxs), At, cx, t


def shapes_for(route):
    from dispatch_grid import expected_route
    from test_gpu_ragged_batch import t_vector
    return [(m, n, tm) for (m, n, tm) in CANDIDATES if route in expected_route(len(t_vector(n, tm)), m, n, tm)]


def route_cases():
    cases = []
    for route in CONSTRAINT_ROUTES:
        sh = shapes_for(route)
        assert sh, f"no candidate shape reaches {route}"
        cases.append(pytest.param(route, *sh[0], id=f"{route}-{sh[0][0]}x{sh[0][1]}x{sh[0][2]}"))
    return cases


def changed_start(As, cxs, n, t_max, seed):
    """The working sets the batch is factored with first, and the flags of the problems that change on the way to (As, cxs):
    problem 0 ends with t = 0 (starts with two rows), problem 2 gets its last row back, problem 3 drops a row it started with."""
    rows = synth.normal_stream(seed, 9, 3 * n).reshape(3, n)
    As0, cxs0 = [A.copy() for A in As], [np.array(c, dtype=np.float64, copy=True) for c in cxs]
    As0[0], cxs0[0] = rows[:min(2, t_max)].copy(), np.array([0.25, -0.5])[:min(2, t_max)]
    As0[2], cxs0[2] = As[2][:-1].copy(), cxs0[2][:-1].copy()
    As0[3], cxs0[3] = np.vstack([As[3], rows[2:3]]), np.append(cxs0[3], 0.125)
    flags = np.zeros(len(As), dtype=np.int64)
    flags[[0, 2, 3]] = 1
    return As0, cxs0, flags


# ---- 1. every constraint route: factor, change a third of the working sets, solve ------------------------------------------------
@pytest.mark.parametrize("route,m,n,t_max", route_cases())
def test_routes_bitwise_against_ragged(solver, ref_solver, route, m, n, t_max):
    from dispatch_grid import expected_route
    from test_gpu_ragged_batch import check_problem, make_batch, t_vector
    ts = t_vector(n, t_max)
    B = len(ts)
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=7, deficient=(B - 1,))
    As = [A if t else np.zeros((0, n)) for A, t in zip(As, ts)]
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    want = ref_solver.solve_batched_ragged(J, rx, At, cx, t)

    As0, cxs0, flags = changed_start(As, cxs, n, t_max, seed=m + n)
    _, _, At0, cx0, t0 = pack(Js, rxs, As0, cxs0, t_max)
    assert t0[0] > 0 and t[0] == 0 and t0[2] == t[2] - 1 and t0[3] == t[3] + 1 <= t_max
    infos0 = solver.factor_constraints_batched(m, At0, cx0, t0)
    assert solver.constraint_refactored() == B
    routes = {r for r in expected_route(B, m, n, t_max) if r.startswith("constraint_")}
    assert route in solver.route() and routes <= solver.route()
    assert infos0[1][:2] == (want[3][1][0], want[3][1][2])           # a kept problem: rankA, code already final
    # the slots of the kept problems are not read: poison them
    At1, cx1 = At.copy(), cx.copy()
    At1[flags == 0] = np.nan
    cx1[flags == 0] = np.nan
    got = solver.solve_factored_batched(J, rx, At1, cx1, t, flags)
    assert solver.constraint_refactored() == int(flags.sum()) == 3
    same_outputs(got, want)
    same_factors(solver, ref_solver, (4, 2))                          # one kept, one refactored
    assert want[3][-1][2] == -1 and want[3][-1][0] < ts[-1]           # the rank-deficient member
    for k, tk in enumerate(ts):
        check_problem(got, k, tk, Js[k], rxs[k], As[k], cxs[k])

    # no flag at all: no constraint kernel, the same bits
    solver.factor_constraints_batched(m, At, cx, t)
    got = solver.solve_factored_batched(J, rx, At1, cx1, t, None)
    assert solver.constraint_refactored() == 0
    same_outputs(got, want)
    same_factors(solver, ref_solver, (4, 2))


def test_every_constraint_route_has_a_shape():
    assert len(CONSTRAINT_ROUTES) == 12
    for route in CONSTRAINT_ROUTES:
        assert shapes_for(route), route


# ---- 2. the first estimate before any J -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,t_max", [(128, 48, 8), (192, 100, 20)])
def test_first_estimate_before_any_J(solver, ref_solver, m, n, t_max):
    from test_gpu_ragged_batch import make_batch
    ts = [t_max, 0, t_max // 2, 1, t_max, t_max - 1]
    B = len(ts)
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=13)
    As = [A if t else np.zeros((0, n)) for A, t in zip(As, ts)]
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    G = np.stack([Jk.T @ r for Jk, r in zip(Js, rxs)])
    ref_solver.solve_batched_ragged(J, rx, At, cx, t)
    lam_w, gres_w, st_w, rc_w = ref_solver.first_lagrange_batched(t_max, 0, B, G)
    infos = solver.factor_constraints_batched(m, At, cx, t)
    assert [i[0] for i in infos] == [min(n, tk) for tk in ts]
    lam, gres, st, rc = solver.first_lagrange_batched(t_max, 0, B, G)
    assert rc == rc_w and np.array_equal(st, st_w)
    assert solver.consumer_form() == ref_solver.consumer_form() == (1 if max(n, t_max) <= 64 else 0)
    if solver.consumer_form() == 0:
        assert same(lam, lam_w) and same(gres, gres_w)
    else:       # the wave-per-problem form: the rounding bound of tests/test_gpu_batched_multipliers.py
        for k in range(B):
            nb = np.linalg.norm(lam_w[k])
            assert np.linalg.norm(lam[k] - lam_w[k]) <= 1e-12 * nb if nb > 0 else not lam[k].any()
            assert abs(gres[k] - gres_w[k]) <= 1e-12 * abs(gres_w[k])
    # without grad_fx, and everything that needs J: the "only F_A / F_L11 are resident" error
    L = solver._lib
    out = np.zeros((B, max(n, m, t_max)))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.enlsip_gn_first_lagrange_batched(solver._h, 0, B, None, None, 1e-8, p(out), None, None) == -1
    assert b"only F_A / F_L11" in L.enlsip_gn_last_error(solver._h)
    assert L.enlsip_gn_second_lagrange_batched(solver._h, 0, B, p(out), None, 1e-8, p(out), None) == -1
    assert L.enlsip_gn_gradient_batched(solver._h, 0, B, p(out)) == -1
    assert L.enlsip_gn_get_diagR(solver._h, 2, 0, p(out)) == -1
    assert L.enlsip_gn_get_JQ1(solver._h, 0, p(np.zeros((n, m))), m) == -1
    # the constraint-side accessors answer with each problem's own t
    for k, tk in enumerate(ts):
        assert solver.factor(0, k).shape == (min(n, tk), tk)
        assert same(solver.factor(0, k).diagR(), ref_solver.factor(0, k).diagR())
        assert same(solver.factor(1, k).R, ref_solver.factor(1, k).R)
    assert same(solver.diagR_batched(0, t_max, 0, B), ref_solver.diagR_batched(0, t_max, 0, B))


# ---- 3. pipelined halves ----------------------------------------------------------------------------------------------------------
def test_pipelined_halves(solver, ref_solver):
    from test_gpu_ragged_batch import make_batch
    m, n, t_max, B = 96, 72, 5, 130
    ts = [(3 + k) % (t_max + 1) for k in range(B)]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=17)
    As = [A if t else np.zeros((0, n)) for A, t in zip(As, ts)]
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    want = ref_solver.solve_batched_ragged(J, rx, At, cx, t)
    assert ref_solver.pipeline_split() == 65
    # start: the flagged problems, on both sides of problem 65, with one row fewer (or one more when they end with none)
    flags = np.zeros(B, dtype=np.int64)
    flags[[1, 40, 64, 65, 66, 129]] = 1
    As0, cxs0 = list(As), list(cxs)
    extra = synth.normal_stream(5, 9, n)
    for k in np.flatnonzero(flags):
        if ts[k]:
            As0[k], cxs0[k] = As[k][:-1], np.asarray(cxs[k])[:-1]
        else:
            As0[k], cxs0[k] = extra[None, :], np.array([0.5])
    _, _, At0, cx0, t0 = pack(Js, rxs, As0, cxs0, t_max)
    solver.factor_constraints_batched(m, At0, cx0, t0)
    assert solver.pipeline_split() == 65 and solver.constraint_refactored() == B
    # a range of the first estimate that straddles the halves, between the two calls
    G = np.stack([Jk.T @ r for Jk, r in zip(Js, rxs)])
    lam, gres, st, _ = solver.first_lagrange_batched(t_max, 60, 10, G[60:70])
    from enlsip_gn import GNSolver
    one = GNSolver(device=0)
    try:
        for k in (60, 64, 65, 69):
            A0 = np.asarray(As0[k]).reshape(-1, n)
            one.factor_constraints(m, A0, cxs0[k])
            if t0[k]:
                lam1, gres1 = one.first_lagrange(int(t0[k]), G[k])
                assert np.linalg.norm(lam[k - 60, :t0[k]] - lam1) <= 1e-12 * np.linalg.norm(lam1)
                assert abs(gres[k - 60] - gres1) <= 1e-12 * max(abs(gres1), 1.0)
            assert not lam[k - 60, t0[k]:].any()
    finally:
        one.close()
    got = solver.solve_factored_batched(J, rx, At, cx, t, flags)
    assert solver.pipeline_split() == 65 and "pipeline_split" in solver.route()
    assert solver.constraint_refactored() == 6
    same_outputs(got, want)
    same_factors(solver, ref_solver, (0, 64, 65, 129))
    # a solve that would split differently: profiling toggled in between
    solver.factor_constraints_batched(m, At, cx, t)
    solver.set_profiling(True)
    try:
        with pytest.raises(Exception, match="error -1"):
            solver.solve_factored_batched(J, rx, At, cx, t, None)
    finally:
        solver.set_profiling(False)


# ---- 4. state errors --------------------------------------------------------------------------------------------------------------
def test_state_errors():
    import torch
    from enlsip_gn import GNSolver
    from test_gpu_ragged_batch import make_batch
    m, n, t_max, B = 48, 12, 4, 5
    ts = [4, 2, 0, 3, 4]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=19)
    As = [A if t else np.zeros((0, n)) for A, t in zip(As, ts)]
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    s = GNSolver(device=0)
    try:
        def rc_of(call):
            try:
                call()
            except Exception as e:      # GNError: "libenlsip_gn error <rc>: ..."
                return int(re.search(r"error (-?\d+)", str(e)).group(1))
            return 0
        assert rc_of(lambda: s.solve_factored_batched(J, rx, At, cx, t)) == -1            # no factor call
        s.factor_constraints_batched(m, At, cx, t)
        assert rc_of(lambda: s.solve_factored_batched(J[:4], rx[:4], At[:4], cx[:4], t[:4])) == -1      # another batch
        s.factor_constraints_batched(m, At, cx, t)
        At5, cx5 = np.concatenate([At, np.zeros((B, 1, n))], axis=1), np.concatenate([cx, np.zeros((B, 1))], axis=1)
        assert rc_of(lambda: s.solve_factored_batched(J, rx, At5, cx5, t)) == -1          # another t_max
        s.factor_constraints_batched(m, At, cx, t)
        t_bad = t.copy()
        t_bad[1] = 3
        with pytest.raises(Exception, match=r"error -6: t\[1\]"):
            s.solve_factored_batched(J, rx, At, cx, t_bad)
        s.solve_factored_batched(J, rx, At, cx, t)                                        # the state survives a -6
        # device form: another dAt
        dev = torch.device("cuda:0")
        dJ, drx = torch.from_numpy(J).to(dev), torch.from_numpy(rx).to(dev)
        dAt, dAt2, dcx = torch.from_numpy(At).to(dev), torch.from_numpy(At).to(dev), torch.from_numpy(cx).to(dev)
        s.factor_constraints_batched_dev(B, m, n, t_max, t, dAt.data_ptr(), n, n * t_max, dcx.data_ptr())
        args = (B, m, n, t_max, t, None, dJ.data_ptr(), m, m * n, drx.data_ptr())
        assert rc_of(lambda: s.solve_factored_batched_dev(*args, dAt2.data_ptr(), n, n * t_max, dcx.data_ptr())) == -11
        s.factor_constraints_batched_dev(B, m, n, t_max, t, dAt.data_ptr(), n, n * t_max, dcx.data_ptr())
        dp = torch.zeros((B, n), dtype=torch.float64, device=dev)
        s.solve_factored_batched_dev(*args, dAt.data_ptr(), n, n * t_max, dcx.data_ptr(), dp=dp.data_ptr())
        torch.cuda.synchronize()
        want = GNSolver(device=0)
        try:
            assert same(dp.cpu().numpy(), want.solve_batched_ragged(J, rx, At, cx, t)[0])
        finally:
            want.close()
        # above the launch limit: refused on the arguments alone (the pointers are never followed)
        big = 32769
        tb = np.zeros(big, dtype=np.int64)
        L, one = s._lib, C.c_void_p(8)
        assert L.enlsip_gn_factor_constraints_batched(s._h, big, m, n, t_max, tb.ctypes.data_as(C.c_void_p), one, n, n * t_max,
                                                      one, 1e-8, None) == -2
        assert L.enlsip_gn_solve_factored_batched_dev(s._h, big, m, n, t_max, tb.ctypes.data_as(C.c_void_p), None, one, m, m * n,
                                                      one, one, n, n * t_max, one, 1e-8, None, None, None, None, None, None,
                                                      None) == -2
    finally:
        s.close()


# ---- 5. magnitudes beyond the plain range -----------------------------------------------------------------------------------------
def test_magnitudes(solver, ref_solver):
    from test_gpu_ragged_batch import make_batch
    m, n, t_max, B = 64, 16, 4, 4
    ts = [4, 4, 3, 4]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=23)
    As[1], cxs[1] = As[1] * 2.0 ** 600, np.asarray(cxs[1]) * 2.0 ** 600       # kept
    Js[3], rxs[3] = Js[3] * 2.0 ** -600, rxs[3] * 2.0 ** -600
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    want = ref_solver.solve_batched_ragged(J, rx, At, cx, t)
    assert "rescaled" in ref_solver.route()
    As0, cxs0 = list(As), list(cxs)
    As0[2], cxs0[2] = np.vstack([As[2], synth.normal_stream(3, 9, n)[None, :]]), np.append(cxs[2], 0.5)
    _, _, At0, cx0, t0 = pack(Js, rxs, As0, cxs0, t_max)
    flags = np.array([0, 0, 1, 0])
    infos0 = solver.factor_constraints_batched(m, At0, cx0, t0)
    assert "rescaled" in solver.route() and infos0[1][:2] == (want[3][1][0], want[3][1][2])
    got = solver.solve_factored_batched(J, rx, At, cx, t, flags)
    assert "rescaled" in solver.route()
    assert got[3] == want[3]
    for a, b in zip(got[4:], want[4:]):
        assert np.array_equal(a, b)
    for a, b in zip(got[:3], want[:3]):
        for k in range(B):
            nb = np.linalg.norm(b[k])
            assert np.isfinite(a[k]).all() and np.linalg.norm(a[k] - b[k]) <= 1e-11 * nb


# ---- 6. the driver: update_working_set for a batch ----------------------------------------------------------------------------------
def test_driver_against_per_problem_loop(solver, ref_solver):
    from enlsip_gn import working_set as ws
    m, n, l, q, B = 40, 10, 6, 2, 8
    eps = ws.SQRT_EPS
    fires = [True, False, True, True, False, False, True, False]

    def build():
        Ws, Cs, its, Js, rxs, As, Gs, ps = [], [], [], [], [], [], [], []
        for k in range(B):
            A = synth.normal_stream(100 + k, 1, l * n).reshape(l, n)
            J = synth.normal_stream(100 + k, 2, m * n).reshape(m, n)
            rx = synth.normal_stream(100 + k, 3, m)
            W = ws.WorkingSet.create(q, l)
            W.add_constraint(1)                      # inequalities 3 and 4 active: t = 4
            W.add_constraint(1)
            assert W.t == 4 and list(W.active[:4]) == [1, 2, 3, 4]
            Aact = A[W.active[:W.t] - 1, :].copy()
            lam_star = np.ones(W.t)
            if fires[k]:
                lam_star[2 + k % 2] = -1.0           # a clearly negative multiplier at an inequality
            Ws.append(W); As.append(A); Js.append(J); rxs.append(rx)
            Cs.append(ws.Constraint(np.zeros(W.t), Aact, False, np.ones(W.t)))
            Gs.append(Aact.T @ lam_star)
            its.append(ws.IterationRecord()); ps.append(np.zeros(n))
        return Ws, Cs, its, Js, rxs, As, Gs, ps

    # the firing set on the CPU, from the host restatement of the estimate and the deletion test
    Ws, Cs, its, Js, rxs, As, Gs, ps = build()
    import scipy.linalg as sla

    class HostQR:
        def __init__(self, At):
            self.Q, self.R, p = sla.qr(At, pivoting=True)
            self.p = p + 1
        def Qt_mul(self, v):
            return self.Q.T @ v
    fired = []
    for k in range(B):
        it = ws.IterationRecord()
        lam = ws.first_lagrange_mult_estimate(Cs[k].A, Gs[k], Cs[k].cx, False, Cs[k].diag_scale, HostQR(Cs[k].A.T), it, eps)
        assert it.grad_res <= 1e-12
        fired.append(ws.check_constraint_deletion(q, Cs[k].A, lam, False, Cs[k].diag_scale, it.grad_res) != 0)
    assert fired == fires and any(fired) and not all(fired)

    ws.update_working_set_batched(solver, Ws, rxs, As, Cs, Gs, Js, ps, its, eps)
    Ws1, Cs1, its1, Js1, rxs1, As1, Gs1, ps1 = build()
    for k in range(B):
        ws.update_working_set(ref_solver, Ws1[k], rxs1[k], As1[k], Cs1[k], Gs1[k], Js1[k], ps1[k], its1[k], eps)

    def close(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return a.shape == b.shape and np.linalg.norm(a - b) <= 1e-11 * np.linalg.norm(b)
    for k in range(B):
        assert np.array_equal(Ws[k].active, Ws1[k].active) and Ws[k].t == Ws1[k].t, k
        assert (its[k].delete, its[k].index_del) == (its1[k].delete, its1[k].index_del), k
        assert (its[k].rankA, its[k].rankJ2, its[k].dimA, its[k].dimJ2) == (its1[k].rankA, its1[k].rankJ2, its1[k].dimA, its1[k].dimJ2)
        assert close(ps[k], ps1[k]) and close(its[k].b_gn, its1[k].b_gn) and close(its[k].d_gn, its1[k].d_gn), k
        assert close(its[k].lam, its1[k].lam), k
