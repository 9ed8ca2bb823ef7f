"""Ragged batches (enlsip_gn_solve_batched_ragged): every problem with its own number of active constraints t[k] <= t_max.
Each problem is checked against the CPU oracle on its own t[k] rows and against enlsip_gn_solve of that problem alone; the
padded output slots must be zero; with all t[k] == t_max the outputs must be bitwise those of enlsip_gn_solve_batched."""
import ctypes as C
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import gn_oracle as go, synth

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

TOL = 1e-11


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a)


def make_batch(m, n, ts, seed=0, deficient=()):
    """Problems with their own t_k; a problem listed in `deficient` gets a repeated constraint row (rank-deficient A')."""
    Js, rxs, As, cxs = [], [], [], []
    for k, tk in enumerate(ts):
        J, rx, A, cx = synth.make_problem(1000 * seed + k, m, n, int(tk))
        if k in deficient and tk >= 2:
            A = A.copy()
            A[-1] = A[0]
        Js.append(J); rxs.append(rx); As.append(A); cxs.append(cx)
    return Js, rxs, As, cxs


def run_ragged(s, Js, rxs, As, cxs):
    from enlsip_gn import GNSolver
    n = Js[0].shape[1]
    As_n = [A if A.size else np.zeros((0, n)) for A in As]
    At, cx, t = GNSolver.pack_ragged(As_n, cxs)
    J = np.stack([np.asfortranarray(Jk).T for Jk in Js])       # (batch, n, m): J[k].T is the m x n matrix
    rx = np.stack(rxs)
    return s.solve_batched_ragged(J, rx, At, cx, t), t, At, cx


def check_problem(out, k, tk, J, rx, A, cx, single=None, oracle=True):
    p, b, d, infos, jA, jL, jJ = out
    n = J.shape[1]
    kA = min(n, tk)
    rankA, rankJ2, code, dimA, dimJ2, status = infos[k]
    # padded slots
    assert np.all(b[k, tk:] == 0.0) and np.all(jA[k, tk:] == 0) and np.all(jL[k, kA:] == 0)
    if oracle:
        ref = go.gn_subproblem(J, rx, A, cx)
        assert (rankA, rankJ2, code) == (ref.rankA, ref.rankJ2, ref.code), (k, tk, infos[k], ref.rankA, ref.rankJ2, ref.code)
        assert rel(p[k], ref.p) <= TOL
        if code == 1:
            # a rank-deficient member repeats a constraint row: two equal columns of A' tie in the pivoting, and the reflectors
            # past rankA come from a residual at rounding level (J2's columns are not determined by the data); the single
            # solve below pins those pivots bit for bit
            assert np.array_equal(jA[k, :tk], ref.jpvtA)
            assert np.array_equal(jL[k, :kA], ref.jpvtL[:kA])
            assert np.array_equal(jJ[k, :rankJ2], ref.jpvtJ2[:rankJ2])
            if tk:
                assert rel(b[k, :tk], ref.b) <= 1e-10
    if single is not None:
        assert (rankA, rankJ2, code, dimA, dimJ2, status) == (single.rankA, single.rankJ2, single.code, single.dimA,
                                                              single.dimJ2, single.status)
        assert rel(p[k], single.p) <= TOL and rel(d[k], single.d) <= TOL
        if tk:
            assert rel(b[k, :tk], single.b) <= TOL
        assert np.array_equal(jA[k, :tk], single.jpvtA) and np.array_equal(jL[k, :kA], single.jpvtL)
        n2 = n - rankA
        assert np.array_equal(jJ[k, :n2], single.jpvtJ2[:n2])


# Every constraint route the header names, each reached at a shape that tests/dispatch_grid.expected_route (read-only) predicts
# for it: the ragged batch is routed by t_max as if it were uniform.  A retune of the thresholds that leaves a route without a
# candidate below fails the test instead of dropping the route from coverage.
ROOT = Path(__file__).resolve().parents[1]
CONSTRAINT_ROUTES = [nm.lower() for nm in
                     re.findall(r"ENLSIP_GN_ROUTE_(CONSTRAINT_\w+)", (ROOT / "include" / "enlsip_gn.h").read_text())]
CANDIDATES = [  # (m, n, t_max)
    (64, 16, 24), (128, 48, 40), (160, 64, 64), (192, 100, 40), (288, 200, 30), (480, 400, 16), (880, 800, 8),
    (680, 600, 20), (288, 200, 50), (480, 400, 30), (640, 512, 80), (160, 100, 120),
]


def t_vector(n, t_max):
    ts = [0, 1, t_max, max(t_max // 2, 1), t_max, max(t_max - 3, 0)]
    if t_max > n:
        ts.append(min(t_max, n + 1))         # a t_k > n
    ts.append(t_max)                         # rank-deficient member (last)
    return ts


def shapes_for(route):
    from dispatch_grid import expected_route
    out = [(m, n, tm) for (m, n, tm) in CANDIDATES if route in expected_route(len(t_vector(n, tm)), m, n, tm)]
    return out


def route_cases():
    cases = []
    for route in CONSTRAINT_ROUTES:
        sh = shapes_for(route)
        assert sh, f"no candidate shape reaches {route}"
        cases += [pytest.param(route, *x, id=f"{route}-{x[0]}x{x[1]}x{x[2]}") for x in sh[:2]]
    return cases


@pytest.mark.parametrize("route,m,n,t_max", route_cases())
def test_routes_against_oracle_and_single(solver, route, m, n, t_max):
    from dispatch_grid import expected_route
    ts = t_vector(n, t_max)
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=7, deficient=(len(ts) - 1,))
    out, t, _, _ = run_ragged(solver, Js, rxs, As, cxs)
    got = solver.route()
    want = {r for r in expected_route(len(ts), m, n, t_max) if r.startswith("constraint_")}
    assert route in got and want <= got, (want, got)
    infos = out[3]
    assert infos[-1][2] == -1 and infos[-1][0] < ts[-1]          # rank deficient: code -1
    from enlsip_gn import GNSolver
    single = GNSolver(device=0)
    try:
        for k, tk in enumerate(ts):
            sk = single.solve(Js[k], rxs[k], As[k] if tk else np.zeros((0, n)), cxs[k])
            check_problem(out, k, tk, Js[k], rxs[k], As[k] if tk else np.zeros((0, n)), cxs[k], single=sk)
    finally:
        single.close()


@pytest.mark.parametrize("pair", ["auto", "pairs"])
@pytest.mark.parametrize("m,n,t", [(512, 64, 8), (256, 32, 4), (1024, 256, 64)])
def test_uniform_t_bitwise(m, n, t, pair):
    from enlsip_gn import GNSolver
    old = os.environ.get("ENLSIP_GN_PAIR")
    if pair == "pairs":
        os.environ["ENLSIP_GN_PAIR"] = "1"
    try:
        s = GNSolver(device=0)
    finally:
        if pair == "pairs":
            if old is None:
                del os.environ["ENLSIP_GN_PAIR"]
            else:
                os.environ["ENLSIP_GN_PAIR"] = old
    try:
        batch = 6
        Js, rxs, As, cxs = make_batch(m, n, [t] * batch, seed=3)
        out_r, tv, At, cx = run_ragged(s, Js, rxs, As, cxs)
        J = np.stack([np.asfortranarray(Jk).T for Jk in Js])
        out_u = s.solve_batched(J, np.stack(rxs), At, cx)
        for a, b in zip(out_r, out_u):
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, b)
            else:
                assert a == b
    finally:
        s.close()


def test_no_needless_second_attempt(solver):
    m, n, t_max = 512, 64, 8
    ts = [1, 8, 3, 0, 5, 8, 2, 7]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=11)
    out, _, _, _ = run_ragged(solver, Js, rxs, As, cxs)
    assert "second_attempt" not in solver.route()
    for k in (0, 3, 5):
        check_problem(out, k, ts[k], Js[k], rxs[k], As[k] if ts[k] else np.zeros((0, n)), cxs[k])
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=12, deficient=(1,))
    out, _, _, _ = run_ragged(solver, Js, rxs, As, cxs)
    for k in (0, 1, 3):
        check_problem(out, k, ts[k], Js[k], rxs[k], As[k] if ts[k] else np.zeros((0, n)), cxs[k])


def test_pipelined_halves(solver):
    m, n, t_max = 1024, 128, 64
    batch = 128
    rng = np.random.default_rng(5)
    ts = list(rng.integers(48, 65, batch))
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=21)
    out, _, _, _ = run_ragged(solver, Js, rxs, As, cxs)
    assert "pipeline_split" in solver.route()
    for k in (0, 1, 63, 64, 65, 127):
        check_problem(out, k, ts[k], Js[k], rxs[k], As[k], cxs[k])


def test_chunks_above_launch_limit(solver):
    m, n, t_max = 32, 8, 4
    batch = 32768 + 40
    rng = np.random.default_rng(9)
    ts = rng.integers(0, t_max + 1, batch)
    J = rng.standard_normal((batch, n, m))
    rx = rng.standard_normal((batch, m))
    At = rng.standard_normal((batch, t_max, n))
    cx = rng.standard_normal((batch, t_max))
    out = solver.solve_batched_ragged(J, rx, At, cx, ts)
    assert "chunked" in solver.route()
    half = (batch + 1) // 2
    for k in (0, 1, half - 1, half, half + 1, batch - 1):
        tk = int(ts[k])
        check_problem(out, k, tk, J[k].T, rx[k], At[k, :tk], cx[k, :tk])


def test_rescued_members(solver):
    m, n, t_max = 256, 32, 4
    ts = [4, 2, 3, 0, 1, 4]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=31)
    Js[1] = Js[1] * 2.0 ** 600; rxs[1] = rxs[1] * 2.0 ** 600
    As[2] = As[2] * 2.0 ** -600; cxs[2] = cxs[2] * 2.0 ** -600
    out, _, _, _ = run_ragged(solver, Js, rxs, As, cxs)
    assert "rescaled" in solver.route()
    for k in range(len(ts)):
        A = As[k] if ts[k] else np.zeros((0, n))
        ref = go.gn_subproblem(Js[k], rxs[k], A, cxs[k])
        info = out[3][k]
        assert (info[0], info[1]) == (ref.rankA, ref.rankJ2)
        assert np.array_equal(out[4][k, :ts[k]], ref.jpvtA)
        assert rel(out[0][k], ref.p) <= TOL
    # accessors on the rescued problems answer in the caller's scale
    for k in (1, 2):
        A = As[k]
        ref = go.gn_subproblem(Js[k], rxs[k], A, cxs[k])
        R = solver.factor(0, k).R
        assert R.shape == ref.F_A.R.shape
        assert rel(np.abs(np.diag(R)), np.abs(ref.F_A.diagR())) <= 1e-12


def test_accessors_match_single(solver):
    from enlsip_gn import GNSolver
    m, n, t_max = 128, 16, 24
    ts = [24, 5, 12, 0, 17, 24]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=41, deficient=(5,))
    out, _, _, _ = run_ragged(solver, Js, rxs, As, cxs)
    single = GNSolver(device=0)
    rng = np.random.default_rng(0)
    try:
        for k in (0, 1, 2, 3, 4, 5):
            tk = ts[k]
            A = As[k] if tk else np.zeros((0, n))
            r = single.solve(Js[k], rxs[k], A, cxs[k])
            for which in (0, 1):
                fb, fs = solver.factor(which, k), single.factor(which, 0)
                assert fb.shape == fs.shape
                assert np.allclose(fb.R, fs.R, rtol=1e-12, atol=1e-13)
                assert np.array_equal(fb.p, fs.p)
            if tk:
                v = rng.standard_normal(tk)
                assert np.allclose(solver.factor(1, k).Qt_mul(v), single.factor(1, 0).Qt_mul(v), rtol=1e-12, atol=1e-13)
                assert np.allclose(solver.factor(1, k).Q_mul(v), single.factor(1, 0).Q_mul(v), rtol=1e-12, atol=1e-13)
            lb, gb = solver.first_lagrange(tk, prob=k)
            ls, gs = single.first_lagrange(tk)
            assert np.allclose(lb, ls, rtol=1e-10, atol=1e-12) and abs(gb - gs) <= 1e-10 * max(1.0, abs(gs))
            if tk:
                l2b = solver.second_lagrange(tk, out[0][k], prob=k)
                l2s = single.second_lagrange(tk, r.p)
                assert np.allclose(l2b, l2s, rtol=1e-10, atol=1e-12)
            pv = rng.standard_normal(n)
            Jpb, Apb = solver.jacobian_times(m, tk, pv, prob=k)
            Jps, Aps = single.jacobian_times(m, tk, pv)
            assert np.allclose(Jpb, Jps, rtol=1e-13) and np.allclose(Apb, Aps, rtol=1e-13)
            if k == 5:       # rank deficient: re-solve with code -1
                pb, bb, db = solver.resolve(m, n, tk, max(out[3][k][0] - 1, 0), out[3][k][4], -1, prob=k)
                ps, bs, ds = single.resolve(m, n, tk, max(r.rankA - 1, 0), r.dimJ2, -1)
                assert rel(pb, ps) <= TOL and rel(bb, bs) <= TOL
            if k == 1:       # full-rank member with t < n: Newton direction
                G = rng.standard_normal((n, n)); G = G + G.T
                pnb, eb = solver.newton_direction(G, prob=k)
                pns, es = single.newton_direction(G)
                assert eb == es and rel(pnb, pns) <= 1e-10
    finally:
        single.close()


def test_stale_workspace(solver):
    m, n = 256, 32
    ts = [1, 4, 0, 3]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=51)
    run_ragged(solver, Js, rxs, As, cxs)
    # a uniform solve with a larger t and NaN in the slots the next ragged solve leaves as padding
    t_big = 8
    Jb, rb, Ab, cb = make_batch(m, n, [t_big] * 4, seed=52)
    J = np.stack([np.asfortranarray(Jk).T for Jk in Jb])
    At = np.stack(Ab); cx = np.stack(cb)
    At[:, 4:, :] = np.nan
    cx[:, 4:] = np.nan
    solver.solve_batched(J, np.stack(rb), At, cx)
    out, _, _, _ = run_ragged(solver, Js, rxs, As, cxs)
    for arr in out[:3]:
        assert np.all(np.isfinite(arr))
    for k, tk in enumerate(ts):
        check_problem(out, k, tk, Js[k], rxs[k], As[k] if tk else np.zeros((0, n)), cxs[k])


@pytest.mark.parametrize("batch,m,n,t_max,tlo", [(1024, 512, 64, 8, 0), (8192, 256, 32, 4, 1)], ids=["C3", "C5"])
def test_full_size(solver, batch, m, n, t_max, tlo):
    rng = np.random.default_rng(61)
    ts = rng.integers(tlo, t_max + 1, batch)
    J = rng.standard_normal((batch, n, m))
    rx = rng.standard_normal((batch, m))
    At = rng.standard_normal((batch, t_max, n))
    cx = rng.standard_normal((batch, t_max))
    out = solver.solve_batched_ragged(J, rx, At, cx, ts)
    for k in list(range(0, batch, batch // 8)) + [batch - 1]:
        tk = int(ts[k])
        check_problem(out, k, tk, J[k].T, rx[k], At[k, :tk], cx[k, :tk])


def test_argument_errors(solver):
    from enlsip_gn import _lib as L
    lib, h = solver._lib, solver._h
    m, n, t_max, batch = 64, 16, 4, 3
    J = np.zeros((batch, n, m)) + 1.0
    rx = np.ones((batch, m)); At = np.ones((batch, t_max, n)); cx = np.ones((batch, t_max))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    def call(t, tm=t_max, ldat=n, sAt=n * t_max, A=At, c=cx):
        tv = None if t is None else np.ascontiguousarray(t, dtype=np.int64)
        return lib.enlsip_gn_solve_batched_ragged(h, batch, m, n, tm, None if tv is None else p(tv), p(J), m, m * n, p(rx),
                                                  None if A is None else p(A), ldat, sAt, None if c is None else p(c), 1e-8,
                                                  None, None, None, None, None, None, None)
    cases = [dict(t=None), dict(t=[1, -1, 2]), dict(t=[1, 5, 2]), dict(t=[1, 2, 3], tm=2000, sAt=n * 2000),
             dict(t=[1, 2, 3], ldat=n - 1, sAt=(n - 1) * t_max), dict(t=[1, 2, 3], sAt=n * t_max - 1), dict(t=[1, 2, 3], A=None),
             dict(t=[1, 2, 3], c=None)]
    for kw in cases:
        rc = call(**kw)
        assert rc < 0, kw
        assert lib.enlsip_gn_last_error(h)
    Js, rxs, As, cxs = make_batch(m, n, [1, 4, 2], seed=71)
    out, _, _, _ = run_ragged(solver, Js, rxs, As, cxs)
    check_problem(out, 1, 4, Js[1], rxs[1], As[1], cxs[1])


@pytest.mark.parametrize("scale", [600, -600])
def test_rescued_batch_of_one_with_garbage_padding(scale):
    """A ragged batch of ONE problem whose inputs need rescaling: it is solved with its own t[0] < t_max; what lies past t[0] in
    A' and cx (NaN here) is never read, and the accessors (F_A and F_L11 R) answer in the caller's scale."""
    from enlsip_gn import GNSolver
    m, n, t_max, tk = 256, 32, 8, 5
    J, rx, A, cx = synth.make_problem(4242, m, n, tk)
    if scale > 0:
        J, rx = J * 2.0 ** scale, rx * 2.0 ** scale
    else:
        A, cx = A * 2.0 ** scale, cx * 2.0 ** scale
    At = np.full((1, t_max, n), np.nan); At[0, :tk] = A
    cxp = np.full((1, t_max), np.nan); cxp[0, :tk] = cx
    s = GNSolver(device=0)
    single = GNSolver(device=0)
    try:
        out = s.solve_batched_ragged(np.asfortranarray(J).T[None].copy(), rx[None].copy(), At, cxp, np.array([tk]))
        assert "rescaled" in s.route()
        ref = go.gn_subproblem(J, rx, A, cx)
        r = single.solve(J, rx, A, cx)
        info = out[3][0]
        assert (info[0], info[1], info[2]) == (ref.rankA, ref.rankJ2, ref.code)
        assert np.array_equal(out[4][0, :tk], ref.jpvtA) and np.all(out[4][0, tk:] == 0) and np.all(out[1][0, tk:] == 0)
        assert rel(out[0][0], ref.p) <= TOL and rel(out[1][0, :tk], r.b) <= TOL
        for which in (0, 1):
            Rb, Rs = s.factor(which, 0).R, single.factor(which, 0).R
            assert Rb.shape == Rs.shape
            assert np.all(np.isfinite(Rb))
            assert rel(Rb, Rs) <= 1e-12
        assert rel(np.abs(s.factor(1, 0).diagR()), np.abs(ref.F_L11.diagR())) <= 1e-12
    finally:
        s.close()
        single.close()
