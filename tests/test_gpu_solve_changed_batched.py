"""The changed-problems solve (enlsip_gn_solve_changed_batched): on a fully solved resident ragged batch, the problems with a flag
get their constraint stage AND their Jacobian side again, in place.  Per flagged problem the outputs and the resident factors must
be bit for bit what enlsip_gn_solve_batched_ragged on the whole batch with the final working sets leaves; of an unflagged problem
no output slot and no resident factor may change; the Jacobian-side kernels are launched over exactly the flagged problems."""
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
HOLD = -2
JAC_ROUTES = [nm for nm in (x.lower() for x in re.findall(r"ENLSIP_GN_ROUTE_((?:JQ1|SWEEP|PIVOT)_\w+)",
                                                         (ROOT / "include" / "enlsip_gn.h").read_text()))]
NOT_RUN = {"jq1_rows64", "sweep_upper_input"}      # leading dimensions beyond 2^23 / the TSQR combine stage only
SHAPES = [(256, 32, 4), (40, 32, 4), (300, 64, 1), (192, 128, 64), (320, 256, 64), (448, 384, 64), (576, 512, 64), (192, 100, 40),
          (600, 91, 0), (700, 129, 3), (900, 257, 1), (1000, 449, 1), (1100, 513, 0), (700, 600, 20), (20, 100, 4)]
# bits no default handle reaches at a small size: (environment set before the handle is created, handle flags)
OWN_HANDLE = {"sweep_pairs": ({"ENLSIP_GN_PAIR": "1"}, 0), "sweep_lookahead": ({"ENLSIP_GN_PAIR": "1", "ENLSIP_GN_LOOKAHEAD": "1"}, 0),
              "jq1_plain": ({}, 2), "sweep_reflectors": ({}, 2), "pivot_steps": ({"ENLSIP_GN_QRCP_HYBRID": "0"}, 0),
              "sweep_xmap": ({"ENLSIP_GN_PAIR": "1", "ENLSIP_GN_LOOKAHEAD": "0"}, 0)}
# more than 512 rows of R0; 16 tiles for the XCD-local grid of a pair's far update (at most 8 problems); the others: (1100, 200, 8)
OWN_SHAPE = {"pivot_steps": (1100, 600, 8), "sweep_xmap": (8192, 100, 8)}
UNIFORM = {"sweep_lookahead", "sweep_xmap"}        # both need one width for the whole part


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


def snapshot(s, probs):
    FACTORS = (0, 1, 2)
    return {(k, w): (s.factor(w, k).R, s.factor(w, k).diagR(), s.factor(w, k).p) for k in probs for w in FACTORS}


def assert_snapshot(s, snap):
    from test_gpu_factored_batched import same
    for (k, w), (R, dg, piv) in snap.items():
        F = s.factor(w, k)
        assert same(F.R, R) and same(F.diagR(), dg) and np.array_equal(F.p, piv), (k, w)


def assert_flagged(got, want, flags, s=None, r=None):
    """flagged slots bitwise `want`, unflagged slots still as the wrapper made them (NaN / zero); factors of the flagged bitwise"""
    from test_gpu_factored_batched import same
    n = got[0].shape[1]
    for k in range(len(flags)):
        if flags[k]:
            for i in (0, 1, 2, 4, 5):
                assert same(got[i][k], want[i][k]), (k, i)
            assert got[3][k] == want[3][k], (k, got[3][k], want[3][k])
            n2 = n - want[3][k][0]
            assert same(got[6][k, :n2], want[6][k, :n2]), k
            if s is not None:
                for w in (0, 1, 2):
                    assert same(s.factor(w, k).R, r.factor(w, k).R), (k, w)
                    assert same(s.factor(w, k).diagR(), r.factor(w, k).diagR()), (k, w)
                    assert np.array_equal(s.factor(w, k).p, r.factor(w, k).p), (k, w)
        else:
            assert all(np.isnan(got[i][k]).all() for i in (0, 1, 2)), k
            assert not any(got[i][k].any() for i in (4, 5, 6)) and got[3][k] == (0, 0, 0, 0, 0, 0), k


def jacobian_route(B, m, n, t_max, t_min):
    """The Jacobian-side bits of a ragged batch: J*Q1 is chosen from t_max (the plan's kA), the sweep and the pivoted stage from
    the launch width n - min(n, t_min); the fused small kernel needs both."""
    from dispatch_grid import PB, Q1R_MAXK, expected_route
    by_max, by_min = expected_route(B, m, n, t_max), expected_route(B, m, n, t_min)
    n2 = n - min(n, t_min)
    fused = m <= 256 and n <= 32 and min(n, t_max) <= Q1R_MAXK and 1 <= n2 < PB and m >= n2       # small_fused_applies
    r = {b for b in by_max if b.startswith("jq1_") and b != "jq1_fused_small"}
    if fused:
        return {"jq1_fused_small"} | {b for b in by_min if b.startswith("pivot_")}
    if "jq1_fused_small" in by_max:
        r.add("jq1_rows32")
    return r | {b for b in by_min if b.startswith(("sweep_", "pivot_"))}


def case_for(route):
    """(m, n, t_max, B, t_min): the cheapest candidate whose prediction holds the bit; t_min = 0 (problem 0 ends without a
    constraint) where that reaches it, else 1"""
    from test_gpu_factored_batched import CANDIDATES
    best = None
    for (m, n, tm) in SHAPES + CANDIDATES:
        if tm < 1:
            continue            # the flow needs a row to gain and one to lose
        for tmin in (0, 1):
            if tmin > tm:
                continue
            for B in ((1,) if route == "pivot_wave32" else (5,)):
                if route in jacobian_route(B, m, n, tm, tmin):
                    cost = B * m * n * n
                    if best is None or cost < best[0]:
                        best = (cost, (m, n, tm, B, tmin))
    return best[1] if best else None


def route_cases():
    cases = []
    for route in JAC_ROUTES:
        if route in NOT_RUN:
            continue
        if route in OWN_HANDLE:
            m, n, tm = OWN_SHAPE.get(route, (1100, 200, 8))
            # the look-ahead sweep and the grid remap need one width for the whole part: every problem ends with t_max rows (t_min = -1)
            cases.append(pytest.param(route, m, n, tm, 5, -1 if route in UNIFORM else 0, id=f"{route}-{m}x{n}x{tm}"))
            continue
        c = case_for(route)
        if c is not None:
            cases.append(pytest.param(route, *c, id=f"{route}-{c[0]}x{c[1]}x{c[2]}x{c[3]}"))
    return cases


def final_sets(m, n, t_max, B, t_min, seed):
    """final working sets: problem 0 ends with t_min rows, the others between 1 and t_max; B = 1: the one problem loses a row"""
    from test_gpu_ragged_batch import make_batch
    if B == 1:
        ts = [max(t_max - 1, 0)]
    elif t_min < 0:
        ts = [t_max] * B
    else:
        ts = [t_min, max(t_max // 2, 1), t_max, t_max - 1, t_max] + [t_max] * (B - 5)
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=seed)
    As = [A if t else np.zeros((0, n)) for A, t in zip(As, ts)]
    return ts, Js, rxs, As, cxs


def start_sets(As, cxs, n, t_max, seed):
    """as test_gpu_factored_batched.changed_start: problem 0 starts with one row more than it ends with (two when it ends with
    none), problem 2 gains its last row, problem 3 loses a row it started with"""
    rows = synth.normal_stream(seed, 9, 3 * n).reshape(3, n)
    As0, cxs0 = [A.copy() for A in As], [np.array(c, dtype=np.float64, copy=True) for c in cxs]
    B = len(As)
    if B == 1:
        As0[0], cxs0[0] = np.vstack([As[0].reshape(-1, n), rows[:1]]), np.append(cxs0[0], 0.25)
        return As0, cxs0, np.ones(1, dtype=np.int64)
    if all(A.shape[0] == t_max for A in As):       # uniform final sets: the three problems each gain their last row
        for k in (0, 2, 3):
            As0[k], cxs0[k] = As[k][:-1].copy(), cxs0[k][:-1].copy()
        flags = np.zeros(B, dtype=np.int64)
        flags[[0, 2, 3]] = 1
        return As0, cxs0, flags
    t0 = As[0].shape[0]
    add = min(2, t_max) if t0 == 0 else 1
    As0[0] = np.vstack([As[0].reshape(-1, n), rows[:add]])
    cxs0[0] = np.append(cxs0[0], [0.25, -0.5][:add])
    As0[2], cxs0[2] = As[2][:-1].copy(), cxs0[2][:-1].copy()
    As0[3], cxs0[3] = np.vstack([As[3], rows[2:3]]), np.append(cxs0[3], 0.125)
    flags = np.zeros(B, dtype=np.int64)
    flags[[0, 2, 3]] = 1
    return As0, cxs0, flags


def poisoned(At, cx, flags):
    At1, cx1 = At.copy(), cx.copy()
    At1[flags == 0] = np.nan
    cx1[flags == 0] = np.nan
    return At1, cx1


# ---- 1. every Jacobian-side route ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,m,n,t_max,B,t_min", route_cases())
def test_routes_bitwise_against_ragged(route, m, n, t_max, B, t_min, monkeypatch):
    from enlsip_gn import GNSolver
    from test_gpu_factored_batched import pack
    from test_gpu_ragged_batch import check_problem
    env, hflags = OWN_HANDLE.get(route, ({}, 0))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, r = GNSolver(device=0, flags=hflags), GNSolver(device=0, flags=hflags)
    try:
        ts, Js, rxs, As, cxs = final_sets(m, n, t_max, B, t_min, seed=11)
        J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
        want = r.solve_batched_ragged(J, rx, At, cx, t)
        assert route in r.route(), (route, r.route())
        As0, cxs0, flags = start_sets(As, cxs, n, t_max, seed=m + n)
        _, _, At0, cx0, t0 = pack(Js, rxs, As0, cxs0, t_max)
        start = s.solve_batched_ragged(J, rx, At0, cx0, t0)
        assert s.jacobian_resolved() == B
        keep = [k for k in range(B) if not flags[k]][:2]
        snap = snapshot(s, keep)
        At1, cx1 = poisoned(At, cx, flags)
        got = s.solve_changed_batched(At1, cx1, t, flags)
        assert route in s.route(), (route, s.route())
        assert s.jacobian_resolved() == s.constraint_refactored() == int(flags.sum()) == (1 if B == 1 else 3)
        assert_flagged(got, want, flags, s, r)
        assert_snapshot(s, snap)
        # every problem against the oracle, from the handle under test: a flagged problem's results are this call's, an unflagged
        # one's those of the start solve (its working set did not change, and the snapshot above shows its factors did not either)
        merged = tuple([g[k] if flags[k] else st[k] for k in range(B)] if isinstance(g, list) else np.where(flags[:, None] != 0, g, st)
                       for g, st in zip(got, start))
        for k, tk in enumerate(ts):
            check_problem(merged, k, tk, Js[k], rxs[k], As[k], cxs[k])
    finally:
        s.close()
        r.close()


def test_every_jacobian_route_has_a_case():
    have = {c.values[0] for c in route_cases()}
    assert len(JAC_ROUTES) == 36
    assert set(JAC_ROUTES) - NOT_RUN == have, set(JAC_ROUTES) - NOT_RUN - have


# ---- 2. second attempt --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deficient_flagged", [True, False])
def test_second_attempt(solver, ref_solver, deficient_flagged):
    from test_gpu_factored_batched import pack
    from test_gpu_ragged_batch import check_problem, make_batch
    m, n, t_max, B = 192, 100, 6, 5
    ts = [6, 5, 6, 5, 6]              # the rank-deficient member has the smallest t: its J2 is wider than the launch speculates
    bad = 3 if deficient_flagged else 1
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=29)
    As[bad] = As[bad].copy()
    As[bad][-1] = As[bad][0]                       # a duplicated row: rankA < t
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    want = ref_solver.solve_batched_ragged(J, rx, At, cx, t)
    assert "second_attempt" in ref_solver.route() and want[3][bad][0] < ts[bad]
    As0, cxs0 = list(As), list(cxs)
    flags = np.zeros(B, dtype=np.int64)
    flags[[2, 3]] = 1
    As0[2], cxs0[2] = As[2][1:-1], np.asarray(cxs[2])[1:-1]
    As0[3], cxs0[3] = As[3][:-1], np.asarray(cxs[3])[:-1]           # (a): starts without the repeated row
    _, _, At0, cx0, t0 = pack(Js, rxs, As0, cxs0, t_max)
    solver.solve_batched_ragged(J, rx, At0, cx0, t0)
    snap = snapshot(solver, (0, 1, 4))
    got = solver.solve_changed_batched(*poisoned(At, cx, flags), t, flags)
    if deficient_flagged:
        assert "second_attempt" in solver.route()
    else:           # the launch width comes from the resident n2 of the unflagged member: one attempt
        assert "second_attempt" not in solver.route()
    assert solver.jacobian_resolved() == 2
    assert_flagged(got, want, flags, solver, ref_solver)
    assert_snapshot(solver, snap)
    for k in (2, 3):
        check_problem(want, k, ts[k], Js[k], rxs[k], As[k], cxs[k])


# ---- 3. the launch width changes ----------------------------------------------------------------------------------------------------
def test_width_changes_and_consumers_follow(solver, ref_solver):
    from test_gpu_factored_batched import pack
    from test_gpu_ragged_batch import make_batch
    m, n, t_max, B = 96, 64, 8, 5
    ts0 = [3, 8, 1, 5, 2]
    Js, rxs, As0, cxs0 = make_batch(m, n, ts0, seed=31)
    As, cxs = list(As0), list(cxs0)
    As[2], cxs[2] = np.zeros((0, n)), np.zeros(0)                    # t = 0: n2 + 1 = 65, the pivot kernel form flips
    As[3], cxs[3] = As0[3][:-1], np.asarray(cxs0[3])[:-1]
    ts = [3, 8, 0, 4, 2]
    flags = np.array([0, 0, 1, 1, 0])
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    _, _, At0, cx0, t0 = pack(Js, rxs, As0, cxs0, t_max)
    want = ref_solver.solve_batched_ragged(J, rx, At, cx, t)
    solver.solve_batched_ragged(J, rx, At0, cx0, t0)
    assert "pivot_wave64" in solver.route() and "pivot_lds_r1_512" in ref_solver.route()
    snap = snapshot(solver, (0, 1, 4))
    got = solver.solve_changed_batched(*poisoned(At, cx, flags), t, flags)
    assert "pivot_lds_r1_512" in solver.route()
    assert_flagged(got, want, flags, solver, ref_solver)
    assert_snapshot(solver, snap)
    for k in range(B):
        assert solver.factor(0, k).shape == (min(n, ts[k]), ts[k])

    def close(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        nb = np.linalg.norm(b)
        return np.linalg.norm(a - b) <= 1e-12 * nb if nb > 0 else not a.any()
    G = np.stack([Jk.T @ r for Jk, r in zip(Js, rxs)])
    assert close(solver.gradient_batched(n, 0, B), ref_solver.gradient_batched(n, 0, B))
    a, b = solver.first_lagrange_batched(t_max, 0, B, G), ref_solver.first_lagrange_batched(t_max, 0, B, G)
    assert all(close(a[0][k], b[0][k]) and close(a[1][k], b[1][k]) for k in range(B)) and np.array_equal(a[2], b[2])
    pg = np.where(np.isnan(got[0]), want[0], got[0])
    a, b = solver.second_lagrange_batched(t_max, pg), ref_solver.second_lagrange_batched(t_max, want[0])
    assert all(close(a[0][k], b[0][k]) for k in range(B))
    dA, dJ, cd = ([i[j] for i in want[3]] for j in (0, 1, 2))         # the default dimensions: each problem's own ranks and code
    (oa, ra), (ob, rb) = solver.resolve_batched(m, n, t_max, dA, dJ, cd, 0, B), ref_solver.resolve_batched(m, n, t_max, dA, dJ, cd, 0, B)
    assert ra == rb and np.array_equal(oa["info"], ob["info"])
    assert all(close(oa[x][k], ob[x][k]) for x in ("p", "b", "d") for k in range(B))
    Gam = np.stack([np.eye(n) * (1.0 + 0.1 * k) for k in range(B)])
    (pa, sa, _), (pb, sb, _) = solver.newton_direction_batched(Gam, 0, B), ref_solver.newton_direction_batched(Gam, 0, B)
    assert list(sa) == list(sb) and all(close(pa[k], pb[k]) for k in range(B) if sb[k] == 0)


# ---- 4. pipelined halves ------------------------------------------------------------------------------------------------------------
def test_pipelined_halves(solver, ref_solver):
    from test_gpu_factored_batched import pack
    from test_gpu_ragged_batch import make_batch
    m, n, t_max, B = 96, 72, 5, 130
    ts = [(3 + k) % (t_max + 1) for k in range(B)]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=17)
    As = [A if t else np.zeros((0, n)) for A, t in zip(As, ts)]
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    want = ref_solver.solve_batched_ragged(J, rx, At, cx, t)
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
    solver.solve_batched_ragged(J, rx, At0, cx0, t0)
    assert solver.pipeline_split() == 65 and solver.jacobian_resolved() == B
    snap = snapshot(solver, (0, 128))
    got = solver.solve_changed_batched(*poisoned(At, cx, flags), t, flags)
    assert solver.pipeline_split() == 65 and solver.jacobian_resolved() == solver.constraint_refactored() == 6
    assert_flagged(got, want, flags, solver, ref_solver)
    assert_snapshot(solver, snap)
    # flags on the second half only, then on the first only: the other stream runs nothing
    for ks in ((66, 129), (1,)):
        f1 = np.zeros(B, dtype=np.int64)
        f1[list(ks)] = 1
        got = solver.solve_changed_batched(*poisoned(At, cx, f1), t, f1)
        assert solver.pipeline_split() == 65 and solver.jacobian_resolved() == len(ks)
        assert_flagged(got, want, f1, solver, ref_solver)
    assert_snapshot(solver, snap)
    # a call that would split differently: profiling toggled in between
    solver.set_profiling(True)
    try:
        with pytest.raises(Exception, match="error -1"):
            solver.solve_changed_batched(At, cx, t, flags)
    finally:
        solver.set_profiling(False)
    solver.solve_changed_batched(At, cx, t, flags)


# ---- 5. state and argument errors ---------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
    import torch
    from enlsip_gn import GNSolver
    from test_gpu_factored_batched import pack, same
    from test_gpu_ragged_batch import make_batch
    m, n, t_max, B = 48, 12, 4, 5
    ts = [4, 2, 0, 3, 4]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=19)
    As = [A if t else np.zeros((0, n)) for A, t in zip(As, ts)]
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    flags = np.array([1, 0, 0, 1, 0])
    s, w = GNSolver(device=0), GNSolver(device=0)
    try:
        def rc_of(call):
            try:
                call()
            except Exception as e:      # GNError: "libenlsip_gn error <rc>: ..."
                return int(re.search(r"error (-?\d+)", str(e)).group(1))
            return 0
        changed = lambda **kw: s.solve_changed_batched(At, cx, t, flags, m=m, **kw)
        assert rc_of(changed) == -1                                                  # nothing resident
        s.factor_constraints_batched(m, At, cx, t)
        assert rc_of(changed) == -1                                                  # only F_A / F_L11 resident
        s.solve_batched(J, rx, At, cx)
        assert rc_of(changed) == -1                                                  # a uniform batch
        # a TSQR solve (one rank, no communicator: the exchange is a device copy) leaves no whole problem resident
        from enlsip_gn.tsqr import tsqr_solve_lib
        dev = torch.device("cuda:0")
        s.solve_batched_ragged(J, rx, At, cx, t)
        s._chk(s._lib.enlsip_gn_tsqr_set_exchange(s._h, None, None, 1, 0))
        tsqr_solve_lib(s, torch.from_numpy(np.ascontiguousarray(J[0])).to(dev), torch.from_numpy(rx[0]).to(dev),
                       torch.from_numpy(np.ascontiguousarray(At[0])).to(dev), torch.from_numpy(cx[0]).to(dev))
        with pytest.raises(Exception, match=r"error -1: .*TSQR"):
            changed()
        want = w.solve_batched_ragged(J, rx, At, cx, t)
        s.solve_batched_ragged(J, rx, At, cx, t)
        assert rc_of(lambda: s.solve_changed_batched(At[:4], cx[:4], t[:4], flags[:4])) == -1      # another batch
        t_bad = t.copy()
        t_bad[1] = 3
        with pytest.raises(Exception, match=r"error -6: t\[1\]"):
            s.solve_changed_batched(At, cx, t_bad, flags)
        L, one = s._lib, C.c_void_p(8)
        ip = lambda a: a.ctypes.data_as(C.c_void_p)
        tail = (1e-8, None, None, None, None, None, None, None)
        assert L.enlsip_gn_solve_changed_batched(s._h, B, m, n, t_max, ip(t), None, ip(At), n, n * t_max, ip(cx), *tail) == -7
        assert L.enlsip_gn_solve_changed_batched(s._h, B, m, n, t_max, ip(t), ip(flags), ip(At), n - 1, n * t_max, ip(cx), *tail) == -9
        assert L.enlsip_gn_solve_changed_batched(s._h, B, m, n, t_max, ip(t), ip(flags), ip(At), n, n * t_max - 1, ip(cx), *tail) == -10
        assert L.enlsip_gn_solve_changed_batched(s._h, B, m, n, t_max, ip(t), ip(flags), ip(At), n, n * t_max, None, *tail) == -11
        big = 32769
        tb = np.zeros(big, dtype=np.int64)
        assert L.enlsip_gn_solve_changed_batched(s._h, big, m, n, t_max, ip(tb), ip(tb), one, n, n * t_max, one, *tail) == -2
        # all-zero flags: nothing launched, nothing written
        snap = snapshot(s, range(B))
        got = s.solve_changed_batched(At, cx, t, np.zeros(B, dtype=np.int64))
        assert s.jacobian_resolved() == s.constraint_refactored() == 0
        assert all(np.isnan(got[i]).all() for i in (0, 1, 2)) and not any(got[i].any() for i in (4, 5, 6))
        assert_snapshot(s, snap)
        # a valid call after the errors
        got = s.solve_changed_batched(*poisoned(At, cx, flags), t, flags)
        assert_flagged(got, want, flags, s, w)
        # device form: the resident solve was a host-form one / another dAt
        dJ, drx = torch.from_numpy(J).to(dev), torch.from_numpy(rx).to(dev)
        dAt, dAt2, dcx = torch.from_numpy(At).to(dev), torch.from_numpy(At).to(dev), torch.from_numpy(cx).to(dev)
        dargs = (B, m, n, t_max, t, flags)
        assert rc_of(lambda: s.solve_changed_batched_dev(*dargs, dAt.data_ptr(), n, n * t_max, dcx.data_ptr())) == -8
        s.solve_batched_ragged_dev(B, m, n, t_max, t, dJ.data_ptr(), m, m * n, drx.data_ptr(), dAt.data_ptr(), n, n * t_max, dcx.data_ptr())
        assert rc_of(lambda: s.solve_changed_batched_dev(*dargs, dAt2.data_ptr(), n, n * t_max, dcx.data_ptr())) == -8
        assert rc_of(changed) == -1                                                  # host form on a device-form resident batch
        # ---- 8. device form: outputs bitwise those of the host form --------------------------------------------------------------
        dp = torch.full((B, n), float("nan"), dtype=torch.float64, device=dev)
        dd = torch.full((B, m), float("nan"), dtype=torch.float64, device=dev)
        db = torch.full((B, t_max), float("nan"), dtype=torch.float64, device=dev)
        kA = min(n, t_max)
        djA, djL, djJ = (torch.zeros((B, c), dtype=torch.int64, device=dev) for c in (t_max, kA, n))
        dinfo = torch.full((B, 6), -7, dtype=torch.int64, device=dev)
        s.solve_changed_batched_dev(*dargs, dAt.data_ptr(), n, n * t_max, dcx.data_ptr(), dp=dp.data_ptr(), db=db.data_ptr(),
                                    dd=dd.data_ptr(), dinfo=dinfo.data_ptr(), djA=djA.data_ptr(), djL=djL.data_ptr(),
                                    djJ=djJ.data_ptr())
        torch.cuda.synchronize()
        assert s.jacobian_resolved() == 2
        for a, b in ((dp, got[0]), (db, got[1]), (dd, got[2]), (djA, got[4]), (djL, got[5])):
            assert same(a.cpu().numpy(), b)
        hinfo, hjJ = dinfo.cpu().numpy(), djJ.cpu().numpy()
        for k in range(B):
            if flags[k]:        # the info record, and the n2 = n - rankA pivots the library writes
                assert tuple(hinfo[k]) == got[3][k] == want[3][k]
                assert np.array_equal(hjJ[k, :n - got[3][k][0]], got[6][k, :n - got[3][k][0]])
            else:               # not written: as they were made above
                assert np.all(hinfo[k] == -7) and not hjJ[k].any()
    finally:
        s.close()
        w.close()


# ---- 6. held results ----------------------------------------------------------------------------------------------------------------
def test_held_results(solver, ref_solver):
    from test_gpu_factored_batched import pack
    from test_gpu_ragged_batch import make_batch
    m, n, t_max, B = 128, 48, 6, 4
    ts = [6, 4, 5, 3]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=37)
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    flags = np.array([0, 0, 1, 0])
    for s in (solver, ref_solver):
        s.solve_batched_ragged(J, rx, At, cx, t)
    code = np.array([0, -1, -1, 0])
    dA = np.array([0, 3, 3, 0])
    dJ = np.array([0, 20, 20, 0])
    hold = np.full(B, HOLD, dtype=np.int64)
    want, _ = ref_solver.resolve_batched(m, n, t_max, dA, dJ, code, 0, B)
    solver.resolve_batched(m, n, t_max, dA, hold, code, 0, B)
    solver.solve_changed_batched(At, cx, t, flags)
    out, rc = solver.resolve_batched(m, n, t_max, hold, dJ, code, 0, B)
    assert rc == 1 and list(out["status"]) == [-1, 0, 3, -1]
    assert np.array_equal(out["p"][1], want["p"][1]) and np.array_equal(out["info"][1], want["info"][1])


# ---- 7. magnitudes beyond the plain range -------------------------------------------------------------------------------------------
def test_magnitudes(solver, ref_solver):
    from test_gpu_factored_batched import pack
    from test_gpu_ragged_batch import make_batch
    m, n, t_max, B = 64, 16, 4, 4
    ts = [4, 4, 3, 4]
    Js, rxs, As0, cxs0 = make_batch(m, n, ts, seed=23)
    As, cxs = list(As0), list(cxs0)
    As[2], cxs[2] = As0[2] * 2.0 ** 600, np.asarray(cxs0[2]) * 2.0 ** 600
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    _, _, At0, cx0, t0 = pack(Js, rxs, As0, cxs0, t_max)
    flags = np.array([0, 0, 1, 0])

    def agree(got, want, k):
        assert got[3][k] == want[3][k]
        for a, b in zip(got[4:], want[4:]):
            assert np.array_equal(a[k], b[k])
        for a, b in zip(got[:3], want[:3]):
            assert np.isfinite(a[k]).all() and np.linalg.norm(a[k] - b[k]) <= 1e-11 * np.linalg.norm(b[k])
    want = ref_solver.solve_batched_ragged(J, rx, At, cx, t)
    assert "rescaled" in ref_solver.route()
    solver.solve_batched_ragged(J, rx, At0, cx0, t0)
    assert "rescaled" not in solver.route()
    got = solver.solve_changed_batched(At, cx, t, flags)
    assert "rescaled" in solver.route() and solver.jacobian_resolved() == 1
    agree(got, want, 2)
    assert np.allclose(solver.factor(0, 2).diagR(), ref_solver.factor(0, 2).diagR(), rtol=1e-11, atol=0)
    # back to ordinary data: the problem returns from its rescue handle to the batch's slots
    want0 = ref_solver.solve_batched_ragged(J, rx, At0, cx0, t0)
    got = solver.solve_changed_batched(At0, cx0, t0, flags)
    assert "rescaled" not in solver.route()
    assert_flagged(got, want0, flags, solver, ref_solver)


# ---- 9. the driver: update_working_set for a batch ----------------------------------------------------------------------------------
def test_driver_uses_the_changed_call(solver, ref_solver):
    from enlsip_gn import working_set as ws
    m, n, l, q, B = 40, 10, 6, 2, 8
    eps = ws.SQRT_EPS
    fires = [True, False, True, True, False, False, True, False]

    def build():            # the fixture of test_gpu_factored_batched.test_driver_against_per_problem_loop
        Ws, Cs, its, Js, rxs, As, Gs, ps = [], [], [], [], [], [], [], []
        for k in range(B):
            A = synth.normal_stream(100 + k, 1, l * n).reshape(l, n)
            J = synth.normal_stream(100 + k, 2, m * n).reshape(m, n)
            rx = synth.normal_stream(100 + k, 3, m)
            W = ws.WorkingSet.create(q, l)
            W.add_constraint(1)
            W.add_constraint(1)
            Aact = A[W.active[:W.t] - 1, :].copy()
            lam_star = np.ones(W.t)
            if fires[k]:
                lam_star[2 + k % 2] = -1.0
            Ws.append(W); As.append(A); Js.append(J); rxs.append(rx)
            Cs.append(ws.Constraint(np.zeros(W.t), Aact, False, np.ones(W.t)))
            Gs.append(Aact.T @ lam_star)
            its.append(ws.IterationRecord()); ps.append(np.zeros(n))
        return Ws, Cs, its, Js, rxs, As, Gs, ps

    calls = []

    class Recording:
        def __init__(self, inner):
            self._inner = inner

        def __getattr__(self, name):
            f = getattr(self._inner, name)
            if name not in ("factor_constraints_batched", "solve_factored_batched", "solve_changed_batched"):
                return f

            def wrapped(*a, **kw):
                out = f(*a, **kw)
                calls.append((name, int(np.sum(a[3])) if name == "solve_changed_batched" else None, self._inner.jacobian_resolved()))
                return out
            return wrapped

    Ws, Cs, its, Js, rxs, As, Gs, ps = build()
    ws.update_working_set_batched(Recording(solver), Ws, rxs, As, Cs, Gs, Js, ps, its, eps)
    names = [c[0] for c in calls]
    assert names[:2] == ["factor_constraints_batched", "solve_factored_batched"]
    assert len(names) > 2 and set(names[2:]) == {"solve_changed_batched"}
    for name, nflag, resolved in calls[2:]:
        assert resolved == nflag and 0 < nflag < B
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
