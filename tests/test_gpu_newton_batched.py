"""Batched Newton direction (enlsip_gn_newton_direction_batched*) on the GPU.

Per case: status equals the verdict of the references; rel(p, p_mp) <= C_NEWTON u cond(sW22) against the mpmath reference
(tests/newton_reference.py) for the sampled problems (the first members of every case small enough for mpmath: n <= 40, m <= 300);
for EVERY problem rel(p_batched, p_per_problem) <= 2 C_NEWTON u cond(sW22) against enlsip_gn_newton_direction on a second handle
that solved the same batch; the kernel form is the one the predicate of gn_newton_batched.inc asks for.  C_NEWTON is set by
tests/test_newton_reference.py (CPU)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import newton_reference as nr  # noqa: E402
from oracle import gn_oracle as go, synth  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x7FF8DEADBEEF0000          # a NaN payload no kernel produces
MP_SAMPLES = 2


def rel(a, b):
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


def make_solver(monkeypatch, **env):
    from enlsip_gn import GNSolver
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return GNSolver(device=0)


def solve(s, probs, t_max, ragged):
    J = np.stack([np.ascontiguousarray(p[0].T) for p in probs])
    rx = np.stack([p[1] for p in probs])
    n = probs[0][0].shape[1]
    if ragged:
        At, cx, t = s.pack_ragged([p[2] for p in probs], [p[3] for p in probs], n=n)
        return s.solve_batched_ragged(J, rx, At, cx, t)
    At = np.stack([np.ascontiguousarray(p[2]) for p in probs]) if t_max else None
    cx = np.stack([p[3] for p in probs]) if t_max else None
    return s.solve_batched(J, rx, At, cx)


MAKERS = {"plain": synth.make_problem, "rankdefJ": synth.make_rank_deficient_J, "rankdefA": synth.make_rank_deficient_A,
          "wide_rankdefA": nr.make_wide_rankdef_A}

# name, m, n, t_max, members [(t_k, maker)] (None: B uniform plain members), B, environment, ranges (prob0, count)
GRID = [
    ("n1_t0", 20, 1, 0, None, 5, {}, [(0, 5), (1, 3)]),
    ("n2_t1", 30, 2, 1, None, 6, {}, [(0, 6), (3, 2)]),
    ("n63", 200, 63, 5, None, 3, {}, [(0, 3)]),
    ("n64", 200, 64, 5, None, 3, {}, [(0, 3), (1, 2)]),
    ("n65", 200, 65, 5, None, 3, {}, [(0, 3)]),
    ("t0_300x40", 300, 40, 0, None, 6, {}, [(0, 6), (1, 5)]),
    ("t_eq_n_40x9", 40, 9, 9, None, 5, {}, [(0, 5)]),
    ("wide_m_lt_n2", 10, 24, 4, None, 5, {}, [(0, 5), (2, 3)]),
    ("rankdefJ_300x40_t6", 300, 40, 6, [(6, "rankdefJ")] * 3, 3, {}, [(0, 3)]),
    ("ragged_60x12", 60, 12, 6, [(6, "plain"), (0, "plain"), (3, "plain"), (6, "plain"), (0, "plain"), (5, "plain"), (6, "plain")],
     7, {}, [(0, 7), (1, 5)]),
    # t >= n > rankA (E re-indexed), n > t > rankA (status 2), rankA == n (p1 returned) and a full-rank member in one batch
    ("mixed_rankdef", 50, 10, 12, [(12, "wide_rankdefA"), (5, "rankdefA"), (12, "plain"), (4, "plain"), (12, "wide_rankdefA")],
     5, {}, [(0, 5), (1, 3)]),
    ("n130_t20", 500, 130, 20, None, 3, {}, [(0, 3)]),
    ("c2_batch3", 4096, 512, 64, None, 3, {}, [(0, 3)]),
    ("pipelined", 256, 32, 4, None, 160, {"ENLSIP_GN_PIPELINE": "1"}, [(0, 160), (73, 21)]),
]


def build_case(case):
    name, m, n, t_max, members, B, env, ranges = case
    members = members or [(t_max, "plain")] * B
    seed0 = 13000 + 131 * [g[0] for g in GRID].index(name)
    probs = [MAKERS[kind](seed0 + k, m, n, tk) for k, (tk, kind) in enumerate(members)]
    refs = [go.gn_subproblem(*p) for p in probs]
    gam = [nr.make_gammas(seed0 + 7 * k, p[0], p[2], r) for k, (p, r) in enumerate(zip(probs, refs))]
    return probs, refs, gam, [tk for tk, _ in members]


def verdict(prob, ref, Gam, tk):
    """(status, cond(sW22)) from the FP64 oracle: 2 undefined, 1 not positive definite, 0"""
    n = prob[0].shape[1]
    if tk != ref.rankA and tk < n:
        return 2, 1.0
    if ref.rankA == n:
        return 0, 1.0
    ev = np.linalg.eigvalsh(nr._sW22_oracle(prob[0], prob[2], ref, Gam))
    return (0, float(ev[-1] / ev[0])) if ev[0] > 0 else (1, 1.0)


def per_problem(s, k, Gam, n):
    """the per-problem entry point with the batched call's status convention: its return code -7 is status 2"""
    G = np.asfortranarray(Gam, dtype=np.float64)
    p = np.full(n, np.nan)
    bad = C.c_int64(0)
    rc = s._lib.enlsip_gn_newton_direction(s._h, k, G.ctypes.data_as(C.c_void_p), n, p.ctypes.data_as(C.c_void_p), C.byref(bad))
    assert rc in (0, -7), (k, rc)
    return (np.full(n, np.nan), 2) if rc == -7 else (p, int(bad.value))


@pytest.mark.parametrize("case", GRID, ids=[g[0] for g in GRID])
def test_grid(case, monkeypatch):
    name, m, n, t_max, members, B, env, ranges = case
    probs, refs, gam, ts = build_case(case)
    ragged = members is not None and len({tk for tk, _ in members}) > 1
    want = [verdict(probs[k], refs[k], gam[k][0], ts[k]) for k in range(B)]
    if name == "mixed_rankdef":
        assert [w[0] for w in want] == [0, 2, 0, 0, 0] and refs[2].rankA == n and refs[0].rankA < n <= ts[0]
    if name == "wide_m_lt_n2":
        assert all(m < n - r.rankA for r in refs)
    if name.startswith("rankdefJ"):
        assert all(r.rankJ2 < n - r.rankA for r in refs)
    small = [k for k in range(B) if n <= 40 and m <= 300][:MP_SAMPLES]
    if name == "mixed_rankdef":
        small = [0, 3]
    his = {k: nr.NewtonReference(*probs[k], gam[k][0], refs[k]) for k in small}
    s, s1 = make_solver(monkeypatch, **env), make_solver(monkeypatch, **env)
    try:
        solve(s, probs, t_max, ragged)
        solve(s1, probs, t_max, ragged)
        if env:
            split = s.pipeline_split()
            assert B >= 128 and 0 < split < B, split
            assert any(p0 < split < p0 + cnt for p0, cnt in ranges)
        per = [per_problem(s1, k, gam[k][0], n) for k in range(B)]
        for p0, cnt in ranges:
            G = np.stack([gam[p0 + j][0] for j in range(cnt)])
            p, st, rc = s.newton_direction_batched(G, p0, cnt)
            assert s.newton_form() == nr.expected_newton_form(n)
            assert list(st) == [want[p0 + j][0] for j in range(cnt)], (name, list(st))
            assert rc == (1 if any(st) else 0)
            for j in range(cnt):
                k = p0 + j
                code, cond = want[k]
                assert per[k][1] == code, (k, per[k][1], code)
                if code == 2:
                    assert np.all(np.isnan(p[j]))
                    continue
                bound = nr.newton_bound(cond)
                e_per = rel(p[j], per[k][0])
                print(f"{name}[{k}] range ({p0},{cnt}): vs per-problem {e_per:.2e} (bound {2 * bound:.2e}) cond {cond:.2e}")
                assert e_per <= 2 * bound, (name, k, e_per, 2 * bound)
                if k in his:
                    assert not his[k].error
                    e_mp = rel(p[j], his[k].p)
                    print(f"{name}[{k}]: vs mpmath {e_mp:.2e} = {e_mp / (nr.U * max(cond, 1.0)):.2f} u cond (bound {bound:.2e})")
                    assert e_mp <= bound, (name, k, e_mp, bound)
    finally:
        s.close()
        s1.close()


def test_rescaled_member(monkeypatch):
    """a member scaled by 2^600 lives on a rescue handle of the second pipelined half: its slot is the per-problem entry point's"""
    B, m, n, t = 192, 1024, 48, 16
    kr = 150
    J = synth.normal_stream(10000, 0, B * m * n).reshape(B, n, m)
    rx = synth.normal_stream(10000, 1, B * m).reshape(B, m)
    At = synth.normal_stream(10000, 2, B * t * n).reshape(B, t, n)
    cx = synth.normal_stream(10000, 3, B * t).reshape(B, t)
    J[kr] *= 2.0 ** 600
    rx[kr] *= 2.0 ** 600
    rng = np.random.default_rng(3)
    S = rng.standard_normal((n, n))
    Gam = 0.3 * (S + S.T) + 0.03 * rng.standard_normal((n, n)) + 40.0 * np.eye(n)
    s, s1 = make_solver(monkeypatch), make_solver(monkeypatch)
    try:
        s.solve_batched(J, rx, At, cx)
        s1.solve_batched(J, rx, At, cx)
        assert 0 < s.pipeline_split() <= kr and "rescaled" in s.route()
        p0, cnt = kr - 5, 11
        G = np.stack([Gam] * cnt)
        p, st, rc = s.newton_direction_batched(G, p0, cnt)
        for j in range(cnt):
            k = p0 + j
            pk, bad = s1.newton_direction(G[j], k)
            if k == kr:          # (J'J of this member is beyond the FP64 range: whatever the per-problem entry point says)
                assert np.array_equal(p[j], pk, equal_nan=True) and st[j] == int(bad) and rc == int(bad)
                continue
            assert not bad and st[j] == 0
            prob = (J[k].T, rx[k], At[k], cx[k])
            ev = np.linalg.eigvalsh(nr._sW22_oracle(prob[0], prob[2], go.gn_subproblem(*prob), G[j]))
            assert ev[0] > 0 and rel(p[j], pk) <= 2 * nr.newton_bound(ev[-1] / ev[0]), (k, rel(p[j], pk))
    finally:
        s.close()
        s1.close()


def test_take_and_indefinite_partner(monkeypatch):
    case = next(g for g in GRID if g[0] == "t0_300x40")
    name, m, n, t_max, members, B, env, ranges = case
    probs, refs, gam, ts = build_case(case)
    s = make_solver(monkeypatch)
    try:
        solve(s, probs, t_max, False)
        take = np.array([1, 0, 1, 1, 0, 1], dtype=np.int64)
        G = np.stack([gam[k][1] if k == 3 else gam[k][0] for k in range(B)])        # problem 3: the indefinite partner
        hi = nr.NewtonReference(*probs[3], gam[3][1], refs[3])
        assert hi.error and hi.lam_min < -1e-3 * hi.norm
        p = np.full((B, n), SENT, dtype=np.int64).view(np.float64)
        st = np.full(B, -77, dtype=np.int32)
        full, st_full, _ = s.newton_direction_batched(np.stack([gam[k][0] for k in range(B)]))
        p, st, rc = s.newton_direction_batched(G, 0, B, take=take, out_p=p, out_status=st)
        assert rc == 1 and list(st) == [0, -77, 0, 1, -77, 0]
        for k in (1, 4):
            assert np.all(p[k].view(np.int64) == SENT)
        assert np.all(p[3] == 0.0)
        for k in (0, 2, 5):
            assert np.array_equal(p[k], full[k])
    finally:
        s.close()


def test_untaken_problem_keeps_its_held_result(monkeypatch):
    """take[j] == 0 touches no state: a result held by ENLSIP_GN_DIM_HOLD survives on the untaken problems and is dropped on the
    taken ones (status 3 of the re-solve)"""
    B, m, n, t = 6, 256, 32, 4
    probs = [synth.make_problem(14500 + k, m, n, t) for k in range(B)]
    refs = [go.gn_subproblem(*p) for p in probs]
    gam = [nr.make_gammas(14500 + k, p[0], p[2], r)[0] for k, (p, r) in enumerate(zip(probs, refs))]
    dA = np.array([max(r.rankA - 1, 0) for r in refs], dtype=np.int64)
    dJ = np.array([max(r.rankJ2 - 2, 0) for r in refs], dtype=np.int64)
    hold = np.full(B, -2, dtype=np.int64)
    take = np.array([1, 0, 0, 1, 0, 1], dtype=np.int64)
    s = make_solver(monkeypatch)
    try:
        solve(s, probs, t, False)
        want, rc = s.resolve_batched(m, n, t, dA, dJ, -1, 0, B)
        assert rc == 0
        _, rc = s.resolve_batched(m, n, t, dA, hold, -1, 0, B)
        assert rc == 0
        _, st, rc = s.newton_direction_batched(np.stack(gam), 0, B, take=take)
        assert rc == 0 and list(st) == [0, -1, -1, 0, -1, 0]
        out, rc = s.resolve_batched(m, n, t, hold, dJ, -1, 0, B)
        assert rc == 1 and list(out["status"]) == [3, 0, 0, 3, 0, 3]
        for k in (1, 2, 4):
            assert np.array_equal(out["p"][k], want["p"][k]) and np.array_equal(out["info"][k], want["info"][k])
    finally:
        s.close()


def snapshot(s, m, n, B):
    from enlsip_gn import FACTOR_A, FACTOR_J2, FACTOR_L11
    snap = []
    for k in range(B):
        for which in (FACTOR_A, FACTOR_L11, FACTOR_J2):
            f = s.factor(which, k)
            snap += [f.R.copy(), f.p.copy(), f.diagR().copy()]
        snap.append(s.JQ1(m, n, k))          # debug_copy_W
    return snap


@pytest.mark.parametrize("shape", [(6, 256, 32, 4), (4, 700, 130, 20)], ids=["wave", "general"])
def test_state_and_later_consumers(shape, monkeypatch):
    B, m, n, t = shape
    probs = [synth.make_problem(13900 + k, m, n, t) for k in range(B)]
    refs = [go.gn_subproblem(*p) for p in probs]
    gam = [nr.make_gammas(13900 + k, p[0], p[2], r)[0] for k, (p, r) in enumerate(zip(probs, refs))]
    conds = []
    for p, r, g in zip(probs, refs, gam):
        ev = np.linalg.eigvalsh(nr._sW22_oracle(p[0], p[2], r, g))
        conds.append(float(ev[-1] / ev[0]))
    G = np.stack(gam)
    s, s1 = make_solver(monkeypatch), make_solver(monkeypatch)
    try:
        solve(s, probs, t, False)
        solve(s1, probs, t, False)
        first, st, rc = s.newton_direction_batched(G)
        assert rc == 0
        # a truncated re-solve on half of the range: the batched Newton step still uses the default p1
        half = B // 2
        dA = np.array([max(r.rankA - 2, 0) for r in refs[:half]], dtype=np.int64)
        dJ = np.array([max(r.rankJ2 - 3, 0) for r in refs[:half]], dtype=np.int64)
        _, rc = s.resolve_batched(m, n, t, dA, dJ, -1, 0, half)
        assert rc == 0
        for k in range(half):
            s1.resolve(m, n, t, int(dA[k]), int(dJ[k]), -1, k)
        before = snapshot(s, m, n, B)
        again, st, rc = s.newton_direction_batched(G)
        assert rc == 0 and np.array_equal(again, first)
        after = snapshot(s, m, n, B)
        for a, b in zip(before, after):
            assert np.array_equal(a, b)          # F_A, F_L11, F_J2, their pivots and diagonals, W: bitwise untouched
        loop = [s1.newton_direction(gam[k], k)[0] for k in range(B)]        # the other handle runs the per-problem loop
        for k in range(B):
            bound = 2 * nr.newton_bound(conds[k])
            assert rel(again[k], loop[k]) <= bound
            lam, lam1 = s.second_lagrange(t, again[k], prob=k), s1.second_lagrange(t, again[k], prob=k)
            # the factors of the two handles are bitwise the same, the second estimate reads only them and its argument, and
            # enlsip_gn_resolve / enlsip_gn_newton_direction recompute b and p1 themselves: bitwise
            assert np.array_equal(lam, lam1), (k, rel(lam, lam1))
            a, b = s.resolve(m, n, t, refs[k].rankA, refs[k].rankJ2, -1, k), s1.resolve(m, n, t, refs[k].rankA, refs[k].rankJ2, -1, k)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (k, [rel(x, y) for x, y in zip(a, b)])
            pn, e = s.newton_direction(gam[k], k)
            pn1, e1 = s1.newton_direction(gam[k], k)
            assert not e and not e1 and np.array_equal(pn, pn1), (k, rel(pn, pn1))
    finally:
        s.close()
        s1.close()


def test_argument_errors(monkeypatch):
    B, m, n, t = 4, 120, 12, 3
    probs = [synth.make_problem(14100 + k, m, n, t) for k in range(B)]
    s = make_solver(monkeypatch)
    lib, h = s._lib, s._h
    G = np.zeros((B, n, n)) + np.eye(n)
    p = np.zeros((B, n))
    st = np.zeros(B, dtype=np.int32)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    call = lambda p0, cnt, g=G, ldg=n, sg=n * n, out=p: lib.enlsip_gn_newton_direction_batched(
        h, p0, cnt, None if g is None else vp(g), ldg, sg, None, None if out is None else vp(out), vp(st))
    try:
        assert call(0, 1) == -1                                          # before any solve
        s.factor_constraints(m, probs[0][2], probs[0][3])
        assert call(0, 1) == -1                                          # only F_A / F_L11 are resident
        solve(s, probs, t, False)
        before = snapshot(s, m, n, B)
        assert call(0, 0) == -2
        assert call(B, 1) == -3 and call(B - 1, 2) == -3
        assert call(0, 1, g=None) == -4 and call(0, 1, out=None) == -4
        assert call(0, 2, ldg=n - 1) == -5 and call(0, 2, sg=n * n - 1) == -5
        assert np.all(p == 0.0)
        for a, b in zip(before, snapshot(s, m, n, B)):
            assert np.array_equal(a, b)
        assert call(0, B) == 0
    finally:
        s.close()


@pytest.mark.parametrize("shape", [(100, 10, 6), (300, 80, 12)], ids=["wave", "general"])
def test_dev_form_equals_host_form(shape, monkeypatch):
    import torch
    m, n, t = shape
    B, prob0, count, g = 8, 1, 6, 2
    probs = [synth.make_problem(14300 + k, m, n, t) for k in range(B)]
    refs = [go.gn_subproblem(*p) for p in probs]
    gam = [nr.make_gammas(14300 + k, p[0], p[2], r)[0] for k, (p, r) in enumerate(zip(probs, refs))]
    s = make_solver(monkeypatch)
    try:
        solve(s, probs, t, False)
        take = np.array([1, 0, 1, 1, 0, 1], dtype=np.int64)
        G = np.stack([gam[prob0 + j] for j in range(count)])
        ldg, sG = n + 3, (n + 3) * n + 5
        Gd = torch.zeros(count * sG, dtype=torch.float64, device="cuda:0")
        for j in range(count):
            Gd[j * sG:j * sG + ldg * n].view(n, ldg)[:, :n] = torch.from_numpy(np.ascontiguousarray(G[j].T)).to("cuda:0")
        pd = torch.full((count + 2 * g, n), SENT, dtype=torch.int64, device="cuda:0").view(torch.float64)
        sd = torch.full((count + 2 * g,), -77, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        rc = s.newton_direction_batched_dev(prob0, count, Gd.data_ptr(), ldg, sG, pd.data_ptr() + g * n * 8, sd.data_ptr() + g * 4, take=take)
        torch.cuda.synchronize()
        assert rc == 0
        host, st, rc = s.newton_direction_batched(G, prob0, count, take=take)
        assert rc == 0
        pdev, sdev = pd.cpu().numpy(), sd.cpu().numpy()
        assert np.all(pdev[:g].view(np.int64) == SENT) and np.all(pdev[g + count:].view(np.int64) == SENT)
        assert np.all(sdev[:g] == -77) and np.all(sdev[g + count:] == -77)
        for j in range(count):
            if take[j]:
                assert np.array_equal(pdev[g + j], host[j]) and sdev[g + j] == st[j] == 0
            else:
                assert np.all(pdev[g + j].view(np.int64) == SENT) and sdev[g + j] == -77
    finally:
        s.close()


def test_profiling_changes_no_result(monkeypatch):
    """set_profiling(True) after the solve keeps the resident split: the same call over a range straddling the pipelined halves
    gives the same bits and return code with the HIP events around the stages of both halves, and their times are reported"""
    case = next(g for g in GRID if g[0] == "pipelined")
    name, m, n, t_max, members, B, env, ranges = case
    probs = [synth.make_problem(13000 + k, m, n, t_max) for k in range(B)]
    s = make_solver(monkeypatch, **env)
    try:
        solve(s, probs, t_max, False)
        split = s.pipeline_split()
        assert 0 < split < B
        p0, cnt = split - 7, 21
        gam = []
        for k in range(p0, p0 + cnt):
            ref = go.gn_subproblem(*probs[k])
            gam.append(nr.make_gammas(13000 + 7 * k, probs[k][0], probs[k][2], ref)[k % 5 == 0])     # every fifth one indefinite
        G = np.stack(gam)
        take = np.array([j != 3 for j in range(cnt)], dtype=np.int64)
        p_off, st_off, rc_off = s.newton_direction_batched(G, p0, cnt, take=take)
        assert rc_off == 1 and sorted(set(st_off)) == [-1, 0, 1]
        s.set_profiling(True)
        try:
            p_on, st_on, rc_on = s.newton_direction_batched(G, p0, cnt, take=take)
            ms = s.newton_stage_ms()
        finally:
            s.set_profiling(False)
        assert s.pipeline_split() == split
        assert rc_on == rc_off
        assert np.array_equal(p_on, p_off, equal_nan=True) and np.array_equal(st_on, st_off)
        assert len(ms) == 4 and all(np.isfinite(x) and x >= 0 for x in ms) and sum(ms) > 0, ms
    finally:
        s.close()
