"""Batched subspace re-solve (enlsip_gn_resolve_batched*, enlsip_gn_get_diagR_batched) on the GPU.

Parity: every re-solved problem against oracle.gn_oracle.sub_search_direction on the oracle's factors, with the tolerances of
tests/test_gpu_parity.py::test_resolve_truncated_dims (rel p 1e-11, or 1e-9 where A is rank deficient as in
test_batched_matches_single; rel b 1e-12; ||d|| 1e-12; |d[:dimJ2]| 1e-10).  Against the per-problem entry point: 1e-13 relative
(rounding of another summation order: p1 no longer comes from a refactorisation, Q0' is applied block-wise)."""
import ctypes as C

import numpy as np
import pytest

from oracle import enlsip_outer as eo, gn_oracle as go, synth

pytestmark = pytest.mark.gpu

HOLD = -2
SENT = 0x7FF8DEADBEEF0000          # a NaN payload no kernel produces


def rel(a, b):
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


def make_solver(monkeypatch, **env):
    from enlsip_gn import GNSolver
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return GNSolver(device=0)


def make_batch(seed, B, m, n, t, ts=None, deficient=()):
    """B problems (J, rx, A, cx); ts: each problem's own t (ragged), deficient: members with a rank-deficient A"""
    probs = []
    for k in range(B):
        tk = t if ts is None else ts[k]
        gen = synth.make_rank_deficient_A if k in deficient else synth.make_problem
        probs.append(gen(seed + k, m, n, tk))
    return probs


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


def requests(refs, ts):
    """per-problem (dimA, dimJ2, code), mixed inside one call: full ranks, truncated ranks, (0, 0), dimA = rankA with a small
    dimJ2, code 1 where rankA == t, and code 0 holes at odd positions.  dimA <= rankA and dimJ2 <= rankJ2 everywhere.
    A member with a rank-deficient A keeps dimJ2 = rankJ2: the trailing columns of F_A.Q are built from reflectors of
    rounding-level columns, so J2 = (J F_A.Q)[:, rankA+1:] is only determined up to a rotation — p with the full dimJ2 does not
    depend on it, a truncated dimJ2 (and the single entries of d) would."""
    out = []
    for j, (ref, tk) in enumerate(zip(refs, ts)):
        rA, rJ = ref.rankA, ref.rankJ2
        kind = j % 8
        if rA < tk and kind not in (1, 5):
            out.append(((rA, rA // 2, 0, rA - 1)[kind % 4], rJ, -1))
            continue
        if kind in (1, 5):
            out.append((0, 0, 0))
        elif kind == 0:
            out.append((rA, rJ, -1))
        elif kind == 2:
            out.append((rA // 2, rJ // 2, -1))
        elif kind == 3:
            out.append((rA, min(rJ, 3), -1))
        elif kind == 4:
            out.append((0, 0, -1))
        elif kind == 6:
            out.append((rA, rJ, 1) if rA == tk else (rA, rJ, -1))
        else:
            out.append((max(rA - 1, 0), max(rJ - 2, 0), -1))
    return out


def oracle_resolve(prob, ref, dimA, dimJ2, code):
    J, rx, A, cx = prob
    n, t = J.shape[1], A.shape[0] if A.size else 0
    JQ1 = ref.F_A.rmul_Q(J) if t else J
    return go.sub_search_direction(JQ1[:, :ref.rankA], rx, cx, ref.F_A, ref.F_L11, ref.F_J2, n, t, ref.rankA, dimA, dimJ2, code)


def deficient_member_determinacy(prob, ref):
    """CPU only: what of a rank-deficient member is determined.  A 1e-15 relative perturbation of A (a rounding) is applied in the
    oracle: returns the relative changes of p with the full dimJ2, of ||d||, of |d[:rankJ2]| and of p with dimJ2 = rankJ2 // 2."""
    J, rx, A, cx = prob
    A2 = A * (1.0 + 1e-15 * np.random.default_rng(5).uniform(-1, 1, A.shape))
    ref2 = go.gn_subproblem(J, rx, A2, cx)
    assert (ref2.rankA, ref2.rankJ2) == (ref.rankA, ref.rankJ2)
    rJ = ref.rankJ2
    nd = np.linalg.norm(ref.d)
    pa, _, _ = oracle_resolve(prob, ref, ref.rankA, rJ // 2, -1)
    pb, _, _ = oracle_resolve((J, rx, A2, cx), ref2, ref.rankA, rJ // 2, -1)
    return (rel(ref2.p, ref.p), abs(np.linalg.norm(ref2.d) - nd) / nd, rel(np.abs(ref2.d[:rJ]), np.abs(ref.d[:rJ])), rel(pb, pa))


def assert_deficient_member_is_compared_where_determined(prob, ref):
    """the comparisons kept for such a member (p at the full dimJ2 to 1e-9, ||d|| to 1e-12) are stable under a rounding of A, the
    ones left out (entries of d, p at a truncated dimJ2) move by far more than their bounds of 1e-10 / 1e-9"""
    dp, dn, dd, dpt = deficient_member_determinacy(prob, ref)
    assert dp <= 1e-12 and dn <= 1e-13, (dp, dn)
    assert dd >= 1e-3 and dpt >= 1e-3, (dd, dpt)


def check_against_oracle(probs, refs, ts, reqs, out, t_max, prob0=0):
    for j, (dA, dJ, cd) in enumerate(reqs):
        k = prob0 + j
        if cd == 0:
            for key in ("p", "b", "d"):
                assert np.all(np.isnan(out[key][j])), (key, j)
            assert out["status"][j] == -1 and np.all(out["info"][j] == -1)
            continue
        assert out["status"][j] == 0, (j, out["status"][j])
        ref, tk = refs[k], ts[k]
        p_ref, b_ref, d_ref = oracle_resolve(probs[k], ref, dA, dJ, cd)
        tol_p = 1e-11 if ref.code == 1 else 1e-9
        assert rel(out["p"][j], p_ref) <= tol_p, (j, rel(out["p"][j], p_ref))
        if tk:
            assert rel(out["b"][j, :tk], b_ref) <= 1e-12, (j, rel(out["b"][j, :tk], b_ref))
        assert np.all(out["b"][j, tk:] == 0.0)
        nd = np.linalg.norm(d_ref)
        assert abs(np.linalg.norm(out["d"][j]) - nd) <= 1e-12 * nd, j
        if ref.rankA == tk:          # (rank-deficient A: only ||d|| is determined, see requests)
            assert rel(np.abs(out["d"][j][:dJ]), np.abs(d_ref[:dJ])) <= 1e-10, j
        assert tuple(out["info"][j]) == (ref.rankA, ref.rankJ2, cd, dA, dJ, 0), (j, out["info"][j])


# name, B, m, n, t, ragged ts (None: uniform), rank-deficient members, environment, expected form, route names that must be set
SHAPES = [
    ("c5", 12, 256, 32, 4, None, (2,), {}, 1, ()),
    ("c3_pipelined", 160, 512, 64, 8, None, (6,), {"ENLSIP_GN_PIPELINE": "1"}, 1, ("pipeline_split",)),
    ("general_ragged", 11, 600, 40, 6, [6, 3, 6, 0, 6, 6, 5, 6, 6, 2, 6], (4,), {}, 1, ()),
    ("general_pairs", 5, 2048, 128, 16, None, (2,), {"ENLSIP_GN_PAIR": "1"}, 0, ("sweep_pairs", "sweep_tree")),
    ("distributed", 4, 500, 200, 100, None, (), {}, 0, ("constraint_dist",)),
    ("c2_small_batch", 2, 4096, 512, 64, None, (), {}, 0, ("sweep_tree",)),
]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_parity_with_oracle(shape, monkeypatch):
    name, B, m, n, t, ts, deficient, env, form, routes = shape
    probs = make_batch(9100, B, m, n, t, ts, deficient)
    ts_ = ts or [t] * B
    refs = [go.gn_subproblem(*p) for p in probs]
    for k in deficient:
        assert refs[k].rankA < ts_[k]
        assert_deficient_member_is_compared_where_determined(probs[k], refs[k])       # on the CPU, before the GPU is consulted
    reqs = requests(refs, ts_)
    s = make_solver(monkeypatch, **env)
    try:
        sol = solve(s, probs, t, ts is not None)
        route = {r.lower() for r in s.route()}
        for r in routes:
            assert any(r in x for x in route), (r, sorted(route))
        if "PIPELINE" in "".join(env):
            assert 0 < s.pipeline_split() < B
        for k, ref in enumerate(refs):
            assert sol[3][k][0] == ref.rankA and sol[3][k][1] == ref.rankJ2
        dA, dJ, cd = (np.array(x, dtype=np.int64) for x in zip(*reqs))
        out, rc = s.resolve_batched(m, n, t, dA, dJ, cd, 0, B)
        assert rc == 0 and s.resolve_form() == form
        check_against_oracle(probs, refs, ts_, reqs, out, t)
        # an inner range from an odd prob0 (straddling the pipelined halves where there are any)
        p0 = max(s.pipeline_split() - 3, 1) | 1
        cnt = min(7, B - p0)
        out2, rc = s.resolve_batched(m, n, t, dA[p0:p0 + cnt], dJ[p0:p0 + cnt], cd[p0:p0 + cnt], p0, cnt)
        assert rc == 0
        check_against_oracle(probs, refs, ts_, reqs[p0:p0 + cnt], out2, t, p0)
        # diag(F.R) of the range: the per-problem accessor's, zeros past each problem's own length
        from enlsip_gn import FACTOR_A, FACTOR_J2, FACTOR_L11
        for which, stride in ((FACTOR_A, min(n, t)), (FACTOR_L11, min(n, t)), (FACTOR_J2, min(m, n))):
            D = s.diagR_batched(which, stride, 0, B)
            for k in range(0, B, max(B // 5, 1)):
                dk = s.factor(which, k).diagR()
                assert np.array_equal(D[k, :dk.size], dk) and np.all(D[k, dk.size:] == 0.0)
    finally:
        s.close()


def snapshot(s, m, n, B):
    from enlsip_gn import FACTOR_A, FACTOR_J2, FACTOR_L11
    snap = []
    for k in range(B):
        for which in (FACTOR_A, FACTOR_L11, FACTOR_J2):
            f = s.factor(which, k)
            snap += [f.R.copy(), f.p.copy()]
        snap.append(s.JQ1(m, n, k))
    return snap


@pytest.mark.parametrize("shape", [(7, 600, 40, 6), (3, 700, 130, 20)], ids=["wave", "general"])
def test_same_as_per_problem_entry_point(shape, monkeypatch):
    B, m, n, t = shape
    probs = make_batch(9300, B, m, n, t)
    refs = [go.gn_subproblem(*p) for p in probs]
    reqs = [(r.rankA - (k % 3), r.rankJ2 - 2 * (k % 4), 1 if k % 3 == 0 else -1) for k, r in enumerate(refs)]
    G = synth.normal_stream(9400, 0, n * n).reshape(n, n)
    G = 0.5 * (G + G.T) * 1e-3
    for (J, rx, A, cx), r in zip(probs, refs):       # CPU: the conditions the consumers below amplify by
        assert r.rankA == t and np.linalg.cond(r.F_A.R[:t, :t]) <= 10.0
        Q = np.column_stack([r.F_A.Q_mul(e) for e in np.eye(n)])
        J2 = (J @ Q)[:, t:]
        W22 = (Q.T @ G @ Q)[t:, t:] + J2.T @ J2
        ev = np.linalg.eigvalsh(0.5 * (W22 + W22.T))
        assert ev[0] > 0 and ev[-1] / ev[0] <= 10.0
    s1, s2 = make_solver(monkeypatch), make_solver(monkeypatch)
    try:
        solve(s1, probs, t, False)
        solve(s2, probs, t, False)
        before = snapshot(s2, m, n, B)
        per = [s1.resolve(m, n, t, dA, dJ, cd, k) for k, (dA, dJ, cd) in enumerate(reqs)]
        dA, dJ, cd = (np.array(x, dtype=np.int64) for x in zip(*reqs))
        out, rc = s2.resolve_batched(m, n, t, dA, dJ, cd, 0, B)
        assert rc == 0
        after = snapshot(s2, m, n, B)
        for a, b in zip(before, after):
            assert np.array_equal(a, b)          # F_A, F_L11, F_J2, their pivots and J*Q1: bitwise untouched
        for k, (p, b, d) in enumerate(per):
            assert rel(out["p"][k], p) <= 1e-13 and rel(out["b"][k], b) <= 1e-13
            assert rel(np.abs(out["d"][k]), np.abs(d)) <= 1e-13
            assert tuple(out["info"][k]) == (refs[k].rankA, refs[k].rankJ2, reqs[k][2], reqs[k][0], reqs[k][1], 0)
        # the consumers that read the resident p1 / state behave the same on both handles, to the same 1e-13.  Both amplify a
        # difference of their inputs by a condition number (R_A in the second estimate, W22 in the Newton step), so the inputs
        # are chosen with both below 10 — checked on the CPU above — and Gamma small enough that W22 is positive definite: the
        # Newton branch must really run (error = False) on every problem.
        for k in range(B):
            lam1, lam2 = s1.second_lagrange(t, per[k][0], prob=k), s2.second_lagrange(t, out["p"][k], prob=k)
            pn1, e1 = s1.newton_direction(G, k)
            pn2, e2 = s2.newton_direction(G, k)
            a = s1.resolve(m, n, t, max(reqs[k][0] - 1, 0), max(reqs[k][1] - 1, 0), -1, k)
            b = s2.resolve(m, n, t, max(reqs[k][0] - 1, 0), max(reqs[k][1] - 1, 0), -1, k)
            print(f"problem {k}: second_lagrange {rel(lam2, lam1):.2e}  newton {rel(pn2, pn1):.2e} (error {e1}, {e2})  "
                  f"resolve {[float(f'{rel(y, x):.2e}') for x, y in zip(a, b)]}")
            assert rel(lam2, lam1) <= 1e-13
            assert not e1 and not e2
            assert rel(pn2, pn1) <= 1e-13
            assert all(rel(y, x) <= 1e-13 for x, y in zip(a, b))
    finally:
        s1.close()
        s2.close()


@pytest.mark.parametrize("shape", [(6, 256, 32, 4), (3, 700, 130, 20)], ids=["wave", "general"])
def test_held_flow(shape, monkeypatch):
    B, m, n, t = shape
    probs = make_batch(9500, B, m, n, t, deficient=(1,))
    refs = [go.gn_subproblem(*p) for p in probs]
    dA = np.array([max(r.rankA - (k % 2), 0) for k, r in enumerate(refs)], dtype=np.int64)
    dJ = np.array([max(r.rankJ2 - 3 * (k % 3), 0) for k, r in enumerate(refs)], dtype=np.int64)
    rA = np.array([r.rankA for r in refs], dtype=np.int64)
    hold = np.full(B, HOLD, dtype=np.int64)
    s = make_solver(monkeypatch)
    try:
        solve(s, probs, t, False)
        one, rc = s.resolve_batched(m, n, t, dA, dJ, -1, 0, B)
        assert rc == 0
        # no held result after a call without HOLD
        o, rc = s.resolve_batched(m, n, t, hold, dJ, -1, 0, B)
        assert rc == 1 and np.all(o["status"] == 3) and np.all(np.isnan(o["p"]))
        first, rc = s.resolve_batched(m, n, t, rA, hold, -1, 0, B)                  # b of :1251
        assert rc == 0 and np.all(np.isnan(first["p"]))
        for k, r in enumerate(refs):
            b_ref = r.F_L11.Qt_mul(-probs[k][3][r.F_A.p - 1])
            assert rel(first["b"][k], b_ref) <= 1e-12
        # asked for b alone (no d, every request held) the call applies no F_J2.Q' and holds nothing
        bonly, rc = s.resolve_batched(m, n, t, rA, hold, -1, 0, B, want=("b", "status"))
        assert rc == 0 and np.array_equal(bonly["b"], first["b"])
        o, rc = s.resolve_batched(m, n, t, hold, dJ, -1, 0, B)
        assert rc == 1 and np.all(o["status"] == 3)
        second, rc = s.resolve_batched(m, n, t, dA, hold, -1, 0, B)                 # d of :1162 with the chosen dimA
        assert rc == 0 and np.all(np.isnan(second["p"]))
        third, rc = s.resolve_batched(m, n, t, hold, dJ, -1, 0, B)                  # p of :1253
        assert rc == 0
        assert np.array_equal(second["b"], one["b"]) and np.array_equal(second["d"], one["d"])
        assert np.array_equal(third["p"], one["p"]) and np.array_equal(third["b"], one["b"]) and np.array_equal(third["d"], one["d"])
        assert np.array_equal(third["info"], one["info"])
        # a per-problem re-solve of problem 2 invalidates its hold, the others keep theirs
        s.resolve_batched(m, n, t, dA, hold, -1, 0, B)
        s.resolve(m, n, t, int(dA[2]), int(dJ[2]), -1, 2)
        o, rc = s.resolve_batched(m, n, t, hold, dJ, -1, 0, B)
        assert rc == 1 and o["status"][2] == 3 and np.all(np.delete(o["status"], 2) == 0)
        assert np.array_equal(np.delete(o["p"], 2, axis=0), np.delete(one["p"], 2, axis=0)) and np.all(np.isnan(o["p"][2]))
        # ... and a solve invalidates all of them
        s.resolve_batched(m, n, t, dA, hold, -1, 0, B)
        solve(s, probs, t, False)
        o, rc = s.resolve_batched(m, n, t, hold, dJ, -1, 0, B)
        assert rc == 1 and np.all(o["status"] == 3)
    finally:
        s.close()


def fabricated_previous(k, prob, ref, t):
    """a previous iterate fixed by the test: one more / one fewer dimension than the ranks in turn, a short or a long step"""
    J, rx, A, cx = prob
    z = np.zeros(0)
    return eo.Iteration(x=z, p=z, rx=rx * (1.05 + 0.01 * (k % 5)), cx=cx * (1.1 + 0.02 * (k % 3)), t=t, alpha=(0.05, 0.5, 1.0)[k % 3],
                        index_alpha_upp=0, lam=z, w=z, rankA=ref.rankA, rankJ2=ref.rankJ2, dimA=max(ref.rankA - (k % 3), 0),
                        dimJ2=max(ref.rankJ2 - 2 * (k % 4), 1), b_gn=z, d_gn=z, predicted_reduction=0.0, progress=0.0, grad_res=0.0,
                        speed=0.0, beta=0.0, restart=False, first=False, add=False, delete=False, index_del=0, code=-1,
                        nb_newton_steps=0)


class _Diag:
    """what choose_subspace_dimensions reads of a factorisation when the library computes the vectors: diag(R), and for F_J2 the
    d the batched call returned"""
    def __init__(self, diag, n, d=None):
        self.R = np.zeros((len(diag), n))
        self.R[np.arange(len(diag)), np.arange(len(diag))] = diag
        self.P = np.eye(n)
        self._d = d

    def Qt_mul(self, _):
        return self._d.copy()


def test_reference_flow(monkeypatch):
    """search_direction_analys' subspace branch (src/enlsip_functions.jl:1249-1253) over a batch: choose_subspace_dimensions on the
    oracle's b, d, diagonals and on the batched calls' must pick the same (dimA, dimJ2) for every problem."""
    B, m, n, t = 16, 600, 40, 6
    probs = [synth.make_graded_J(9700 + k, m, n, t, 3.0 + 0.5 * (k % 4)) if k % 2 else synth.make_problem(9700 + k, m, n, t)
             for k in range(B)]
    refs = [go.gn_subproblem(*p) for p in probs]
    prev = [fabricated_previous(k, probs[k], refs[k], t) for k in range(B)]

    def oracle_choice(k, scale_b=1.0, scale_d=None):
        J, rx, A, cx = probs[k]
        r = refs[k]
        b = r.F_L11.Qt_mul(-cx[r.F_A.p - 1]) * scale_b
        F_J2 = r.F_J2
        if scale_d is not None:
            class F:
                R, P = r.F_J2.R, None
                Qt_mul = staticmethod(lambda v: r.F_J2.Qt_mul(v) * scale_d)
            F_J2 = F
        J1 = r.F_A.rmul_Q(J)[:, :r.rankA]
        return eo.choose_subspace_dimensions(float(rx @ rx), rx, float(cx @ cx), J1, t, r.rankJ2, r.rankA, b, r.F_L11, F_J2, prev[k], False)

    want = [oracle_choice(k) for k in range(B)]
    rng = np.random.default_rng(1)
    for k in range(B):          # the oracle's own choice is stable under a 1e-10 relative perturbation of its b, d (CPU only)
        for _ in range(4):
            sb = 1.0 + 1e-10 * rng.uniform(-1, 1, t)
            sd = 1.0 + 1e-10 * rng.uniform(-1, 1, m)
            assert oracle_choice(k, sb, sd) == want[k], k
        assert want[k][0] <= refs[k].rankA and want[k][1] <= refs[k].rankJ2
    assert len(set(want)) >= 3, sorted(set(want))
    assert any(w[1] < refs[k].rankJ2 for k, w in enumerate(want)) and any(w[1] == refs[k].rankJ2 for k, w in enumerate(want))

    from enlsip_gn import FACTOR_J2, FACTOR_L11
    s = make_solver(monkeypatch)
    try:
        solve(s, probs, t, False)
        rA = np.array([r.rankA for r in refs], dtype=np.int64)
        hold = np.full(B, HOLD, dtype=np.int64)
        first, rc = s.resolve_batched(m, n, t, rA, hold, -1, 0, B)
        assert rc == 0
        DL, DJ = s.diagR_batched(FACTOR_L11, t, 0, B), s.diagR_batched(FACTOR_J2, n, 0, B)

        def gpu_choice(k, d):
            J, rx, A, cx = probs[k]
            r = refs[k]
            J1 = np.zeros((m, r.rankA))         # p1 and J1 p1 are the library's: d comes back from the held call
            return eo.choose_subspace_dimensions(float(rx @ rx), rx, float(cx @ cx), J1, t, r.rankJ2, r.rankA, first["b"][k],
                                                 _Diag(DL[k, :t], t), _Diag(DJ[k, :n - r.rankA], n - r.rankA, d), prev[k], False)
        dimA = np.array([gpu_choice(k, np.zeros(m))[0] for k in range(B)], dtype=np.int64)       # dimA does not depend on d
        second, rc = s.resolve_batched(m, n, t, dimA, hold, -1, 0, B)
        assert rc == 0
        got = [gpu_choice(k, second["d"][k]) for k in range(B)]
        assert got == want
        dimJ2 = np.array([g[1] for g in got], dtype=np.int64)
        third, rc = s.resolve_batched(m, n, t, hold, dimJ2, -1, 0, B)
        assert rc == 0
        for k in range(B):
            p_ref, _, _ = oracle_resolve(probs[k], refs[k], want[k][0], want[k][1], -1)
            assert rel(third["p"][k], p_ref) <= 1e-11, (k, rel(third["p"][k], p_ref))
    finally:
        s.close()


def test_edges_and_refusals(monkeypatch):
    B, m, n, t = 6, 300, 24, 5
    probs = make_batch(9800, B, m, n, t, deficient=(3,))
    refs = [go.gn_subproblem(*p) for p in probs]
    s = make_solver(monkeypatch)
    lib, h = s._lib, s._h
    one = np.array([1], dtype=np.int64)
    z = np.zeros(1, dtype=np.int64)
    call = lambda p0, cnt: lib.enlsip_gn_resolve_batched(h, p0, cnt, z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p),
                                                         (-one).ctypes.data_as(C.c_void_p), None, None, None, None, None)
    try:
        assert call(0, 1) == -1                                          # before any solve
        s.factor_constraints(m, probs[0][2], probs[0][3])
        assert call(0, 1) == -1                                          # only F_A / F_L11 are resident
        solve(s, probs, t, False)
        assert call(0, 0) == -2 and call(B, 1) == -3 and call(B - 1, 2) == -3
        assert lib.enlsip_gn_resolve_batched(h, 0, 1, None, None, None, None, None, None, None, None) == -4
        rA = np.array([r.rankA for r in refs], dtype=np.int64)
        rJ = np.array([r.rankJ2 for r in refs], dtype=np.int64)
        dA, dJ, cd = rA.copy(), rJ.copy(), np.full(B, -1, dtype=np.int64)
        dA[0] = t + 1                   # dimA out of range
        dJ[2] = n - refs[2].rankA + 1   # dimJ2 out of range
        cd[3] = 1                       # code 1 with rankA < t
        dA[5] = -1
        out, rc = s.resolve_batched(m, n, t, dA, dJ, cd, 0, B)
        assert rc == 1 and list(out["status"]) == [1, 0, 2, 4, 0, 1]
        for k in (0, 2, 3, 5):
            assert np.all(np.isnan(out["p"][k])) and np.all(np.isnan(out["d"][k]))
        reqs = [(int(dA[k]), int(dJ[k]), int(cd[k])) if out["status"][k] == 0 else (0, 0, 0) for k in range(B)]
        out["status"][[0, 2, 3, 5]] = -1
        check_against_oracle(probs, refs, [t] * B, reqs, out, t)
    finally:
        s.close()


def test_range_into_an_earlier_chunk(monkeypatch):
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    import consumer_reference as cr
    B = cr.max_launch_batch() + 40
    m, n, t = 6, 3, 2
    J = synth.normal_stream(9900, 0, B * m * n).reshape(B, n, m)
    rx = synth.normal_stream(9900, 1, B * m).reshape(B, m)
    At = synth.normal_stream(9900, 2, B * t * n).reshape(B, t, n)
    cx = synth.normal_stream(9900, 3, B * t).reshape(B, t)
    s = make_solver(monkeypatch)
    try:
        s.solve_batched(J, rx, At, cx)
        assert "chunked" in s.route()
        dA, dJ = np.full(3, t, dtype=np.int64), np.full(3, n - t, dtype=np.int64)
        with pytest.raises(Exception):
            s.resolve_batched(m, n, t, dA, dJ, -1, 5, 3)
        assert s._lib.enlsip_gn_resolve_batched(s._h, 5, 3, dA.ctypes.data_as(C.c_void_p), dJ.ctypes.data_as(C.c_void_p),
                                                dA.ctypes.data_as(C.c_void_p), None, None, None, None, None) == -3
        k0 = B - 4
        out, rc = s.resolve_batched(m, n, t, dA, dJ, -1, k0, 3)
        assert rc == 0
        for j in range(3):
            prob = (J[k0 + j].T, rx[k0 + j], At[k0 + j], cx[k0 + j])
            ref = go.gn_subproblem(*prob)
            p_ref, _, _ = oracle_resolve(prob, ref, t, n - t, -1)
            assert rel(out["p"][j], p_ref) <= 1e-11
    finally:
        s.close()


def test_rescued_member_on_the_second_half(monkeypatch):
    """a member scaled by 2^600 (as in tests/test_gpu_consumer_edges.py) lives on a rescue handle of the second pipelined half: its
    slots are the per-problem entry point's, the neighbours are checked against the oracle"""
    B, m, n, t = 192, 1024, 48, 16
    kr = 150
    J = synth.normal_stream(10000, 0, B * m * n).reshape(B, n, m)
    rx = synth.normal_stream(10000, 1, B * m).reshape(B, m)
    At = synth.normal_stream(10000, 2, B * t * n).reshape(B, t, n)
    cx = synth.normal_stream(10000, 3, B * t).reshape(B, t)
    J[kr] *= 2.0 ** 600
    rx[kr] *= 2.0 ** 600
    s, s1 = make_solver(monkeypatch), make_solver(monkeypatch)
    try:
        s.solve_batched(J, rx, At, cx)
        s1.solve_batched(J, rx, At, cx)
        split = s.pipeline_split()
        assert 0 < split <= kr and "rescaled" in s.route()
        p0, cnt = kr - 5, 11
        dA = np.array([t - (j % 3) for j in range(cnt)], dtype=np.int64)
        dJ = np.array([n - t - 2 * (j % 4) for j in range(cnt)], dtype=np.int64)
        out, rc = s.resolve_batched(m, n, t, dA, dJ, -1, p0, cnt)
        assert rc == 0 and np.all(out["status"] == 0)
        p1, b1, d1 = s1.resolve(m, n, t, int(dA[kr - p0]), int(dJ[kr - p0]), -1, kr)
        assert np.array_equal(out["p"][kr - p0], p1) and np.array_equal(out["b"][kr - p0], b1) and np.array_equal(out["d"][kr - p0], d1)
        for j in (0, kr - p0 - 1, kr - p0 + 1, cnt - 1):
            k = p0 + j
            prob = (J[k].T, rx[k], At[k], cx[k])
            p_ref, b_ref, _ = oracle_resolve(prob, go.gn_subproblem(*prob), int(dA[j]), int(dJ[j]), -1)
            assert rel(out["p"][j], p_ref) <= 1e-11 and rel(out["b"][j], b_ref) <= 1e-12
    finally:
        s.close()
        s1.close()


@pytest.mark.parametrize("shape", [(100, 10, 6), (300, 80, 12)], ids=["wave", "general"])
def test_dev_form_writes_only_its_slots(shape, monkeypatch):
    import torch
    m, n, t = shape
    B, prob0, count, g = 8, 1, 6, 2
    probs = make_batch(10100, B, m, n, t)
    refs = [go.gn_subproblem(*p) for p in probs]
    s = make_solver(monkeypatch)
    try:
        solve(s, probs, t, False)
        cd = np.array([-1, 0, -1, 0, 1, -1], dtype=np.int64)
        dA = np.array([refs[prob0 + j].rankA for j in range(count)], dtype=np.int64)
        dJ = np.array([max(refs[prob0 + j].rankJ2 - j, 0) for j in range(count)], dtype=np.int64)

        def guarded(width, dtype=torch.float64):
            if dtype == torch.float64:
                return torch.full((count + 2 * g, width), SENT, dtype=torch.int64, device="cuda:0").view(torch.float64)
            return torch.full((count + 2 * g, width), -77, dtype=dtype, device="cuda:0")
        bufs = {"p": guarded(n), "b": guarded(t), "d": guarded(m), "info": guarded(6, torch.int64), "status": guarded(1, torch.int32)}
        base = lambda x: x.data_ptr() + g * x[0].numel() * x.element_size()
        torch.cuda.synchronize()
        rc = s.resolve_batched_dev(prob0, count, dA, dJ, cd, base(bufs["p"]), base(bufs["b"]), base(bufs["d"]), base(bufs["info"]),
                                   base(bufs["status"]))
        assert rc == 0
        torch.cuda.synchronize()
        host, _ = s.resolve_batched(m, n, t, dA, dJ, cd, prob0, count)
        for key in ("p", "b", "d"):
            v = bufs[key].view(torch.int64).cpu().numpy()
            untouched = [j for j in range(count + 2 * g) if j < g or j >= g + count or cd[j - g] == 0]
            assert np.all(v[untouched] == SENT), key
            w = bufs[key].cpu().numpy()
            for j in range(count):
                if cd[j]:
                    assert np.array_equal(w[g + j], host[key][j]), (key, j)
        for key in ("info", "status"):
            v = bufs[key].cpu().numpy()
            for j in range(count + 2 * g):
                if j < g or j >= g + count or cd[j - g] == 0:
                    assert np.all(v[j] == -77), (key, j)
                else:
                    assert np.array_equal(v[j].ravel(), np.atleast_1d(host[key][j - g]).ravel()), (key, j)
    finally:
        s.close()


def test_profiling_changes_no_result(monkeypatch):
    """set_profiling(True) after the solve keeps the resident split: the same call over a range straddling the pipelined halves
    gives the same bits and return code with the HIP events around the Q0' launches of both halves, and their time is reported"""
    B, m, n, t = 160, 512, 64, 8
    J = synth.normal_stream(10100, 0, B * m * n).reshape(B, n, m)
    rx = synth.normal_stream(10100, 1, B * m).reshape(B, m)
    At = synth.normal_stream(10100, 2, B * t * n).reshape(B, t, n)
    cx = synth.normal_stream(10100, 3, B * t).reshape(B, t)
    s = make_solver(monkeypatch, ENLSIP_GN_PIPELINE="1")
    try:
        infos = s.solve_batched(J, rx, At, cx)[3]
        split = s.pipeline_split()
        assert 0 < split < B
        p0, cnt = split - 9, 21
        # truncated and full dimensions, a code 0 hole and one request that is refused (dimJ2 beyond kp)
        dA = np.array([infos[p0 + j][0] - (j % 3) for j in range(cnt)], dtype=np.int64)
        dJ = np.array([infos[p0 + j][1] - 5 * (j % 4) for j in range(cnt)], dtype=np.int64)
        cd = np.array([0 if j == 4 else -1 for j in range(cnt)], dtype=np.int64)
        dJ[13] = n + 1
        off, rc_off = s.resolve_batched(m, n, t, dA, dJ, cd, p0, cnt)
        assert rc_off == 1 and off["status"][13] != 0 and np.count_nonzero(off["status"] > 0) == 1
        s.set_profiling(True)
        try:
            on, rc_on = s.resolve_batched(m, n, t, dA, dJ, cd, p0, cnt)
            q0_ms = s.resolve_q0_ms()
        finally:
            s.set_profiling(False)
        assert s.pipeline_split() == split
        assert rc_on == rc_off
        assert set(on) == set(off)
        for key in off:
            assert np.array_equal(on[key], off[key], equal_nan=on[key].dtype.kind == "f"), key
        assert np.isfinite(q0_ms) and q0_ms > 0, q0_ms
    finally:
        s.close()
