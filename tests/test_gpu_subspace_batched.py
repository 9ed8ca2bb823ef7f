"""One-call subspace minimisation (enlsip_gn_subspace_direction_batched*) on the GPU: the dimension choice of
choose_subspace_dimensions (src/enlsip_functions.jl:1118-1176) made on the device between the stages of the batched re-solve.

Reference for the dimensions: oracle.enlsip_outer.choose_subspace_dimensions on the ORACLE's b, d and factors, counted only where
that choice is unchanged under four relative perturbations of 1e-10 of b and d (decisions are thresholds); every problem of every
batch here passes that filter, which is asserted on the CPU before the GPU is consulted.  Reference for p: the oracle re-solve with
the reference's dimensions, rel <= 1e-11 (the tolerance tests/test_gpu_resolve_batched.py::test_reference_flow uses at this shape).
Set-up and oracle helpers are those of tests/test_gpu_resolve_batched.py."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import enlsip_outer as eo, gn_oracle as go, synth

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_gpu_resolve_batched as rb  # noqa: E402

pytestmark = pytest.mark.gpu

HOLD = rb.HOLD
rel = rb.rel


def prev_record(prob, t, it, restart):
    """what choose_subspace_dimensions reads of previous_iter, as the call takes it (:1144, :1165, :1147, :1168)"""
    J, rx, A, cx = prob
    return (abs(it.dimA) + t - it.t, abs(it.dimJ2) + it.t - t, int(restart), it.alpha, float(it.cx @ it.cx) - float(cx @ cx),
            float(it.rx @ it.rx) - float(rx @ rx))


def pack_prev(records):
    from enlsip_gn import GNSolver
    return GNSolver.pack_subspace_prev(len(records), *(np.array(c) for c in zip(*records)))


def reference_choice(prob, ref, t, it, restart, scale_b=1.0, scale_d=None):
    J, rx, A, cx = prob
    m = J.shape[0]
    b = ref.F_L11.Qt_mul(-cx[ref.F_A.p - 1]) * scale_b if t else np.zeros(0)
    F_J2 = ref.F_J2
    if scale_d is not None:
        class F:
            R, P = ref.F_J2.R, None
            Qt_mul = staticmethod(lambda v: ref.F_J2.Qt_mul(v) * scale_d)
        F_J2 = F
    J1 = (ref.F_A.rmul_Q(J) if t else J)[:, :ref.rankA]
    return eo.choose_subspace_dimensions(float(rx @ rx), rx, float(cx @ cx), J1, t, ref.rankJ2, ref.rankA, b, ref.F_L11, F_J2, it,
                                         bool(restart))


def stable_reference_choice(k, prob, ref, t, it, restart):
    want = reference_choice(prob, ref, t, it, restart)
    rng = np.random.default_rng(100 + k)
    m = prob[0].shape[0]
    for _ in range(4):
        sb = 1.0 + 1e-10 * rng.uniform(-1, 1, t)
        sd = 1.0 + 1e-10 * rng.uniform(-1, 1, m)
        assert reference_choice(prob, ref, t, it, restart, sb, sd) == want, k
    return want


@functools.lru_cache(maxsize=None)
def flow_batch(name):
    """the two resident batches of tests 1-3, their previous iterates and the reference's choices (computed once)"""
    B, m, n, t = {"wave": (16, 600, 40, 6), "general": (6, 1100, 96, 8)}[name]
    if name == "wave":      # problems and fabricated previous iterates of test_reference_flow
        probs = [synth.make_graded_J(9700 + k, m, n, t, 3.0 + 0.5 * (k % 4)) if k % 2 else synth.make_problem(9700 + k, m, n, t)
                 for k in range(B)]
        restart = [k in (5, 11) for k in range(B)]
    else:
        probs = [synth.make_graded_J(9900 + k, m, n, t, 3.0 + 0.5 * (k % 4)) if k % 2 else synth.make_problem(9900 + k, m, n, t)
                 for k in range(B)]
        restart = [k == 4 for k in range(B)]
    refs = [go.gn_subproblem(*p) for p in probs]
    its = [rb.fabricated_previous(k, probs[k], refs[k], t) for k in range(B)]
    want = [stable_reference_choice(k, probs[k], refs[k], t, its[k], restart[k]) for k in range(B)]
    recs = [prev_record(probs[k], t, its[k], restart[k]) for k in range(B)]
    return (B, m, n, t), probs, refs, its, restart, want, recs


def check_flow(name, form, monkeypatch):
    (B, m, n, t), probs, refs, its, restart, want, recs = flow_batch(name)
    assert len(set(want)) >= 3, sorted(set(want))
    assert sum(1 for it in its if it.alpha >= 0.2) >= B // 3 and sum(restart) >= 1
    s = rb.make_solver(monkeypatch)
    try:
        rb.solve(s, probs, t, False)
        out, rc = s.subspace_direction_batched(m, n, t, pack_prev(recs), 0, B)
        print(f"{name}: chosen {[tuple(int(x) for x in out['info'][k, 3:5]) for k in range(B)]}\n{name}: wanted {want}")
        assert rc == 0 and np.all(out["status"] == 0), out["status"]
        assert s.subspace_form() == form
        for k in range(B):
            assert tuple(out["info"][k]) == (refs[k].rankA, refs[k].rankJ2, -1, want[k][0], want[k][1], 0), (k, out["info"][k], want[k])
            p_ref, b_ref, d_ref = rb.oracle_resolve(probs[k], refs[k], want[k][0], want[k][1], -1)
            print(f"{name} problem {k}: rel p {rel(out['p'][k], p_ref):.2e}  rel b {rel(out['b'][k], b_ref):.2e}")
            assert rel(out["p"][k], p_ref) <= 1e-11, (k, rel(out["p"][k], p_ref))
            assert rel(out["b"][k], b_ref) <= 1e-12
            assert abs(np.linalg.norm(out["d"][k]) - np.linalg.norm(d_ref)) <= 1e-12 * np.linalg.norm(d_ref)
    finally:
        s.close()


def test_one_wave_form(monkeypatch):
    check_flow("wave", 1, monkeypatch)


def test_general_form(monkeypatch):
    check_flow("general", 0, monkeypatch)


@pytest.mark.parametrize("name", ["wave", "general"])
def test_same_bits_as_the_re_solve_with_the_chosen_dimensions(name, monkeypatch):
    (B, m, n, t), probs, refs, its, restart, want, recs = flow_batch(name)
    s1, s2 = rb.make_solver(monkeypatch), rb.make_solver(monkeypatch)
    try:
        rb.solve(s1, probs, t, False)
        rb.solve(s2, probs, t, False)
        new, rc = s1.subspace_direction_batched(m, n, t, pack_prev(recs), 0, B)
        assert rc == 0
        dA, dJ = new["info"][:, 3].copy(), new["info"][:, 4].copy()
        old, rc = s2.resolve_batched(m, n, t, dA, dJ, -1, 0, B)
        assert rc == 0
        for key in ("p", "b", "d", "info", "status"):
            assert np.array_equal(new[key], old[key]), key
        lam1, st1, _ = s1.second_lagrange_batched(t, new["p"], 0)
        lam2, st2, _ = s2.second_lagrange_batched(t, old["p"], 0)
        assert np.array_equal(lam1, lam2) and np.array_equal(st1, st2) and np.all(np.isfinite(lam1))
        # a held result of a taken problem is dropped
        hold = np.full(B, HOLD, dtype=np.int64)
        s1.resolve_batched(m, n, t, dA, hold, -1, 0, B)
        take = np.ones(B, dtype=np.int64)
        take[1] = 0
        s1.subspace_direction_batched(m, n, t, pack_prev(recs), 0, B, take=take)
        o, rc = s1.resolve_batched(m, n, t, hold, dJ, -1, 0, B)
        assert rc == 1 and o["status"][1] == 0 and np.all(np.delete(o["status"], 1) == 3)
        assert np.array_equal(o["p"][1], old["p"][1])
    finally:
        s1.close()
        s2.close()


def test_the_max_rule_raises_dimA_after_d_was_formed(monkeypatch):
    """previous_alpha >= 0.2 and a previous dimA above the one chosen now: the reference chooses dimJ2 from the d of the CHOSEN
    dimA (:1156-1169) and calls sub_search_direction with the RAISED one (:1171-1174, :1253).  A with graded rows makes the
    choice truncate."""
    B, m, n, t = 5, 300, 24, 6
    probs = []
    for k in range(B):
        J, rx, A, cx = synth.make_problem(10300 + k, m, n, t)
        A = A * (10.0 ** (-np.arange(t) * (0.8 + 0.1 * k)))[:, None]
        probs.append((J, rx, A, cx * 10.0 ** (-np.arange(t) * 0.2)))
    refs = [go.gn_subproblem(*p) for p in probs]
    z = np.zeros(0)
    its = [eo.Iteration(x=z, p=z, rx=p[1] * 1.05, cx=p[3] * 1.1, t=t, alpha=(0.5, 1.0)[k % 2], index_alpha_upp=0, lam=z, w=z,
                        rankA=r.rankA, rankJ2=r.rankJ2, dimA=r.rankA, dimJ2=r.rankJ2, b_gn=z, d_gn=z, predicted_reduction=0.0,
                        progress=0.0, grad_res=0.0, speed=0.0, beta=0.0, restart=False, first=False, add=False, delete=False,
                        index_del=0, code=-1, nb_newton_steps=0) for k, (p, r) in enumerate(zip(probs, refs))]
    want = [stable_reference_choice(k, probs[k], refs[k], t, its[k], False) for k in range(B)]
    # the dimA the reference chose BEFORE the max: the same call after a short step (previous_dimA == rankA: gn_previous_step
    # decides, which does not read the step length)
    chosen = []
    for k in range(B):
        it = its[k]
        short = eo.Iteration(**{**it.__dict__, "alpha": 0.19})
        assert abs(it.dimA) == refs[k].rankA and abs(it.dimJ2) == refs[k].rankJ2
        chosen.append(reference_choice(probs[k], refs[k], t, short, False)[0])
    raised = [k for k in range(B) if want[k][0] > chosen[k]]
    assert raised, (want, chosen)
    recs = [prev_record(probs[k], t, its[k], False) for k in range(B)]
    s = rb.make_solver(monkeypatch)
    try:
        rb.solve(s, probs, t, False)
        out, rc = s.subspace_direction_batched(m, n, t, pack_prev(recs), 0, B)
        assert rc == 0
        for k in range(B):
            assert tuple(out["info"][k, 3:5]) == want[k], (k, out["info"][k], want[k], chosen[k])
            p_ref, b_ref, d_ref = rb.oracle_resolve(probs[k], refs[k], want[k][0], want[k][1], -1)
            assert rel(out["p"][k], p_ref) <= 1e-11, (k, rel(out["p"][k], p_ref))
            assert rel(np.abs(out["d"][k][:want[k][1]]), np.abs(d_ref[:want[k][1]])) <= 1e-10
        old, rc = s.resolve_batched(m, n, t, out["info"][:, 3].copy(), out["info"][:, 4].copy(), -1, 0, B)
        assert rc == 0 and all(np.array_equal(out[key], old[key]) for key in ("p", "b", "d", "info"))
    finally:
        s.close()


def test_ragged_batch(monkeypatch):
    B, m, n, t = 7, 300, 24, 8
    ts = [8, 0, 3, 8, 0, 3, 8]
    probs = rb.make_batch(10400, B, m, n, t, ts)
    refs = [go.gn_subproblem(*p) for p in probs]
    its = [rb.fabricated_previous(k, probs[k], refs[k], ts[k]) for k in range(B)]
    want = [stable_reference_choice(k, probs[k], refs[k], ts[k], its[k], False) for k in range(B)]
    recs = [prev_record(probs[k], ts[k], its[k], False) for k in range(B)]
    s = rb.make_solver(monkeypatch)
    try:
        rb.solve(s, probs, t, True)
        out, rc = s.subspace_direction_batched(m, n, t, pack_prev(recs), 0, B)
        assert rc == 0 and np.all(out["status"] == 0)
        for k in range(B):
            assert tuple(out["info"][k, 3:5]) == want[k], (k, out["info"][k], want[k])
            assert np.all(out["b"][k, ts[k]:] == 0.0)
            p_ref, b_ref, d_ref = rb.oracle_resolve(probs[k], refs[k], want[k][0], want[k][1], -1)
            assert rel(out["p"][k], p_ref) <= 1e-11, (k, rel(out["p"][k], p_ref))
            if ts[k] == 0:      # rankA <= 0: dimA = 0, d = F_J2.Q' (-rx)   (:1136-1140, :1161-1163)
                assert refs[k].rankA == 0 and out["info"][k, 3] == 0
                d0 = refs[k].F_J2.Qt_mul(-probs[k][1])
                assert abs(np.linalg.norm(out["d"][k]) - np.linalg.norm(d0)) <= 1e-12 * np.linalg.norm(d0)
                kk = want[k][1]
                assert rel(np.abs(out["d"][k][:kk]), np.abs(d0[:kk])) <= 1e-10
    finally:
        s.close()


def test_range_over_the_pipelined_halves(monkeypatch):
    B, m, n, t = 130, 64, 8, 2
    J = synth.normal_stream(10500, 0, B * m * n).reshape(B, n, m)
    rx = synth.normal_stream(10500, 1, B * m).reshape(B, m)
    At = synth.normal_stream(10500, 2, B * t * n).reshape(B, t, n)
    cx = synth.normal_stream(10500, 3, B * t).reshape(B, t)
    from enlsip_gn import GNSolver
    pv = GNSolver.pack_subspace_prev(B, [2 - (k % 2) for k in range(B)], [6 - (k % 4) for k in range(B)],
                                     [int(k % 9 == 0) for k in range(B)], [(0.05, 0.5, 1.0)[k % 3] for k in range(B)],
                                     [0.21 * float(cx[k] @ cx[k]) for k in range(B)], [0.1 * float(rx[k] @ rx[k]) for k in range(B)])
    s = rb.make_solver(monkeypatch, ENLSIP_GN_PIPELINE="1")
    try:
        s.solve_batched(J, rx, At, cx)
        split = s.pipeline_split()
        assert 60 < split < 70
        whole, rc = s.subspace_direction_batched(m, n, t, pv, 0, B)
        assert rc == 0 and len({tuple(x) for x in whole["info"][:, 3:5]}) >= 2
        part, rc = s.subspace_direction_batched(m, n, t, pv[60:70], 60, 10)
        assert rc == 0
        for key in ("p", "b", "d", "info", "status"):
            assert np.array_equal(part[key], whole[key][60:70]), key
    finally:
        s.close()


def growth_case(name):
    """a resident batch, its previous iterates and the small range of the first call, which the whole-batch call outgrows"""
    from enlsip_gn import GNSolver
    if name == "halves":      # the batch of test_range_over_the_pipelined_halves: both half handles grow their own scratch
        B, m, n, t = 130, 64, 8, 2
        J = synth.normal_stream(10500, 0, B * m * n).reshape(B, n, m)
        rx = synth.normal_stream(10500, 1, B * m).reshape(B, m)
        At = synth.normal_stream(10500, 2, B * t * n).reshape(B, t, n)
        cx = synth.normal_stream(10500, 3, B * t).reshape(B, t)
        pv = GNSolver.pack_subspace_prev(B, [2 - (k % 2) for k in range(B)], [6 - (k % 4) for k in range(B)],
                                         [int(k % 9 == 0) for k in range(B)], [(0.05, 0.5, 1.0)[k % 3] for k in range(B)],
                                         [0.21 * float(cx[k] @ cx[k]) for k in range(B)], [0.1 * float(rx[k] @ rx[k]) for k in range(B)])
        return (B, m, n, t), lambda s: s.solve_batched(J, rx, At, cx), pv, {"ENLSIP_GN_PIPELINE": "1"}
    B, m, n, t = {"wave": (6, 64, 8, 3), "general": (6, 300, 80, 12)}[name]
    probs = rb.make_batch(11000, B, m, n, t)
    refs = [go.gn_subproblem(*p) for p in probs]
    pv = pack_prev([prev_record(probs[k], t, rb.fabricated_previous(k, probs[k], refs[k], t), False) for k in range(B)])
    return (B, m, n, t), lambda s: rb.solve(s, probs, t, False), pv, {}


@pytest.mark.parametrize("name", ["wave", "general", "halves"])
def test_scratch_growth_changes_no_result(name, monkeypatch):
    """the per-call scratch (requests on the device, their pinned copy, the staging of the host-buffer form) grows between a call
    over two problems and one over the whole batch on the SAME solver: the second call answers bit for bit as on a solver that
    never made the first.  halves: the first range is the last problem of one pipelined half and the first of the other."""
    (B, m, n, t), solve, pv, env = growth_case(name)
    grown, fresh = rb.make_solver(monkeypatch, **env), rb.make_solver(monkeypatch, **env)
    try:
        solve(grown)
        solve(fresh)
        first = grown.pipeline_split() - 1 if name == "halves" else 0
        assert first >= 0 and grown.pipeline_split() == fresh.pipeline_split()
        _, rc = grown.subspace_direction_batched(m, n, t, pv[first:first + 2], first, 2)
        assert rc in (0, 1)
        got, rc_got = grown.subspace_direction_batched(m, n, t, pv, 0, B)
        want, rc_want = fresh.subspace_direction_batched(m, n, t, pv, 0, B)
        assert grown.subspace_form() == fresh.subspace_form() == (0 if name == "general" else 1)
        print(f"{name}: rc {rc_got} / {rc_want}, statuses {sorted(set(int(x) for x in want['status']))}")
        assert rc_got == rc_want == 0 and np.all(want["status"] == 0)      # every slot was answered in full
        for key in ("p", "b", "d", "info", "status"):
            assert got[key].tobytes() == want[key].tobytes(), key
    finally:
        grown.close()
        fresh.close()


def test_statuses_and_refusals(monkeypatch):
    B, m, n, t = 6, 300, 24, 5
    probs = rb.make_batch(10600, B, m, n, t)
    refs = [go.gn_subproblem(*p) for p in probs]
    its = [rb.fabricated_previous(k, probs[k], refs[k], t) for k in range(B)]
    recs = [list(prev_record(probs[k], t, its[k], False)) for k in range(B)]
    recs[1][1] = refs[1].rankJ2 + 2                                   # tau / rho past rankJ2 without a restart: 5
    recs[4][0], recs[4][3] = t + 4, 1.0                               # b[1:previous_dimA] past t: 5
    pv = pack_prev([tuple(r) for r in recs])
    take = np.array([1, 1, 0, 1, 1, 1], dtype=np.int64)
    s = rb.make_solver(monkeypatch)
    lib, h = s._lib, s._h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda p0, cnt, prev=pv: lib.enlsip_gn_subspace_direction_batched(h, p0, cnt, None, vp(prev) if prev is not None else None,
                                                                             None, None, None, None, None)
    try:
        assert call(0, 1) == -1                                          # before any solve
        s.factor_constraints(m, probs[0][2], probs[0][3])
        assert call(0, 1) == -1                                          # only F_A / F_L11 are resident
        sol = rb.solve(s, probs, t, False)
        assert call(0, 0) == -2 and call(B, 1) == -3 and call(B - 1, 2) == -3 and call(0, 1, None) == -4
        hold = np.full(B, HOLD, dtype=np.int64)
        rA = np.array([r.rankA for r in refs], dtype=np.int64)
        _, rc = s.resolve_batched(m, n, t, rA, hold, -1, 0, B)            # every problem holds a result
        assert rc == 0
        out, rc = s.subspace_direction_batched(m, n, t, pv, 0, B, take=take)
        assert rc == 1 and list(out["status"]) == [0, 5, -1, 0, 5, 0], out["status"]
        for k in (1, 2, 4):                                              # nothing written
            assert all(np.all(np.isnan(out[key][k])) for key in ("p", "b", "d")) and np.all(out["info"][k] == -1)
        for k in (0, 3, 5):
            want = stable_reference_choice(k, probs[k], refs[k], t, its[k], False)
            assert tuple(out["info"][k, 3:5]) == want
        # state records: the untaken problem and the two found out of bounds before any launch still hold their result and
        # answer as the solve left them; the taken ones dropped theirs
        dJ = np.array([r.rankJ2 for r in refs], dtype=np.int64)
        o, rc = s.resolve_batched(m, n, t, hold, dJ, -1, 0, B)
        assert list(o["status"]) == [3, 0, 0, 3, 0, 3], o["status"]
        for k in (1, 2, 4):
            assert tuple(o["info"][k]) == (refs[k].rankA, refs[k].rankJ2, -1, refs[k].rankA, refs[k].rankJ2, 0)
            p_ref, _, _ = rb.oracle_resolve(probs[k], refs[k], refs[k].rankA, refs[k].rankJ2, -1)
            assert rel(o["p"][k], p_ref) <= 1e-11
    finally:
        s.close()


def test_final_dimension_out_of_range(monkeypatch):
    """status 2: previous_dimJ2 above min(m, n - rankA) after a step of 1.  Where rankJ2 > 0 such a previous dimension lies beyond
    rankJ2 and the reference is out of bounds first (status 5, above); with n - rankA = 0 nothing is indexed (:1058) and the max of
    :1173 carries the previous dimension out of range: b and d are written, p is not."""
    B, m, n, t = 2, 50, 4, 4
    probs = rb.make_batch(10650, B, m, n, t)
    refs = [go.gn_subproblem(*p) for p in probs]
    assert all(r.rankA == n and r.rankJ2 == 0 for r in refs)
    its = [eo.Iteration(**{**rb.fabricated_previous(k, probs[k], refs[k], t).__dict__, "alpha": 1.0, "dimJ2": k}) for k in range(B)]
    want = [stable_reference_choice(k, probs[k], refs[k], t, its[k], False) for k in range(B)]
    assert [w[1] for w in want] == [0, 1]
    recs = [prev_record(probs[k], t, its[k], False) for k in range(B)]
    s = rb.make_solver(monkeypatch)
    try:
        rb.solve(s, probs, t, False)
        out, rc = s.subspace_direction_batched(m, n, t, pack_prev(recs), 0, B)
        assert rc == 1 and list(out["status"]) == [0, 2], out["status"]
        assert np.all(np.isnan(out["p"][1]))
        for k in range(B):
            assert tuple(out["info"][k, 3:5]) == want[k], (k, out["info"][k], want[k])
            p_ref, b_ref, d_ref = rb.oracle_resolve(probs[k], refs[k], want[k][0], 0, -1)
            assert rel(out["b"][k], b_ref) <= 1e-12 and rel(out["d"][k], d_ref) <= 1e-12
        assert rel(out["p"][0], rb.oracle_resolve(probs[0], refs[0], want[0][0], 0, -1)[0]) <= 1e-11
    finally:
        s.close()


def test_rescued_member(monkeypatch):
    """a member scaled by 2^600 lives on a rescue handle: it is answered through the per-problem re-solve with the dimensions chosen
    by the host instantiation of the routine — the reference's on the unscaled problem (the choice does not depend on the scale)"""
    B, m, n, t = 3, 300, 24, 5
    probs = rb.make_batch(10700, B, m, n, t)
    refs = [go.gn_subproblem(*p) for p in probs]
    z = np.zeros(0)
    its = [rb.fabricated_previous(k, probs[k], refs[k], t) for k in range(B)]
    its[1] = eo.Iteration(**{**its[1].__dict__, "alpha": 0.5, "dimJ2": refs[1].rankJ2 - 3})      # no progress test after a long step
    want = [stable_reference_choice(k, probs[k], refs[k], t, its[k], False) for k in range(B)]
    recs = [prev_record(probs[k], t, its[k], False) for k in range(B)]
    J = np.stack([np.ascontiguousarray(p[0].T) for p in probs])
    rx = np.stack([p[1] for p in probs])
    At = np.stack([np.ascontiguousarray(p[2]) for p in probs])
    cx = np.stack([p[3] for p in probs])
    J[1] *= 2.0 ** 600
    rx[1] *= 2.0 ** 600
    s = rb.make_solver(monkeypatch)
    try:
        s.solve_batched(J, rx, At, cx)
        assert "rescaled" in s.route()
        out, rc = s.subspace_direction_batched(m, n, t, pack_prev(recs), 0, B)
        assert rc == 0 and np.all(out["status"] == 0)
        for k in range(B):
            assert tuple(out["info"][k, 3:5]) == want[k], (k, out["info"][k], want[k])
        p_ref, _, _ = rb.oracle_resolve(probs[1], refs[1], want[1][0], want[1][1], -1)
        assert rel(out["p"][1], p_ref) <= 1e-11
    finally:
        s.close()


def test_out_of_bounds_found_on_the_device(monkeypatch):
    """previous_dimR == rankR + 1 after a step below 0.2 is the one case the host cannot decide before the launches: with the
    bad-step test (:879-881) false the reference reads rho[rankR + 1] (the oracle raises IndexError), with it true it returns rankR.
    Problem 1 has that for dimJ2 (found by k_subspace_dimj2, after b, p1 and the state record were set for the chosen dimA: its
    held result is dropped), problem 2 — a rank-deficient A, so that rankA + 1 <= t — for dimA (found by k_subspace_head before
    anything is written: every later launch skips it and its held result stays), problem 4 the bad-step case, which is answered."""
    B, m, n, t = 6, 300, 24, 5
    probs = rb.make_batch(10800, B, m, n, t, deficient=(2,))
    refs = [go.gn_subproblem(*p) for p in probs]
    assert refs[2].rankA == t - 1 and all(r.rankA == t for k, r in enumerate(refs) if k != 2)
    its = [rb.fabricated_previous(k, probs[k], refs[k], t) for k in range(B)]
    recs = [list(prev_record(probs[k], t, its[k], False)) for k in range(B)]
    rx2 = [float(p[1] @ p[1]) for p in probs]
    recs[1][1], recs[1][3], recs[1][5] = refs[1].rankJ2 + 1, 0.05, 10.0 * rx2[1]
    recs[2][0], recs[2][3], recs[2][4] = refs[2].rankA + 1, 0.05, 10.0 * float(probs[2][3] @ probs[2][3])
    recs[4][1], recs[4][3], recs[4][5] = refs[4].rankJ2 + 1, 0.05, -1.0
    z = np.zeros(0)

    def iteration(k):      # the previous iterate that gives recs[k]
        pa, pj, _, alpha, cprog, rprog = recs[k]
        J, rx, A, cx = probs[k]
        return eo.Iteration(**{**its[k].__dict__, "dimA": pa, "dimJ2": pj, "alpha": alpha,
                               "cx": cx * np.sqrt(1.0 + cprog / float(cx @ cx)), "rx": rx * np.sqrt(1.0 + rprog / float(rx @ rx))})
    for k in (1, 2):
        with pytest.raises(IndexError):
            reference_choice(probs[k], refs[k], t, iteration(k), False)
    want = {k: stable_reference_choice(k, probs[k], refs[k], t, iteration(k), False) for k in (0, 3, 4, 5)}
    assert want[4][1] == refs[4].rankJ2
    pv = pack_prev([tuple(r) for r in recs])
    s = rb.make_solver(monkeypatch)
    try:
        rb.solve(s, probs, t, False)
        hold = np.full(B, HOLD, dtype=np.int64)
        rA = np.array([r.rankA for r in refs], dtype=np.int64)
        dJ = np.array([r.rankJ2 for r in refs], dtype=np.int64)
        _, rc = s.resolve_batched(m, n, t, rA, hold, -1, 0, B)            # every problem holds a result
        assert rc == 0
        out, rc = s.subspace_direction_batched(m, n, t, pv, 0, B)
        assert rc == 1 and list(out["status"]) == [0, 5, 5, 0, 0, 0], out["status"]
        for k in (1, 2):                                                  # nothing written to the caller's slots
            assert all(np.all(np.isnan(out[key][k])) for key in ("p", "b", "d")) and np.all(out["info"][k] == -1)
        for k, w in want.items():                                         # the neighbours are answered as ever
            assert tuple(out["info"][k]) == (refs[k].rankA, refs[k].rankJ2, -1, w[0], w[1], 0), (k, out["info"][k], w)
            p_ref, b_ref, _ = rb.oracle_resolve(probs[k], refs[k], w[0], w[1], -1)
            assert rel(out["p"][k], p_ref) <= 1e-11 and rel(out["b"][k], b_ref) <= 1e-12
        # problem 2 was skipped by every launch: it still holds its result and answers from it; problem 1 (and the answered ones)
        # dropped theirs
        o, rc = s.resolve_batched(m, n, t, hold, dJ, -1, 0, B)
        assert rc == 1 and list(o["status"]) == [3, 3, 0, 3, 3, 3], o["status"]
        assert tuple(o["info"][2]) == (refs[2].rankA, refs[2].rankJ2, -1, refs[2].rankA, refs[2].rankJ2, 0)
        p_ref, _, _ = rb.oracle_resolve(probs[2], refs[2], refs[2].rankA, refs[2].rankJ2, -1)
        assert rel(o["p"][2], p_ref) <= 1e-9          # rank-deficient A: the bound of test_gpu_resolve_batched.check_against_oracle
        # the resident b, p1 and state record of problem 1 are those of a re-solve with the dimA its choice made: a call with a
        # previous iterate the reference accepts answers it from there, bitwise as on a handle that never saw the refused call
        recs[1] = list(prev_record(probs[1], t, its[1], False))
        w1 = stable_reference_choice(1, probs[1], refs[1], t, its[1], False)
        again, rc = s.subspace_direction_batched(m, n, t, pack_prev([tuple(recs[1])]), 1, 1)
        assert rc == 0 and tuple(again["info"][0, 3:5]) == w1
        s2 = rb.make_solver(monkeypatch)
        try:
            rb.solve(s2, probs, t, False)
            fresh, rc = s2.subspace_direction_batched(m, n, t, pack_prev([tuple(recs[1])]), 1, 1)
            assert rc == 0 and all(np.array_equal(again[key], fresh[key]) for key in ("p", "b", "d", "info", "status"))
        finally:
            s2.close()
    finally:
        s.close()


def test_many_constraints_general_form(monkeypatch):
    """t_max = 760 with n = 900: the head's LDS (b, the triangular block, tau, rho, the diagonal) is 8 (2 * 904 + 4160 + 8 +
    3 * 760) = 66.0 KB, beyond the 64 KB a kernel gets without the opt-in.  Bound on p: 1e-11 as elsewhere — eps (1.1e-16) times
    cond(R_A) (about 24 for a 760 x 900 Gaussian A), cond(J2) (about 5 for 300 x 140) and sqrt(n) = 30 is 4e-13, well below it."""
    B, m, n, t = 1, 300, 900, 760
    probs = rb.make_batch(10900, B, m, n, t)
    refs = [go.gn_subproblem(*p) for p in probs]
    its = [rb.fabricated_previous(k, probs[k], refs[k], t) for k in range(B)]
    want = [stable_reference_choice(k, probs[k], refs[k], t, its[k], False) for k in range(B)]
    recs = [prev_record(probs[k], t, its[k], False) for k in range(B)]
    s = rb.make_solver(monkeypatch)
    try:
        rb.solve(s, probs, t, False)
        out, rc = s.subspace_direction_batched(m, n, t, pack_prev(recs), 0, B)
        assert rc == 0 and np.all(out["status"] == 0) and s.subspace_form() == 0
        for k in range(B):
            assert tuple(out["info"][k, 3:5]) == want[k], (k, out["info"][k], want[k])
            p_ref, b_ref, _ = rb.oracle_resolve(probs[k], refs[k], want[k][0], want[k][1], -1)
            print(f"problem {k}: rel p {rel(out['p'][k], p_ref):.2e}  rel b {rel(out['b'][k], b_ref):.2e}")
            assert rel(out["p"][k], p_ref) <= 1e-11 and rel(out["b"][k], b_ref) <= 1e-12
        old, rc = s.resolve_batched(m, n, t, out["info"][:, 3].copy(), out["info"][:, 4].copy(), -1, 0, B)
        assert rc == 0 and all(np.array_equal(out[key], old[key]) for key in ("p", "b", "d", "info"))
    finally:
        s.close()
