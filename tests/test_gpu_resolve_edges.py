"""The batched re-solve family at the edges no other test reaches (the case grid and its branch list: tests/resolve_edges.py; what
the CPU knows about the reference before the GPU is consulted: tests/test_resolve_edges_host.py).

Every request of every case is compared with oracle.gn_oracle.sub_search_direction on the oracle's factors through
check_against_oracle of tests/test_gpu_resolve_batched.py, at that file's tolerances (rel p 1e-11, or 1e-9 where A is rank deficient;
rel b 1e-12; ||d|| 1e-12; |d[:dimJ2]| 1e-10), and with the per-problem entry point at its 1e-13.  Set-up and oracle helpers are those
of tests/test_gpu_resolve_batched.py; the growth shapes are those of tests/test_gpu_subspace_batched.py."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import synth

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dispatch_grid  # noqa: E402
import resolve_edges as edges  # noqa: E402
from test_gpu_resolve_batched import HOLD, SENT, check_against_oracle, make_batch, make_solver, rel, solve  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in edges.grid()}
# a case as it stands, and once more with panel pairs forced for its batches whose plan has three panels or more
VARIANTS = [(c.name, False) for c in CASES.values()] + [(c.name, True) for c in CASES.values() if any(b.pair_variant for b in c.batches)]
IDS = [nm + ("-pairs" if pairs else "") for nm, pairs in VARIANTS]

# route names a ragged batch must report (a uniform one: dispatch_grid.expected_route): the narrow last panel only d rode through
RAGGED_ROUTES = {"code1_blocks": ("sweep_passenger",), "codem1_blocks": ("sweep_passenger",), "mixed_kp": ("sweep_passenger",)}


def batches_of(name, pairs):
    return [b for b in CASES[name].batches if b.pair_variant or not pairs]


def resident(b, pairs, monkeypatch):
    """a solver with batch b resident: (solver, probs, refs, sol); the problems are make_batch's (synth.make_problem(seed + k))"""
    probs, refs = edges.problems(b)
    again = make_batch(b.seed, b.B, b.m, b.n, b.t, list(b.ts))
    assert all(np.array_equal(x, y) for p, q in zip(probs, again) for x, y in zip(p, q))
    s = make_solver(monkeypatch, **({"ENLSIP_GN_PAIR": "1"} if pairs else {}))
    try:
        sol = solve(s, probs, b.t, b.ragged)
        route = {r.lower() for r in s.route()}
        print(f"{b.name}{' (pairs)' if pairs else ''}: route {sorted(route)}")
        if pairs:
            want = {"sweep_pairs"}
        elif b.ragged:
            want = set(RAGGED_ROUTES[b.name])
        else:
            want = dispatch_grid.expected_route(b.B, b.m, b.n, b.t)
        assert want <= route, (b.name, sorted(want - route))
        assert s.plan_uses_pairs() == pairs
        for k, ref in enumerate(refs):
            assert sol[3][k][0] == ref.rankA and sol[3][k][1] == ref.rankJ2, (b.name, k)
    except BaseException:
        s.close()
        raise
    return s, probs, refs, sol


def arrays(rnd):
    return tuple(np.array(x, dtype=np.int64) for x in zip(*rnd))


@pytest.mark.parametrize("name,pairs", VARIANTS, ids=IDS)
def test_edge_case_against_oracle(name, pairs, monkeypatch):
    failures = []
    for b in batches_of(name, pairs):
        s, probs, refs, _ = resident(b, pairs, monkeypatch)
        try:
            for r, rnd in enumerate(b.rounds):
                dA, dJ, cd = arrays(rnd)
                out, rc = s.resolve_batched(b.m, b.n, b.t, dA, dJ, cd, 0, b.B)
                assert rc == 0 and s.resolve_form() == (1 if b.small else 0)
                for k, req in enumerate(rnd):          # slot by slot, so that every slot that is wrong is named
                    try:
                        check_against_oracle(probs, refs, list(b.ts), [req], {key: v[k:k + 1] for key, v in out.items()}, b.t, k)
                    except AssertionError as e:
                        failures.append((b.name, f"round {r}", f"slot {k}", f"t_k {b.ts[k]}", req, "oracle", str(e).splitlines()[0]))
                    if req[2] == 0:
                        continue
                    p, bb, d = s.resolve(b.m, b.n, b.t, *req, k)          # the per-problem entry point
                    errs = (rel(out["p"][k], p), rel(out["b"][k], bb), rel(np.abs(out["d"][k]), np.abs(d)))
                    if not all(e <= 1e-13 for e in errs):
                        failures.append((b.name, f"round {r}", f"slot {k}", f"t_k {b.ts[k]}", req, "per-problem", errs))
        finally:
            s.close()
    assert not failures, "\n".join(str(f) for f in failures)


@pytest.mark.parametrize("name,pairs", VARIANTS, ids=IDS)
def test_full_dims_reproduce_the_solve(name, pairs, monkeypatch):
    """dimA = rankA, dimJ2 = rankJ2 and the solve's own code: the p of the solve that made the factors (no oracle involved)"""
    for b in batches_of(name, pairs):
        s, probs, refs, sol = resident(b, pairs, monkeypatch)
        try:
            infos = sol[3]
            rA, rJ, cd = (np.array([i[c] for i in infos], dtype=np.int64) for c in (0, 1, 2))
            assert all(c == (1 if r.rankA == tk else -1) for c, r, tk in zip(cd, refs, b.ts))
            out, rc = s.resolve_batched(b.m, b.n, b.t, rA, rJ, cd, 0, b.B)
            assert rc == 0 and np.all(out["status"] == 0)
            for k in range(b.B):
                e = rel(out["p"][k], sol[0][k])
                print(f"{b.name} problem {k}: {e:.2e}")
                assert e <= 1e-13, (b.name, k, e)
        finally:
            s.close()


def test_held_flow_at_the_block_edges(monkeypatch):
    """b, then d for dimA, then p for dimJ2 in three calls: bit for bit the one-call result (code1_blocks and codem1_blocks share their
    resident batch)"""
    b1, bm = CASES["code1_blocks"].batches[0], CASES["codem1_blocks"].batches[0]
    assert (b1.ts, b1.seed, b1.m, b1.n) == (bm.ts, bm.seed, bm.m, bm.n)
    s, probs, refs, _ = resident(b1, False, monkeypatch)
    same = lambda x, y: x.tobytes() == y.tobytes()
    try:
        rA = np.array([r.rankA for r in refs], dtype=np.int64)
        hold = np.full(b1.B, HOLD, dtype=np.int64)
        for rnd in b1.rounds + bm.rounds:
            dA, dJ, cd = arrays(rnd)
            m, n, t, B = b1.m, b1.n, b1.t, b1.B
            one, rc = s.resolve_batched(m, n, t, dA, dJ, cd, 0, B)
            assert rc == 0
            first, rc = s.resolve_batched(m, n, t, rA, hold, cd, 0, B)
            assert rc == 0 and np.all(np.isnan(first["p"]))
            second, rc = s.resolve_batched(m, n, t, dA, hold, cd, 0, B)
            assert rc == 0 and np.all(np.isnan(second["p"]))
            third, rc = s.resolve_batched(m, n, t, hold, dJ, cd, 0, B)
            assert rc == 0
            assert same(second["b"], one["b"]) and same(second["d"], one["d"]), rnd
            for key in ("p", "b", "d", "info", "status"):
                assert same(third[key], one[key]), (key, rnd)
    finally:
        s.close()


# ---- the five families interleaved on one handle, each growing its own scratch -------------------------------------------------
G = 2       # guard rows around every host output


def guarded(count, width, dtype=np.float64):
    if dtype == np.float64:
        full = np.full((count + 2 * G, width), SENT, dtype=np.int64).view(np.float64)
    else:
        full = np.full((count + 2 * G, width) if width else (count + 2 * G,), -77, dtype=dtype)
    return full, full[G:G + count]


def family_sequence(s, shape, sol, pv, Gam, small, whole):
    """Every family on solver s, first over a small range and then over the whole one, interleaved: re-solve (small), Newton
    direction, multipliers, deletion and restore, subspace call, re-solve (whole).  small = (prob0, slots of the re-solve / Newton /
    subspace calls, slots of the multiplier calls, problems of the small deletion batch).  Every call must answer every slot in
    full (rc 0, status 0).  Returns every output with its guard rows, and the guarded ones again."""
    import torch
    import test_gpu_delete_constraints_batched as dl
    B, m, n, t = shape
    infos = sol[3]
    got, guards = [], []

    def outs(count):
        full, view = {}, {}
        for key, width, dt in (("p", n, np.float64), ("b", t, np.float64), ("d", m, np.float64), ("info", 6, np.int64), ("status", 0, np.int32)):
            full[key], view[key] = guarded(count, width, dt)
        guards.extend(full.values())
        return full, view

    def resolve(p0, cnt):
        dA = np.array([infos[p0 + j][0] for j in range(cnt)], dtype=np.int64)
        dJ = np.array([max(infos[p0 + j][1] - (j % 2), 0) for j in range(cnt)], dtype=np.int64)
        full, view = outs(cnt)
        _, rc = s.resolve_batched(m, n, t, dA, dJ, -1, p0, cnt, out=view)
        assert rc == 0 and np.all(view["status"] == 0), ("resolve", p0, cnt, rc, view["status"])
        got.extend(full.values())

    def subspace(p0, cnt):
        full, view = outs(cnt)
        _, rc = s.subspace_direction_batched(m, n, t, pv[p0:p0 + cnt], p0, cnt, out=view)
        assert rc == 0 and np.all(view["status"] == 0), ("subspace", p0, cnt, rc, view["status"])
        got.extend(full.values())

    def newton(p0, cnt):
        pf, pview = guarded(cnt, n)
        sf, sview = guarded(cnt, 0, np.int32)
        guards.extend([pf, sf])
        _, _, rc = s.newton_direction_batched(Gam[p0:p0 + cnt], p0, cnt, out_p=pview, out_status=sview)
        assert rc == 0 and np.all(sview == 0) and np.all(np.isfinite(pview)), ("newton", p0, cnt, rc, sview)      # the Newton branch ran
        got.extend([pf, sf])

    def multipliers(p0, cnt):
        lam, gres, st, rc = s.first_lagrange_batched(t, p0, cnt)
        assert rc == 0 and np.all(st == 0), ("first_lagrange", p0, cnt, rc, st)
        got.extend([lam, gres, st])
        lam, st, rc = s.second_lagrange_batched(t, np.ascontiguousarray(sol[0][p0:p0 + cnt]), p0)
        assert rc == 0 and np.all(st == 0), ("second_lagrange", p0, cnt, rc, st)
        got.extend([lam, st])

    def deletion(batch):          # device buffers of its own: any batch size, whatever is resident
        tt, q = dl.batch_t_q(t, seed=17 * n + batch, batch=batch)
        buf = dl.Buffers(n, t, tt, True, seed=batch)
        buf.upload()
        sd = s.delete_constraints_batched_dev(batch, n, t, tt, q, True, buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(),
                                              dgrad_res=buf.ptr("gres"), dsaved=buf.ptr("saved"))
        after = buf.download()
        s.restore_constraints_batched_dev(batch, n, t, tt - (sd != 0), sd, buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(), buf.ptr("saved"))
        back = buf.download()
        for nm in ("At", "cx", "lam", "ds"):          # the restore is the exact inverse
            assert back[nm].tobytes() == getattr(buf, nm).tobytes(), nm
        got.extend([sd] + list(after.values()) + list(back.values()))

    p0s, c2, c3, cdel = small
    resolve(p0s, c2)
    newton(p0s, c2)
    newton(*whole)
    multipliers(p0s, c3)
    multipliers(*whole)
    deletion(cdel)
    deletion(B)
    subspace(p0s, c2)
    subspace(*whole)
    resolve(*whole)
    torch.cuda.synchronize()
    return got, guards


@pytest.mark.parametrize("name", ["wave", "general", "halves"])
def test_interleaved_families_match_a_pregrown_handle(name, monkeypatch):
    """The re-solve, the Newton direction, the multipliers and the subspace call keep a per-call scratch EACH (rsb_dims / rsb_io,
    nwb_ws / nwb_io, lagb_scr / lagb_io, ssb_req / ssb_io, with their pinned copies): no buffer is shared between two of these
    families, what they share is the code that grows and stages them.  The deletion step places its records in rec_scr / h_rec, the
    one record scratch of the calls on the caller's buffers, which none of the other four touches
    (tests/test_gpu_record_scratch.py runs the calls that do share it).  On X every family is called over a small
    range and then over the whole one, with the other families' calls in between, so each family's own scratch grows between its two
    calls; on Y one whole-range call of every family came first, so nothing grows later.  Every output of the same sequence is bit
    for bit the same on both, every slot is answered in full, and the guard rows around the host outputs keep their fill.
    halves: the small ranges straddle the pipelined split, so both half handles grow."""
    import test_gpu_subspace_batched as sb
    shape, solve_fn, pv, env = sb.growth_case(name)
    B, m, n, t = shape
    Gam = synth.normal_stream(12900, 0, B * n * n).reshape(B, n, n)
    Gam = 0.5 * (Gam + Gam.transpose(0, 2, 1)) * 1e-3
    X, Y = make_solver(monkeypatch, **env), make_solver(monkeypatch, **env)
    try:
        sol = solve_fn(X)
        solve_fn(Y)
        split = X.pipeline_split()
        assert split == Y.pipeline_split() and ((0 < split < B) if name == "halves" else split in (0, B))
        small = (split - 1 if name == "halves" else 0, 2, 3, 3)
        whole = (0, B)
        # Y: every family over the whole range first, then the solve again
        family_sequence(Y, shape, sol, pv, Gam, (0, B, B, B), whole)
        sol_y = solve_fn(Y)
        assert all(np.array_equal(a, b) for a, b in zip(sol[:3], sol_y[:3]))
        want, _ = family_sequence(Y, shape, sol_y, pv, Gam, small, whole)
        got, guards = family_sequence(X, shape, sol, pv, Gam, small, whole)
        assert X.resolve_form() == Y.resolve_form() == X.subspace_form() == X.newton_form() == (0 if name == "general" else 1)
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), i
        for a in guards:          # no output slot outside a call's range changed
            fill = SENT if a.dtype == np.float64 else -77
            v = a.view(np.int64) if a.dtype == np.float64 else a
            assert np.all(v[:G] == fill) and np.all(v[-G:] == fill)
    finally:
        X.close()
        Y.close()
