"""The CAQR pair sweep at its column-window, tile and schedule edges (tests/sweep_edge_cases.py: the table and the restated sweep;
tests/test_sweep_edge_cases_host.py: its CPU certification).  One test id per case of the table.  Each case creates its handle
under the case's environment, solves twice on it (events, the second stream and the plan are reused) and then

* holds the reported route against the trace: sweep_pairs, sweep_plain / sweep_passenger, sweep_tree, sweep_lookahead and sweep_xmap
  are reported exactly when the trace says so;
* checks the defining identities of EVERY problem of the batch (tests/factor_identities.py) over every column of F_J2 and d over its
  full length, under that module's TOL_COL, TOL_GRAM and TOL_D;
* compares rankA, rankJ2, jpvtJ2 with the oracle's, p to 1e-11 and ||d|| to 1e-12 relative (the bounds of
  test_lookahead_sweep_matches_the_one_stream_sweep);
* where only the schedule differs, compares bit for bit: family D against the same sweep with ENLSIP_GN_LOOKAHEAD=0, family E every
  problem of the mixed batch against the same problem alone on a handle of the same environment, family C (a test of its own)
  problem k of a batch of 9 (remap off) against batches of 1, 2 and 8 (remap on).

Family E, routes: the route of a batch is the union over its problems and is decided by the launch shape (t_max for the constraint
stage, the widest J2 for the sweep), so a problem alone reports other constraint_* / sweep_* / pivot_* bits than the mixed batch it
came from (a narrow one has no pair at all, the widest one meets the uniform kernels of its own t).  The bits are compared only when
the routes agree, as the rule says; the differing bits are printed, and the identities and the oracle comparison hold either way.

Guard rows: GNSolver.solve, solve_batched and solve_batched_ragged allocate their outputs themselves, exactly sized; the Python
layer offers no way to hand them a buffer with guard rows, so none are placed here (tests/test_gpu_record_scratch.py guards the
caller's-buffer calls).  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

import factor_identities as fi
import sweep_edge_cases as se
from oracle import gn_oracle as go

CASES = se.cases()
SWEEP_BITS = {"sweep_plain", "sweep_pairs", "sweep_passenger", "sweep_tree", "sweep_lookahead", "sweep_xmap"}


class _Out:
    def __init__(self, p, d, rankA, rankJ2, jpvtJ2):
        self.p, self.d, self.rankA, self.rankJ2, self.jpvtJ2 = p, d, rankA, rankJ2, jpvtJ2


@functools.lru_cache(maxsize=None)
def _problem(seed: int, m: int, n: int, t: int):
    """(problem, oracle solution), once per distinct problem of the file (cases of one shape share their problems)."""
    from oracle import synth
    P = synth.make_problem(seed, m, n, t)
    return P, go.gn_subproblem(*P)


def _problems(c, batch=None):
    return [_problem(se.problem_seed(c, k), c["m"], c["n"], c["t_list"][k] if c["t_list"] else c["t"])
            for k in range(c["batch"] if batch is None else batch)]


def _handle(c, **env):
    from enlsip_gn import GNSolver
    with fi.handle_env(dict(c["env"], **env)):
        return GNSolver(device=0, tile_rows=c["tile_rows"])


def _solve(s, c, probs, single_call=True):
    """One solve of the problems on handle s: a list of _Out.  single_call: a batch of one goes through enlsip_gn_solve."""
    n = c["n"]
    if len(probs) == 1 and single_call:
        o = s.solve(*probs[0][0])
        return [_Out(o.p, o.d, o.rankA, o.rankJ2, o.jpvtJ2)]
    Jb = np.stack([np.ascontiguousarray(P[0].T) for P, _ in probs])
    rxb = np.stack([P[1] for P, _ in probs])
    if c["t_list"]:
        from enlsip_gn import GNSolver
        At, cxb, tk = GNSolver.pack_ragged([P[2] for P, _ in probs], [P[3] for P, _ in probs], n=n)
        p, b, d, infos, jA, jL, jJ = s.solve_batched_ragged(Jb, rxb, At, cxb, tk)
    else:
        p, b, d, infos, jA, jL, jJ = s.solve_batched(Jb, rxb, np.stack([np.ascontiguousarray(P[2]) for P, _ in probs]),
                                                     np.stack([P[3] for P, _ in probs]))
    return [_Out(p[k], d[k], infos[k][0], infos[k][1], jJ[k][:n - infos[k][0]].copy()) for k in range(len(probs))]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _against_oracle(tag, out, ref):
    ep, ed = _rel(out.p, ref.p), abs(np.linalg.norm(out.d) - np.linalg.norm(ref.d)) / np.linalg.norm(ref.d)
    print(f"oracle {tag}: p {ep:.1e} ||d|| {ed:.1e} ranks {(out.rankA, out.rankJ2)}")
    assert (out.rankA, out.rankJ2) == (ref.rankA, ref.rankJ2), tag
    assert np.array_equal(out.jpvtJ2, ref.jpvtJ2), (tag, "pivots of F_J2 differ from the oracle's")
    assert ep <= 1e-11 and ed <= 1e-12, (tag, ep, ed)


def _resident(s, outs):
    """What a schedule must not change: R of F_J2, its pivots, d and p of every problem."""
    return [(np.array(s.factor(fi.FACTOR_J2, k).R), np.array(o.jpvtJ2), np.array(o.d), np.array(o.p)) for k, o in enumerate(outs)]


def _same_bits(tag, a, b):
    for name, x, y in zip(("R", "jpvtJ2", "d", "p"), a, b):
        assert x.shape == y.shape and np.array_equal(x, y), (tag, name, "differs by", float(np.abs(x - y).max()))


def _check_route(c, got):
    want, never = se.expected_sweep_route(se.trace_of(c), c["env"])
    print(f"route {c['id']}: {sorted(got & SWEEP_BITS)}")
    assert want <= got, (c["id"], "missing", sorted(want - got))
    assert not (never & got), (c["id"], "unexpected", sorted(never & got))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_sweep_edge_case(c):
    probs = _problems(c)
    s = _handle(c)
    try:
        for _ in range(2):
            outs = _solve(s, c, probs)
        got = s.route()
        _check_route(c, got)
        for k, ((J, rx, A, cx), ref) in enumerate(probs):
            res = fi.check_solve_identities(fi.SolverAccess(s, c["m"], c["n"], k), J, rx, A, cx, outs[k],
                                            cols_J2=np.arange(c["n"] - outs[k].rankA))
            print(f"identities {c['id']} prob {k}: " + " ".join(f"{key}={v:.1e}" for key, v in sorted(res.items())))
            fi.assert_within(res, "full", (c["id"], k))
            _against_oracle((c["id"], k), outs[k], ref)
        mine = _resident(s, outs)
    finally:
        s.close()
    if c["family"] == "D":          # the same sweep on one stream: the same kernels on the same data
        s = _handle(c, ENLSIP_GN_LOOKAHEAD="0")
        try:
            for _ in range(2):
                base = _solve(s, c, probs)
            assert got - s.route() == {"sweep_lookahead"} and s.route() <= got, (sorted(got), sorted(s.route()))
            _same_bits(c["id"], mine[0], _resident(s, base)[0])
        finally:
            s.close()
    if c["family"] == "E":          # every problem alone, same environment
        for k in range(c["batch"]):
            s = _handle(c)
            try:
                for _ in range(2):
                    solo = _solve(s, c, probs[k:k + 1])
                alone = s.route()
                one = _resident(s, solo)[0]
            finally:
                s.close()
            _against_oracle((c["id"], k, "alone"), solo[0], probs[k][1])
            if alone == got:
                _same_bits((c["id"], k), mine[k], one)
            else:
                print(f"mixed {c['id']} prob {k}: routes differ in {sorted(alone ^ got)}; p differs by {_rel(mine[k][3], one[3]):.1e}")


@pytest.mark.gpu
def test_grid_remap_changes_no_bit():
    """Family C: problem k of a batch of 9 (no remap: the batch is above the limit) against the same problem in batches of 1, 2 and
    8 (remap on), 16 tiles, ENLSIP_GN_PAIR=1 and ENLSIP_GN_LOOKAHEAD=0: the remap only renames workgroups.  Every batch goes through
    enlsip_gn_solve_batched, so that the handles report the same route apart from sweep_xmap (asserted)."""
    c9 = next(c for c in CASES if c["family"] == "C" and c["batch"] == 9)
    probs = _problems(c9)
    res, routes = {}, {}
    for b in (9, 1, 2, 8):
        s = _handle(c9)
        try:
            for _ in range(2):
                outs = _solve(s, c9, probs[:b], single_call=False)
            routes[b] = s.route()
            res[b] = _resident(s, outs)
        finally:
            s.close()
    for b in (1, 2, 8):
        print(f"batch {b}: route differs from the batch of 9 in {sorted(routes[b] ^ routes[9])}")
        assert routes[b] - routes[9] == {"sweep_xmap"} and routes[9] <= routes[b], (b, sorted(routes[b] ^ routes[9]))
        for k in range(b):
            _same_bits((b, k), res[b][k], res[9][k])
