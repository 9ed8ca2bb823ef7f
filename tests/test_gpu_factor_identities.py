"""The resident factors of a solve by their defining identities (tests/factor_identities.py), one test id per case of its
rule-made list: every route bit the dispatch grid reaches below the size cap, every kind, the forced variants (panel pairs, 256-row
tiles, reflector-by-reflector update, launch-per-step pivoted QR, the unfused small shape) and the problem-index cases (a batch of
5, both pipeline halves of 128, a ragged batch).  Each case is solved on a fresh handle, must report the route it was picked
for, and has F_A, F_L11, F_J2 (R, p, Q'v and Qv over the full length, both directions), the J1 columns the routed J*Q1 kernel
left in W, get_JQ1 and out.d (full length, with its sign) checked against their definitions — no oracle, no sign convention.
Every figure is printed before it is asserted."""
import numpy as np
import pytest

import factor_identities as fi

CASES = fi.cases()


class _Out:
    def __init__(self, p, d, rankA):
        self.p, self.d, self.rankA = p, d, rankA


def _solve(s, c):
    """Solves case c on handle s; returns [(k, (J, rx, A, cx), out)] for the problems to check."""
    from enlsip_gn import GNSolver
    m, n, t, batch = c["m"], c["n"], c["t"], c["batch"]
    if batch == 1:
        P = fi.problem(c, 0)
        return [(0, P, s.solve(*P))]
    probs = [fi.problem(c, k) for k in range(batch)]
    Jb = np.stack([np.ascontiguousarray(P[0].T) for P in probs])
    rxb = np.stack([P[1] for P in probs])
    if c["t_list"]:
        At, cxb, tk = GNSolver.pack_ragged([P[2] for P in probs], [P[3] for P in probs], n=n)
        p, b, d, infos, jA, jL, jJ = s.solve_batched_ragged(Jb, rxb, At, cxb, tk)
    else:
        p, b, d, infos, jA, jL, jJ = s.solve_batched(Jb, rxb, np.stack([np.ascontiguousarray(P[2]) for P in probs]) if t else None,
                                                     np.stack([P[3] for P in probs]) if t else None)
    return [(k, probs[k], _Out(p[k], d[k], infos[k][0])) for k in c["probs"]]


def _solve_and_check(s, c):
    solved = _solve(s, c)
    got = s.route()
    assert c["want"] <= got, (c["id"], sorted(c["want"] - got), sorted(got))
    for k, (J, rx, A, cx), out in solved:
        res = fi.check_solve_identities(fi.SolverAccess(s, c["m"], c["n"], k), J, rx, A, cx, out, kind=c["kind"])
        print(f"identities {c['id']} prob {k}: " + " ".join(f"{key}={v:.1e}" for key, v in sorted(res.items())))
        fi.assert_within(res, c["kind"], (c["id"], k))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_resident_factors_satisfy_their_definitions(c):
    from enlsip_gn import GNSolver
    with fi.handle_env(c["env"]):
        s = GNSolver(device=0, flags=c["flags"], tile_rows=c["tile_rows"])        # fresh handle: no plan of an earlier shape
    try:
        _solve_and_check(s, c)
    finally:
        s.close()


@pytest.mark.gpu
def test_accessors_follow_the_current_plan():
    """One handle through a multi-tile blocked shape, the fused one-tile shape and a wide shape: after each solve the accessors
    must walk the storage of THAT solve (panel count, tree levels, tile rows, leading dimensions), not of an earlier plan."""
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    try:
        for (m, n, t) in ((700, 129, 3), (256, 32, 4), (33, 80, 10)):
            _solve_and_check(s, fi._case(dict(batch=1, m=m, n=n, t=t, kind="full"), "plan"))
    finally:
        s.close()
