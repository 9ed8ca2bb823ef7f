"""Row-sharded TSQR where something is degenerate: a rank-deficient A (the second attempt of the local pass), a J2 whose stacked
pivoted QR truncates, n2 == 0, shards shorter than n2 or on either side of the 512-row tile, a shard of zeros, and shards used in
place (J + lo with ldj = m).  Every case runs through the two-stage form (plain and scaled stages, three row blocks on one handle)
and through the library's one-rank collective, against the oracle (real LAPACK) on the whole matrix.  Cases and the expected
(rankA, code, n2, rankJ2): tests/tsqr_edge_cases.py; that no sharded factorisation can legitimately decide a rank or a pivot
differently, and that the tolerances are not the binding ones, is proved on the CPU in tests/test_tsqr_edges_host.py.  What the
inputs do not determine is not compared (tsqr_edge_cases.comparable): entries of dlead beyond rankJ2 where the pivoted QR truncates,
and, for a rank-deficient A, the pivots of J2 and the entries of dlead — ranks, code, p (1e-11) and d_norm (1e-12) always are."""
import numpy as np
import pytest

from oracle import gn_oracle as go

import tsqr_edge_cases as ec
import tsqr_magnitude_cases as mc

pytestmark = pytest.mark.gpu

NAMES = list(ec.CASES)


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


_refs = {}


def _ref(name):
    """The inputs and the oracle's solve of a case, computed once and shared."""
    if name not in _refs:
        J, rx, A, cx = ec.build(name)
        _refs[name] = (J, rx, A, cx, go.gn_subproblem(J, rx, A, cx, ec.get(name).eps_rank))
    return _refs[name]


def _shards(solver, name, scaled, in_place=False):
    from enlsip_gn.tsqr import tsqr_solve_shards
    J, rx, A, cx, _ = _ref(name)
    c = ec.get(name)
    return tsqr_solve_shards(solver, J, rx, A, cx, len(c.blocks), c.eps_rank, scaled=scaled, row_blocks=c.blocks, in_place=in_place)


def _device(J, rx, A, cx):
    import torch
    dev = torch.device("cuda", 0)
    t = A.shape[0]
    Jd = torch.tensor(np.ascontiguousarray(J.T), dtype=torch.float64, device=dev)
    rd = torch.tensor(rx, dtype=torch.float64, device=dev)
    Ad = torch.tensor(np.ascontiguousarray(A), dtype=torch.float64, device=dev) if t else None
    cd = torch.tensor(cx, dtype=torch.float64, device=dev) if t else None
    torch.cuda.synchronize()
    return Jd, rd, Ad, cd


def _one_rank(solver, name):
    from enlsip_gn.tsqr import tsqr_solve_lib
    J, rx, A, cx, _ = _ref(name)
    Jd, rd, Ad, cd = _device(J, rx, A, cx)
    solver._chk(solver._lib.enlsip_gn_tsqr_set_exchange(solver._h, None, None, 1, 0))
    return tsqr_solve_lib(solver, Jd, rd, Ad, cd, ec.get(name).eps_rank)


def _local_routes(solver, J, rx, A, cx, blocks, eps, scaled, in_place):
    """The route bits (enlsip_gn_get_route) of each block's local stage alone, contiguous or in place."""
    import torch
    from enlsip_gn.tsqr import hip_local_stage, hip_local_stage_scaled
    Jd, rd, Ad, cd = _device(J, rx, A, cx)
    n, m = Jd.shape
    t = A.shape[0]
    R = torch.empty((n * n,), dtype=torch.float64, device=Jd.device)
    z = torch.empty((n,), dtype=torch.float64, device=Jd.device)
    routes = []
    for lo, mg in zip(ec.offsets(blocks), blocks):
        if in_place:
            keep, pJ, ldj, prx = None, Jd.data_ptr() + 8 * lo, m, rd.data_ptr() + 8 * lo
        else:
            keep = (Jd[:, lo:lo + mg].contiguous(), rd[lo:lo + mg].contiguous())
            pJ, ldj, prx = keep[0].data_ptr(), mg, keep[1].data_ptr()
        torch.cuda.synchronize()
        stage = hip_local_stage_scaled if scaled else hip_local_stage
        stage(solver, mg, n, t, pJ, ldj, prx, Ad.data_ptr() if t else 0, cd.data_ptr() if t else 0, R.data_ptr(), z.data_ptr(), eps)
        routes.append(frozenset(solver.route()))
        del keep
    return routes


def _check(out, name, tag):
    ref = _ref(name)[4]
    assert (out.rankA, out.code, out.n2, out.rankJ2) == ec.get(name).expected, (tag, out.rankA, out.code, out.n2, out.rankJ2)
    mc.check_against_oracle(out, ref, tag, **ec.comparable(ref))


def _same_bits(a, b, tag):
    assert (a.rankA, a.rankJ2, a.code, a.n2) == (b.rankA, b.rankJ2, b.code, b.n2), tag
    assert np.array_equal(a.jpvtJ2, b.jpvtJ2), tag
    assert np.array_equal(a.p, b.p), (tag, float(np.abs(a.p - b.p).max()))
    assert np.array_equal(a.dlead, b.dlead), tag
    assert a.d_norm == b.d_norm, (tag, a.d_norm, b.d_norm)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("name", NAMES)
def test_two_stage_form(name, scaled, solver):
    """tsqr_solve_shards over the case's row blocks: the literal ranks, the oracle's pivots on the leading rankJ2 positions, p to
    1e-11, dlead to 1e-10, d_norm to 1e-12 (pivots and dlead where the inputs determine them).  In band the scaled stages scale
    nothing."""
    from enlsip_gn.tsqr import tsqr_scale
    out = _shards(solver, name, scaled)
    if scaled:
        assert tsqr_scale(solver) == (0, 0) and "rescaled" not in solver.route(), name
    _check(out, name, f"{name} {'scaled' if scaled else 'plain'} stages")
    J, rx, A, cx, _ = _ref(name)
    c = ec.get(name)
    routes = _local_routes(solver, J, rx, A, cx, c.blocks, c.eps_rank, scaled, False)
    print(f"{name} local-stage routes: " + " | ".join(",".join(sorted(r)) for r in routes), flush=True)


@pytest.mark.parametrize("name", NAMES)
def test_one_rank_library_collective(name, solver):
    """enlsip_gn_solve_tsqr on the whole matrix as one shard, no communicator: the message is packed from n, moved by a device
    copy and unpacked again; with n2 == 0 nothing is unpacked and the rank tags read -1."""
    from enlsip_gn.tsqr import tsqr_exchange, tsqr_scale, tsqr_transport
    out = _one_rank(solver, name)
    assert tsqr_transport(solver) == "none"
    assert tsqr_scale(solver) == (0, 0) and "rescaled" not in solver.route(), name
    _check(out, name, f"{name} one rank")
    print(f"{name} one-rank routes: " + ",".join(sorted(solver.route())), flush=True)
    seen = tsqr_exchange(solver)["rank_tags_seen"]
    if name == "t_eq_n_9":
        ref = _ref(name)[4]
        nd = float(np.linalg.norm(ref.d))
        assert seen == -1
        assert np.all(np.isfinite(out.p)) and out.dlead.size == 0 and out.jpvtJ2.size == 0
        assert abs(out.d_norm - nd) <= 1e-12 * nd, (out.d_norm, nd)
    else:
        assert seen == 1, (name, seen)


def _in_place_against_contiguous(solver, J, rx, A, cx, blocks, eps, scaled, run, tag):
    """Ranks and pivots of the in-place run equal the contiguous run's; p bit for bit where every block's local stage took the same
    route (a different J*Q1 kernel behind launch_jq1_v2's alignment gate may round differently)."""
    contiguous = run(False)
    in_place = run(True)
    in_place.route = solver.route()                 # of the whole in-place run, before the local stages below run again
    r_c = _local_routes(solver, J, rx, A, cx, blocks, eps, scaled, False)
    r_i = _local_routes(solver, J, rx, A, cx, blocks, eps, scaled, True)
    same = r_c == r_i
    diff = float(np.abs(in_place.p - contiguous.p).max())
    print(f"{tag}: routes {'agree' if same else 'DIFFER'}, max |p in place - p contiguous| {diff:.2e}", flush=True)
    for g, (a, b) in enumerate(zip(r_c, r_i)):
        if a != b:
            print(f"{tag}: block {g}: contiguous only {sorted(a - b)}, in place only {sorted(b - a)}", flush=True)
    assert (in_place.rankA, in_place.rankJ2, in_place.code, in_place.n2) == (contiguous.rankA, contiguous.rankJ2, contiguous.code,
                                                                            contiguous.n2), tag
    assert np.array_equal(in_place.jpvtJ2, contiguous.jpvtJ2), tag
    if same:
        _same_bits(in_place, contiguous, tag)
    return contiguous, in_place, same


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("name", ec.IN_PLACE + [ec.GATE.name])
def test_shards_in_place(name, scaled, solver):
    """Shards as views J + lo with ldj = m (bases at odd and even rows): the oracle's answer to the same tolerances, and the
    contiguous run's bits wherever the routes agree."""
    J, rx, A, cx, _ = _ref(name)
    c = ec.get(name)
    tag = f"{name} in place {'scaled' if scaled else 'plain'}"
    contiguous, in_place, same = _in_place_against_contiguous(
        solver, J, rx, A, cx, c.blocks, c.eps_rank, scaled, lambda ip: _shards(solver, name, scaled, in_place=ip), tag)
    _check(in_place, name, tag)
    _check(contiguous, name, tag + " (contiguous partner)")
    if name == ec.GATE.name:
        # the case exists to cross the gate: block 1 (64 rows of an n = 128, kA = 64 problem) is served by k_jq1_v2 as a
        # contiguous copy and, at its odd row offset, by the general kernel in place
        assert not same, "the gate case no longer changes the J*Q1 kernel: choose another shape"


def test_shards_in_place_out_of_band(solver):
    """The mixed-shards magnitude case (block 0 times 2^600) in place: the out-of-band block goes through scaled_copies with
    ldj != m_loc, the others are read where they lie."""
    from enlsip_gn.tsqr import tsqr_solve_shards
    c = mc.build("n96_t8", "mixed_shards")
    ref = go.gn_subproblem(c.J, c.rx, c.A, c.cx, c.eps_rank)
    run = lambda ip: tsqr_solve_shards(solver, c.J, c.rx, c.A, c.cx, len(c.blocks), c.eps_rank, scaled=True, row_blocks=c.blocks,
                                       in_place=ip)
    tag = "n96_t8 mixed_shards in place"
    contiguous, in_place, _ = _in_place_against_contiguous(solver, c.J, c.rx, c.A, c.cx, c.blocks, c.eps_rank, True, run, tag)
    assert "rescaled" in in_place.route
    mc.check_against_oracle(in_place, ref, tag)
    mc.check_against_oracle(contiguous, ref, tag + " (contiguous partner)")


def test_handle_reuse_across_degenerate_shapes(solver):
    """The second attempt of the local pass (rankA < t), then n2 == 0, then a one-row shard, then the first again, on ONE handle:
    each result is bit for bit that of a fresh handle, in the two-stage form and in the library's collective."""
    from enlsip_gn import GNSolver
    fresh = {}
    for name in dict.fromkeys(ec.REUSE_ORDER):
        s = GNSolver(device=0)
        try:
            fresh[name] = (_shards(s, name, True), _one_rank(s, name))
        finally:
            s.close()
    one = GNSolver(device=0)
    try:
        for k, name in enumerate(ec.REUSE_ORDER):
            _same_bits(_shards(one, name, True), fresh[name][0], f"reuse step {k} {name} two-stage")
            _same_bits(_one_rank(one, name), fresh[name][1], f"reuse step {k} {name} one rank")
    finally:
        one.close()
    for name, (a, b) in fresh.items():
        _check(a, name, f"{name} fresh handle two-stage")
        _check(b, name, f"{name} fresh handle one rank")
