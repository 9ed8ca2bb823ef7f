"""Row-sharded TSQR at any input magnitude: enlsip_gn_solve_tsqr (one rank) and the scaled stage pair
enlsip_gn_tsqr_local_scaled_dev / _combine_scaled_dev (three row blocks on one handle, enlsip_gn.tsqr.tsqr_solve_shards(scaled=True))
against the oracle (real LAPACK) on the SAME scaled whole matrix.  Cases, shapes and tolerances: tests/tsqr_magnitude_cases.py;
that no case can pass on plain arithmetic is proved on the CPU in tests/test_tsqr_scaled_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gn_oracle as go

import tsqr_magnitude_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


_refs = {}


def _ref(shape, case):
    """The oracle's solve of a case, computed once and shared."""
    if (shape, case) not in _refs:
        c = mc.build(shape, case)
        _refs[(shape, case)] = (c, go.gn_subproblem(c.J, c.rx, c.A, c.cx, c.eps_rank))
    return _refs[(shape, case)]


def _one_rank(solver, J, rx, A, cx, eps):
    import torch
    from enlsip_gn.tsqr import tsqr_solve_lib
    dev = torch.device("cuda", 0)
    t = A.shape[0]
    Jd = torch.tensor(np.ascontiguousarray(J.T), dtype=torch.float64, device=dev)
    rd = torch.tensor(rx, dtype=torch.float64, device=dev)
    Ad = torch.tensor(np.ascontiguousarray(A), dtype=torch.float64, device=dev) if t else None
    cd = torch.tensor(cx, dtype=torch.float64, device=dev) if t else None
    torch.cuda.synchronize()
    solver._chk(solver._lib.enlsip_gn_tsqr_set_exchange(solver._h, None, None, 1, 0))
    return tsqr_solve_lib(solver, Jd, rd, Ad, cd, eps)


def _three_blocks(solver, J, rx, A, cx, eps, blocks, scaled=True):
    from enlsip_gn.tsqr import tsqr_solve_shards
    return tsqr_solve_shards(solver, J, rx, A, cx, len(blocks), eps, scaled=scaled, row_blocks=blocks)


@pytest.mark.parametrize("shape,case", mc.case_ids())
def test_tsqr_magnitudes_match_lapack(shape, case, solver):
    from enlsip_gn.tsqr import tsqr_scale
    c, ref = _ref(shape, case)
    outs = {"one rank": _one_rank(solver, c.J, c.rx, c.A, c.cx, c.eps_rank)}
    assert "rescaled" in solver.route(), (shape, case)
    e1 = tsqr_scale(solver)
    assert e1[0] != 0 or case == "A_up_600", (shape, case, e1)         # only A', cx out of the band: J's exponent stays 0
    outs["three blocks"] = _three_blocks(solver, c.J, c.rx, c.A, c.cx, c.eps_rank, c.blocks)
    assert "rescaled" in solver.route(), (shape, case)
    for path, out in outs.items():
        mc.check_against_oracle(out, ref, f"{shape} {case} {path}")
    if case in mc.BITWISE:
        # power-of-two scaling is exact: the same call on the unscaled inputs returns the same bits of p, the same ranks and pivots,
        # and dlead, d_norm divided by exactly that power of two
        k = mc.BITWISE[case]
        J0, rx0, A0, cx0 = c.base
        base = {"one rank": _one_rank(solver, J0, rx0, A0, cx0, c.eps_rank),
                "three blocks": _three_blocks(solver, J0, rx0, A0, cx0, c.eps_rank, c.blocks)}
        for path, out in outs.items():
            b = base[path]
            tag = (shape, case, path)
            assert (out.rankA, out.rankJ2, out.code) == (b.rankA, b.rankJ2, b.code), tag
            assert np.array_equal(out.jpvtJ2, b.jpvtJ2), tag
            assert np.array_equal(out.p, b.p), (tag, float(np.abs(out.p - b.p).max()))
            assert np.array_equal(out.dlead, np.ldexp(b.dlead, k)), tag
            assert out.d_norm == float(np.ldexp(b.d_norm, k)), (tag, out.d_norm, b.d_norm)


@pytest.mark.parametrize("shape", list(mc.SHAPES))
def test_in_band_inputs_are_not_rescaled(shape, solver):
    """Inside the band nothing is scaled: both exponents are 0, the route bit is clear and the result is the oracle's; J 2^600 on
    the same handle reports an exponent and sets the bit."""
    from enlsip_gn.tsqr import tsqr_scale
    c, _ = _ref(shape, "all_up_600")
    J0, rx0, A0, cx0 = c.base
    ref0 = go.gn_subproblem(J0, rx0, A0, cx0, c.eps_rank)
    for path in ("one rank", "three blocks"):
        run = (lambda *a: _one_rank(solver, *a)) if path == "one rank" else (lambda *a: _three_blocks(solver, *a, c.blocks))
        out = run(J0, rx0, A0, cx0, c.eps_rank)
        assert tsqr_scale(solver) == (0, 0) and "rescaled" not in solver.route(), (shape, path)
        mc.check_against_oracle(out, ref0, f"{shape} in band {path}")
        run(np.ldexp(J0, 600), rx0, A0, cx0, c.eps_rank)
        e_local, e_common = tsqr_scale(solver)
        assert e_common != 0 and "rescaled" in solver.route(), (shape, path, e_local, e_common)
        if path == "one rank":
            assert e_local == e_common


def test_old_stage_pair_stays_plain(solver):
    """enlsip_gn_tsqr_local_dev / _combine_dev cannot carry an exponent and stay outside the magnitude contract (include/enlsip_gn.h):
    J 2^600 comes back with rankJ2 = 0 or with something that is not finite, as before.  Pinned so that a change is noticed."""
    c, ref = _ref("n96_t0", "J_up_600")
    out = _three_blocks(solver, c.J, c.rx, c.A, c.cx, c.eps_rank, c.blocks, scaled=False)
    assert ref.rankJ2 == 96
    assert out.rankJ2 == 0 or not (np.all(np.isfinite(out.p)) and np.isfinite(out.d_norm) and np.all(np.isfinite(out.dlead)))


def test_two_processes_exchange_two_exponents():
    """The mixed-shards case at n = 96 with two real ranks on the one device (tests/tsqr_scaled_rank_worker.py): gloo carries the
    message through the host-callback transport, rank 0's block is scaled by 2^600 and rank 1's is not, so two different exponents
    cross the header; both ranks must see both rank tags and reproduce the oracle.  Each child has its own time limit; when one
    fails or runs out of time the other is ended and nothing more is started."""
    import socket
    import time
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    worker = os.path.join(ROOT, "tests", "tsqr_scaled_rank_worker.py")
    limit = 150.0
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   TSQR_CASE_SHAPE="n96_t0")
        procs.append(subprocess.Popen([sys.executable, worker], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    start = time.monotonic()
    failed = None
    pending = set(range(2))
    while pending and failed is None:
        for r in sorted(pending):
            try:
                rc = procs[r].wait(timeout=0.2)
            except subprocess.TimeoutExpired:
                if time.monotonic() - start > limit:
                    failed = f"rank {r} exceeded its time limit of {limit:.0f} s"
                    break
                continue
            pending.discard(r)
            if rc != 0:
                failed = f"rank {r} exited with {rc}"
                break
    for r in pending:                      # a failure: end the other rank, start nothing more
        procs[r].kill()
    outs = [p.communicate()[0] for p in procs]
    text = "\n".join(o[-1500:] for o in outs)
    assert failed is None, failed + "\n" + text
    for r in range(2):
        assert f"rank {r}: exponents" in outs[r] and " ok" in outs[r] and "FAIL" not in outs[r], text
        assert "tags 2 " in outs[r], text
