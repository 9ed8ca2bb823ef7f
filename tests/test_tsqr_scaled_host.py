"""CPU tests of the scaled TSQR driver (enlsip_gn.tsqr.tsqr_solve(scaled=True)): every rank factors its shard at a power-of-two
scale of its own, (e_g, tail_g^2) are gathered next to the triangles, and the combine brings the blocks to one scale.  The HIP
stages are replaced by NumPy stand-ins built from the oracle (test infrastructure only), which return R, z, tail^2 at scale
2^-e_g with a DIFFERENT e_g on every rank; world size 1 and gloo world size 2.

The file also proves, from the oracle alone, the premise of every case of tests/test_gpu_tsqr_magnitudes.py: LAPACK on the scaled
whole matrix finds the expected rank and a finite p, while a plain sum of squares over a column of one shard leaves the range
(inf or 0) — so no case can pass on plain arithmetic.  One case is different by construction: at 2^505 a column's sum of squares
is still finite (that is what "R is still finite" means); its premise is that the column norm lies above 2^440, the nomination
threshold, beyond which other plain sums of the stage (||J_shard||_F^2, the row norms) overflow."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import gn_oracle as go, lapack_semantics as ls, synth

import tsqr_magnitude_cases as mc


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_exponent(J_loc, rx_loc, rank):
    """What a rank may choose on its own: the exponent of its largest entry, moved by a rank-dependent amount so that no two ranks
    agree."""
    big = max(float(J_loc.abs().max()), float(rx_loc.abs().max()))
    return int(np.frexp(big)[1]) - 1 + 3 * rank - 2


def _make_local(rank):
    def local(J_loc, rx_loc, At, cx, R, z, eps_rank):
        """Stand-in for enlsip_gn_tsqr_local_scaled_dev: the unscaled stand-in of tests/test_tsqr_host.py on the shard times 2^-e."""
        e = _rank_exponent(J_loc, rx_loc, rank)
        Jl = np.ldexp(J_loc.numpy().T.copy(), -e)
        rl = np.ldexp(rx_loc.numpy(), -e)
        n = Jl.shape[1]
        t = 0 if At is None else At.shape[0]
        A = At.numpy() if t else np.zeros((0, n))
        c = cx.numpy() if t else np.zeros(0)
        F_A = go.qr_colnorm(A.T)
        rankA = go.pseudo_rank(F_A.diagR(), eps_rank)
        JQ1 = F_A.rmul_Q(Jl)
        b = -c[F_A.p - 1] if t else np.zeros(0)
        p1 = np.linalg.solve(F_A.R[:t, :t].T, b) if t else np.zeros(0)      # full-rank A in these tests
        d = -JQ1[:, :rankA] @ p1 - rl
        n2 = n - rankA
        f, tau = ls.geqr2(JQ1[:, rankA:])
        dq = ls.apply_qt(f, tau, d)
        kp = min(Jl.shape[0], n2)
        Rl = np.zeros((n2, n2))
        Rl[:kp] = np.triu(f[:kp, :n2])
        R[: n2 * n2] = torch.from_numpy(Rl.reshape(-1, order="F").copy())
        zz = np.zeros(n2)
        zz[:kp] = dq[:kp]
        z[:n2] = torch.from_numpy(zz)
        return n2, float(dq[kp:] @ dq[kp:]), e
    return local


def _make_combine(A, cx):
    def combine(G, n, n2, Rstack, zstack, es, tails, eps_rank):
        """Stand-in for enlsip_gn_tsqr_combine_scaled_dev: blocks to the common scale 2^-E, LAPACK on the stack, the absolute rank
        test on the diagonal scaled back, d_norm scaled back."""
        assert es.shape == (G,) and tails.shape == (G,) and es.dtype == np.int64
        E = int(es.max())
        Rs = Rstack.numpy().reshape(G, n2, n2).transpose(0, 2, 1)        # each block column-major
        stack = np.concatenate([np.ldexp(Rs[g], int(es[g]) - E) for g in range(G)], axis=0)
        zs = np.concatenate([np.ldexp(zstack.numpy()[g * n2:(g + 1) * n2], int(es[g]) - E) for g in range(G)])
        F = go.qr_colnorm(stack)
        rankJ2 = go.pseudo_rank(np.ldexp(F.diagR(), E), eps_rank)
        dq = F.Qt_mul(zs)
        dp2 = np.linalg.solve(F.R[:rankJ2, :rankJ2], dq[:rankJ2])
        p2 = np.concatenate([dp2, np.zeros(n2 - rankJ2)])[go.invperm(F.p)]
        t = A.shape[0]
        F_A = go.qr_colnorm(A.T)
        b = -cx[F_A.p - 1] if t else np.zeros(0)
        p1 = np.linalg.solve(F_A.R[:t, :t].T, b) if t else np.zeros(0)
        p = F_A.Q_mul(np.concatenate([p1, p2])) if t else p2
        tail = sum(float(np.ldexp(tails[g], 2 * (int(es[g]) - E))) for g in range(G))
        d_norm = float(np.ldexp(np.sqrt(tail + float(dq @ dq)), E))
        return p, np.ldexp(dq[:n2], E), d_norm, t, rankJ2, 1, F.p.copy()
    return combine


def _problem(m, n, t, eJ):
    J, rx, A, cx = synth.make_problem(79, m, n, t)
    return np.ldexp(J, eJ), np.ldexp(rx, eJ), A, cx


def _solve_rank(rank, world, m, n, t, eJ):
    from enlsip_gn.tsqr import tsqr_solve, row_range
    J, rx, A, cx = _problem(m, n, t, eJ)
    lo, hi = row_range(m, world, rank)
    J_loc = torch.from_numpy(np.ascontiguousarray(J[lo:hi].T))
    rx_loc = torch.from_numpy(rx[lo:hi].copy())
    At = torch.from_numpy(np.ascontiguousarray(A)) if t else None
    cxt = torch.from_numpy(cx.copy()) if t else None
    return tsqr_solve(None, J_loc, rx_loc, At, cxt, go.SQRT_EPS, local_stage=_make_local(rank),
                      combine_stage=_make_combine(A, cx), scaled=True)


def _worker(rank, world, port, m, n, t, eJ, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = _solve_rank(rank, world, m, n, t, eJ)
    np.savez(out + f".{rank}.npz", p=res.p, d_norm=res.d_norm, rankJ2=res.rankJ2, n2=res.n2, jp=res.jpvtJ2)
    dist.barrier()
    dist.destroy_process_group()


def _check(r, m, n, t, eJ):
    J, rx, A, cx = _problem(m, n, t, eJ)
    ref = go.gn_subproblem(J, rx, A, cx)
    assert np.all(np.isfinite(ref.p))
    assert np.linalg.norm(r["p"] - ref.p) <= 1e-11 * np.linalg.norm(ref.p)
    assert int(r["rankJ2"]) == ref.rankJ2 and int(r["n2"]) == n - ref.rankA
    nd, k = mc.safe_norm(ref.d)
    assert abs(float(np.ldexp(float(r["d_norm"]), -k)) - nd) <= 1e-12 * nd
    assert np.array_equal(r["jp"], ref.jpvtJ2)


@pytest.mark.parametrize("m,n,t,eJ", [(600, 24, 0, 600), (601, 20, 3, -300), (400, 16, 2, 0)])
def test_scaled_driver_world1(m, n, t, eJ):
    res = _solve_rank(0, 1, m, n, t, eJ)
    _check({"p": res.p, "d_norm": res.d_norm, "rankJ2": res.rankJ2, "n2": res.n2, "jp": res.jpvtJ2}, m, n, t, eJ)


@pytest.mark.parametrize("m,n,t,eJ", [(600, 24, 0, 600), (601, 20, 3, -300)])
def test_scaled_driver_gloo_world2(tmp_path, m, n, t, eJ):
    """Two ranks with different exponents (they differ by 3 and by what the blocks' largest entries differ)."""
    port = _free_port()
    out = str(tmp_path / "res")
    mp.spawn(_worker, args=(2, port, m, n, t, eJ, out), nprocs=2, join=True)
    r0, r1 = np.load(out + ".0.npz"), np.load(out + ".1.npz")
    for r in (r0, r1):
        _check(r, m, n, t, eJ)
    assert np.array_equal(r0["p"], r1["p"])


@pytest.mark.parametrize("shape,case", mc.case_ids())
def test_premise_of_the_gpu_cases(shape, case):
    c = mc.build(shape, case)
    n, t, _ = mc.SHAPES[shape]
    ref = go.gn_subproblem(c.J, c.rx, c.A, c.cx, c.eps_rank)
    assert ref.rankA == t and np.all(np.isfinite(ref.p))
    assert ref.rankJ2 == (n - t if c.rankJ2_full else 0)
    with np.errstate(over="ignore", under="ignore"):
        ss = float(np.sum(c.probe ** 2))
    if c.premise == "inf":
        assert np.isinf(ss)
    elif c.premise == "zero":
        assert ss == 0.0 and np.abs(c.probe).max() > 0.0
    else:
        assert np.isfinite(ss) and ss > 2.0 ** 880            # the column norm is above 2^440


def test_scaled_entry_points_are_exported():
    """Fails on a library without the feature."""
    import __graft_entry__ as ge
    ge.build()
    import enlsip_gn._lib as L
    lib = L.load()
    for name in ("enlsip_gn_tsqr_local_scaled_dev", "enlsip_gn_tsqr_combine_scaled_dev", "enlsip_gn_tsqr_get_scale"):
        assert name in L.PROTOTYPES and hasattr(lib, name), name
