"""One rank of the consumers on a row-sharded J (enlsip_gn_tsqr_products, _first_lagrange, _second_lagrange) on a real device,
started by tests/test_gpu_tsqr_products.py: RANK / WORLD_SIZE processes share device 0, the process group is gloo and the library's
exchange runs over the caller-supplied transport (enlsip_gn.tsqr.tsqr_attach(transport="host")).  Every rank builds the same seeded
problem, keeps its row block on the GPU, joins the sharded solve and the collectives after it, checks its outputs against the
references and writes them to TSQR_PRODUCTS_OUT.<rank>.npz for the bitwise comparison between the ranks.
TSQR_PRODUCTS_RCCL=1 (one rank): the same through a one-rank RCCL communicator, the exchange as a self-gather."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (os.path.join(ROOT, "enlsip.jl_amd", "python"), ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)
import numpy as np

N, T = 12, 3


def problem(world):
    """(J, rx, A, cx, shard heights): a shard shorter than n (two ranks), a one-row shard (three ranks), a chunk edge in both"""
    import consumer_reference as cr
    import tsqr_product_cases as pc
    CH = pc.chunk_height()
    heights = {1: [CH + 65], 2: [CH + 1, 7], 3: [65, CH + 1, 1]}[world]
    J, rx, A, cx = cr.make_problem(6600 + world, sum(heights), N, T)
    return J, rx, A, cx, heights


def main():
    import torch
    import torch.distributed as dist
    import consumer_reference as cr
    import tsqr_product_cases as pc
    from oracle import gn_oracle as go
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    rccl = os.environ.get("TSQR_PRODUCTS_RCCL") == "1"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if world > 1:
        dist.init_process_group("gloo")
    from enlsip_gn import GNSolver
    from enlsip_gn.tsqr import (tsqr_attach, tsqr_solve_lib, tsqr_products_lib, tsqr_first_lagrange_lib, tsqr_second_lagrange_lib,
                                tsqr_transport)
    s = GNSolver(device=0)
    tsqr_attach(s, transport="rccl" if rccl else "host")
    J, rx, A, cx, heights = problem(world)
    lo = sum(heights[:rank])
    hi = lo + heights[rank]
    Jl = torch.tensor(np.ascontiguousarray(J[lo:hi].T), dtype=torch.float64, device=dev)
    rl = torch.tensor(rx[lo:hi], dtype=torch.float64, device=dev)
    At = torch.tensor(np.ascontiguousarray(A), dtype=torch.float64, device=dev)
    cd = torch.tensor(cx, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eps = go.SQRT_EPS
    sol = tsqr_solve_lib(s, Jl, rl, At, cd, eps)
    p = sol.p
    Jp = torch.zeros((hi - lo,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    g0 = tsqr_products_lib(s, N, T, None)
    gp = tsqr_products_lib(s, N, T, p, Jp)
    lam1, gres = tsqr_first_lagrange_lib(s, N, T, None, None, eps)
    lam2 = tsqr_second_lagrange_lib(s, N, T, p, None, eps)
    transport = tsqr_transport(s)
    bad = []
    for tag, out, pp in (("J' rx", g0, None), ("J'(rx + J p)", gp, p)):
        ref = pc.Reference(J, rx, pp, world)
        why = ref.check(out.grad, out.sums, tag)
        if why:
            bad.append(why)
        if pp is not None:
            if not np.all(np.abs(Jp.cpu().numpy() - ref.Jp[lo:hi]) <= ref.Jp_bound[lo:hi]):
                bad.append("this rank's J p")
            Ap_ref, Ap_bound = cr.exact_matvec(A, pp)
            if not np.all(np.abs(out.Ap - Ap_ref) <= Ap_bound):
                bad.append("A p")
    F = go.qr_colnorm(A.T)
    S, _ = cr.kept_set(F.p, F.diagR(), eps)
    R = cr.EstimateReference(A, S)
    g_exact = cr.exact_gradient(J, rx)
    kS = cr.kappa(A[S])
    lam1_r, gres_r = R.first(g_exact, cx)
    b1 = cr.estimate_bound(kS, cr.gamma_rhs(J, rx) * R.first_cancellation(g_exact, cx))
    if cr.rel_err(lam1, lam1_r) > b1 or abs(gres - gres_r) > b1 * np.linalg.norm(g_exact):
        bad.append(f"first estimate {cr.rel_err(lam1, lam1_r):.2e} > {b1:.2e}")
    b2 = cr.estimate_bound(kS, cr.gamma_rhs(J, rx, p))
    if cr.rel_err(lam2, R.second(J, rx, p)) > b2:
        bad.append(f"second estimate {cr.rel_err(lam2, R.second(J, rx, p)):.2e} > {b2:.2e}")
    want = "rccl" if rccl else ("callback" if world > 1 else "none")
    if transport != want:
        bad.append(f"transport {transport}, expected {want}")
    print(f"rank {rank}/{world} transport {transport}: {'ok' if not bad else 'FAIL ' + '; '.join(bad)}", flush=True)
    out = os.environ.get("TSQR_PRODUCTS_OUT")
    if out:
        np.savez(f"{out}.{rank}.npz", p=p, g0_grad=g0.grad, g0_sums=g0.sums, gp_grad=gp.grad, gp_sums=gp.sums, Ap=gp.Ap, lam1=lam1,
                 gres=np.array([gres]), lam2=lam2)
    s.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
