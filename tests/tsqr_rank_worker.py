"""One rank of the row-sharded TSQR (the library's collective enlsip_gn_solve_tsqr, and the two-stage form with the exchange done
by torch.distributed: enlsip_gn.tsqr.tsqr_solve_lib / tsqr_solve) on a real device, launched by
tests/test_gpu_robustness.py under torch.distributed.run: every rank builds the same seeded problem, keeps its row block on the
GPU, joins the collective solve and compares the result with the oracle's single solve.  On this pool's one-GPU boxes the ranks
share device 0, the process group is gloo and the library's exchange runs over its caller-supplied transport (RCCL refuses two
ranks on one device); on a multi-GPU node the same script runs with TSQR_BACKEND=nccl, one device per rank, and the library
creates its own RCCL communicator.

TSQR_CASES=edges runs the degenerate cases of tests/tsqr_edge_cases.py instead (rank-deficient A, n2 == 0, every shard shorter
than n2, a truncating J2) through enlsip_gn_solve_tsqr and tsqr_solve(scaled=True), with the checks of
tsqr_magnitude_cases.check_against_oracle; unset, the three full-rank shapes below."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enlsip.jl_amd", "python")); sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.distributed as dist


def main():
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("TSQR_BACKEND", "gloo")
    devidx = local if backend == "nccl" else local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(devidx)
    dev = torch.device("cuda", devidx)
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group(backend)
    from enlsip_gn import GNSolver
    from enlsip_gn.tsqr import tsqr_attach
    bad = 0
    s = GNSolver(device=devidx)
    tsqr_attach(s, transport="rccl" if backend == "nccl" else "host")
    which = os.environ.get("TSQR_CASES", "")
    if which == "edges":
        bad = edge_cases(s, rank, world, dev)
    elif which:
        raise SystemExit(f"TSQR_CASES={which}: unknown case list")
    else:
        bad = full_rank_shapes(s, rank, world, dev)
    s.close()
    dist.barrier()
    dist.destroy_process_group()
    return 1 if bad else 0


def full_rank_shapes(s, rank, world, dev):
    from oracle import gn_oracle as go, synth
    from enlsip_gn.tsqr import tsqr_solve, tsqr_solve_lib, row_range
    bad = 0
    for (m, n, t) in [(3001, 48, 5), (6000, 300, 0), (2500, 130, 40)]:
        J, rx, A, cx = synth.make_problem(4400 + m, m, n, t)
        ref = go.gn_subproblem(J, rx, A, cx)
        lo, hi = row_range(m, world, rank)
        Jl = torch.tensor(np.ascontiguousarray(J[lo:hi].T), dtype=torch.float64, device=dev)
        rl = torch.tensor(rx[lo:hi], dtype=torch.float64, device=dev)
        At = torch.tensor(np.ascontiguousarray(A), dtype=torch.float64, device=dev) if t else None
        cd = torch.tensor(cx, dtype=torch.float64, device=dev) if t else None
        torch.cuda.synchronize()
        for name, fn in (("lib", tsqr_solve_lib), ("two-stage", tsqr_solve)):
            out = fn(s, Jl, rl, At, cd)
            err = float(np.linalg.norm(out.p - ref.p) / np.linalg.norm(ref.p))
            dn = abs(out.d_norm - float(np.linalg.norm(ref.d))) / float(np.linalg.norm(ref.d))
            n2 = n - ref.rankA
            dl = float(np.abs(np.abs(out.dlead) - np.abs(ref.d[:n2])).max() / max(np.abs(ref.d).max(), 1e-300)) if n2 else 0.0
            ok = (err <= 1e-10 and dn <= 1e-10 and dl <= 1e-9 and (out.rankA, out.rankJ2) == (ref.rankA, ref.rankJ2)
                  and np.array_equal(out.jpvtJ2, ref.jpvtJ2))
            print(f"rank {rank}/{world} {name} m={m} n={n} t={t}: rel p {err:.1e} rel |d| {dn:.1e} lead {dl:.1e} "
                  f"ranks ({out.rankA},{out.rankJ2}) {'ok' if ok else 'FAIL'}", flush=True)
            bad += 0 if ok else 1
    return bad


def edge_cases(s, rank, world, dev):
    """Shards from row_range(m, world, rank): with two ranks all_short_n24_t4 gives 8 and 7 rows, both shorter than n2 = 20 — the
    packed triangle with kp < n2 on every rank."""
    from functools import partial
    from oracle import gn_oracle as go
    from enlsip_gn.tsqr import tsqr_solve, tsqr_solve_lib, tsqr_exchange, row_range
    import tsqr_edge_cases as ec
    import tsqr_magnitude_cases as mc
    bad = 0
    for name in ec.RANK_WORKER:
        c = ec.get(name)
        J, rx, A, cx = ec.build(name)
        m, t = J.shape[0], A.shape[0]
        ref = go.gn_subproblem(J, rx, A, cx, c.eps_rank)
        lo, hi = row_range(m, world, rank)
        Jl = torch.tensor(np.ascontiguousarray(J[lo:hi].T), dtype=torch.float64, device=dev)
        rl = torch.tensor(rx[lo:hi], dtype=torch.float64, device=dev)
        At = torch.tensor(np.ascontiguousarray(A), dtype=torch.float64, device=dev) if t else None
        cd = torch.tensor(cx, dtype=torch.float64, device=dev) if t else None
        torch.cuda.synchronize()
        for form, fn in (("lib", tsqr_solve_lib), ("two-stage scaled", partial(tsqr_solve, scaled=True))):
            out = fn(s, Jl, rl, At, cd, c.eps_rank)
            tag = f"rank {rank}/{world} {form} {name} rows {lo}:{hi}"
            try:
                assert (out.rankA, out.code, out.n2, out.rankJ2) == c.expected, (out.rankA, out.code, out.n2, out.rankJ2)
                mc.check_against_oracle(out, ref, tag, **ec.comparable(ref))
                if form == "lib":
                    seen = tsqr_exchange(s)["rank_tags_seen"]
                    assert seen == (world if out.n2 > 0 else -1), ("rank tags", seen)
                print(f"{tag}: ok", flush=True)
            except AssertionError as err:
                bad += 1
                print(f"{tag}: FAIL {err}", flush=True)
    return bad


if __name__ == "__main__":
    sys.exit(main())
