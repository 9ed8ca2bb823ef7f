"""One rank of the mixed-shards magnitude case (tests/tsqr_magnitude_cases.py, n = 96) through the library's collective
enlsip_gn_solve_tsqr, launched by tests/test_gpu_tsqr_magnitudes.py with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set: two
processes share device 0, the process group is gloo and the library's exchange runs over the host-callback transport.  Rank 0
holds the block whose rows are scaled by 2^600, rank 1 the ordinary rest: two different exponents cross the message header.
Prints one line "rank r: ... ok|FAIL" and exits 0 only if everything held."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enlsip.jl_amd", "python")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.distributed as dist


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert world == 2
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)                      # torch's HIP runtime comes up before the library's
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import gn_oracle as go
    import tsqr_magnitude_cases as mc
    from enlsip_gn import GNSolver
    from enlsip_gn.tsqr import tsqr_solve_lib, tsqr_attach, tsqr_exchange, tsqr_scale
    shape = os.environ.get("TSQR_CASE_SHAPE", "n96_t0")
    c = mc.build(shape, "mixed_shards")
    n, t, blocks = mc.SHAPES[shape]
    ref = go.gn_subproblem(c.J, c.rx, c.A, c.cx, c.eps_rank)
    lo, hi = (0, blocks[0]) if rank == 0 else (blocks[0], sum(blocks))
    s = GNSolver(device=0)
    tsqr_attach(s, transport="host")
    Jl = torch.tensor(np.ascontiguousarray(c.J[lo:hi].T), dtype=torch.float64, device=dev)
    rl = torch.tensor(c.rx[lo:hi], dtype=torch.float64, device=dev)
    At = torch.tensor(np.ascontiguousarray(c.A), dtype=torch.float64, device=dev) if t else None
    cd = torch.tensor(c.cx, dtype=torch.float64, device=dev) if t else None
    torch.cuda.synchronize()
    out = tsqr_solve_lib(s, Jl, rl, At, cd, c.eps_rank)
    ok = True
    try:
        mc.check_against_oracle(out, ref, f"rank {rank}")
        ex = tsqr_exchange(s)
        e_local, e_common = tsqr_scale(s)
        assert ex["rank_tags_seen"] == 2 and ex["transport"] == "callback", ex
        assert (e_local != 0) == (rank == 0) and e_common > 400, (e_local, e_common)
        assert "rescaled" in s.route()
    except AssertionError as err:
        ok = False
        print(f"rank {rank}: assertion failed: {err!r}", flush=True)
    print(f"rank {rank}: exponents {tsqr_scale(s)} tags {tsqr_exchange(s)['rank_tags_seen']} {'ok' if ok else 'FAIL'}", flush=True)
    s.close()
    dist.barrier()
    dist.destroy_process_group()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
