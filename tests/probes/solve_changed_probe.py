"""Probe (not a test): enlsip_gn_solve_changed_batched_dev at 0 / 10 / 50 / 100 % flagged problems against the whole pair
(enlsip_gn_factor_constraints_batched_dev + enlsip_gn_solve_factored_batched_dev) on the same working sets, at the batch shapes of
C2, C3 and C5 (C5 at the launch limit of 32768 problems: a larger batch is chunked and not resident as a whole).  The handle is
created on a stream of the probe's own and the HIP events are recorded on that stream, around the calls.  Every one of these calls
ends with a host synchronisation of the streams it used (the second pipelined half runs on a stream of the library's), so an
interval is the call as its caller sees it: device work plus the host work between the launches.  The 0 % column, which launches
nothing, is host overhead only.  Prints one line per shape and share; DESIGN.md §5.7 holds the table.

    python tests/probes/solve_changed_probe.py [C2 C3 C5]
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))
from enlsip_gn import GNSolver  # noqa: E402

SHAPES = {"C2": (384, 4096, 512, 64), "C3": (1024, 512, 64, 8), "C5": (32768, 256, 32, 4)}
REPS = 5


def timed(fn, stream):
    """median over REPS of the interval between two events on `stream`, the handle's"""
    samples = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1))
    return float(np.median(samples))


def main(names):
    dev = torch.device("cuda:0")
    for name in names:
        B, m, n, tm = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(1)
        J = torch.randn((B, n, m), dtype=torch.float64, device=dev, generator=g)
        rx = torch.randn((B, m), dtype=torch.float64, device=dev, generator=g)
        At = torch.randn((B, tm, n), dtype=torch.float64, device=dev, generator=g)
        cx = torch.randn((B, tm), dtype=torch.float64, device=dev, generator=g)
        t = np.full(B, tm, dtype=np.int64)
        info = torch.zeros((B, 6), dtype=torch.int64, device=dev)          # the info records are asked for, as a driver would
        torch.cuda.synchronize()                    # the inputs are complete before another stream reads them
        stream = torch.cuda.Stream(device=dev)
        s = GNSolver(device=0, stream=stream.cuda_stream)
        try:
            A = (At.data_ptr(), n, n * tm, cx.data_ptr())
            Jr = (J.data_ptr(), m, m * n, rx.data_ptr())

            def pair():
                s.factor_constraints_batched_dev(B, m, n, tm, t, *A)
                s.solve_factored_batched_dev(B, m, n, tm, t, None, *Jr, *A, dinfo=info.data_ptr())
            s.solve_batched_ragged_dev(B, m, n, tm, t, *Jr, *A)
            whole = timed(pair, stream)
            print(f"{name} B={B} ({m}x{n}, t={tm}): whole pair {whole:.3f} ms")
            for share in (0.0, 0.1, 0.5, 1.0):
                flags = np.zeros(B, dtype=np.int64)
                flags[:int(round(share * B))] = 1
                ms = timed(lambda: s.solve_changed_batched_dev(B, m, n, tm, t, flags, *A, dinfo=info.data_ptr()), stream)
                assert s.jacobian_resolved() == int(flags.sum())
                print(f"{name} changed {int(share * 100):3d} %: {ms:.3f} ms  ({ms / whole:.2f} of the pair)")
        finally:
            s.close()


if __name__ == "__main__":
    main(sys.argv[1:] or list(SHAPES))
