"""Probe (not collected by pytest): ragged batches against a uniform batch at t_max and against "group by t" (one
solve_batched_dev call per distinct t), timed with HIP events on device buffers.  Prints one line per shape.

    python tests/probes/ragged_batch_probe.py [--reps 20]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))

from enlsip_gn import GNSolver  # noqa: E402

SHAPES = [  # name, batch, m, n, t_max, t_lo
    ("C5", 8192, 256, 32, 4, 1),
    ("C3", 1024, 512, 64, 8, 0),
    ("C2", 384, 4096, 512, 64, 48),
]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    s = GNSolver(device=0)
    dev = torch.device("cuda:0")
    for name, batch, m, n, t_max, t_lo in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        J = torch.randn(batch, n, m, device=dev, dtype=torch.float64, generator=g)
        rx = torch.randn(batch, m, device=dev, dtype=torch.float64, generator=g)
        At = torch.randn(batch, t_max, n, device=dev, dtype=torch.float64, generator=g)
        cx = torch.randn(batch, t_max, device=dev, dtype=torch.float64, generator=g)
        p = torch.empty(batch, n, device=dev, dtype=torch.float64)
        t = np.random.default_rng(2).integers(t_lo, t_max + 1, batch).astype(np.int64)
        ragged = lambda: s.solve_batched_ragged_dev(batch, m, n, t_max, t, J.data_ptr(), m, m * n, rx.data_ptr(), At.data_ptr(),
                                                    n, n * t_max, cx.data_ptr(), dp=p.data_ptr())
        uniform = lambda: s.solve_batched_dev(batch, m, n, t_max, J.data_ptr(), m, m * n, rx.data_ptr(), At.data_ptr(), n,
                                              n * t_max, cx.data_ptr(), dp=p.data_ptr())
        order = np.argsort(t, kind="stable")
        Jg, rxg, Atg, cxg = J[order].contiguous(), rx[order].contiguous(), At[order].contiguous(), cx[order].contiguous()
        groups = [(int(v), int(np.searchsorted(t[order], v)), int((t == v).sum())) for v in np.unique(t)]

        def grouped():
            for v, k0, cnt in groups:
                s.solve_batched_dev(cnt, m, n, v, Jg[k0].data_ptr(), m, m * n, rxg[k0].data_ptr(), Atg[k0].data_ptr(), n,
                                    n * t_max, cxg[k0].data_ptr(), dp=p[k0].data_ptr())
        tr, tu, tg = timed(ragged, args.reps), timed(uniform, args.reps), timed(grouped, args.reps)
        print(f"{name}: batch {batch} m {m} n {n} t in [{t_lo},{t_max}]  ragged {tr:.3f} ms  uniform(t_max) {tu:.3f} ms  "
              f"group-by-t {tg:.3f} ms ({len(groups)} calls)  ragged/uniform throughput {tu / tr:.2f}x  vs grouped {tg / tr:.2f}x")
        # per-stage split (HIP events between the stages; profiling adds stream bubbles, so only the shares are meaningful)
        s.set_profiling(True)
        for label, fn in (("ragged", ragged), ("uniform", uniform)):
            fn()
            torch.cuda.synchronize()
            st = s.stage_ms()
            print(f"    {label:8s} " + "  ".join(f"{k} {v:.3f}" for k, v in st.items()) + "  route " + ",".join(sorted(s.route())))
        s.set_profiling(False)
    s.close()


if __name__ == "__main__":
    main()
