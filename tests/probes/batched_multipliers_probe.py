"""Probe (not collected by pytest): the batched consumers of a solve against the per-problem loop they replace.  For C5, C3 and
C2: the batch's own solve, the per-problem loop of enlsip_gn_first_lagrange + enlsip_gn_second_lagrange (host round trip per
problem), and the batched first + second estimate on device buffers (wall clock around a synchronise, warmed up, best of
--reps).  At C2 also the batched gradient and second estimate as bytes/s, against enlsip_gn_measure_stream in this process.

    python tests/probes/batched_multipliers_probe.py [--reps 5] [--loop-max 2048]
"""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))

from enlsip_gn import GNSolver, SQRT_EPS  # noqa: E402

SHAPES = [  # name, batch, m, n, t
    ("C5", 8192, 256, 32, 4),
    ("C3", 1024, 512, 64, 8),
    ("C2", 384, 4096, 512, 64),
]


def best_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-max", type=int, default=2048, help="problems timed in the per-problem loop (scaled to the batch)")
    args = ap.parse_args()
    s = GNSolver(device=0)
    dev = torch.device("cuda:0")
    for name, B, m, n, t in SHAPES:
        g = torch.Generator(device=dev).manual_seed(3)
        J = torch.randn(B, n, m, device=dev, dtype=torch.float64, generator=g)
        rx = torch.randn(B, m, device=dev, dtype=torch.float64, generator=g)
        At = torch.randn(B, t, n, device=dev, dtype=torch.float64, generator=g)
        cx = torch.randn(B, t, device=dev, dtype=torch.float64, generator=g)
        p = torch.empty(B, n, device=dev, dtype=torch.float64)
        lam = torch.empty(B, t, device=dev, dtype=torch.float64)
        gres = torch.empty(B, device=dev, dtype=torch.float64)
        st = torch.empty(B, device=dev, dtype=torch.int32)
        grad = torch.empty(B, n, device=dev, dtype=torch.float64)

        def solve():
            s.solve_batched_dev(B, m, n, t, J.data_ptr(), m, m * n, rx.data_ptr(), At.data_ptr(), n, n * t, cx.data_ptr(),
                                dp=p.data_ptr())
        t_solve = best_ms(solve, args.reps)
        solve()
        torch.cuda.synchronize()
        P = p.cpu().numpy()

        def first():
            s.first_lagrange_batched_dev(0, B, lam.data_ptr(), dgrad_res=gres.data_ptr(), dstatus=st.data_ptr())

        def second():
            s.second_lagrange_batched_dev(0, B, p.data_ptr(), lam.data_ptr(), dstatus=st.data_ptr())
        t_first, t_second = best_ms(first, args.reps), best_ms(second, args.reps)
        form = s.consumer_form()
        # the per-problem loop: host buffers, one call (and one stream synchronisation) per problem and estimate
        L, h = s._lib, s._h
        lam_h, g_h = np.zeros(t), C.c_double(0.0)
        nl = min(B, args.loop_max)

        def loop():
            for k in range(nl):
                L.enlsip_gn_first_lagrange(h, k, None, None, SQRT_EPS, lam_h.ctypes.data_as(C.c_void_p), C.byref(g_h))
                L.enlsip_gn_second_lagrange(h, k, P[k].ctypes.data_as(C.c_void_p), None, SQRT_EPS,
                                            lam_h.ctypes.data_as(C.c_void_p))
        t_loop = best_ms(loop, max(1, args.reps // 2)) * B / nl
        t_both = t_first + t_second
        print(f"{name}: batch {B} m {m} n {n} t {t}  solve {t_solve:.3f} ms  batched first {t_first:.3f} + second {t_second:.3f}"
              f" = {t_both:.3f} ms (form {form})  per-problem loop {t_loop:.1f} ms (timed on {nl})  "
              f"loop/batched {t_loop / t_both:.0f}x  batched/solve {t_both / t_solve:.2f}")
        if name == "C2":
            def gradient():
                s.gradient_batched_dev(0, B, grad.data_ptr())
            t_grad = best_ms(gradient, args.reps)
            gb_grad = B * (m * n + m + n) * 8 / 1e9
            # second estimate: J and rx read, rx + J p written and read back, J1 (m x t) read
            gb_second = B * (m * n + 3 * m + m * t + n + 2 * t) * 8 / 1e9
            ceiling = s.measure_stream(1 << 30, 5)
            print(f"    C2 gradient {t_grad:.3f} ms {gb_grad / t_grad * 1e3:.0f} GB/s  second {t_second:.3f} ms "
                  f"{gb_second / t_second * 1e3:.0f} GB/s  stream ceiling {ceiling:.0f} GB/s  "
                  f"ratios {gb_grad / t_grad * 1e3 / ceiling:.2f} / {gb_second / t_second * 1e3 / ceiling:.2f}")
        del J, rx, At, cx
        torch.cuda.empty_cache()
    s.close()


if __name__ == "__main__":
    main()
