"""Times enlsip_gn_termination_batched_dev against the flow it replaces, over the same problems:

    call      the batched call on the device buffers (J' rx, every sum, the decision), wall time of the call
    parent    J, rx, cx, x, x_prev, p, d_gn, lambda, w and the active slot come down, then the per-problem loop through the library's
              host routines (enlsip_gn_termination_sums, enlsip_gn_check_termination_criteria)

Shapes: the three of DESIGN.md section 5.12 (C5-like: batch 8192, n = 32, l = 8; C3-like: 1024, n = 64, l = 16; general: 256,
n = 128, l = 256) with the m of their workloads, and C2 (batch 384, m = 4096, n = 512) with l = 2 n, which is an ASSUMPTION: bench.py
fixes no l.  Median of 20 runs after 3 warm-ups (the parent flow of C2: --parent-runs).  With the call's time the probe prints the
bytes of J over it, next to enlsip_gn_measure_stream of the same process.  DESIGN.md section 5.13 holds the table.  No test asserts
a time.

    python tests/probes/termination_probe.py [--shapes C5,C3,G,C2] [--runs 20] [--parent-runs 20]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))

SHAPES = {"C5": (8192, 256, 32, 8), "C3": (1024, 512, 64, 16), "G": (256, 1024, 128, 256), "C2": (384, 4096, 512, 1024)}   # batch, m, n, l


def run(name, runs, parent_runs):
    import torch
    from enlsip_gn import GNSolver
    from enlsip_gn import termination as T
    B, m, n, l = SHAPES[name]
    t = min(l // 2, n)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device=dev, generator=g)
    d = dict(J=rnd(B, n * m), rx=rnd(B, m), cx_all=rnd(B, l).abs() + 0.1, x=rnd(B, n) + 2.0, x_prev=rnd(B, n) + 2.0, p=rnd(B, n),
             d_gn=rnd(B, n), lam=rnd(B, t).abs() + 0.5, cx_active=rnd(B, t) * 1e-7, diag_scale=rnd(B, t).abs() + 0.5, At=rnd(B, n * t),
             w=rnd(B, l).abs() * 0.01, grad=torch.zeros(B, n, dtype=torch.float64, device=dev))
    p = lambda nm: d[nm].data_ptr()
    bufs = T.TerminationBuffers(dJ=p("J"), drx=p("rx"), dcx_all=p("cx_all"), dx=p("x"), dx_prev=p("x_prev"), dp=p("p"), dd_gn=p("d_gn"),
                                dlambda=p("lam"), dcx_active=p("cx_active"), ddiag_scale=p("diag_scale"), dAt=p("At"), dw=p("w"),
                                dgrad=p("grad"))
    act = np.zeros((B, l), dtype=np.int64)
    ina = np.zeros((B, l), dtype=np.int64)
    act[:, :t] = np.arange(1, t + 1)
    ina[:, :l - t] = np.arange(t + 1, l + 1)
    states = (T.TermState * B)(*[T.make_state(code=1, grad_res=1e-9, nb_iter=3, delta_time=-1.0, q=0, t=t, l=l, dimJ2=n, psi0=1.0)] * B)
    tol = T.make_tol(100, 1e-10, 1e-5, 1e-3, 1e-4)
    s = GNSolver(device=0)
    out = {"shape": name, "batch": B, "m": m, "n": n, "l": l, "t": t}
    try:
        def call():
            return T.termination_raw(s, B, m, n, l, t, states, tol, act, ina, bufs, False)

        def parent():
            h = {k: v.cpu().numpy() for k, v in d.items() if k != "grad"}
            codes = np.zeros(B, dtype=np.int64)
            for k in range(B):
                sums, _ = T.termination_sums(J=h["J"][k].reshape(n, m).T, rx=h["rx"][k], cx_all=h["cx_all"][k], x=h["x"][k],
                                             x_prev=h["x_prev"][k], p=h["p"][k], d_gn=h["d_gn"][k], dimJ2=n, lam=h["lam"][k],
                                             cx_active=h["cx_active"][k], diag_scale=h["diag_scale"][k], At=h["At"][k].reshape(t, n).T,
                                             w=h["w"][k], active=act[k], inactive=ina[k], q=0, t=t, scaling=False, psi0=1.0)
                codes[k] = T.check_termination_criteria(states[k], sums, tol)
            return codes

        for label, fn, reps in (("call_ms", call, runs), ("parent_ms", parent, parent_runs)):
            ms = []
            for i in range(reps + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= 3:
                    ms.append((time.perf_counter() - t0) * 1e3)
            out[label] = round(statistics.median(ms), 3)
            out[label + "_min_max"] = [round(min(ms), 3), round(max(ms), 3)]
        out["form"] = T.termination_form(s)
        out["J_GB_per_s"] = round(B * m * n * 8 / (out["call_ms"] * 1e-3) / 1e9, 1)
        out["stream_GB_per_s"] = round(s.measure_stream(), 1)
    finally:
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C5,C3,G,C2")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--parent-runs", type=int, default=20)
    a = ap.parse_args()
    for name in a.shapes.split(","):
        print(json.dumps(run(name, a.runs, a.parent_runs)), flush=True)


if __name__ == "__main__":
    main()
