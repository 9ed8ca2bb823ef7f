"""Times enlsip_gn_add_constraints_batched_dev against the flow it replaces, over the same problems:

    call      the batched call on the device buffers (walk + rebuild of the padded slot), wall time of the call
    parent    cx comes down, the host walk per problem (the library's host routine, so that the walk itself is not a Python loop),
              GNSolver.pack_ragged of the scaled active rows, cx and diag_scale, and their upload

Shapes: C5-like (batch 8192, n = 32, t = 4, l = 2 t) and C3-like (1024, n = 64, t = 8, l = 2 t), both wave form, and one general
form shape (256, n = 128, l = 256).  Median of 20 runs after 3 warm-ups.  DESIGN.md section 5.12 holds the table.  No test asserts
a time.

    python tests/probes/add_constraints_probe.py [--shapes C5,C3,G] [--runs 20]
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

SHAPES = {"C5": (8192, 32, 8), "C3": (1024, 64, 16), "G": (256, 128, 256)}      # name: batch, n, l


def problems(B, n, l, seed):
    rng = np.random.default_rng(seed)
    t0 = min(l // 2, n)
    t = np.full(B, t0, dtype=np.int64)
    q = np.zeros(B, dtype=np.int64)
    act, ina = np.zeros((B, l), dtype=np.int64), np.zeros((B, l), dtype=np.int64)
    for k in range(B):
        a = np.sort(rng.choice(np.arange(1, l + 1), size=t0, replace=False))
        act[k, :t0] = a
        ina[k, :l - t0] = np.setdiff1d(np.arange(1, l + 1), a)
    cx = rng.standard_normal((B, l)) + 0.5
    A = rng.standard_normal((B, n, l))      # problem k column-major l x n
    return q, t, act, ina, np.zeros(B, dtype=np.int64), cx, A


def run(name, runs):
    import torch
    from enlsip_gn import GNSolver, evaluate_violated_constraints, gather_active_constraints
    B, n, l = SHAPES[name]
    t_max = min(l, max(l // 2, min(l, n)))
    q, t, act, ina, iau, cx, A = problems(B, n, l, 1)
    dev = torch.device("cuda:0")
    dA, dcxa = torch.from_numpy(A).to(dev), torch.from_numpy(cx).to(dev)
    dAt = torch.zeros((B, n * t_max), dtype=torch.float64, device=dev)
    dcx, dds = (torch.zeros((B, t_max), dtype=torch.float64, device=dev) for _ in range(2))
    s = GNSolver(device=0)
    out = {"shape": name, "batch": B, "n": n, "l": l, "t_max": t_max}
    try:
        def call():
            return s.add_constraints_batched_dev(B, n, l, t_max, q, t, act, ina, iau, True, dA.data_ptr(), l, l * n, dcxa.data_ptr(),
                                                 dAt.data_ptr(), n, n * t_max, dcx.data_ptr(), dds.data_ptr())

        def parent():
            cxh = dcxa.cpu().numpy()
            As, cs, dss = [], [], []
            for k in range(B):
                tk, a, _, _, _ = evaluate_violated_constraints(l, n, int(q[k]), int(t[k]), act[k], ina[k], cxh[k], int(iau[k]))
                At, ca, ds = gather_active_constraints(a, tk, A[k].T, cxh[k], True)
                As.append(At); cs.append(ca); dss.append(ds)
            At_h, cx_h, _ = GNSolver.pack_ragged(As, cs, n=n)
            ds_h = np.ones((B, max(At_h.shape[1], 1)))
            for k, d in enumerate(dss):
                ds_h[k, :d.size] = d
            up = [torch.from_numpy(x).to(dev) for x in (At_h, cx_h, ds_h)]
            torch.cuda.synchronize()
            return up

        for label, fn in (("call_ms", call), ("parent_ms", parent)):
            ms = []
            for i in range(runs + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= 3:
                    ms.append((time.perf_counter() - t0) * 1e3)
            out[label] = round(statistics.median(ms), 3)
            out[label + "_min_max"] = [round(min(ms), 3), round(max(ms), 3)]
        out["form"] = s.addition_form()
    finally:
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C5,C3,G")
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    for name in a.shapes.split(","):
        print(json.dumps(run(name, a.runs)), flush=True)


if __name__ == "__main__":
    main()
