"""Probe (not collected by pytest): the set-up of the line search (src/enlsip_functions.jl:2226-2229, :2149-2178 and the sums of
:1561-1584 / :2269) for a batch whose p, A, cx, Jp and rx are in device buffers, in two flows:
  (a) the per-problem loop that was the only route: enlsip_gn_full_constraints_times per problem (A of the problem comes down to
      be staged up again by that call: it takes a host matrix), upper_bound_steplength on the host (the library's host routine), and a
      download of Jp and rx for three NumPy dot products per problem;
  (b) one enlsip_gn_linesearch_setup_batched_dev call.
Shapes: C5 (65536 problems, m = 256, n = 32), C3 (1024, m = 512, n = 64) and C2 (384 problems of m = 4096, n = 512, the batch at which
Jp is the 12.6 MB of DESIGN section 5.9).  l = 2 n with n inactive rows per problem: NO BASELINE CONFIGURATION FIXES l, THIS IS AN
ASSUMPTION of the probe.  Flow (a) at C5 runs over the first 4096 problems only and is scaled to the batch (it is linear in it).
Best of 5 after one warm-up, wall clock around the flow and a device synchronisation.  Both flows must name the same rows.  For C2
also the rate of the product over the bytes of A (batch * l * n * 8 / time of a call without the sums) next to
enlsip_gn_measure_stream in the same process.  One JSON line per shape on stdout:

    python tests/probes/linesearch_setup_probe.py [--out profiles/linesearch_setup.json]

DESIGN.md section 5.9 holds the table.  No test asserts a time.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))

SHAPES = {"C5": (65536, 256, 32), "C3": (1024, 512, 64), "C2": (384, 4096, 512)}      # name: batch, m, n
LOOP_CAP = 4096
REPS = 5


def best(fn, sync):
    ms = []
    for i in range(REPS + 1):
        t0 = time.perf_counter()
        out = fn()
        sync()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
    return min(ms), out


def one(name):
    import numpy as np
    import torch
    from enlsip_gn import GNSolver, upper_bound_steplength
    B, m, n = SHAPES[name]
    l = 2 * n
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device=dev, generator=g)
    dA, dp, dcx, dJp, drx = rnd(B, n, l), rnd(B, n), rnd(B, l), rnd(B, m), rnd(B, m)
    dAp = torch.zeros((B, l), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(11)
    inactive = np.zeros((B, l), dtype=np.int64)
    for k in range(B):
        inactive[k, :n] = np.sort(rng.permutation(l)[:n]) + 1
    n_inactive = np.full(B, n, dtype=np.int64)
    s = GNSolver(device=0)
    sync = torch.cuda.synchronize
    Bl = min(B, LOOP_CAP)

    def flow_a():
        A = dA[:Bl].cpu().numpy()
        p, cx = dp[:Bl].cpu().numpy(), dcx[:Bl].cpu().numpy()
        Jp, rx = dJp[:Bl].cpu().numpy(), drx[:Bl].cpu().numpy()
        alpha, index, sums = np.zeros(Bl), np.zeros(Bl, dtype=np.int64), np.zeros((Bl, 3))
        for k in range(Bl):
            Ap = s.full_constraints_times(A[k].T, p[k])
            alpha[k], index[k] = upper_bound_steplength(inactive[k], n, 0, cx[k], Ap)
            sums[k] = Jp[k] @ Jp[k], Jp[k] @ rx[k], rx[k] @ rx[k]
        return alpha, index, sums

    def flow_b(sums=True):
        return s.linesearch_setup_batched_dev(B, m, n, l, dp.data_ptr(), dA.data_ptr(), l, l * n, dcx.data_ptr(), inactive, n_inactive,
                                              dAp.data_ptr(), dJp=dJp.data_ptr() if sums else 0, drx=drx.data_ptr() if sums else 0)

    res = {"shape": name, "batch": B, "m": m, "n": n, "l": l, "l_is_an_assumption": True, "reps": REPS}
    ta, a = best(flow_a, sync)
    tb, b = best(flow_b, sync)
    assert np.array_equal(a[1], b[1][:Bl]), "the two flows name different rows"
    assert np.allclose(a[0], b[0][:Bl], rtol=1e-9) and np.allclose(a[2], b[2][:Bl], rtol=1e-9, atol=1e-9)
    res["loop_problems"] = Bl
    res["loop_ms_measured"] = ta
    res["loop_ms_for_batch"] = ta * B / Bl
    res["one_call_ms"] = tb
    res["form"] = s.linesearch_form()
    if name == "C2":
        tp, _ = best(lambda: flow_b(False), sync)
        res["no_sums_ms"] = tp
        res["product_GBps_over_A"] = B * l * n * 8 / (tp * 1e-3) / 1e9
        res["stream_GBps"] = s.measure_stream(1 << 30, 5)
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="C5,C3,C2")
    a = ap.parse_args()
    import torch      # before the library: see tests/conftest.py
    torch.zeros(1, device="cuda:0")
    out = []
    for name in a.shapes.split(","):
        out.append(one(name))
        print(json.dumps(out[-1]), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
