"""Probe (not collected by pytest): the polynomial fit of the line search (src/enlsip_functions.jl:1665-1689, :1986-1998, :1841-1862,
:2023-2026) of a batch whose operands are in device buffers, in two flows:
  (a) what the batched call replaces: the download of the seven vectors (rx, rx_new, Jp, cx, cx_new, Ap, w: 3 m + 4 l doubles per
      problem) and the library's host routines (enlsip_gn_linesearch_coefficients, enlsip_gn_linesearch_fit) in a loop;
  (b) one enlsip_gn_linesearch_fit_batched_dev call, without and with psi_new.
Inside (b) two shares are reported: the call with no problem taken (the records are still packed, uploaded and the kernels
launched, but no sum is formed and the scalar stage does not run: the floor that packing and the copies set), and the host scalar
stage as a loop of enlsip_gn_linesearch_fit over the returned sums (an UPPER bound: every iteration pays a foreign-function call).
Shapes: C5 (65536 problems, m = 256, n = 32, t = 4) and C3 (1024, m = 512, n = 64, t = 8), l = 2 n (NO BASELINE CONFIGURATION FIXES l:
AN ASSUMPTION of the probe, as in penalty_weights_probe.py).  The host loops at C5 run over the first 4096 problems and are scaled
to the batch (they are linear in it); the copies are those of the whole batch.  Three runs of each flow, each the median of 5 calls
after a warm-up, wall clock with a synchronisation; the JSON line holds the three medians, so that a difference can be set against
the run-to-run spread.  One JSON line per shape on stdout:

    python tests/probes/linesearch_fit_probe.py [--out profiles/linesearch_fit.json]

DESIGN.md section 5.11 holds the table.  No test asserts a time.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))

SHAPES = {"C5": (65536, 256, 32, 4), "C3": (1024, 512, 64, 8)}      # name: batch, m, n, t
LOOP_CAP = 4096
RUNS, REPS = 3, 5


def medians(fn, sync):
    out = []
    for _ in range(RUNS):
        ms = []
        for i in range(REPS + 1):
            t0 = time.perf_counter()
            fn()
            sync()
            if i:
                ms.append((time.perf_counter() - t0) * 1e3)
        out.append(statistics.median(ms))
    return out


def one(name):
    import numpy as np
    import torch
    import enlsip_gn._lib as Lm
    from enlsip_gn import GNSolver, linesearch_coefficients, linesearch_fit
    B, m, n, t = SHAPES[name]
    l = 2 * n
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    s = GNSolver(device=0)
    res = {"shape": name, "batch": B, "m": m, "n": n, "t": t, "l": l, "l_is_an_assumption": True, "runs": RUNS, "reps": REPS}
    rng = np.random.default_rng(11)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device=dev, generator=g)
    active = np.zeros((B, t), dtype=np.int64)
    inactive = np.zeros((B, l), dtype=np.int64)
    for k in range(B):
        perm = rng.permutation(l) + 1
        active[k] = perm[:t]
        inactive[k, :l - t] = perm[t:]
    alpha = np.full(B, 0.5)
    o = dict(rx=rnd(B, m), Jp=rnd(B, m), cx=rnd(B, l), Ap=rnd(B, l), w=rnd(B, l).abs() + 0.1)
    o["rx_new"] = o["rx"] + 0.5 * o["Jp"] + 0.25 * rnd(B, m)
    o["cx_new"] = o["cx"] + 0.5 * o["Ap"] + 0.25 * rnd(B, l)
    sync()
    tk = np.full(B, t, dtype=np.int64)
    ni = np.full(B, l - t, dtype=np.int64)
    a_min, a_max = np.full(B, 1e-3), np.full(B, 3.0)
    names = ("rx", "rx_new", "Jp", "cx", "cx_new", "Ap", "w")

    def batched(psi, take=None):
        return s.linesearch_fit_batched_dev(B, m, l, t, tk, active, inactive, ni, alpha, alpha, a_min, a_max,
                                            *[o[k].data_ptr() for k in names], take=take, psi=psi)

    Bl = min(B, LOOP_CAP)

    def host_flow():
        h = {k: o[k].cpu().numpy() for k in names}
        t0 = time.perf_counter()
        for k in range(Bl):
            sums = linesearch_coefficients(active[k], t, inactive[k], l - t, h["rx"][k], h["rx_new"][k], h["Jp"][k], h["cx"][k],
                                           h["cx_new"][k], h["Ap"][k], h["w"][k], alpha[k])
            linesearch_fit(sums, alpha[k], alpha[k], a_min[k], a_max[k])
        host_flow.loop_ms = (time.perf_counter() - t0) * 1e3

    a = []
    for _ in range(RUNS):                 # the loop is long: one timed pass per run
        sync()
        t0 = time.perf_counter()
        host_flow()
        sync()
        total = (time.perf_counter() - t0) * 1e3
        a.append(total + host_flow.loop_ms * (B / Bl - 1.0))
    res["host_flow_ms"] = a
    res["one_call_ms"] = medians(lambda: batched(False), sync)
    res["one_call_with_psi_ms"] = medians(lambda: batched(True), sync)
    res["one_call_nothing_taken_ms"] = medians(lambda: batched(False, take=np.zeros(B, dtype=np.int64)), sync)
    sums = batched(False)[0]
    L = Lm.load()
    out, arm = np.zeros(6), C.c_int(0)
    po = out.ctypes.data_as(C.c_void_p)

    def scalar_stage():
        for k in range(Bl):
            L.enlsip_gn_linesearch_fit(sums[k].ctypes.data_as(C.c_void_p), 0.5, 0.5, 1e-3, 3.0, po, C.byref(arm))

    res["scalar_stage_loop_upper_bound_ms"] = [v * (B / Bl) for v in medians(scalar_stage, lambda: None)]
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="C5,C3")
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
