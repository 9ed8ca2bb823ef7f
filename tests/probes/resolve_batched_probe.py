"""Probe (not collected by pytest): the subspace re-solve of a whole resident batch, timed with HIP events on device buffers.

For C5, C3 and C2 it measures
  (a) the loop of enlsip_gn_resolve over the batch (the per-problem entry point: refactors, synchronises twice per problem),
  (b) one enlsip_gn_resolve_batched_dev call over the batch,
  (c) the three-call held flow (b; d with the chosen dimA; p with the chosen dimJ2),
  (q) the Q0' stage alone — HIP events around its launches inside the library (profiling on, enlsip_gn_get_resolve_q0_ms;
      summed over the pipelined halves) — against its byte floor 8 m n2 batch / (in-place stream rate of
      enlsip_gn_measure_stream on the same device); the whole held call (b, p1, d_temp, Q0', Qt') is recorded next to it.
Every shape runs in a child process of its own under a time limit; the first failure ends the run.  One JSON file:

    python tests/probes/resolve_batched_probe.py [--out profiles/resolve_batched.json]
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))

SHAPES = {  # name: batch, m, n, t, time limit (s)
    "C5": (8192, 256, 32, 4, 240),
    "C3": (1024, 512, 64, 8, 180),
    "C2": (384, 4096, 512, 64, 240),
}


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": reps}


def one(name, skip_loop=False):
    import numpy as np
    import torch
    from enlsip_gn import DIM_HOLD, GNSolver
    batch, m, n, t, _ = SHAPES[name]
    dev = torch.device("cuda:0")
    s = GNSolver(device=0)
    g = torch.Generator(device=dev).manual_seed(1)
    J = torch.randn(batch, n, m, device=dev, dtype=torch.float64, generator=g)
    rx = torch.randn(batch, m, device=dev, dtype=torch.float64, generator=g)
    At = torch.randn(batch, t, n, device=dev, dtype=torch.float64, generator=g)
    cx = torch.randn(batch, t, device=dev, dtype=torch.float64, generator=g)
    p = torch.empty(batch, n, device=dev, dtype=torch.float64)
    b = torch.empty(batch, t, device=dev, dtype=torch.float64)
    d = torch.empty(batch, m, device=dev, dtype=torch.float64)
    s.solve_batched_dev(batch, m, n, t, J.data_ptr(), m, m * n, rx.data_ptr(), At.data_ptr(), n, n * t, cx.data_ptr(), dp=p.data_ptr())
    torch.cuda.synchronize()
    n2 = n - t
    rng = np.random.default_rng(3)
    dimA = rng.integers(max(t - 2, 0), t + 1, batch).astype(np.int64)
    dimJ2 = rng.integers(max(n2 - 8, 1), n2 + 1, batch).astype(np.int64)
    full_A = np.full(batch, t, dtype=np.int64)
    hold = np.full(batch, DIM_HOLD, dtype=np.int64)
    hp, hb, hd = np.zeros(n), np.zeros(t), np.zeros(m)
    ptr = lambda a: a.ctypes.data

    def loop():
        for k in range(batch):
            s._lib.enlsip_gn_resolve(s._h, k, int(dimA[k]), int(dimJ2[k]), -1, ptr(hp), ptr(hb), ptr(hd))

    def batched():
        s.resolve_batched_dev(0, batch, dimA, dimJ2, -1, p.data_ptr(), b.data_ptr(), d.data_ptr())

    def held_one():
        s.resolve_batched_dev(0, batch, dimA, hold, -1, 0, b.data_ptr(), d.data_ptr())

    def held_flow():
        s.resolve_batched_dev(0, batch, full_A, hold, -1, 0, b.data_ptr(), 0)
        s.resolve_batched_dev(0, batch, dimA, hold, -1, 0, 0, d.data_ptr())
        s.resolve_batched_dev(0, batch, hold, dimJ2, -1, p.data_ptr(), 0, 0)

    res = {"batch": batch, "m": m, "n": n, "t": t, "form": None}
    res["b_batched"] = timed(torch, batched, 10)
    res["form"] = s.resolve_form()
    res["c_held_flow"] = timed(torch, held_flow, 10)
    res["q_held_call"] = timed(torch, held_one, 10)
    res["a_per_problem_loop"] = timed(torch, loop, 2) if not skip_loop else {"median_ms": float("nan")}
    stream = s.measure_stream(1 << 30, 5)
    bytes_q0 = 8.0 * m * n2 * batch
    res["stream_gbs"] = stream
    res["q0_bytes"] = bytes_q0
    res["q0_floor_ms"] = bytes_q0 / (stream * 1e9) * 1e3
    s.set_profiling(True)
    q0 = []
    for _ in range(11):
        held_one()
        q0.append(s.resolve_q0_ms())
    s.set_profiling(False)
    q0 = sorted(q0[1:])
    res["q0_stage"] = {"median_ms": q0[len(q0) // 2], "min_ms": q0[0], "max_ms": q0[-1], "reps": len(q0)}
    res["q0_rate_gbs"] = bytes_q0 / (res["q0_stage"]["median_ms"] * 1e-3) / 1e9
    res["q0_fraction_of_stream"] = res["q0_rate_gbs"] / stream
    res["ratio_a_over_b"] = res["a_per_problem_loop"]["median_ms"] / res["b_batched"]["median_ms"]
    res["ratio_c_over_2b"] = res["c_held_flow"]["median_ms"] / (2 * res["b_batched"]["median_ms"])
    s.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resolve_batched.json"))
    ap.add_argument("--one")
    ap.add_argument("--skip-loop", action="store_true", help="with --one: leave the per-problem loop out (kernel traces)")
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.skip_loop)
    out = {"when": time.strftime("%Y-%m-%d"), "shapes": {}}
    for name, shape in SHAPES.items():
        r = subprocess.run([sys.executable, __file__, "--one", name], capture_output=True, text=True, timeout=shape[4])
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{name}: failed (exit {r.returncode}); stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            sys.exit(1)
        out["shapes"][name] = json.loads(line[0][7:])
        v = out["shapes"][name]
        print(f"{name}: loop {v['a_per_problem_loop']['median_ms']:.1f} ms  batched {v['b_batched']['median_ms']:.3f} ms  held flow "
              f"{v['c_held_flow']['median_ms']:.3f} ms  held call {v['q_held_call']['median_ms']:.3f} ms  Q0' {v['q0_stage']['median_ms']:.3f} ms = {v['q0_rate_gbs']:.0f} GB/s, "
              f"{v['q0_fraction_of_stream']:.2f} of the stream rate {v['stream_gbs']:.0f} GB/s (floor {v['q0_floor_ms']:.3f} ms)")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
