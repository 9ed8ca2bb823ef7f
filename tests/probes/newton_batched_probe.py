"""Probe (not collected by pytest): the Newton direction of a whole resident batch, batched call against the per-problem loop.

For C2, C3 and C5 it measures, median of 7 timed calls after 2 warm-ups, wall time with a stream synchronisation:
  (a) the loop of enlsip_gn_newton_direction over the batch (the per-problem entry point: re-runs the constraint stage,
      recomputes J * F_A.Q, two m-deep products, two synchronisations per problem),
  (b) one enlsip_gn_newton_direction_batched_dev call over the batch,
  (s) the four stages of (b) — HIP events inside the library (profiling on, enlsip_gn_get_newton_stage_ms; summed over the
      pipelined halves): default b / p1 / d; E = F_A.Q' Gamma F_A.Q; sW22 and the right-hand side; Cholesky, solves and p.
      Stage E moves 4 * 8 n^2 bytes per problem (read and write once per side): its rate against the in-place stream rate of
      enlsip_gn_measure_stream on the same device.  Stage sW22 does n2^3 / 3 flops per problem in R'R: its rate against the FP64
      matrix-pipe rate measured by tests/microbench/mfma_f64_rate.hip (--mfma-tflops, default the 70 TF/s of profiles/r1_notes.md).
Every shape runs in a child process of its own under a time limit; the first failure ends the run.  One JSON file:

    python tests/probes/newton_batched_probe.py [--out profiles/newton_batched.json]
"""
import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))

SHAPES = {  # name: batch, m, n, t, time limit (s)
    "C5": (8192, 256, 32, 4, 300),
    "C3": (1024, 512, 64, 8, 240),
    "C2": (384, 4096, 512, 64, 420),
}
WARMUP, REPS = 2, 7


def wall(torch, fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": REPS}


def one(name, mfma_tflops):
    import numpy as np
    import torch
    from enlsip_gn import GNSolver
    batch, m, n, t, _ = SHAPES[name]
    dev = torch.device("cuda:0")
    s = GNSolver(device=0)
    g = torch.Generator(device=dev).manual_seed(1)
    J = torch.randn(batch, n, m, device=dev, dtype=torch.float64, generator=g)
    rx = torch.randn(batch, m, device=dev, dtype=torch.float64, generator=g)
    At = torch.randn(batch, t, n, device=dev, dtype=torch.float64, generator=g)
    cx = torch.randn(batch, t, device=dev, dtype=torch.float64, generator=g)
    p = torch.empty(batch, n, device=dev, dtype=torch.float64)
    st = torch.empty(batch, device=dev, dtype=torch.int32)
    s.solve_batched_dev(batch, m, n, t, J.data_ptr(), m, m * n, rx.data_ptr(), At.data_ptr(), n, n * t, cx.data_ptr(), dp=p.data_ptr())
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    S = rng.standard_normal((n, n))
    Gh = np.asfortranarray(0.3 * (S + S.T) + 0.03 * rng.standard_normal((n, n)))      # J'J ~ m I dominates: positive definite
    Gd = torch.from_numpy(np.ascontiguousarray(Gh.T)).to(dev).expand(batch, n, n).contiguous()
    hp = np.zeros(n)
    bad = C.c_int64(0)
    gptr, pptr = Gh.ctypes.data_as(C.c_void_p), hp.ctypes.data_as(C.c_void_p)

    def loop():
        for k in range(batch):
            rc = s._lib.enlsip_gn_newton_direction(s._h, k, gptr, n, pptr, C.byref(bad))
            assert rc == 0 and bad.value == 0, (k, rc, bad.value)

    def batched():
        rc = s.newton_direction_batched_dev(0, batch, Gd.data_ptr(), n, n * n, p.data_ptr(), st.data_ptr())
        assert rc == 0, rc

    n2 = n - t
    res = {"batch": batch, "m": m, "n": n, "t": t}
    res["b_batched"] = wall(torch, batched)
    res["form"] = s.newton_form()
    batched()
    p_b = p.cpu().numpy().copy()
    loop()
    res["last_problem_rel_diff"] = float(np.linalg.norm(p_b[batch - 1] - hp) / np.linalg.norm(hp))
    res["a_per_problem_loop"] = wall(torch, loop)
    res["ratio_a_over_b"] = res["a_per_problem_loop"]["median_ms"] / res["b_batched"]["median_ms"]
    s.set_profiling(True)
    rows = []
    for _ in range(WARMUP + REPS):
        batched()
        rows.append(s.newton_stage_ms())
    s.set_profiling(False)
    rows = np.array(rows[WARMUP:])
    med = np.median(rows, axis=0)
    res["stage_ms"] = dict(zip(("default_b_p1_d", "E", "sW22_rhs", "cholesky_solves_p"), [float(x) for x in med]))
    stream = s.measure_stream(1 << 30, 5)
    res["stream_gbs"] = stream
    res["E_bytes"] = 4.0 * 8.0 * n * n * batch
    res["E_rate_gbs"] = res["E_bytes"] / (med[1] * 1e-3) / 1e9
    res["E_fraction_of_stream"] = res["E_rate_gbs"] / stream
    res["sW22_flops"] = n2 ** 3 / 3.0 * batch
    res["sW22_tflops"] = res["sW22_flops"] / (med[2] * 1e-3) / 1e12
    res["mfma_f64_tflops"] = mfma_tflops
    res["sW22_fraction_of_mfma"] = res["sW22_tflops"] / mfma_tflops
    s.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "newton_batched.json"))
    ap.add_argument("--one")
    ap.add_argument("--shapes", default="C5,C3,C2")
    ap.add_argument("--mfma-tflops", type=float, default=70.0)
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.mfma_tflops)
    out = {"when": time.strftime("%Y-%m-%d"), "shapes": {}}
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        r = subprocess.run([sys.executable, __file__, "--one", name, "--mfma-tflops", str(args.mfma_tflops)],
                           capture_output=True, text=True, timeout=shape[4])
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{name}: failed (exit {r.returncode}); stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            sys.exit(1)
        v = out["shapes"][name] = json.loads(line[0][7:])
        sm = v["stage_ms"]
        print(f"{name}: loop {v['a_per_problem_loop']['median_ms']:.1f} ms  batched {v['b_batched']['median_ms']:.3f} ms  "
              f"(x{v['ratio_a_over_b']:.1f}, form {v['form']})  stages {sm['default_b_p1_d']:.3f} / {sm['E']:.3f} / {sm['sW22_rhs']:.3f} / "
              f"{sm['cholesky_solves_p']:.3f} ms  E {v['E_rate_gbs']:.0f} GB/s = {v['E_fraction_of_stream']:.2f} of stream "
              f"{v['stream_gbs']:.0f}  sW22 {v['sW22_tflops']:.2f} TF/s = {v['sW22_fraction_of_mfma']:.3f} of {v['mfma_f64_tflops']:.0f}")
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
