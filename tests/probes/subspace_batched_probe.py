"""Probe (not collected by pytest): the subspace branch of a whole resident batch in one call against the held three-call flow.

For C5, C3 and C2, on the same resident batch and in the same process, medians of 10 runs (wall clock around call + synchronise,
since the older route has host work in it), in two legs that differ in the previous iterate of every problem:
  kept    previous_alpha = 0.1 (below 0.2: the max of :1171-1174 does not apply; progress large, so no bad step): no dimA is raised,
          b, p1 and d are formed once;
  raised  previous_alpha = 0.5, previous_dimA = t: wherever the choice truncates dimA the max raises it again and the call forms
          b, p1 and d a second time, as the reference's call at :1253 does.
Per leg:
  (n) one enlsip_gn_subspace_direction_batched_dev call: dimension choice on the device;
  (l) the three enlsip_gn_resolve_batched_dev calls of the held flow alone, with the dimensions call (n) returned (in the raised
      leg that flow forms d once, with the final dimA: it does less than the reference's literal flow);
and in the kept leg, where the held flow around a host choice IS the reference's flow:
  (r) the whole older route: the three calls, the device-to-host copies of b, d and of the two diagonal sets
      (enlsip_gn_get_diagR_batched), and the host choice through enlsip_gn_determine_solving_dim.  The host choice is a ctypes
      call per problem and dimension and is mostly interpreter overhead: it is reported on its own, and the route without it too.
Every shape runs in a child process of its own under a time limit; the first failure ends the run.  One JSON file:

    python tests/probes/subspace_batched_probe.py [--out profiles/subspace_batched.json]

Kernel split of call (n) alone (5 calls of one leg, nothing else timed):

    rocprofv3 --kernel-trace --stats -d out -- python tests/probes/subspace_batched_probe.py --trace C2:kept
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
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": reps}


def one(name, trace=None):
    import numpy as np
    import torch
    from enlsip_gn import DIM_HOLD, FACTOR_J2, FACTOR_L11, GNSolver, determine_solving_dim
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
    info = torch.empty(batch, 6, device=dev, dtype=torch.int64)
    status = torch.empty(batch, device=dev, dtype=torch.int32)
    s.solve_batched_dev(batch, m, n, t, J.data_ptr(), m, m * n, rx.data_ptr(), At.data_ptr(), n, n * t, cx.data_ptr(), dp=p.data_ptr())
    torch.cuda.synchronize()
    n2 = n - t
    cx2 = (cx * cx).sum(1).cpu().numpy()
    rx2 = (rx * rx).sum(1).cpu().numpy()
    prevA, prevJ = t, n2 - 2
    legs = {"kept": (0.1, 10.0 * cx2, 10.0 * rx2), "raised": (0.5, 0.21 * cx2, 0.1 * rx2)}
    full_A = np.full(batch, t, dtype=np.int64)
    hold = np.full(batch, DIM_HOLD, dtype=np.int64)

    def new_call(prev):
        rc = s.subspace_direction_batched_dev(0, batch, prev, None, p.data_ptr(), b.data_ptr(), d.data_ptr(), info.data_ptr(), status.data_ptr())
        assert rc == 0

    if trace:
        alpha, cprog, rprog = legs[trace]
        prev = GNSolver.pack_subspace_prev(batch, prevA, prevJ, 0, alpha, cprog, rprog)
        for _ in range(5):
            new_call(prev)
        torch.cuda.synchronize()
        s.close()
        return

    def choose(prevd, rank, y, D, prog, alpha):
        out = np.empty(batch, dtype=np.int64)
        nrm = np.linalg.norm(y, axis=1)
        nprev = np.linalg.norm(y[:, :prevd], axis=1)
        for k in range(batch):
            out[k] = determine_solving_dim(prevd, rank, nrm[k], prog[k], nprev[k], D[k], y[k], alpha, False)
        return out

    res = {"batch": batch, "m": m, "n": n, "t": t, "d_bytes": 8 * m * batch, "legs": {}}
    for leg, (alpha, cprog, rprog) in legs.items():
        prev = GNSolver.pack_subspace_prev(batch, prevA, prevJ, 0, alpha, cprog, rprog)
        v = res["legs"][leg] = {"previous_alpha": alpha}
        v["n_one_call"] = timed(torch, lambda: new_call(prev), 10)
        inf = info.cpu().numpy()
        dimA, dimJ2 = inf[:, 3].copy(), inf[:, 4].copy()
        p_new = p.clone()
        v["distinct_pairs"] = len({(int(a), int(c)) for a, c in zip(dimA, dimJ2)})
        v["problems_with_dimA_below_t"] = int(np.count_nonzero(dimA < t))

        def three_calls():
            s.resolve_batched_dev(0, batch, full_A, hold, -1, 0, b.data_ptr(), 0)
            s.resolve_batched_dev(0, batch, dimA, hold, -1, 0, 0, d.data_ptr())
            s.resolve_batched_dev(0, batch, hold, dimJ2, -1, p.data_ptr(), 0, 0)

        v["l_three_calls"] = timed(torch, three_calls, 10)
        v["same_p_bits"] = bool(torch.equal(p, p_new))
        v["ratio_three_calls_over_one_call"] = v["l_three_calls"]["median_ms"] / v["n_one_call"]["median_ms"]
        if leg != "kept":
            continue
        parts = {"host_choice_ms": [], "copies_ms": []}
        chosen = {}

        def older_route():
            s.resolve_batched_dev(0, batch, full_A, hold, -1, 0, b.data_ptr(), 0)
            t0 = time.perf_counter()
            hb = b.cpu().numpy()
            DL = s.diagR_batched(FACTOR_L11, t, 0, batch)
            t1 = time.perf_counter()
            dA = choose(prevA, t, hb, DL, cprog, alpha)
            t2 = time.perf_counter()
            s.resolve_batched_dev(0, batch, dA, hold, -1, 0, 0, d.data_ptr())
            t3 = time.perf_counter()
            hd = d.cpu().numpy()
            DJ = s.diagR_batched(FACTOR_J2, n2, 0, batch)
            t4 = time.perf_counter()
            dJ = choose(prevJ, n2, hd, DJ, rprog, alpha)
            t5 = time.perf_counter()
            s.resolve_batched_dev(0, batch, hold, dJ, -1, p.data_ptr(), 0, 0)
            parts["copies_ms"].append(((t1 - t0) + (t4 - t3)) * 1e3)
            parts["host_choice_ms"].append(((t2 - t1) + (t5 - t4)) * 1e3)
            chosen["dimA"], chosen["dimJ2"] = dA, dJ

        v["r_older_route"] = timed(torch, older_route, 10)
        med = lambda x: sorted(x[1:])[len(x[1:]) // 2]
        v["r_copies_ms"] = med(parts["copies_ms"])
        v["r_host_choice_ms"] = med(parts["host_choice_ms"])
        v["r_without_host_choice_ms"] = v["r_older_route"]["median_ms"] - v["r_host_choice_ms"]
        v["same_dimensions_as_host_choice"] = bool(np.array_equal(dimA, chosen["dimA"]) and np.array_equal(dimJ2, chosen["dimJ2"]))
        v["ratio_older_route_without_host_choice_over_one_call"] = v["r_without_host_choice_ms"] / v["n_one_call"]["median_ms"]
    res["form"] = s.subspace_form()
    s.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "subspace_batched.json"))
    ap.add_argument("--one")
    ap.add_argument("--trace", help="SHAPE:LEG: five one-call runs of that leg and nothing else (for rocprofv3 --kernel-trace)")
    args = ap.parse_args()
    if args.trace:
        return one(*args.trace.split(":"))
    if args.one:
        return one(args.one)
    out = {"when": time.strftime("%Y-%m-%d"), "shapes": {}}
    for name, shape in SHAPES.items():
        r = subprocess.run([sys.executable, __file__, "--one", name], capture_output=True, text=True, timeout=shape[4])
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{name}: failed (exit {r.returncode}); stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            sys.exit(1)
        v = out["shapes"][name] = json.loads(line[0][7:])
        for leg, w in v["legs"].items():
            print(f"{name} {leg}: one call {w['n_one_call']['median_ms']:.3f} ms  three calls {w['l_three_calls']['median_ms']:.3f} ms  "
                  f"same p bits {w['same_p_bits']}  dimA below t {w['problems_with_dimA_below_t']}" +
                  (f"  older route {w['r_older_route']['median_ms']:.1f} ms (copies {w['r_copies_ms']:.2f} ms, host choice "
                   f"{w['r_host_choice_ms']:.1f} ms)  same dimensions {w['same_dimensions_as_host_choice']}" if "r_older_route" in w else ""))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
