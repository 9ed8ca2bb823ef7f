"""Probe (not collected by pytest): the penalty weights (src/enlsip_functions.jl:2238, :1545-1629) and the merit function (:1307-1340)
of a batch whose operands are in device buffers, each in two flows:
  weights (a) what the batched call replaces: the download of active_Ap, cx, w_old and K, the library's host routine in a loop,
              the upload of w and K;
          (b) one enlsip_gn_penalty_weights_batched_dev call (Euclidean norm, no scaling);
  merit   (a) the download of rx_new and cx_new plus a NumPy sum per problem;
          (b) one enlsip_gn_merit_batched_dev call.
Shapes: C5 (65536 problems, m = 256, n = 32, t = 4) and C3 (1024, m = 512, n = 64, t = 8), l = 2 n (NO BASELINE CONFIGURATION FIXES l:
AN ASSUMPTION of the probe, as in linesearch_setup_probe.py).  The host loop of flow (a) at C5 runs over the first 4096 problems and
is scaled to the batch (it is linear in it); the copies are those of the whole batch.  At C5 the wave form (l = 64) is also timed
against the general form on the same problems with one more constraint (l = 65, just outside the wave form's predicate).
Three runs of each flow, each the median of 5 calls after a warm-up; the JSON line holds the three medians, so that a difference
can be set against the run-to-run spread.  One JSON line per shape on stdout:

    python tests/probes/penalty_weights_probe.py [--out profiles/penalty_weights.json]

DESIGN.md section 5.10 holds the table.  No test asserts a time.
"""
import argparse
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
    from enlsip_gn import GNSolver, penalty_weight_update
    B, m, n, t = SHAPES[name]
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    s = GNSolver(device=0)
    res = {"shape": name, "batch": B, "m": m, "n": n, "t": t, "l_is_an_assumption": True, "runs": RUNS, "reps": REPS}
    rng = np.random.default_rng(11)

    def operands(l):
        g = torch.Generator(device=dev).manual_seed(11)
        rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device=dev, generator=g)
        active = np.zeros((B, t), dtype=np.int64)
        inactive = np.zeros((B, l), dtype=np.int64)
        for k in range(B):
            perm = rng.permutation(l) + 1
            active[k] = perm[:t]
            inactive[k, :l - t] = perm[t:]
        K = torch.sort(rnd(B, 4, l).abs() + 0.1, dim=1, descending=True).values.contiguous()
        return dict(l=l, active=active, inactive=inactive, w_old=rnd(B, l).abs() + 0.1, K=K, cx=rnd(B, l), Ap=rnd(B, t), rx=rnd(B, m),
                    sums=np.abs(rng.standard_normal((B, 3))) + 1.0, w=torch.zeros((B, l), dtype=torch.float64, device=dev))

    tk = np.full(B, t, dtype=np.int64)
    dimA = np.full(B, t // 2, dtype=np.int64)

    def batched(o):
        return s.penalty_weights_batched_dev(B, o["l"], t, tk, dimA, o["active"], 2, False, o["w_old"].data_ptr(), o["Ap"].data_ptr(), 0,
                                             o["cx"].data_ptr(), o["K"].data_ptr(), o["sums"], o["w"].data_ptr())

    def host_flow(o):
        Bl = min(B, LOOP_CAP)
        Ap, cx, w_old, K = o["Ap"].cpu().numpy(), o["cx"].cpu().numpy(), o["w_old"].cpu().numpy(), o["K"].cpu().numpy()
        w = np.empty_like(w_old)
        t0 = time.perf_counter()
        for k in range(Bl):
            w[k] = penalty_weight_update(w_old[k], o["active"][k], t, int(dimA[k]), 2, Ap[k], cx[k], K[k], *o["sums"][k])[0]
        host_flow.loop_ms = (time.perf_counter() - t0) * 1e3
        o["w"].copy_(torch.from_numpy(w))
        o["K"].copy_(torch.from_numpy(K))

    o = operands(2 * n)
    K0 = o["K"].clone()
    reset = lambda: o["K"].copy_(K0)
    a = []
    for _ in range(RUNS):                 # the loop is seconds long: one timed pass per run
        reset(); sync()
        t0 = time.perf_counter()
        host_flow(o)
        sync()
        total = (time.perf_counter() - t0) * 1e3
        a.append(total + host_flow.loop_ms * (B / min(B, LOOP_CAP) - 1.0))
    res["weights_host_flow_ms"] = a
    res["weights_one_call_ms"] = medians(lambda: batched(o), sync)
    res["weights_form"] = s.penalty_form()
    if name == "C5":
        o65 = operands(2 * n + 1)
        res["weights_general_form_l65_ms"] = medians(lambda: batched(o65), sync)
        res["weights_general_form"] = s.penalty_form()
        del o65

    ni = np.full(B, o["l"] - t, dtype=np.int64)

    def merit_dev():
        return s.merit_batched_dev(B, m, o["l"], t, tk, o["active"], o["inactive"], ni, o["rx"].data_ptr(), o["cx"].data_ptr(),
                                   o["w_old"].data_ptr())

    def merit_host():
        rx, cx, w = o["rx"].cpu().numpy(), o["cx"].cpu().numpy(), o["w_old"].cpu().numpy()
        rows = np.arange(B)[:, None]
        ca, wa = cx[rows, o["active"] - 1], w[rows, o["active"] - 1]
        idx = np.maximum(o["inactive"] - 1, 0)
        ci, wi = cx[rows, idx], w[rows, idx]
        mask = (o["inactive"] > 0) & (ci < 0.0)
        return 0.5 * ((rx * rx).sum(1) + (wa * ca * ca).sum(1) + np.where(mask, wi * ci * ci, 0.0).sum(1))

    psi_d, psi_h = merit_dev(), merit_host()
    assert np.allclose(psi_d, psi_h, rtol=1e-12), "the two merit flows disagree"
    res["merit_host_flow_ms"] = medians(merit_host, sync)
    res["merit_one_call_ms"] = medians(merit_dev, sync)
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
