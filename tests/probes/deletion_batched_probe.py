"""Probe (not collected by pytest): the step between the stages of a batched update_working_set — the deletion test
(src/enlsip_functions.jl:574-603) and the removal of the row it names (:708-719) — timed alone, for a batch whose lambda, grad_res,
diag_scale, A' and cx are in device buffers, in two flows:
  (a) the device-form flow without the new call: lambda, grad_res and diag_scale come down, the host loop of
      working_set.update_working_set_batched runs the test and edits the host copies of A', cx and diag_scale per problem, and the
      padded A', cx and diag_scale go up again (one copy each: cheaper than a copy per changed slot);
  (b) one enlsip_gn_delete_constraints_batched_dev call.
Shapes: C5 (batch 8192, m = 256, n = 32, t = 4) and C3 (1024, n = 64, t = 8); m plays no part in the step.  Median of 20 runs after
3 warm-ups, wall clock around the flow and a device synchronisation; the buffers are reset from pristine device copies outside the
timed region.  Both flows must name the same rows.  One JSON line per shape on stdout:

    python tests/probes/deletion_batched_probe.py [--out profiles/deletion_batched.json]

DESIGN.md section 5.8 holds the table.  No test asserts a time.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))

SHAPES = {"C5": (8192, 256, 32, 4), "C3": (1024, 512, 64, 8)}      # name: batch, m, n, t
WARMUP, REPS = 3, 20


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": len(ms)}


def one(name):
    import numpy as np
    import torch
    from enlsip_gn import GNSolver, working_set as ws
    B, m, n, t = SHAPES[name]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    At0, cx0 = rng.standard_normal((B, t, n)), rng.standard_normal((B, t))
    lam0, ds0 = rng.standard_normal((B, t)), rng.uniform(0.5, 2.0, (B, t))
    gres0 = np.where(np.arange(B) % 2 == 0, 0.0, 1e-3)
    tk, q = np.full(B, t, dtype=np.int64), np.ones(B, dtype=np.int64)
    pristine = {nm: torch.from_numpy(a).to(dev) for nm, a in (("At", At0), ("cx", cx0), ("lam", lam0), ("ds", ds0), ("gres", gres0))}
    d = {nm: x.clone() for nm, x in pristine.items()}
    dsaved = torch.zeros((B, n + 3), dtype=torch.float64, device=dev)
    s = GNSolver(device=0)

    host = {}

    def reset():
        for nm in d:
            d[nm].copy_(pristine[nm])
        host["At"], host["cx"] = At0.copy(), cx0.copy()      # the host copies a host-side driver keeps: not part of the step
        torch.cuda.synchronize()

    def flow_a():
        lam, gres, ds = d["lam"].cpu().numpy(), d["gres"].cpu().numpy(), d["ds"].cpu().numpy()
        At, cx = host["At"], host["cx"]
        out = np.zeros(B, dtype=np.int64)
        for k in range(B):
            sk = ws.check_constraint_deletion(int(q[k]), At[k], lam[k], True, ds[k], float(gres[k]))
            out[k] = sk
            if sk:
                At[k] = np.concatenate([np.delete(At[k], sk - 1, axis=0), np.zeros((1, n))])
                cx[k] = np.append(np.delete(cx[k], sk - 1), 0.0)
                ds[k] = np.append(np.delete(ds[k], sk - 1), 1.0)
        d["At"].copy_(torch.from_numpy(At))
        d["cx"].copy_(torch.from_numpy(cx))
        d["ds"].copy_(torch.from_numpy(ds))
        return out

    def flow_b():
        return s.delete_constraints_batched_dev(B, n, t, tk, q, True, d["lam"].data_ptr(), d["ds"].data_ptr(), d["At"].data_ptr(), n,
                                                n * t, d["cx"].data_ptr(), dgrad_res=d["gres"].data_ptr(), dsaved=dsaved.data_ptr())

    res = {"shape": name, "batch": B, "m": m, "n": n, "t": t}
    rows = {}
    for label, fn in (("host_loop", flow_a), ("one_call", flow_b)):
        ms = []
        for i in range(WARMUP + REPS):
            reset()
            t0 = time.perf_counter()
            rows[label] = fn()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms.append((time.perf_counter() - t0) * 1e3)
        res[label] = stats(ms)
    assert np.array_equal(rows["host_loop"], rows["one_call"]), "the two flows name different rows"
    res["deleted"] = int(np.count_nonzero(rows["one_call"]))
    res["form"] = s.deletion_form()
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
