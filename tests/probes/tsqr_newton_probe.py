"""Timing probe of the Newton direction on a row shard (not collected by pytest): after a sharded solve of the C4 shard of DESIGN.md
section 7 (32768 rows, t = 16, one rank), the whole enlsip_gn_tsqr_newton_direction_dev call and its four stages under
ENLSIP_GN_NEWTON_WIDE=0 (the one-workgroup factorisation) and =1 (the device-wide one), for n2 = n - 16 in N2S.  Per figure: WARM
warm-up calls, RUNS timed calls, min and max in ms; the call's time is wall clock around a call that ends with a stream
synchronisation, the stage times are the library's HIP events of a profiled call.  The default threshold of gn_tsqr_newton.inc is the
smallest swept n2 from which the device-wide form's max lies below the one-workgroup form's min at that and every larger swept n2;
the probe prints it with the table, one JSON line.

One process; its GPU step runs under a time limit of its own (LIMIT_S seconds, SIGALRM).  Run it as
    timeout -k 10 900 python tests/probes/tsqr_newton_probe.py"""
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "enlsip.jl_amd", "python"))
sys.path.insert(0, ROOT)
import torch

WARM, RUNS = 3, 9
N2S = (64, 128, 256, 512, 1008)
M, T = 32768, 16
LIMIT_S = 600


def gpu_step():
    from enlsip_gn import GNSolver
    from enlsip_gn.tsqr import tsqr_solve_lib, tsqr_newton_direction_dev
    dev = torch.device("cuda", 0)
    res = {"box": torch.cuda.get_device_name(0), "shard": [M, "n2 + 16", T], "warmup": WARM, "runs": RUNS, "rows": []}
    for n2 in N2S:
        n = n2 + T
        gen = torch.Generator(device=dev).manual_seed(7 + n2)
        Jd = torch.randn((n, M), dtype=torch.float64, device=dev, generator=gen)            # column-major M x n
        rxd = torch.randn((M,), dtype=torch.float64, device=dev, generator=gen)
        At = torch.randn((T, n), dtype=torch.float64, device=dev, generator=gen)
        cx = torch.randn((T,), dtype=torch.float64, device=dev, generator=gen)
        S = torch.randn((n, n), dtype=torch.float64, device=dev, generator=gen)
        Gd = (0.3 * (S + S.T)).contiguous()       # ||Gamma|| ~ 0.6 sqrt(n) against lambda_min(J'J) ~ (sqrt(M) - sqrt(n))^2: positive definite
        pd = torch.zeros((n,), dtype=torch.float64, device=dev)
        st = torch.zeros((1,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        row = {"n2": n2}
        for wide in (0, 1):
            os.environ["ENLSIP_GN_NEWTON_WIDE"] = str(wide)          # read at handle creation
            s = GNSolver(device=0)
            sol = tsqr_solve_lib(s, Jd, rxd, At, cx)
            assert sol.n2 == n2, (sol.n2, n2)
            call = lambda: tsqr_newton_direction_dev(s, n, Gd, pd, st)
            for _ in range(WARM):
                call()
            assert int(st.cpu()[0]) == 0 and s.newton_form() == (2 if wide else (1 if n <= 64 else 0))
            ts = []
            for _ in range(RUNS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                ts.append((time.perf_counter() - t0) * 1e3)
            s.set_profiling(True)
            stages = []
            for _ in range(WARM + RUNS):
                call()
                stages.append(s.newton_stage_ms())
            s.set_profiling(False)
            stages = stages[WARM:]
            row["wide" if wide else "one_wg"] = {
                "call_ms": [min(ts), max(ts)],
                "stages_ms": {name: [min(x[i] for x in stages), max(x[i] for x in stages)]
                              for i, name in enumerate(("setup", "E", "W22_rhs", "chol_solves_p"))},
                "p_norm": float(torch.linalg.norm(pd).cpu()),
            }
            s.close()
        res["rows"].append(row)
    os.environ.pop("ENLSIP_GN_NEWTON_WIDE", None)
    wins = [r["wide"]["call_ms"][1] < r["one_wg"]["call_ms"][0] for r in res["rows"]]
    thr = None
    for i in range(len(wins)):
        if all(wins[i:]):
            thr = N2S[i]
            break
    res["threshold_n2"] = thr      # None: the device-wide form is not faster at any swept size (or not from some size upward)
    return res


def main():
    def expired(signum, frame):
        raise TimeoutError(f"the GPU step did not finish in {LIMIT_S} s")
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(LIMIT_S)
    try:
        res = gpu_step()
    finally:
        signal.alarm(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
