"""Timing of enlsip_gn_hessian_points_batched_dev and enlsip_gn_hessian_sums_batched_dev at the shapes of C3 and C5 with 64 taken
problems.  Not collected by pytest.

    python tests/probes/hessian_sums_probe.py            both shapes, each in a child process under its own time limit
    python tests/probes/hessian_sums_probe.py NAME       one shape, in this process

Per shape, for one pair range of PAIRS pairs: the median (and the range) of 20 timed runs after 3 warm-ups of
  points   the points call (one launch, one synchronisation)
  sums     the sums call (records up, one launch, one synchronisation), and its rate counting (4 m + 4 l) * 8 bytes per pair
  torch    the same contraction as a torch expression on the same buffers (differences, products, a sum over m, the division;
           torch's own summation order), timed to a device synchronisation
  host     the flow the calls replace: F and G down to the host, enlsip_gn_hessian_sums per problem (the library's host routine,
           faster than a callback written in Python), Gamma up
and a check that sums and host give the same bytes.  The first child that fails or runs out of time ends the probe."""
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
SHAPES = {  # name: (taken problems, m, n, l, t, pairs per range)
    "C5": (64, 256, 32, 4, 4, 528), "C3": (64, 512, 64, 8, 8, 520)}
LIMIT = 240      # seconds per child


def median_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def one(name):
    import torch
    import __graft_entry__ as ge
    ge.build()
    from enlsip_gn import GNSolver
    from enlsip_gn import direction as D
    N, m, n, l, t, npairs = SHAPES[name]
    g = torch.Generator(device="cuda:0").manual_seed(1)
    rnd = lambda *s: torch.randn(s, dtype=torch.float64, device="cuda:0", generator=g)
    dx, drx, dlam = rnd(N, n), rnd(N, m), rnd(N, t)
    dF = rnd(N, npairs, 1, m) + 1e-6 * rnd(N, npairs, 4, m)
    dG = rnd(N, npairs, 1, l) + 1e-6 * rnd(N, npairs, 4, l)
    dX = torch.empty((N, npairs, 4, n), dtype=torch.float64, device="cuda:0")
    dGam = torch.zeros((N, n, n), dtype=torch.float64, device="cuda:0")
    active = np.tile(np.arange(1, l + 1, dtype=np.int64), (N, 1))
    ts = [t] * N
    torch.cuda.synchronize()
    s = GNSolver(device=0)
    points = lambda: D.hessian_points_dev(s, N, n, 0, npairs, dx.data_ptr(), dX.data_ptr())
    sums = lambda: D.hessian_sums_dev(s, N, m, n, l, t, 0, npairs, ts, active, None, dx.data_ptr(), dF.data_ptr(), drx.data_ptr(),
                                      dG.data_ptr(), dlam.data_ptr(), dGam.data_ptr(), n, n * n)
    eps = torch.clamp(dx.abs(), min=1.0) * float(np.finfo(np.float64).eps) ** (1.0 / 3.0)
    kj = torch.tensor([(k, j) for k in range(n) for j in range(k + 1)][:npairs], device="cuda:0")
    div = 4 * eps[:, kj[:, 1]] * eps[:, kj[:, 0]]

    def torch_expr():
        r = (((dF[:, :, 0] - dF[:, :, 1]) - dF[:, :, 2] + dF[:, :, 3]) * drx[:, None, :]).sum(-1) / div
        c = (((dG[:, :, 0] - dG[:, :, 1]) - dG[:, :, 2] + dG[:, :, 3]) * dlam[:, None, :]).sum(-1) / div
        out = r - c
        torch.cuda.synchronize()
        return out
    xh, rxh, lamh = dx.cpu().numpy(), drx.cpu().numpy(), dlam.cpu().numpy()

    def host():
        Fh, Gh = dF.cpu().numpy(), dG.cpu().numpy()
        Gam = np.zeros((N, n, n))
        for k in range(N):
            D.hessian_sums(xh[k], Fh[k], rxh[k], Gh[k], lamh[k], active[k], t, Gamma=Gam[k])
        up = torch.from_numpy(Gam).to("cuda:0")
        torch.cuda.synchronize()
        return Gam, up
    res = dict(shape=name, problems=N, m=m, n=n, l=l, t=t, pairs=npairs)
    for label, fn in (("points", points), ("sums", sums), ("torch", torch_expr), ("host", host)):
        med, lo, hi = median_ms(fn, reps=5 if label == "host" else 20, warm=1 if label == "host" else 3)
        res[label + "_ms"] = [round(v, 4) for v in (med, lo, hi)]
    res["sums_bytes"] = N * npairs * (4 * m + 4 * l) * 8
    res["sums_TB_per_s"] = round(res["sums_bytes"] / (res["sums_ms"][0] * 1e-3) / 1e12, 3)
    res["torch_TB_per_s"] = round(res["sums_bytes"] / (res["torch_ms"][0] * 1e-3) / 1e12, 3)
    res["points_bytes_written"] = N * npairs * 4 * n * 8
    sums()
    res["same_bytes_as_host"] = bool(dGam.cpu().numpy().tobytes() == host()[0].tobytes())
    s.close()
    print(json.dumps(res), flush=True)
    return 0 if res["same_bytes_as_host"] else 1


if __name__ == "__main__":
    if len(sys.argv) > 1:
        sys.exit(one(sys.argv[1]))
    for nm in SHAPES:
        rc = subprocess.run([sys.executable, __file__, nm], timeout=LIMIT).returncode
        if rc != 0:
            print(f"{nm}: exit {rc}; the probe stops here")
            sys.exit(rc)
