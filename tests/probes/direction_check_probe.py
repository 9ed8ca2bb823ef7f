"""Timing of enlsip_gn_direction_check_batched_dev against the flow it replaces.  Not collected by pytest.

    python tests/probes/direction_check_probe.py            every shape, each in a child process under its own time limit
    python tests/probes/direction_check_probe.py NAME       one shape, in this process

Per shape: the median (and the range) of 20 timed runs after 3 warm-ups of
  call     the batched call: records up, one launch, sums down, the decisions on the host
  parent   the parent flow: b, d, lambda, diag_scale and cx down to the host (one synchronising copy each), the sums of the whole
           batch by vectorised NumPy, then the per-problem loop through the library's host routine enlsip_gn_check_gn_direction
and a check that both give the same codes (the data keep every comparison far from its threshold, so the summation order of the
parent's NumPy sums decides nothing).  The first child that fails or runs out of time ends the probe."""
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
SHAPES = {  # name: (batch, m, n, l, t), the shapes of DESIGN.md 5.13; l = 2 n at C2 is an assumption, bench.py fixes no l
    "C5-like": (8192, 256, 32, 8, 4), "C3-like": (1024, 512, 64, 16, 8), "general": (256, 1024, 128, 256, 128),
    "C2": (384, 4096, 512, 1024, 512)}
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
    B, m, n, l, t = SHAPES[name]
    rng = np.random.default_rng(0)
    host = dict(b=rng.standard_normal((B, t)), d=rng.standard_normal((B, m)), lam=rng.standard_normal((B, t)),
                diag_scale=rng.random((B, t)) + 0.5, cx_all=rng.standard_normal((B, l)))
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in host.items()}
    active = np.tile(np.concatenate([np.arange(1, t + 1), np.zeros(l - t, dtype=np.int64)]), (B, 1))
    inactive = np.tile(np.concatenate([np.arange(t + 1, l + 1), np.zeros(t, dtype=np.int64)]), (B, 1))
    fields = [dict(iter_number=3, q=t // 2, t=t, l=l, rankA=t, dimA=t, dimJ2=n - t, prev_code=(1, -1, 2)[k % 3], prev_dimJ2=n - t,
                   prev_t=t, prev_beta=1.0, prev_progress=1.0, prev_predicted_reduction=1.0, prev_alpha=1.0) for k in range(B)]
    states = (D.DirState * B)(*[D.make_state(**f) for f in fields])
    one_state = [D.make_state(**f) for f in fields]
    s = GNSolver(device=0)
    out = [None]

    def call():
        out[0] = s.direction_check_batched_dev(B, m, n, l, t, states, active, inactive, False, dev["b"].data_ptr(), dev["d"].data_ptr(),
                                               dev["lam"].data_ptr(), dev["diag_scale"].data_ptr(), dev["cx_all"].data_ptr())

    codes = np.zeros(B, dtype=np.int64)

    rec = np.zeros(B, dtype=D.SUMS_DTYPE)

    def parent():
        h = {k: v.cpu().numpy() for k, v in dev.items()}
        sq = h["d"] * h["d"]
        rec["b1_sq"] = np.einsum("ij,ij->i", h["b"], h["b"])              # dimA = t
        rec["d_sq"], rec["d1_sq"], rec["d1_asprev_sq"] = sq.sum(1), sq[:, :n - t].sum(1), sq[:, :n - t - 1].sum(1)
        rec["active_c_sum"] = (h["cx_all"][:, :t] ** 2).sum(1)          # active = 1..t
        q = t // 2
        rec["n_lm_ge"] = (h["lam"][:, q:] * h["diag_scale"][:, q:] >= -1.4901161193847656e-08).sum(1)
        rec["n_lm_neg"] = (h["lam"][:, q:] < 0).sum(1)
        rec["n_inactive_lt_delta"] = (h["cx_all"][:, t:] < 0.1).sum(1)
        for k in range(B):
            codes[k] = D.check_gn_direction(one_state[k], rec[k], m, n)[0]

    c = median_ms(call)
    p = median_ms(parent)
    assert np.array_equal(out[0].method_code, codes)
    down = sum(v.nbytes for v in host.values())
    print(f"{name}: batch {B} m {m} n {n} l {l} t {t} form {s.direction_form()}  call {c[0]:.3f} ms ({c[1]:.3f}-{c[2]:.3f})  "
          f"parent {p[0]:.2f} ms ({p[1]:.2f}-{p[2]:.2f})  bytes down in the parent flow {down}", flush=True)
    s.close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        one(sys.argv[1])
    else:
        for name in SHAPES:
            r = subprocess.run([sys.executable, __file__, name], timeout=LIMIT)
            if r.returncode != 0:
                sys.exit(f"{name}: exit status {r.returncode}; nothing more is started")
