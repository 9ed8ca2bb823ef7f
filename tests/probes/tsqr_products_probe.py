"""Timing probe of the row-sharded products (not collected by pytest): one C4 shard (32768 x 1024, t = 16) at one rank and the
eight shards of the 262144 x 1024 matrix in sequence on one device.  Yardstick: enlsip_gn_gradient + enlsip_gn_jacobian_times
after enlsip_gn_solve on the same 32768 x 1024 matrix, and the stream ceiling of enlsip_gn_measure_stream on the same box.
Every figure: WARM warm-up calls, RUNS timed calls (wall clock around calls that end with a stream synchronisation), min / median /
max in ms and the achieved bytes/s over 8 m n per pass at the median.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "enlsip.jl_amd", "python"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

WARM, RUNS = 3, 9


def timed(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"min_ms": ts[0], "median_ms": ts[len(ts) // 2], "max_ms": ts[-1]}


def main():
    from enlsip_gn import GNSolver
    from enlsip_gn.tsqr import (tsqr_solve_lib, tsqr_products_lib, tsqr_first_lagrange_lib, tsqr_second_lagrange_lib,
                                hip_products_local, hip_products_combine, tsqr_products_msg_len)
    m, n, t, G = 32768, 1024, 16, 8
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(5)
    Jall = torch.randn((n, G * m), dtype=torch.float64, device=dev, generator=gen)          # column-major (G m) x n
    rxall = torch.randn((G * m,), dtype=torch.float64, device=dev, generator=gen)
    At = torch.randn((t, n), dtype=torch.float64, device=dev, generator=gen)
    cx = torch.randn((t,), dtype=torch.float64, device=dev, generator=gen)
    Jd = Jall[:, :m].contiguous()
    rxd = rxall[:m].contiguous()
    torch.cuda.synchronize()
    s = GNSolver(device=0)
    res = {"box": torch.cuda.get_device_name(0), "shape": [m, n, t], "warmup": WARM, "runs": RUNS}
    res["stream_ceiling_GBps"] = s.measure_stream()
    sol = tsqr_solve_lib(s, Jd, rxd, At, cx)
    p = sol.p
    Jp = torch.empty((m,), dtype=torch.float64, device=dev)
    pass_bytes = 8.0 * m * n

    def rate(r, passes):
        r["GBps"] = passes * pass_bytes / (r["median_ms"] * 1e-3) / 1e9
        r["of_ceiling"] = r["GBps"] / res["stream_ceiling_GBps"]
        return r

    res["products_p_null_one_pass"] = rate(timed(lambda: tsqr_products_lib(s, n, t, None)), 1)
    res["products_p_two_passes"] = rate(timed(lambda: tsqr_products_lib(s, n, t, p, Jp)), 2)
    res["first_lagrange_null"] = rate(timed(lambda: tsqr_first_lagrange_lib(s, n, t)), 1)
    res["second_lagrange"] = rate(timed(lambda: tsqr_second_lagrange_lib(s, n, t, p)), 2)
    # the exchange and combine alone: n + 3 doubles per rank, one rank (device copy) — a message that is already there
    L = tsqr_products_msg_len(n)
    msg = torch.zeros((L,), dtype=torch.float64, device=dev)
    hip_products_local(s, m, n, Jd.data_ptr(), m, rxd.data_ptr(), 0, 0, msg.data_ptr())
    res["combine_of_one_message"] = timed(lambda: hip_products_combine(s, 1, n, msg.data_ptr()))
    # the eight shards in sequence, read in place (ldj = 8 m)
    pd = torch.as_tensor(p, device=dev)
    msgs = torch.zeros((G, L), dtype=torch.float64, device=dev)
    Jpall = torch.empty((G * m,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def eight():
        for g in range(G):
            hip_products_local(s, m, n, Jall.data_ptr() + 8 * g * m, G * m, rxall.data_ptr() + 8 * g * m, pd.data_ptr(),
                               Jpall.data_ptr() + 8 * g * m, msgs[g].data_ptr())
        hip_products_combine(s, G, n, msgs.data_ptr())
    r = timed(eight)
    r["GBps"] = 2 * G * pass_bytes / (r["median_ms"] * 1e-3) / 1e9
    r["of_ceiling"] = r["GBps"] / res["stream_ceiling_GBps"]
    res["eight_shards_in_sequence_two_passes"] = r
    s.close()
    # yardstick: the one-GPU consumers after enlsip_gn_solve on the same shard as a whole problem
    y = GNSolver(device=0)
    Jh = np.asfortranarray(Jd.cpu().numpy().T)
    y.solve(Jh, rxd.cpu().numpy(), At.cpu().numpy(), cx.cpu().numpy())
    res["yardstick_gradient_k_gemv_t"] = rate(timed(lambda: y.gradient(n)), 1)
    res["yardstick_jacobian_times"] = rate(timed(lambda: y.jacobian_times(m, t, p)), 1)
    y.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
