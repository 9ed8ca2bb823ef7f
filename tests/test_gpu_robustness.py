"""Robustness of the HIP path (GPU): one handle reused across random shapes with degenerate / non-finite inputs (two GPU memory
faults were found this way, profiles/r1_notes.md), and padded leading dimensions / strides on the device entry.  Longer versions:
tests/probes/stress_reuse.py, tests/probes/ld_padding.py, tests/probes/stress_pipelined.py, tests/probes/stress_tsqr.py."""
import os

import numpy as np
import pytest

from oracle import gn_oracle as go, synth

pytestmark = pytest.mark.gpu


def rel(a, b):
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


@pytest.mark.parametrize("seed", [3, 11])
def test_handle_reuse_with_degenerate_inputs(seed):
    from enlsip_gn import GNSolver, GNError, FACTOR_A, FACTOR_L11, FACTOR_J2
    rng = np.random.default_rng(seed)
    s = GNSolver(device=0)
    try:
        for k in range(90):
            cls = rng.integers(0, 4)
            if cls == 0: n = int(rng.integers(4, 65)); m = int(rng.integers(n, 600)); t = int(rng.integers(1, min(n, 60) + 1))
            elif cls == 1: n = int(rng.integers(65, 320)); m = int(rng.integers(n, 1500)); t = int(rng.integers(1, 64))
            elif cls == 2: n = int(rng.integers(320, 700)); m = int(rng.integers(300, 1600)); t = int(rng.integers(1, 64))
            else: n = int(rng.integers(100, 400)); m = int(rng.integers(n, 1200)); t = int(rng.integers(65, min(n, 200)))
            kind = ["full", "rankdefA", "zeroA", "nanA", "dupA", "nanJ", "infJ", "zeroJ"][int(rng.integers(0, 8))]
            J, rx, A, cx = (synth.make_rank_deficient_A if (kind == "rankdefA" and t >= 2) else synth.make_problem)(81000 + k, m, n, t)
            if kind == "zeroA": A[:] = 0.0
            if kind == "nanA": A[int(rng.integers(0, t)), int(rng.integers(0, n))] = np.nan
            if kind == "dupA" and t >= 3: A[1:] = A[0]
            if kind == "nanJ": J[int(rng.integers(0, m)), int(rng.integers(0, n))] = np.nan
            if kind == "infJ": J[int(rng.integers(0, m)), int(rng.integers(0, n))] = np.inf
            if kind == "zeroJ": J[:] = 0.0
            out = s.solve(J, rx, A, cx)
            assert out.p.shape == (n,) and 0 <= out.rankA <= min(n, t)
            if kind == "full" and k % 3 == 0:
                assert rel(out.p, go.gn_subproblem(J, rx, A, cx).p) <= 1e-9
            if k % 4 == 0:      # consumers of whatever the solve left resident: errors are fine, faults are not
                try:
                    for which, ln in ((FACTOR_A, n), (FACTOR_L11, t), (FACTOR_J2, m)):
                        fv = s.factor(which)
                        if fv.R.shape[0]:
                            fv.Qt_mul(np.ones(ln))
                    s.JQ1(m, n); s.gradient(n); s.first_lagrange(t, None, None); s.second_lagrange(t, out.p, None)
                    s.resolve(m, n, t, int(rng.integers(0, out.rankA + 1)), 0, -1)
                except GNError:
                    pass
    finally:
        s.close()


@pytest.mark.parametrize("B,m,n,t,pj,pa", [(2, 4096, 512, 64, 7, 3), (4, 256, 32, 4, 5, 1), (2, 700, 300, 100, 9, 2), (130, 300, 40, 6, 3, 1)])
def test_padded_leading_dimensions_and_strides(B, m, n, t, pj, pa):
    import torch
    from enlsip_gn import GNSolver, SQRT_EPS
    dev = torch.device("cuda", 0)
    ldj, ldat = m + pj, n + pa
    sJ, sAt = ldj * n + 11, ldat * t + 5
    probs = [synth.make_problem(98000 + k, m, n, t) for k in range(B)]
    Jbuf = torch.full((B * sJ,), float("nan"), dtype=torch.float64, device=dev)      # NaN in every gap: never to be read as data
    Abuf = torch.full((B * sAt,), float("nan"), dtype=torch.float64, device=dev)
    for k, (J, rx, A, cx) in enumerate(probs):
        Jp = np.full((n, ldj), np.nan); Jp[:, :m] = J.T
        Jbuf[k * sJ: k * sJ + ldj * n] = torch.tensor(Jp.ravel(), device=dev)
        Ap = np.full((t, ldat), np.nan); Ap[:, :n] = A
        Abuf[k * sAt: k * sAt + ldat * t] = torch.tensor(Ap.ravel(), device=dev)
    rx = torch.tensor(np.stack([p[1] for p in probs]), dtype=torch.float64, device=dev)
    cx = torch.tensor(np.stack([p[3] for p in probs]), dtype=torch.float64, device=dev)
    pout = torch.empty((B, n), dtype=torch.float64, device=dev)
    s = GNSolver(device=0)
    try:
        s.solve_batched_dev(B, m, n, t, Jbuf.data_ptr(), ldj, sJ, rx.data_ptr(), Abuf.data_ptr(), ldat, sAt, cx.data_ptr(), SQRT_EPS,
                            dp=pout.data_ptr())
        torch.cuda.synchronize()
    finally:
        s.close()
    P = pout.cpu().numpy()
    for k in (0, B - 1):
        assert rel(P[k], go.gn_subproblem(*probs[k]).p) <= 1e-10


@pytest.mark.gpu
def test_bench_two_rank_control_flow_rehearsal():
    """bench.py's N > 1 path (rendezvous, barriers, MAX over ranks, rank-0 JSON line) with two ranks sharing this box's one GPU:
    gloo instead of RCCL (which refuses two ranks on one device), everything else as the driver launches it."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ENLSIP_BENCH_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "32", "--cpu-budget", "0", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                  # rank 0 only
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak" and rec["results_check"]["finite_and_within_tolerance"]
    assert rec["results_check"]["problems_checked"] == 32 and rec["config"]["name"] == "C2"
    assert rec["metric"] == "GN subproblem solves/sec at (m=4096,n=512); achieved fraction of HBM roofline"
    assert rec["value"] > 0 and rec["cpu_baseline"] is None and rec["roofline"]["bound"] == "hbm"


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["C5", "C4"])
def test_bench_starts_its_own_ranks(config):
    """`python bench.py --gpus 2 --config ...` with no launcher around it: the script starts its two ranks itself (before it
    touches the GPU) and rank 0 prints the one line.  C5: the ranks own consecutive shards of problems; C4: the ranks own row
    blocks of ONE 262144 x 1024 problem and the library's TSQR collective runs over its caller-supplied transport (gloo through
    host memory here; RCCL when every rank has its own GPU)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ENLSIP_BENCH_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--config", config, "--steps", "2", "--warmup", "1",
           "--cpu-budget", "0", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2500:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["name"] == config and rec["results_check"]["finite_and_within_tolerance"]
    if config == "C5":
        assert rec["scaling"] == "weak" and rec["metric"].startswith("GN subproblem solves/sec at (m=256,n=32)")
        assert rec["results_check"]["problems_checked"] == 8192 and rec["roofline"]["bound"] == "hbm"
    else:
        assert rec["scaling"] == "strong" and rec["metric"].startswith("GN subproblem solves/sec at (m=262144,n=1024)")
        assert rec["results_check"]["rankJ2"] == 1024 and rec["roofline"]["bound"] == "mfma"
        assert rec["stage_ms"]["local"] > 0 and rec["stage_ms"]["combine"] > 0


@pytest.mark.gpu
def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain `bench.py` run prints the headline line only (no results check, roofline or CPU leg) and `--dump-outputs` writes
    what its last timed step returned: float64 arrays of the bench's own shapes, problem 0's p equal to the LAPACK oracle's."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B, m, n, t = 8, 4096, 512, 64
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2500:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["unit"] == "solves/s"
    assert rec["dtype"] == "f64" and rec["higher_is_better"] is True
    assert not {"results_check", "roofline", "cpu_baseline", "single_problem_latency_ms"} & set(rec)
    arrays = {name: np.load(tmp_path / f"{name}.npy") for name in ("p", "b", "d", "jpvtJ2")}
    assert {k: v.shape for k, v in arrays.items()} == {"p": (B, n), "b": (B, t), "d": (B, m), "jpvtJ2": (B, n)}
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in arrays.values())
    ref = go.gn_subproblem(*synth.make_problem(0, m, n, t))
    assert rel(arrays["p"][0], ref.p) <= 1e-11


@pytest.mark.gpu
def test_raw_abi_rejects_bad_arguments_without_touching_the_device():
    """LAPACK-style argument checks of the C ABI (include/enlsip_gn.h: < 0 = bad argument): null pointers, short leading
    dimensions, dimensions outside this build's limits, accessors before any solve and out-of-range problem indices must all
    come back as error codes with a message — never as a launch with those values."""
    import ctypes as C
    from enlsip_gn import GNSolver, SQRT_EPS
    import enlsip_gn._lib as L
    s = GNSolver(device=0)
    lib, h = s._lib, s._h
    fp = lambda a: a.ctypes.data_as(C.c_void_p)
    m, n, t = 40, 6, 2
    J, rx, A, cx = synth.make_problem(5, m, n, t)
    Jf = np.asfortranarray(J); At = np.asfortranarray(A.T)
    p, b, d = np.zeros(n), np.zeros(t), np.zeros(m)
    info = L.Info()
    jA, jL, jJ = np.zeros(t, np.int64), np.zeros(t, np.int64), np.zeros(n, np.int64)

    def solve(mm=m, nn=n, tt=t, Jp=fp(Jf), ldj=m, rxp=fp(rx), Atp=fp(At), ldat=n, cxp=fp(cx)):
        return lib.enlsip_gn_solve(h, mm, nn, tt, Jp, ldj, rxp, Atp, ldat, cxp, SQRT_EPS, -1, -1, fp(p), fp(b), fp(d),
                                   C.byref(info), fp(jA), fp(jL), fp(jJ))

    # accessors before any solve
    r, c = C.c_int64(0), C.c_int64(0)
    assert lib.enlsip_gn_factor_shape(h, 0, 0, C.byref(r), C.byref(c)) != 0
    assert lib.enlsip_gn_get_R(h, 2, 0, fp(np.zeros(36)), 6) != 0
    assert lib.enlsip_gn_resolve(h, 0, 1, 1, -1, fp(p), fp(b), fp(d)) != 0
    for bad in (dict(mm=0), dict(mm=-3), dict(nn=0), dict(nn=1025), dict(tt=-1), dict(tt=1025), dict(Jp=None), dict(ldj=m - 1),
                dict(rxp=None), dict(Atp=None), dict(cxp=None), dict(ldat=n - 1)):
        rc = solve(**bad)
        assert rc < 0, (bad, rc)
        assert lib.enlsip_gn_last_error(h)                      # a message, not an empty string
    # truncation dimensions beyond the triangular factors (they index LDS vectors and factor columns in the kernels)
    for dA, dJ in ((t + 1, -1), (-1, min(m, n) + 1), (10 ** 9, -1), (-1, 10 ** 9)):
        rc = lib.enlsip_gn_solve(h, m, n, t, fp(Jf), m, fp(rx), fp(At), n, fp(cx), SQRT_EPS, dA, dJ, fp(p), fp(b), fp(d),
                                 C.byref(info), fp(jA), fp(jL), fp(jJ))
        assert rc < 0 and b"override" in lib.enlsip_gn_last_error(h), (dA, dJ, rc)
    # a dimJ2 override between kp = min(m, n - rankA) and min(m, n) passes the host check and is clamped on the device
    rc = lib.enlsip_gn_solve(h, m, n, t, fp(Jf), m, fp(rx), fp(At), n, fp(cx), SQRT_EPS, -1, n, fp(p), fp(b), fp(d),
                             C.byref(info), fp(jA), fp(jL), fp(jJ))
    assert rc == 0 and info.dimJ2 == n - t
    assert solve() == 0                                         # and the handle still works
    ref = go.gn_subproblem(J, rx, A, cx)
    assert np.linalg.norm(p - ref.p) <= 1e-11 * np.linalg.norm(ref.p)
    # out-of-range problem index / factor id / dimensions on the resident factors
    assert lib.enlsip_gn_factor_shape(h, 0, 1, C.byref(r), C.byref(c)) != 0
    assert lib.enlsip_gn_factor_shape(h, 7, 0, C.byref(r), C.byref(c)) != 0
    assert lib.enlsip_gn_get_R(h, 2, 0, fp(np.zeros(36)), 1) != 0          # ldr < rows
    assert lib.enlsip_gn_get_R(h, 2, 0, None, 6) != 0
    assert lib.enlsip_gn_resolve(h, 0, t + 1, n - t, -1, fp(p), fp(b), fp(d)) != 0
    assert lib.enlsip_gn_resolve(h, 0, t, n - t + 1, -1, fp(p), fp(b), fp(d)) != 0
    assert lib.enlsip_gn_apply_qt(h, 2, 0, None) != 0
    assert solve() == 0
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_tsqr_driver_with_real_ranks_on_the_device(world):
    """The library's collective enlsip_gn_solve_tsqr (and the two-stage form behind enlsip_gn.tsqr.tsqr_solve) with real ranks:
    `world` processes, each with its own handle and row block on the GPU (tests/tsqr_rank_worker.py); on this one-GPU box the
    exchange runs over the caller-supplied transport (gloo through host memory — RCCL refuses two ranks on one device); every
    rank must reproduce the oracle's single solve."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(29540 + world), os.path.join(root, "tests", "tsqr_rank_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    assert out.stdout.count(" ok") == 2 * 3 * world and "FAIL" not in out.stdout


@pytest.mark.gpu
def test_tsqr_driver_with_real_ranks_on_degenerate_cases():
    """The message path (k_tsqr_pack / k_tsqr_unpack: a packed triangle and a message length taken from n, not n2) where something
    is degenerate, with two real ranks (tests/tsqr_rank_worker.py, TSQR_CASES=edges): a rank-deficient A, n2 == 0, shards of 8 and
    7 rows against n2 = 20, and a J2 whose stacked pivoted QR truncates — each through enlsip_gn_solve_tsqr and through
    tsqr_solve(scaled=True), checked as tests/test_gpu_tsqr_edges.py checks them."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    world = 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", "29548", os.path.join(root, "tests", "tsqr_rank_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, TSQR_CASES="edges"))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1500:]
    assert out.stdout.count(" ok") == 2 * 4 * world and "FAIL" not in out.stdout, out.stdout[-3000:]


@pytest.mark.gpu
def test_solve_tsqr_through_a_one_rank_rccl_communicator():
    """The RCCL leg of enlsip_gn_solve_tsqr on the one GPU there is: unique id, ncclCommInitRank with one rank, and the exchange
    itself as ncclAllGather on the handle's stream (an attached communicator is used even with one rank: a self-gather, so the
    hand-declared prototype, the ncclFloat64 constant and the element count meet RCCL here) — the handle reports which transport
    moved the message, and the result is checked against the oracle.  (More ranks need one GPU each: tests/tsqr_rank_worker.py with
    TSQR_BACKEND=nccl.)  Shapes: n2 = 89 and 300 (CAQR + blocked pivoted QR in the combine stage), n2 = 40 (the one-wave route)."""
    import ctypes as C
    import torch
    from enlsip_gn import GNSolver
    from enlsip_gn.tsqr import tsqr_solve_lib, tsqr_stage_ms, tsqr_transport
    s = GNSolver(device=0)
    try:
        ident = C.create_string_buffer(128)
        assert s._lib.enlsip_gn_tsqr_unique_id(ident) == 0
        s._chk(s._lib.enlsip_gn_tsqr_init_rccl(s._h, ident, 1, 0))
        dev = torch.device("cuda", 0)
        for (m, n, t) in [(5000, 96, 7), (3000, 300, 0), (700, 48, 8)]:
            J, rx, A, cx = synth.make_problem(7700 + m, m, n, t)
            ref = go.gn_subproblem(J, rx, A, cx)
            Jd = torch.tensor(np.ascontiguousarray(J.T), dtype=torch.float64, device=dev)
            rd = torch.tensor(rx, dtype=torch.float64, device=dev)
            Ad = torch.tensor(np.ascontiguousarray(A), dtype=torch.float64, device=dev) if t else None
            cd = torch.tensor(cx, dtype=torch.float64, device=dev) if t else None
            torch.cuda.synchronize()
            s.set_profiling(True)
            out = tsqr_solve_lib(s, Jd, rd, Ad, cd)
            s.set_profiling(False)
            assert rel(out.p, ref.p) <= 1e-11 and (out.rankA, out.rankJ2) == (ref.rankA, ref.rankJ2)
            assert np.array_equal(out.jpvtJ2, ref.jpvtJ2)
            assert abs(out.d_norm - np.linalg.norm(ref.d)) <= 1e-12 * np.linalg.norm(ref.d)
            ms = tsqr_stage_ms(s)
            assert ms["local"] > 0 and ms["combine"] > 0
            assert tsqr_transport(s) == "rccl"
        # back to no communicator: the same call is a device copy and says so
        s._chk(s._lib.enlsip_gn_tsqr_set_exchange(s._h, None, None, 1, 0))
        out2 = tsqr_solve_lib(s, Jd, rd, Ad, cd)
        assert tsqr_transport(s) == "none" and rel(out2.p, ref.p) <= 1e-11
    finally:
        s.close()


def _solver_with_env(**env):
    """A handle created under the given environment switches (they are read at enlsip_gn_create)."""
    from enlsip_gn import GNSolver
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return GNSolver(device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [1, 0])
@pytest.mark.parametrize("m,n,t", [(9000, 200, 8), (20000, 330, 0), (5000, 96, 3)])
def test_lookahead_sweep_matches_the_one_stream_sweep(m, n, t, pair):
    """Look-ahead forced (ENLSIP_GN_LOOKAHEAD=1) in the paired sweep (ENLSIP_GN_PAIR=1: the far update of a pair split over two
    streams with events between them) and in the plain sweep (ENLSIP_GN_PAIR=0: every panel's trailing updates split into the next
    panel's columns and the rest) against the oracle and against the same sweep on one stream: R0 and p must not depend on the
    schedule."""
    J, rx, A, cx = synth.make_problem(6100 + m + n, m, n, t)
    ref = go.gn_subproblem(J, rx, A, cx)
    outs = []
    for la in (1, 0):
        s = _solver_with_env(ENLSIP_GN_PAIR=pair, ENLSIP_GN_LOOKAHEAD=la)
        try:
            for _ in range(2):                  # twice on one handle: events and the second stream are reused
                out = s.solve(J, rx, A, cx)
            assert ("sweep_lookahead" in s.route()) == bool(la)
            outs.append(out)
        finally:
            s.close()
        assert rel(out.p, ref.p) <= 1e-11 and (out.rankA, out.rankJ2) == (ref.rankA, ref.rankJ2)
        assert np.array_equal(out.jpvtJ2, ref.jpvtJ2)
        assert abs(np.linalg.norm(out.d) - np.linalg.norm(ref.d)) <= 1e-12 * np.linalg.norm(ref.d)
    assert np.array_equal(outs[0].p, outs[1].p) and np.array_equal(outs[0].d, outs[1].d)     # same kernels on the same data: bit for bit


@pytest.mark.gpu
def test_blocked_qrcp_form_hints_never_change_a_result():
    """The blocked pivoted QR of R0 launches, per block id, only the forms of its select / factor kernel that the PREVIOUS solve of the
    same shape on the handle needed (run_qrcp_block, SbArgs::rows_stat).  Problems of one shape but very different block structure,
    one after the other on ONE handle — random (long blocks), graded spectrum (norm recomputations, short blocks), rank deficient J
    (the stage ends early), random again — so that every solve starts on hints that do not fit it: each must match the oracle and
    a fresh handle that has no hints (bit for bit: the same kernels run on the same numbers, only empty launches differ)."""
    from enlsip_gn import GNSolver
    m, n, t = 1500, 330, 30            # kp = 300: register forms for 448 / 256 / 128 rows all in use
    gens = [synth.make_problem, synth.make_graded_J, synth.make_rank_deficient_J, synth.make_problem, synth.make_graded_J]
    probs = [g(7700 + i, m, n, t) for i, g in enumerate(gens)]
    one = GNSolver(device=0)
    try:
        for i, (J, rx, A, cx) in enumerate(probs):
            ref = go.gn_subproblem(J, rx, A, cx)
            for _ in range(2):                       # the second time the hints DO fit
                out = one.solve(J, rx, A, cx)
                fresh = _solver_with_env(ENLSIP_GN_SB_FORM_HINTS=0)
                try:
                    base = fresh.solve(J, rx, A, cx)
                finally:
                    fresh.close()
                assert np.array_equal(out.p, base.p) and np.array_equal(out.jpvtJ2, base.jpvtJ2) and out.rankJ2 == base.rankJ2, i
                assert (out.rankA, out.rankJ2, out.code) == (ref.rankA, ref.rankJ2, ref.code), i
                r = ref.rankJ2
                assert np.array_equal(out.jpvtJ2[:r], ref.jpvtJ2[:r]), i
                assert rel(out.p, ref.p) <= (1e-9 if gens[i] is synth.make_problem else 1e-5), i
    finally:
        one.close()


def _half_graded_problem(pid, m, n, t, flat):
    """J whose first `flat` singular values are 1 and the rest fall by eight decades: the pivoted QR of R0 opens with long blocks
    (32 steps each) and ends in many short ones (norm recomputations)."""
    J0, rx, A, cx = synth.make_problem(pid, m, n, t)
    U, _ = np.linalg.qr(J0)
    V, _ = np.linalg.qr(synth.normal_stream(pid, 4, n * n).reshape((n, n), order="F"))
    sv = np.ones(n)
    sv[flat:] = 10.0 ** (-8.0 * np.arange(1, n - flat + 1) / (n - flat))
    return (U * sv) @ V.T, rx, A, cx


@pytest.mark.gpu
def test_blocked_qrcp_slow_start_after_a_long_hinted_chunk():
    """a solve with a fast start and a long tail of short blocks leaves (a) a large first chunk and (b) hints that
    suppress the 448 / 256-row forms from the fifth block id on; the NEXT solve of the shape starts slowly (graded from the first
    column: short blocks all the way), is still above 256 rows when the hints stop launching the large form, idles to the end of the
    hinted chunk and falls back.  Until round 5 the fall-back gated the forms on kp - (blocks launched), found 'at most 250 rows'
    and never launched the large form again: the loop ran out and the factors were assembled half done.  The forms are now gated on
    an upper bound of the real row counts (run_qrcp_block: rows_bound).  Bit for bit against a handle without hints, and the oracle."""
    from enlsip_gn import GNSolver
    m, n, t = 1500, 330, 30            # kp = 300
    fast_then_short = _half_graded_problem(7801, m, n, t, 170)
    slow = synth.make_graded_J(7802, m, n, t)
    one = GNSolver(device=0)
    try:
        for (J, rx, A, cx) in (fast_then_short, slow, fast_then_short, slow):
            ref = go.gn_subproblem(J, rx, A, cx)
            out = one.solve(J, rx, A, cx)
            fresh = _solver_with_env(ENLSIP_GN_SB_FORM_HINTS=0)
            try:
                base = fresh.solve(J, rx, A, cx)
            finally:
                fresh.close()
            assert np.array_equal(out.p, base.p) and np.array_equal(out.jpvtJ2, base.jpvtJ2) and out.rankJ2 == base.rankJ2
            assert (out.rankA, out.rankJ2, out.code) == (ref.rankA, ref.rankJ2, ref.code)
            r = ref.rankJ2
            assert np.array_equal(out.jpvtJ2[:r], ref.jpvtJ2[:r])
            assert rel(out.p, ref.p) <= 1e-5
    finally:
        one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,t", [(900, 640, 20), (1100, 1024, 0), (700, 600, 88)])
def test_hybrid_pivoted_qr_matches_the_launch_per_step_form(m, n, t):
    """More than 512 rows of R0: the stage opens with one launch per pivot step and hands the last 512 rows to the register
    blocks (run_qrcp_block, jhead); ENLSIP_GN_QRCP_HYBRID=0 keeps one launch per step to the end.  Same pivots, ranks and exit
    codes in both forms and in the oracle, on a random, a graded (norm recomputations, short blocks) and a rank-deficient J
    (the stage meets zero columns); kp = 620 / 1024 / 512 (the last one: no head at all, the hand-over offset is zero)."""
    from enlsip_gn import GNSolver
    for i, gen in enumerate([synth.make_problem, synth.make_graded_J, synth.make_rank_deficient_J]):
        J, rx, A, cx = gen(9100 + 7 * i + m, m, n, t)
        ref = go.gn_subproblem(J, rx, A, cx)
        outs = []
        for hyb in (1, 0):
            s = _solver_with_env(ENLSIP_GN_QRCP_HYBRID=hyb)
            try:
                outs.append(s.solve(J, rx, A, cx))
                if min(m, n - t) > 512:
                    assert ("pivot_hybrid" if hyb else "pivot_steps") in s.route()
            finally:
                s.close()
        a, b = outs
        assert (a.rankA, a.rankJ2, a.code) == (b.rankA, b.rankJ2, b.code) == (ref.rankA, ref.rankJ2, ref.code), (i, m, n, t)
        r = ref.rankJ2
        assert np.array_equal(a.jpvtJ2[:r], ref.jpvtJ2[:r]) and np.array_equal(b.jpvtJ2[:r], ref.jpvtJ2[:r]), (i, m, n, t)
        tol = 1e-9 if gen is synth.make_problem else 1e-5
        assert rel(a.p, ref.p) <= tol and rel(b.p, ref.p) <= tol, (i, rel(a.p, ref.p), rel(b.p, ref.p))
        assert rel(a.p, b.p) <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,t,batch", [(169, 124, 105, 5), (141, 126, 122, 2), (150, 128, 100, 3), (200, 96, 70, 4)])
def test_two_problem_waves_with_more_than_64_constraint_reflectors(m, n, t, batch):
    """Batches whose J2 is narrow (n2 + 1 <= 32: two problems per wave in the pivot + solve stage, k_pivot_small2) while Q1 has MORE
    THAN 64 reflectors (many active constraints, n <= 128): the side-by-side tail applies F_A.Q with all tau held in registers, one
    word per 32 reflectors — a build that kept two words served reflectors 64.. with the other half-wave's tau (found by
    tests/probes/fuzz_batched.py, seeds 61 / 62: ranks right, p wrong by 10-80 %).  Against the oracle, every problem of the batch."""
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    try:
        probs = [synth.make_problem(88000 + 17 * k + m, m, n, t) for k in range(batch)]
        refs = [go.gn_subproblem(J, rx, A, cx) for (J, rx, A, cx) in probs]
        p, b, d, infos, jA, jL, jJ = s.solve_batched(np.stack([np.ascontiguousarray(J.T) for (J, _, _, _) in probs]),
                                                     np.stack([rx for (_, rx, _, _) in probs]),
                                                     np.stack([np.ascontiguousarray(A) for (_, _, A, _) in probs]),
                                                     np.stack([cx for (_, _, _, cx) in probs]))
        for k, ref in enumerate(refs):
            assert (infos[k][0], infos[k][1], infos[k][2]) == (ref.rankA, ref.rankJ2, ref.code), k
            assert rel(p[k], ref.p) <= 1e-9, (k, rel(p[k], ref.p))
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("probe,count,seed", [("fuzz_batched", 16, 62), ("fuzz_batched", 16, 5), ("fuzz_batched", 16, 19),
                                              ("fuzz_gpu", 70, 71), ("fuzz_gpu", 70, 3), ("fuzz_gpu", 70, 29),
                                              ("fuzz_accessors", 20, 1), ("fuzz_accessors", 20, 2), ("fuzz_accessors", 20, 3),
                                              ("fuzz_tsqr", 5, 1), ("fuzz_tsqr", 5, 2), ("fuzz_tsqr", 5, 3),
                                              ("fuzz_magnitudes", 30, 1), ("fuzz_magnitudes", 30, 2), ("fuzz_magnitudes", 30, 3)])
def test_randomised_shapes_against_the_oracle(probe, count, seed, monkeypatch):
    """The randomised sweeps of tests/probes (mixed batches: full rank, rank-deficient A / J2, graded J2, zero A; single problems of
    every size class; the accessors and the re-solve on random shapes; row-sharded TSQR solves; random shapes at random power-of-two
    scales far outside the range of plain sums of squares: the rescale path) as part of the suite, three fixed seeds each — seed 62 of the batched sweep is the one that found the defect pinned by
    test_two_problem_waves_with_more_than_64_constraint_reflectors.  The shapes that cross every kernel-selection boundary are
    not left to chance: tests/test_dispatch_grid.py."""
    import importlib.util, pathlib, sys
    path = pathlib.Path(__file__).resolve().parent / "probes" / (probe + ".py")
    spec = importlib.util.spec_from_file_location("probe_" + probe, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", [str(path), str(count), str(seed)])
    assert mod.main() == 0


@pytest.mark.gpu
def test_fused_small_kernel_matches_the_two_launch_form():
    """One-tile problems with one narrow panel (C5's shape and neighbours): J*Q1 + panel in one launch (default) and as two launches
    (ENLSIP_GN_FUSE_SMALL=0) give the same factors, bit for bit — the fused kernel runs the same factorisation body on the same
    numbers — and both match the oracle; shapes outside the fused kernel's range (n2 = 32, m > 256) take the two-launch form."""
    import torch
    from enlsip_gn import workload as wl
    for (m, n, t, batch) in [(256, 32, 4, 64), (200, 30, 7, 40), (256, 32, 0, 16), (130, 17, 16, 33), (300, 32, 4, 8)]:
        J, rx, At, cx = wl.make_batch(4400 + m + n + t, batch, m, n, t, "cuda:0")
        res = []
        for fuse in (1, 0):
            s = _solver_with_env(ENLSIP_GN_FUSE_SMALL=fuse)
            try:
                p = torch.zeros((batch, n), dtype=torch.float64, device="cuda:0")
                d = torch.zeros((batch, m), dtype=torch.float64, device="cuda:0")
                jJ = torch.zeros((batch, n), dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                s.solve_batched_dev(batch, m, n, t, J.data_ptr(), m, m * n, rx.data_ptr(), At.data_ptr() if t else 0, max(n, 1), n * t,
                                    cx.data_ptr() if t else 0, dp=p.data_ptr(), dd=d.data_ptr(), djJ=jJ.data_ptr())
                res.append((p.cpu().numpy(), d.cpu().numpy(), jJ.cpu().numpy()))
            finally:
                s.close()
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        for k in (0, batch - 1):
            Jh = J[k].cpu().numpy().T
            ref = go.gn_subproblem(Jh, rx[k].cpu().numpy(), At[k].cpu().numpy().reshape(t, n), cx[k].cpu().numpy())
            assert rel(res[0][0][k], ref.p) <= 1e-11


@pytest.mark.gpu
def test_update_table_and_stream_ceiling():
    """Instrumentation of bench.py: the far-update launches one by one (SURVEY 8d bytes and HIP-event time; pairs: one launch per
    two panels) and the in-place stream measurement."""
    import torch
    from enlsip_gn import workload as wl
    m, n, t, batch = 2048, 256, 32, 96
    J, rx, At, cx = wl.make_batch(1234, batch, m, n, t, "cuda:0")
    p = torch.zeros((batch, n), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    for pair, launches in ((1, 4), (0, 7)):          # n2 = 224 = 7 full panels: pairs (0,1) (2,3) (4,5) + the seventh alone (d is its one trailing column)
        s = _solver_with_env(ENLSIP_GN_PAIR=pair)
        try:
            s.set_profiling(True, all_updates=True)
            s.solve_batched_dev(batch, m, n, t, J.data_ptr(), m, m * n, rx.data_ptr(), At.data_ptr(), n, n * t, cx.data_ptr(), dp=p.data_ptr())
            avg_ms, cnt, total = s.update_stats()
            table = s.update_table()
            assert cnt == len(table) == launches and avg_ms > 0
            assert abs(sum(b for b, _ in table) - total) <= 1e-9 * total and all(ms > 0 for _, ms in table)
            # all trailing-update launches: the far passes above + tree levels / second-panel columns; SURVEY 8d bytes of ALL
            # seven panels on every column right of them (the same number whichever way the sweep is launched)
            far_ms, other_ms, other_cnt, all_bytes = s.update_totals()
            mpad = 2048
            want = batch * sum(8.0 * (2.0 * (mpad - 32 * k) * (224 + 1 - 32 * (k + 1)) + (mpad - 32 * k) * 32 + 1024) for k in range(7))
            assert abs(all_bytes - want) <= 1e-9 * want
            assert abs(far_ms - avg_ms * cnt) <= 1e-3 * far_ms and other_ms > 0 and other_cnt > 0
            st = s.stage_ms()
            assert abs(st["update"] - (far_ms + other_ms)) <= 1e-3 * st["update"] and st["panel"] > 0
            if pair:
                gbs = s.measure_stream(1 << 28, 3)
                assert 1000.0 < gbs < 8000.0            # an MI355X streams 5-6 TB/s in place; anything else is a broken measurement
        finally:
            s.close()


def test_one_handle_regrowing_its_workspaces_matches_fresh_handles():
    """One handle through shapes that place the main workspace again (smaller, larger, smaller), use the distributed constraint
    workspace for the first time (t > 64 and n t > 8192) and run the shared staging layout after a larger shape: every output of
    every step is bit for bit that of a fresh handle given the same call."""
    from enlsip_gn import GNSolver

    def batch_inputs(seed, batch, m, n, t):
        ps = [synth.make_problem(seed + k, m, n, t) for k in range(batch)]
        J = np.ascontiguousarray(np.stack([np.asfortranarray(q[0]).T for q in ps]))                  # (batch, n, m): column-major m x n
        rx = np.stack([q[1] for q in ps])
        At = np.ascontiguousarray(np.stack([q[2].reshape(t, n) for q in ps])) if t else None         # (batch, t, n)
        cx = np.stack([q[3] for q in ps]) if t else None
        return J, rx, At, cx

    def flat(out):      # every output of a call as a list of arrays
        if isinstance(out, tuple):      # batched: jpvtJ2 of problem k is defined on its first n2 = n - rankA entries only
            p, b, d, infos, jA, jL, jJ = out
            jJ = jJ.copy()
            for k, info in enumerate(infos):
                jJ[k, jJ.shape[1] - info[0]:] = 0
            return [p, b, d, np.asarray(infos), jA, jL, jJ]
        return [out.p, out.b, out.d, np.array([out.rankA, out.rankJ2, out.code, out.dimA, out.dimJ2, out.status]), out.jpvtA, out.jpvtL,
                out.jpvtJ2]

    def factored(s):
        J, rx, A, cx = synth.make_problem(5150, 33, 32, 1)
        first = s.factor_constraints(33, A, cx)
        return [np.array(first)] + flat(s.solve_factored(J, rx, 1))

    steps = [lambda s: flat(s.solve_batched(*batch_inputs(5110, 3, 33, 32, 1))),
             lambda s: flat(s.solve_batched(*batch_inputs(5120, 2, 200, 128, 65))),
             lambda s: flat(s.solve_batched(*batch_inputs(5130, 2, 1056, 100, 0))),
             lambda s: flat(s.solve_batched(*batch_inputs(5110, 3, 33, 32, 1))),
             factored]
    reused = GNSolver(device=0)
    try:
        for i, step in enumerate(steps):
            got = step(reused)
            fresh = GNSolver(device=0)
            try:
                want = step(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want)
            for j, (a, b) in enumerate(zip(got, want)):
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), (i, j)
    finally:
        reused.close()
