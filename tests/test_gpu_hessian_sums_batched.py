"""The finite-difference Hessian sums of a batch on device buffers (enlsip_gn_hessian_points_batched_dev,
enlsip_gn_hessian_sums_batched_dev).  Points and Gamma are compared bit for bit with the host routines on the same data
(tests/test_hessian_sums_host.py checks those against the reference and exact arithmetic), at row lengths around the wave and the
unrolled stride, with ragged t, pair ranges that are no multiple of four, ldg > n, a stride gap, permuted and negative slots, and
every byte outside the written entries held to a NaN pattern.  The driver and the analysis run on the end-to-end batch of
tests/direction_cases.py."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

import direction_cases as dc  # noqa: E402
import hessian_cases as hc  # noqa: E402

PATTERN = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]      # a NaN with a payload no arithmetic produces


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class Batch:
    """count random problems of one shape with ragged t on the device, evaluations of the pairs pair0 .. pair0 + npairs - 1"""

    def __init__(self, m, n, l, ts, pair0, npairs, seed, problems=None):
        rng = np.random.default_rng(seed)
        self.m, self.n, self.l, self.ts, self.pair0, self.npairs, self.B = m, n, l, list(ts), pair0, npairs, len(ts)
        self.t_max = max(list(ts) + [0])
        self.P = problems or [hc.random_problem(rng, m, n, l, t, npairs=npairs) for t in ts]
        self.upload()

    def upload(self):
        import torch
        B, tm = self.B, max(self.t_max, 1)
        lam = np.full((B, tm), -7.25e33)
        for k, P in enumerate(self.P):
            lam[k, :P["t"]] = P["lam"]
        self.active = np.stack([P["active"] for P in self.P]).reshape(B, self.l)
        self.d = dict(x=dev(np.stack([P["x"] for P in self.P])), F=dev(np.stack([P["F"] for P in self.P])),
                      rx=dev(np.stack([P["rx"] for P in self.P]).reshape(B, self.m)), G=dev(np.stack([P["G"] for P in self.P])),
                      lam=dev(lam[:, :self.t_max]))
        torch.cuda.synchronize()

    def run(self, solver, dGamma, ldg, strideG, slot=None, **over):
        from enlsip_gn import direction as D
        p = lambda nm: self.d[nm].data_ptr() if self.d[nm].numel() else 0
        a = dict(count=self.B, m=self.m, n=self.n, l=self.l, t_max=self.t_max, pair0=self.pair0, npairs=self.npairs, t=self.ts,
                 active=self.active, slot=slot, dx=p("x"), dF=p("F"), drx=p("rx"), dG=p("G"), dlambda=p("lam"), dGamma=dGamma.data_ptr(),
                 ldg=ldg, strideG=strideG)
        a.update(over)
        D.hessian_sums_dev(solver, **a)

    def expected(self, flat, ldg, strideG, slot=None):
        """the pattern-filled flat Gamma buffer with the host routine's entries of every taken problem put in"""
        from enlsip_gn import direction as D
        want = flat.copy()
        for k, P in enumerate(self.P):
            s = k if slot is None else int(slot[k])
            if s < 0:
                continue
            G = D.hessian_sums(P["x"], P["F"], P["rx"], P["G"], P["lam"], P["active"], P["t"], pair0=self.pair0)
            for kk, jj in hc.pairs(self.n)[self.pair0: self.pair0 + self.npairs]:
                want[s * strideG + kk + jj * ldg] = want[s * strideG + jj + kk * ldg] = G[kk, jj]
        return want


def pattern(size):
    return np.full(size, PATTERN)


# ---- the points kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (1, 5))
@pytest.mark.parametrize("n", (1, 2, 5, 65))
def test_points_are_the_host_routine_s_bytes(solver, n, count):
    import torch
    from enlsip_gn import direction as D
    pairs = n * (n + 1) // 2
    rng = np.random.default_rng(50 + n)
    x = np.stack([hc.special_x(n, k) for k in range(count)])
    x[count - 1, n // 2] = rng.standard_normal() * 1e3
    dx = dev(x)
    row = n - 1                                                           # a range cut inside the last row (a single pair when n == 1)
    ranges = {(0, pairs), (pairs - 1, 1), (0, 1), (row * (row + 1) // 2 + row // 2, max(1, row - row // 2))}
    for pair0, npairs in sorted(ranges):
        dX = torch.full((count, npairs, 4, n), float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        D.hessian_points_dev(solver, count, n, pair0, npairs, dx.data_ptr(), dX.data_ptr())
        got = dX.cpu().numpy()
        for k in range(count):
            assert same_bytes(got[k], D.hessian_points(x[k], pair0, npairs)), (n, count, pair0, npairs, k)
    assert same_bytes(dx.cpu().numpy(), x)


# ---- the sums kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 63, 64, 65, 129, 512))
def test_sums_are_the_host_routine_s_bytes_and_nothing_else_is_written(solver, m):
    import torch
    n = 4
    ldg, gap = n + 3, 5
    strideG = ldg * n + gap
    case = 0
    for l, t in ((0, 0), (1, 0), (1, 1), (65, 0), (65, 1), (65, 65)):
        for count in (1, 4, 5):
            for npairs in (1, 3, 4, 5):
                case += 1
                ts = [t, 0, min(1, t), t, t // 2][:count]
                pair0 = (case * 3) % (10 - npairs + 1)
                b = Batch(m, n, l, ts, pair0, npairs, seed=1000 * m + case)
                slot = None if case % 3 == 0 else list(np.random.default_rng(case).permutation(count + 2)[:count])
                if slot is not None and count > 1 and case % 3 == 2:
                    slot[1] = -1
                S = count + 2
                flat = pattern(S * strideG)
                dGam = dev(flat)
                torch.cuda.synchronize()
                b.run(solver, dGam, ldg, strideG, slot=slot)
                assert same_bytes(dGam.cpu().numpy(), b.expected(flat, ldg, strideG, slot)), (m, l, t, count, npairs, pair0, slot)
    assert case == 72


def test_chunking_gives_the_same_gamma(solver):
    import torch
    m, n, l = 130, 5, 6
    ts = [4, 0, 6]
    pairs = n * (n + 1) // 2
    whole = Batch(m, n, l, ts, 0, pairs, seed=5)
    flat = pattern(3 * n * n)
    dG = dev(flat)
    torch.cuda.synchronize()
    whole.run(solver, dG, n, n * n)
    ref = dG.cpu().numpy()
    assert same_bytes(ref, whole.expected(flat, n, n * n)) and not np.isnan(ref).any()
    for chunk in (1, 3, 7):
        dG = dev(flat)
        torch.cuda.synchronize()
        for pair0 in range(0, pairs, chunk):
            npr = min(chunk, pairs - pair0)
            part = [dict(P, F=P["F"][pair0: pair0 + npr], G=P["G"][pair0: pair0 + npr]) for P in whole.P]
            Batch(m, n, l, ts, pair0, npr, seed=0, problems=part).run(solver, dG, n, n * n)
        assert same_bytes(dG.cpu().numpy(), ref), chunk


def test_slot_and_batch_do_not_matter(solver):
    import torch
    m, n, l = 200, 3, 9
    pairs = 6
    big = Batch(m, n, l, [3, 9, 0, 5, 1], 0, pairs, seed=21)
    flat = pattern(8 * n * n)
    dG = dev(flat)
    torch.cuda.synchronize()
    big.run(solver, dG, n, n * n)
    inside = dG.cpu().numpy().reshape(8, n * n)[3]
    alone = Batch(m, n, l, [5], 0, pairs, seed=0, problems=[big.P[3]])
    for slot in (None, [6]):
        dG = dev(flat)
        torch.cuda.synchronize()
        alone.run(solver, dG, n, n * n, slot=slot)
        got = dG.cpu().numpy().reshape(8, n * n)
        assert same_bytes(got[0 if slot is None else 6], inside)
    other = Batch(m, n, l, [9, 5], 0, pairs, seed=0, problems=[big.P[1], big.P[3]])
    dG = dev(flat)
    torch.cuda.synchronize()
    other.run(solver, dG, n, n * n, slot=[4, 2])
    assert same_bytes(dG.cpu().numpy().reshape(8, n * n)[2], inside)


def test_argument_errors_come_before_any_launch_and_leave_gamma(solver):
    import ctypes as C
    import torch
    from enlsip_gn import GNError
    m, n, l = 20, 4, 5
    b = Batch(m, n, l, [3, 0, 2], 0, 10, seed=31)
    flat = pattern(3 * n * n)
    dG = dev(flat)
    torch.cuda.synchronize()

    def raw(code, **over):
        with pytest.raises(GNError) as e:
            b.run(solver, dG, over.pop("ldg", n), over.pop("strideG", n * n), slot=over.pop("slot", None), **over)
        assert f"error {code}:" in str(e.value), (code, str(e.value))
        torch.cuda.synchronize()
        assert same_bytes(dG.cpu().numpy(), flat), code
    raw(-2, n=0)
    raw(-2, m=-1)
    raw(-2, npairs=0)
    raw(-2, pair0=-1)
    raw(-2, pair0=1)
    raw(-4, dx=0)
    raw(-4, dF=0)
    raw(-4, drx=0)
    raw(-4, dG=0)
    raw(-4, dlambda=0)
    raw(-5, t=[3, 0, 4])
    raw(-5, t=[6, 0, 2], t_max=9)
    act = b.active.copy()
    act[0, 1] = l + 1
    raw(-5, active=act)
    raw(-5, ldg=n - 1)
    raw(-5, ldg=n + 1)
    raw(-5, slot=[1, 0, 1])
    lib = solver._lib
    assert lib.enlsip_gn_hessian_sums_batched_dev(None, 1, m, n, l, 3, 0, 10, None, None, None, None, None, None, None, None, None, n, n * n) == -1
    assert lib.enlsip_gn_hessian_points_batched_dev(None, 1, n, 0, 10, None, None) == -1
    h = solver._h
    tt = np.array([3, 0, 2], dtype=np.int64)
    dp = lambda nm: C.c_void_p(b.d[nm].data_ptr())
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.enlsip_gn_hessian_sums_batched_dev(h, 0, m, n, l, 3, 0, 10, hp(tt), hp(b.active), None, dp("x"), dp("F"), dp("rx"), dp("G"),
                                                  dp("lam"), C.c_void_p(dG.data_ptr()), n, n * n) == -2      # count < 1
    assert lib.enlsip_gn_hessian_sums_batched_dev(h, 3, m, n, l, 3, 0, 10, None, hp(b.active), None, dp("x"), dp("F"), dp("rx"), dp("G"),
                                                  dp("lam"), C.c_void_p(dG.data_ptr()), n, n * n) == -4      # t NULL
    assert lib.enlsip_gn_hessian_sums_batched_dev(h, 3, m, n, l, 3, 0, 10, hp(tt), hp(b.active), None, dp("x"), dp("F"), dp("rx"), dp("G"),
                                                  dp("lam"), None, n, n * n) == -4                           # dGamma NULL
    torch.cuda.synchronize()
    assert same_bytes(dG.cpu().numpy(), flat)
    dX = torch.zeros((3, 10, 4, n), dtype=torch.float64, device="cuda:0")
    px, pX = C.c_void_p(b.d["x"].data_ptr()), C.c_void_p(dX.data_ptr())
    assert lib.enlsip_gn_hessian_points_batched_dev(h, 0, n, 0, 10, px, pX) == -2
    assert lib.enlsip_gn_hessian_points_batched_dev(h, 3, n, 1, 10, px, pX) == -2
    assert lib.enlsip_gn_hessian_points_batched_dev(h, 3, n, 0, 10, None, pX) == -4
    assert lib.enlsip_gn_hessian_points_batched_dev(h, 3, n, 0, 10, px, None) == -4
    assert not dX.cpu().numpy().any()
    b.run(solver, dG, n, n * n)                                           # and the same call without an error writes
    assert same_bytes(dG.cpu().numpy(), b.expected(flat, n, n * n))


# ---- the driver and the analysis on the end-to-end batch ------------------------------------------------------------------------------
def e2e_callbacks(Ps, idx):
    """the residuals and constraints of the problems idx of tests/direction_cases.py::e2e_problems wrapped as batched torch
    callbacks: X (N, 4 npairs, n) on the device in, (N, 4 npairs, m) and (N, 4 npairs, l) on the device out, every row by the
    problem's own function, so that the evaluations are the reference's to the bit and only the order of the sums differs"""
    def wrap(name):
        def f(X):
            Xh = X.cpu().numpy()
            return dev(np.array([[Ps[k][name].f(Xh[i, p]) for p in range(Xh.shape[1])] for i, k in enumerate(idx)]))
        return f
    return wrap("r"), wrap("c")


def e2e_entry_tolerance(P):
    """the per-entry bound between two summation orders, from the reference's own evaluations of the problem"""
    m, n, l = dc.E2E_SHAPE
    X = hc.reference_points(P["x"])
    F = np.array([[P["r"].f(X[q, s]) for s in range(4)] for q in range(X.shape[0])])
    G = np.array([[P["c"].f(X[q, s]) for s in range(4)] for q in range(X.shape[0])])
    tol = np.zeros((n, n))
    for e in hc.restated(P["x"], F, P["rx"], G, P["lam"], P["W"].active, P["t"]):
        tol[e["k"], e["j"]] = tol[e["j"], e["k"]] = hc.entry_bound(e, m, P["t"])
    return tol


def test_the_driver_forms_gamma_of_the_end_to_end_problems(solver):
    """Gamma of every taken end-to-end problem by the driver against e2e_hessians, entry by entry within the bound between two
    summation orders of the same rounded terms (tests/hessian_cases.py::entry_bound)."""
    import torch
    from enlsip_gn import direction as D
    m, n, l = dc.E2E_SHAPE
    Ps = dc.e2e_problems()
    idx = [k for k, P in enumerate(Ps) if P["take"]]
    res, con = e2e_callbacks(Ps, idx)
    t_max = max(P["t"] for P in Ps)
    lam = np.zeros((len(idx), t_max))
    for i, k in enumerate(idx):
        lam[i, :Ps[k]["t"]] = Ps[k]["lam"]
    dx, drx, dlam = dev(np.stack([Ps[k]["x"] for k in idx])), dev(np.stack([Ps[k]["rx"] for k in idx])), dev(lam)
    slot = [len(Ps) - 1 - k for k in idx]                                 # a permuted slot list into a batch-sized Gamma
    outs = []
    for ppc in (None, 4):
        dG = torch.full((len(Ps), n, n), float("nan"), dtype=torch.float64, device="cuda:0")
        D.hessian_sums_batched_dev(solver, [Ps[k]["W"] for k in idx], dx, drx, dlam, res, con, dG, slot=slot, pairs_per_call=ppc)
        outs.append(dG.cpu().numpy())
    assert same_bytes(outs[0], outs[1])                                   # the pair ranges do not matter
    got = outs[0]
    for i, k in enumerate(idx):
        P = Ps[k]
        want = dc.e2e_hessians(P)
        tol = e2e_entry_tolerance(P)
        G = got[slot[i]].T
        assert same_bytes(G, G.T)
        # off the diagonal the second difference of these problems is rounding noise (their Hessians are multiples of I): an
        # entry whose terms are all exactly zero has tolerance 0 and must agree exactly
        ratio = np.abs(G - want)[tol > 0] / tol[tol > 0]
        print(f"{P['kind']}: largest |Gamma - reference| {np.abs(G - want).max():.3e}, largest difference / tolerance {ratio.max():.3f}, "
              f"{int((tol == 0).sum())} entries of tolerance 0")
        assert (np.abs(G - want) <= tol).all(), (P["kind"], np.abs(G - want).max(), tol.min())
    untouched = [s for s in range(len(Ps)) if s not in slot]
    assert untouched and all(np.isnan(got[s]).all() for s in untouched)


def records(out):
    """DirectionRecords as comparable tuples (a record that was not formed holds NaN, which equals nothing)"""
    import dataclasses
    return [tuple(repr(v) for v in dataclasses.astuple(r)) for r in out]


def test_the_analysis_with_device_hessians_is_the_host_path_on_the_same_gamma(solver):
    import torch
    from enlsip_gn import direction as D
    m, n, l = dc.E2E_SHAPE
    Ps = dc.e2e_problems()
    B = len(Ps)
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda:0")
    At, cxa, t = solver.pack_ragged([P["aC"].A for P in Ps], [P["aC"].cx for P in Ps], n=n)
    t_max = At.shape[1]
    dJ, drx = dev(np.stack([P["J"].T for P in Ps])), dev(np.stack([P["rx"] for P in Ps]))
    dAt, dcx = dev(At), dev(cxa)
    ds = np.zeros((B, t_max))
    for k, P in enumerate(Ps):
        ds[k, :P["t"]] = P["aC"].diag_scale

    def run(**how):
        bufs = dict(p=zeros(B, n), b=zeros(B, t_max), d=zeros(B, m), lam=zeros(B, t_max), diag_scale=dev(ds),
                    cx_all=dev(np.stack([P["cx"] for P in Ps])), x=dev(np.stack([P["x"] for P in Ps])), rx=drx,
                    Gamma=torch.full((B, n, n), float("nan"), dtype=torch.float64, device="cuda:0"))
        dinfo, dgrad = zeros(B, 6, dtype=torch.int64), zeros(B, n)
        solver.solve_batched_ragged_dev(B, m, n, t_max, t, dJ.data_ptr(), m, m * n, drx.data_ptr(), dAt.data_ptr(), n, n * t_max,
                                        dcx.data_ptr(), dp=bufs["p"].data_ptr(), db=bufs["b"].data_ptr(), dd=bufs["d"].data_ptr(),
                                        dinfo=dinfo.data_ptr())
        solver.gradient_batched_dev(0, B, dgrad.data_ptr())
        assert solver.first_lagrange_batched_dev(0, B, bufs["lam"].data_ptr(), dgrad_fx=dgrad.data_ptr()) == 0
        torch.cuda.synchronize()
        before = {nm: bufs[nm].cpu().numpy() for nm in ("p", "b", "d")}
        out = D.search_direction_analys_batched_dev(solver, [P["W"] for P in Ps], [P["cur"] for P in Ps], [P["prev"] for P in Ps], bufs,
                                                    m=m, n=n, t_max=t_max, iter_number=[P["iter_number"] for P in Ps], scaling=False,
                                                    rx_sum=[float(P["rx"] @ P["rx"]) for P in Ps], take=[P["take"] for P in Ps], **how)
        torch.cuda.synchronize()
        return out, before, {nm: bufs[nm].cpu().numpy() for nm in ("p", "b", "d", "Gamma")}

    # the only code 2 problem that has second derivatives in the host path is the one the device path serves; the one "without
    # hessians" gets Gamma from the device path too, so it is compared apart
    k2 = [k for k, P in enumerate(Ps) if P["kind"] == "code 2 with hessians"][0]
    k4 = [k for k, P in enumerate(Ps) if P["kind"] == "code 2 without hessians"][0]
    res_all, con_all = e2e_callbacks(Ps, [k2, k4])
    out_d, before_d, after_d = run(hessian_evals=(res_all, con_all))
    gam = after_d["Gamma"]
    assert not np.isnan(gam[k2]).any() and not np.isnan(gam[k4]).any()
    assert all(np.isnan(gam[k]).all() for k in range(B) if k not in (k2, k4))      # untaken slots of Gamma keep their bytes
    out_h, before_h, after_h = run(hessians=lambda k: gam[k].T if k in (k2, k4) else None)
    assert all(same_bytes(before_d[nm], before_h[nm]) for nm in before_d)
    assert records(out_d) == records(out_h)                               # the same DirectionRecords
    assert same_bytes(after_d["p"], after_h["p"])                         # the same Gamma through the same Newton kernel
    assert out_d[k2].code == 2 and out_d[k2].nb_newton_steps == 1 and out_d[k2].error_code == 0 and out_d[k4].error_code == 0
    for k, P in enumerate(Ps):                                            # everything but the two Newton slots of p is as before
        if k in (k2, k4) or P["kind"].startswith("code -1"):
            continue
        assert all(same_bytes(after_d[nm][k], before_d[nm][k]) for nm in ("p", "b", "d")), P["kind"]
    for k in (k2, k4):
        assert same_bytes(after_d["b"][k], before_d["b"][k]) and same_bytes(after_d["d"][k], before_d["d"][k])
        assert not same_bytes(after_d["p"][k], before_d["p"][k])
    # and against the records of the host path as the existing end-to-end test runs it (Gamma from the reference's own loops)
    out_ref, _, after_ref = run(hessians=lambda k: dc.e2e_hessians(Ps[k]) if Ps[k]["second"] else None)
    for k, (a, b) in enumerate(zip(out_d, out_ref)):
        if k == k4:
            assert (b.error_code, a.error_code) == (-4, 0)
            continue
        assert records([a]) == records([b]), (Ps[k]["kind"], a, b)
    with pytest.raises(ValueError):
        run(hessians=lambda k: None, hessian_evals=(res_all, con_all))
