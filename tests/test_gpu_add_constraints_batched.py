"""The working-set additions of a batch and the rebuild of its active constraints on device buffers
(enlsip_gn_add_constraints_batched_dev) and the driver built on it (working_set.add_constraints_batched_dev).  Every comparison
is exact: the lists, t, added, status and every byte of the device buffers are those of the two host routines
(enlsip_gn_evaluate_violated_constraints, enlsip_gn_gather_active_constraints: tests/test_violated_constraints_host.py and
tests/test_gather_active_host.py check those against the oracle and a high-precision reference) applied per problem."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

BATCH = 67      # not a multiple of four: the last workgroup of the wave form is partly empty
SHAPES = [(1, 1), (3, 2), (2, 5), (32, 4), (64, 64), (65, 64), (64, 65), (7, 130), (130, 70)]      # (n, l)


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def problems(n, l, B, seed, t_cap=None):
    """q, t, active, inactive (B x l), index_alpha_upp and the full cx of B problems: sorted lists, the equalities first, the
    working set anywhere between q and capacity (t_cap: a smaller bound on t)"""
    rng = np.random.default_rng(seed)
    bnd = min(l, n) if t_cap is None else min(l, n, t_cap)
    q, t, iau = (np.zeros(B, dtype=np.int64) for _ in range(3))
    act, ina = np.zeros((B, l), dtype=np.int64), np.zeros((B, l), dtype=np.int64)
    cx = np.zeros((B, l))
    for k in range(B):
        q[k] = rng.integers(0, bnd + 1)
        t[k] = bnd if k % 3 == 0 else rng.integers(q[k], bnd + 1)      # every third problem at capacity: swaps and cycles
        extra = np.sort(rng.choice(np.arange(q[k] + 1, l + 1), size=t[k] - q[k], replace=False)) if t[k] > q[k] else []
        act[k, :t[k]] = np.concatenate([np.arange(1, q[k] + 1), extra])
        ina[k, :l - t[k]] = np.setdiff1d(np.arange(1, l + 1), act[k, :t[k]])
        cx[k] = rng.standard_normal(l) + float(rng.integers(-1, 2))
        if k % 5 == 0 and l >= 2:      # ties
            cx[k, rng.integers(0, l, size=max(1, l // 3))] = cx[k, 0]
        if k % 11 == 0:
            cx[k, rng.integers(0, l)] = np.nan
        iau[k] = rng.integers(0, l + 1)
    return q, t, act, ina, iau, cx


class Buffers:
    """Host images of the device buffers of one call, NaN outside the live entries, and their upload."""
    names = ("A", "cx_all", "At", "cx", "ds")

    def __init__(self, n, l, t_max, cx_all, padded, seed):
        rng = np.random.default_rng(seed)
        B = cx_all.shape[0]
        self.n, self.l, self.t_max, self.B = n, l, t_max, B
        self.lda = l + 2 if padded else max(l, 1)
        self.strideA = self.lda * n + (3 if padded else 0)
        self.ldat = n + 3 if padded else n
        self.strideAt = self.ldat * t_max + (5 if padded else 0)
        self.A = np.full((B, max(self.strideA, 1)), np.nan)
        for k in range(B):
            self.full_A(k)[:, :] = rng.standard_normal((l, n)) * (1.0 if k % 4 else 1e-3)
        if l and B > 3:
            self.full_A(3)[0, :] = 0.0      # a zero row: the divisor 1.0 under scaling
        self.cx_all = cx_all.copy() if l else np.zeros((B, 1))
        self.At = np.full((B, max(self.strideAt, 1)), np.nan)
        self.cx, self.ds = np.full((B, max(t_max, 1)), np.nan), np.full((B, max(t_max, 1)), np.nan)

    def full_A(self, k):
        """problem k's l x n constraint Jacobian: a view of the column-major block"""
        return self.A[k, :self.lda * self.n].reshape(self.n, self.lda)[:, :self.l].T

    def block(self, k, At):
        return At[k, :self.ldat * self.t_max].reshape(self.t_max, self.ldat)

    def images(self):
        return {nm: getattr(self, nm).copy() for nm in self.names}

    def upload(self):
        import torch
        self.dev = {nm: torch.from_numpy(getattr(self, nm).copy()).to("cuda:0") for nm in self.names}
        torch.cuda.synchronize()
        return self

    def download(self):
        import torch
        torch.cuda.synchronize()
        return {nm: self.dev[nm].cpu().numpy() for nm in self.names}

    def args(self):
        p = lambda nm: self.dev[nm].data_ptr()
        return p("A"), self.lda, self.strideA, p("cx_all"), p("At"), self.ldat, self.strideAt, p("cx"), p("ds")


def host_model(buf, img, q, t, act, ina, iau, take, scaling):
    """what the two host routines give per problem: (t, act, ina, added, status) and the images, edited in place"""
    from enlsip_gn import evaluate_violated_constraints, gather_active_constraints
    n, l, t_max = buf.n, buf.l, buf.t_max
    t, act, ina = t.copy(), act.copy(), ina.copy()
    added, status = np.zeros(buf.B, dtype=np.int64), np.zeros(buf.B, dtype=np.int64)
    for k in range(buf.B):
        tk = 1 if take is None else int(take[k])
        if tk == 0:
            continue
        if tk == 1:
            t[k], act[k], ina[k], ad, status[k] = evaluate_violated_constraints(l, n, int(q[k]), int(t[k]), act[k], ina[k],
                                                                                buf.cx_all[k], int(iau[k]))
            added[k] = int(ad)
        if t_max == 0:
            continue
        blk = buf.block(k, img["At"])
        gather_active_constraints(act[k], int(t[k]), buf.full_A(k), buf.cx_all[k], scaling, ldat=buf.ldat,
                                  out=(blk[:t[k]], img["cx"][k, :t[k]], img["ds"][k, :t[k]]))
        blk[t[k]:, :n] = 0.0
        img["cx"][k, t[k]:] = 0.0
        img["ds"][k, t[k]:] = 1.0
    return t, act, ina, added, status


def same_images(got, want, tag=""):
    for nm in want:
        assert got[nm].tobytes() == want[nm].tobytes(), (nm, tag)


def run_and_compare(solver, n, l, t_max, B, padded, scaling, take, seed, t_cap=None):
    q, t, act, ina, iau, cx = problems(n, l, B, seed, t_cap)
    buf = Buffers(n, l, t_max, cx, padded, seed + 1)
    want = buf.images()
    wt, wact, wina, wadd, wst = host_model(buf, want, q, t, act, ina, iau, take, scaling)
    buf.upload()
    before = (t.copy(), act.copy(), ina.copy())
    gt, gact, gina, gadd, gst = solver.add_constraints_batched_dev(B, n, l, t_max, q, t, act, ina, iau, scaling, *buf.args(), take=take)
    assert solver.addition_form() == (1 if (n <= 64 and l <= 64) else 0)
    assert np.array_equal(t, before[0]) and np.array_equal(act, before[1]) and np.array_equal(ina, before[2])
    assert np.array_equal(gst, wst), np.flatnonzero(gst != wst)
    assert np.array_equal(gt, wt) and np.array_equal(gadd, wadd)
    assert np.array_equal(gact, wact) and np.array_equal(gina, wina)
    assert not (wst == 2).any()
    same_images(buf.download(), want, (n, l, scaling))
    return wst, wadd, buf, (q, t, act, ina, iau)


def mixed_take(B, seed):
    take = np.random.default_rng(seed).integers(0, 3, B).astype(np.int64)
    take[:3] = (1, 2, 0)
    return take


# ---- 1. the walk and the rebuild, both forms, every kind of take -----------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("n,l", SHAPES)
def test_walk_and_rebuild(solver, n, l, padded):
    seen_status, seen_added = set(), set()
    for scaling, take in ((False, None), (True, mixed_take(BATCH, n + l))):
        st, ad, _, _ = run_and_compare(solver, n, l, l, BATCH, padded, scaling, take, seed=100 * n + l + int(scaling))
        seen_status |= set(st.tolist())
        seen_added |= set(ad.tolist())
    if n < l and l >= 4:      # only with more constraints than unknowns is a working set at capacity while candidates remain
        assert seen_status == {0, 1} and seen_added == {0, 1}      # the batch holds problems the reference would spin on


@pytest.mark.parametrize("n,l", [(2, 5), (64, 65), (7, 130), (130, 70)])
def test_t_max_exactly_the_largest_t_a_walk_can_leave(solver, n, l):
    t_max = min(l, n)      # every t <= min(l, n), so max(t, min(l, n)) is exactly t_max
    run_and_compare(solver, n, l, t_max, BATCH, True, True, None, seed=7 * n + l)
    # rebuild only, below capacity: t_max is max(t) and nothing is walked
    cap = max(1, t_max // 2)
    run_and_compare(solver, n, l, cap, BATCH, True, False, np.full(BATCH, 2, dtype=np.int64), seed=9 * n + l, t_cap=cap)


# ---- 2. the two forms agree; slot and batch independence --------------------------------------------------------------------------------
def test_general_form_on_wave_form_problems(solver):
    """the problems of a wave-form shape padded into a general-form shape by constraints that are never violated and sort last:
    the same lists and the same bytes of the slot"""
    n, l, l2, B, t_max = 8, 20, 66, 23, 20
    q, t, act, ina, iau, cx = problems(n, l, B, seed=5)
    small = Buffers(n, l, t_max, cx, False, seed=6)
    cx2 = np.concatenate([cx, np.full((B, l2 - l), 1e3)], axis=1)
    big = Buffers(n, l2, t_max, cx2, False, seed=6)
    for k in range(B):
        big.full_A(k)[:l, :] = small.full_A(k)
    act2 = np.concatenate([act, np.zeros((B, l2 - l), dtype=np.int64)], axis=1)
    ina2 = np.zeros((B, l2), dtype=np.int64)
    for k in range(B):
        ina2[k, :l2 - t[k]] = np.concatenate([ina[k, :l - t[k]], np.arange(l + 1, l2 + 1)])
    small.upload(); big.upload()
    for scaling in (False, True):
        a = solver.add_constraints_batched_dev(B, n, l, t_max, q, t, act, ina, iau, scaling, *small.args())
        assert solver.addition_form() == 1
        b = solver.add_constraints_batched_dev(B, n, l2, t_max, q, t, act2, ina2, iau, scaling, *big.args())
        assert solver.addition_form() == 0
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
        assert set(a[4].tolist()) == {0, 1}
        for k in range(B):
            tk = a[0][k]
            assert np.array_equal(a[1][k, :tk], b[1][k, :tk]) and not b[1][k, tk:].any()
            assert np.array_equal(a[2][k, :l - tk], b[2][k, :l - tk]) and np.array_equal(b[2][k, l - tk:l2 - tk], np.arange(l + 1, l2 + 1))
        ga, gb = small.download(), big.download()
        for nm in ("At", "cx", "ds"):
            assert ga[nm].tobytes() == gb[nm].tobytes(), (nm, scaling)


@pytest.mark.parametrize("n,l", [(8, 12), (70, 66)], ids=["wave", "general"])
def test_slot_and_batch_independence(solver, n, l):
    q, t, act, ina, iau, cx = problems(n, l, BATCH, seed=n)
    last = BATCH - 1
    for x in (q, t, act, ina, iau, cx):
        x[last] = x[0]
    buf = Buffers(n, l, l, cx, True, seed=2)
    buf.A[last] = buf.A[0]
    buf.upload()
    take = mixed_take(BATCH, 3)
    take[0] = take[last] = 1
    full = solver.add_constraints_batched_dev(BATCH, n, l, l, q, t, act, ina, iau, True, *buf.args(), take=take)
    got = buf.download()
    one = Buffers(n, l, l, cx[:1], True, seed=2)
    one.A[0] = buf.A[0]
    one.upload()
    alone = solver.add_constraints_batched_dev(1, n, l, l, q[:1], t[:1], act[:1], ina[:1], iau[:1], True, *one.args())
    ref = one.download()
    for k in (0, last):
        assert all(np.array_equal(np.atleast_1d(full[j][k]), np.atleast_1d(alone[j][0])) for j in range(5)), k
        for nm in ("At", "cx", "ds"):
            assert got[nm][k].tobytes() == ref[nm][0].tobytes(), (nm, k)


def test_one_large_batch(solver):
    """65 600 problems at (2, 3): 656 distinct problems, each a hundred times, so that the host model stays small"""
    n, l, rep = 2, 3, 100
    q, t, act, ina, iau, cx = problems(n, l, 656, seed=11)
    buf = Buffers(n, l, l, cx, False, seed=12)
    want = buf.images()
    wt, wact, wina, wadd, wst = host_model(buf, want, q, t, act, ina, iau, None, True)
    assert set(wst.tolist()) == {0, 1} and set(wadd.tolist()) == {0, 1}
    tile = lambda a: np.tile(a, (rep,) + (1,) * (a.ndim - 1))
    for nm in buf.names:
        setattr(buf, nm, tile(getattr(buf, nm)))
    buf.upload()
    B = 656 * rep
    gt, gact, gina, gadd, gst = solver.add_constraints_batched_dev(B, n, l, l, tile(q), tile(t), tile(act), tile(ina), tile(iau), True,
                                                                   *buf.args())
    assert np.array_equal(gt, tile(wt)) and np.array_equal(gadd, tile(wadd)) and np.array_equal(gst, tile(wst))
    assert np.array_equal(gact, tile(wact)) and np.array_equal(gina, tile(wina))
    same_images(buf.download(), {nm: tile(a) for nm, a in want.items()})


# ---- 3. errors, l == 0 -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_buffers(solver):
    n, l, t_max, B = 5, 6, 5, 6
    q, t, act, ina, iau, cx = problems(n, l, B, seed=1)
    buf = Buffers(n, l, t_max, cx, True, seed=1).upload()
    before = buf.images()
    L, h = solver._lib, solver._h
    v = lambda x: C.c_void_p(x) if x else None
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    added, status = np.full(B, -9, dtype=np.int64), np.full(B, -9, dtype=np.int64)
    dA, lda, sA, dcxa, dAt, ldat, sAt, dcx, dds = buf.args()
    t0, act0, ina0 = t.copy(), act.copy(), ina.copy()

    def call(h=h, batch=B, n=n, l=l, t_max=t_max, q=q, t=t, act=act, ina=ina, iau=iau, take=None, dA=dA, lda=lda, sA=sA, dcxa=dcxa,
             dAt=dAt, ldat=ldat, sAt=sAt, dcx=dcx, dds=dds, added=added, status=status):
        return L.enlsip_gn_add_constraints_batched_dev(h, batch, n, l, t_max, hp(q), hp(t), hp(act), hp(ina), hp(iau), hp(take), 1,
                                                       v(dA), lda, sA, v(dcxa), v(dAt), ldat, sAt, v(dcx), v(dds), hp(added), hp(status))

    def bad(vec, k, val):
        out = vec.copy()
        out[k] = val
        return out

    def bad2(mat, k, i, val):
        out = mat.copy()
        out[k, i] = val
        return out

    k_full = int(np.flatnonzero(t < l)[0])      # a problem with a used inactive entry
    k_act = int(np.flatnonzero(t > 0)[0])
    assert call(h=None) == -1
    checks = [
        (lambda: call(batch=0), -2),
        (lambda: call(n=0), -3), (lambda: call(l=-1), -3), (lambda: call(l=1025, t_max=1025), -3), (lambda: call(t_max=-1), -3),
        (lambda: call(t_max=l + 1), -3), (lambda: call(l=1025), -3),
        (lambda: call(q=None), -4), (lambda: call(t=None), -4), (lambda: call(act=None), -4), (lambda: call(ina=None), -4),
        (lambda: call(added=None), -4), (lambda: call(status=None), -4), (lambda: call(dA=0), -4), (lambda: call(dcxa=0), -4),
        (lambda: call(dAt=0), -4), (lambda: call(dcx=0), -4), (lambda: call(dds=0), -4),
        (lambda: call(t=bad(t, 1, t_max + 1)), -5), (lambda: call(t=bad(t, 1, -1)), -5),
        (lambda: call(t_max=t_max - 1, t=np.minimum(t, t_max - 1), q=np.minimum(q, t_max - 1)), -5),      # min(l, n) > t_max, take 1
        (lambda: call(q=bad(q, 2, t[2] + 1)), -6), (lambda: call(q=bad(q, 2, -1)), -6),
        (lambda: call(act=bad2(act, k_act, 0, l + 1)), -7), (lambda: call(act=bad2(act, k_act, 0, -1)), -7),
        (lambda: call(ina=bad2(ina, k_full, 0, l + 1)), -7), (lambda: call(iau=bad(iau, 4, l + 1)), -7), (lambda: call(iau=bad(iau, 4, -1)), -7),
        (lambda: call(lda=l - 1), -9), (lambda: call(ldat=n - 1), -9),
        (lambda: call(sA=lda * n - 1), -10), (lambda: call(sAt=ldat * t_max - 1), -10),
    ]
    seen = set()
    for i, (fn, want) in enumerate(checks):
        got = fn()
        msg = L.enlsip_gn_last_error(h)
        assert got == want and msg, (i, got, want, msg)
        seen.add(msg)
    assert len(seen) >= 12      # the messages differ by condition
    assert call(t=bad(t, 1, -1)) == -5 and b"t[1]" in L.enlsip_gn_last_error(h)
    assert call(t=bad(t, 3, -1), q=bad(q, 1, -1)) == -6 and b"q[1]" in L.enlsip_gn_last_error(h)      # the lower k wins
    assert np.all(added == -9) and np.all(status == -9)
    assert np.array_equal(t, t0) and np.array_equal(act, act0) and np.array_equal(ina, ina0)
    same_images(buf.download(), before)
    # nothing of a problem that is not taken is checked or read
    take = np.ones(B, dtype=np.int64)
    take[1] = 0
    assert call(t=bad(t, 1, -1), take=take) == 0 and added[1] == 0 and status[1] == 0


def test_no_constraints_at_all(solver):
    B, n = 5, 4
    z = np.zeros(B, dtype=np.int64)
    e = np.zeros((B, 0), dtype=np.int64)
    out = solver.add_constraints_batched_dev(B, n, 0, 0, z, z, e, e, None, True, 0, 1, n, 0, 0, n, 0, 0, 0)
    assert not out[0].any() and not out[3].any() and not out[4].any() and out[1].shape == (B, 0)
    # l > 0 but no slot: only the rebuild of nothing is legal
    l = 3
    q, t, act, ina, iau, cx = problems(n, l, B, seed=2)
    t[:] = 0; q[:] = 0; act[:] = 0; ina[:] = np.arange(1, l + 1)
    out = solver.add_constraints_batched_dev(B, n, l, 0, q, t, act, ina, iau, True, 0, l, l * n, 0, 0, n, 0, 0, 0,
                                             take=np.full(B, 2, dtype=np.int64))
    assert not out[0].any() and np.array_equal(out[2], ina)


# ---- 4. the ragged solve on the slot this call built ---------------------------------------------------------------------------------
def chain(solver, n, l, scaling):
    """enlsip_gn_solve_batched_ragged_dev at m = 16 on the slot the call built and again on the slot the host routines built and
    uploaded: asserts p and info byte for byte and returns, per problem, (p, info row, oracle solution, J, rx, A', cx)"""
    import torch
    from oracle import gn_oracle as go, synth
    m, B = 16, 8
    q, t, act, ina, iau, cx = problems(n, l, B, seed=3 * n)
    cx = np.nan_to_num(cx, nan=0.5)      # finite data for the solve
    buf = Buffers(n, l, l, cx, False, seed=4)
    buf.full_A(3)[0, :] = 0.5            # and no zero row
    buf.upload()
    want = buf.images()
    wt, wact, _, _, _ = host_model(buf, want, q, t, act, ina, iau, None, scaling)
    gt, gact, _, _, _ = solver.add_constraints_batched_dev(B, n, l, l, q, t, act, ina, iau, scaling, *buf.args())
    assert np.array_equal(gt, wt) and np.array_equal(gact, wact)
    J = np.stack([np.asfortranarray(synth.normal_stream(700 + k, 2, m * n).reshape(m, n)).T for k in range(B)])      # (B, n, m)
    rx = np.stack([synth.normal_stream(700 + k, 3, m) for k in range(B)])
    dev = torch.device("cuda:0")
    dJ, drx = torch.from_numpy(J).to(dev), torch.from_numpy(rx).to(dev)
    hAt, hcx = torch.from_numpy(want["At"]).to(dev), torch.from_numpy(want["cx"]).to(dev)

    def solve(dAt, dcx):
        dp = torch.zeros((B, n), dtype=torch.float64, device=dev)
        dinfo = torch.zeros((B, 6), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        solver.solve_batched_ragged_dev(B, m, n, l, gt, dJ.data_ptr(), m, m * n, drx.data_ptr(), dAt.data_ptr(), buf.ldat,
                                        buf.strideAt, dcx.data_ptr(), dp=dp.data_ptr(), dinfo=dinfo.data_ptr())
        solver.synchronize()
        torch.cuda.synchronize()
        return dp.cpu().numpy(), dinfo.cpu().numpy()

    p1, i1 = solve(buf.dev["At"], buf.dev["cx"])
    p2, i2 = solve(hAt, hcx)
    assert p1.tobytes() == p2.tobytes() and i1.tobytes() == i2.tobytes()
    out = []
    for k in range(B):
        tk = int(gt[k])
        Aact, ca = buf.block(k, want["At"])[:tk, :n], want["cx"][k, :tk]
        ref = go.gn_subproblem(J[k].T, rx[k], Aact, ca)
        assert (i1[k, 0], i1[k, 1], i1[k, 2]) == (ref.rankA, ref.rankJ2, ref.code), (k, i1[k], ref.rankA, ref.rankJ2, ref.code)
        out.append((p1[k], i1[k], ref, J[k].T, rx[k], Aact, ca))
    return m, out


def rel_p(p, ref):
    nb = np.linalg.norm(ref.p)
    return np.linalg.norm(p - ref.p) / (nb if nb > 0 else 1.0)


@pytest.mark.parametrize("n,l", [(8, 12), (64, 40)])
def test_chain_into_the_ragged_solve(solver, n, l):
    """The slot as the call leaves it without row scaling: the two solves agree byte for byte and the first agrees with the
    oracle in ranks, code and p, with the tolerance of tests/test_gpu_ragged_batch.py."""
    TOL = 1e-11
    m, out = chain(solver, n, l, False)
    worst = 0.0
    for k, (p, info, ref, J, rx, A, ca) in enumerate(out):
        err = rel_p(p, ref)
        print(f"chain n={n} l={l} k={k} t={len(ca)} rankA={info[0]} rankJ2={info[1]} rel(p, oracle)={err:.3e}")
        worst = max(worst, err)
    assert worst <= TOL


@pytest.mark.parametrize("n,l", [(8, 12), (64, 40)])
def test_chain_into_the_ragged_solve_with_row_scaling(solver, n, l):
    """The same with row scaling.  Every column of the scaled A' has norm 1 up to rounding, so the first pivots of
    qr(A', ColumnNorm()) are ties that rounding decides, and with them the basis Q2 of the null space of A (Q1's range is not
    affected).  Where the subproblem determines p (m >= n - rankA: (8, 12)) that changes nothing and p is compared with the
    oracle as above.  At (64, 40) there are fewer equations than unknowns (16 + 40 < 64): the direction is a basic solution in
    that rounding-determined basis, the oracle itself differs from the host restatement of the kernels (oracle/lapack_semantics.py)
    by rel 0.7 .. 1.7 there, and what is compared is what the data determine: the ranks, the code and the two residual norms, with
    the rule tests/test_dispatch_grid.py uses for such solutions (1e-8 of max(1, norm))."""
    TOL = 1e-11
    m, out = chain(solver, n, l, True)
    for k, (p, info, ref, J, rx, A, ca) in enumerate(out):
        if m >= n - ref.rankA:
            assert rel_p(p, ref) <= TOL, (k, rel_p(p, ref))
            continue
        rj, ra = np.linalg.norm(J @ p + rx), np.linalg.norm(A @ p + ca)
        rj0, ra0 = np.linalg.norm(J @ ref.p + rx), np.linalg.norm(A @ ref.p + ca)
        assert abs(rj - rj0) <= 1e-8 * max(1.0, rj0) and abs(ra - ra0) <= 1e-8 * max(1.0, ra0), (k, rj, rj0, ra, ra0)


# ---- 5. the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling", [False, True, "mixed"], ids=["plain", "scaled", "mixed"])
@pytest.mark.parametrize("n,l", [(6, 9), (66, 70)])
def test_driver_leaves_the_records_of_the_host_flow(solver, n, l, scaling):
    import torch
    from enlsip_gn import working_set as ws
    from enlsip_gn import evaluate_violated_constraints, gather_active_constraints
    B = 13
    q, t, act, ina, iau, cx = problems(n, l, B, seed=n + l)
    buf = Buffers(n, l, l, cx, False, seed=8).upload()
    scal = np.array([(k % 2 == 0) if scaling == "mixed" else bool(scaling) for k in range(B)])
    Ws = [ws.WorkingSet(int(q[k]), int(t[k]), l, act[k].copy(), ina[k, :l - q[k]].copy()) for k in range(B)]
    dsn = torch.full((B, l), float("nan"), dtype=torch.float64, device="cuda:0")
    a = buf.args()
    added, status = ws.add_constraints_batched_dev(solver, Ws, iau, a[0], a[3], a[4], a[7], a[8], n=n, t_max=l, scaling=scal,
                                                   ddsn=dsn.data_ptr())
    got = buf.download()
    gdsn = dsn.cpu().numpy()
    assert set(status.tolist()) == {0, 1}
    for k in range(B):      # the per-problem host flow
        tk, a, i, ad, st = evaluate_violated_constraints(l, n, int(q[k]), int(t[k]), act[k], ina[k], cx[k], int(iau[k]))
        W = Ws[k]
        assert (W.t, int(added[k]), int(status[k])) == (tk, int(ad), st), k
        assert np.array_equal(W.active, a) and np.array_equal(W.inactive, i[:l - W.q]) and W.inactive.size == l - W.q, k
        At, ca, ds = gather_active_constraints(a, tk, buf.full_A(k), cx[k], bool(scal[k]))
        assert buf.block(k, got["At"])[:tk, :n].tobytes() == At.tobytes() and got["cx"][k, :tk].tobytes() == ca.tobytes(), k
        assert (got["ds"] if scal[k] else gdsn)[k, :tk].tobytes() == ds.tobytes(), k
        assert np.isnan((gdsn if scal[k] else got["ds"])[k]).all(), k      # the other kind's buffer is not touched


def test_update_working_set_starts_from_built_device_buffers(solver):
    """update_working_set_batched_dev(..., built=...) on a slot that is already on the device leaves what the default flow
    (pack_ragged and upload inside the call) leaves, bit for bit"""
    import torch
    from enlsip_gn import GNSolver, working_set as ws
    from test_gpu_delete_constraints_batched import build_flow
    m, n, t_max, B = 40, 6, 3, 9
    Ws, Cs, its, Js, rxs, As, Gs, ps, _ = build_flow(m, n, t_max, "mixed")
    ws.update_working_set_batched_dev(solver, Ws, rxs, As, Cs, Gs, Js, ps, its, ws.SQRT_EPS)
    Ws1, Cs1, its1, Js1, rxs1, As1, Gs1, ps1, _ = build_flow(m, n, t_max, "mixed")
    At, cx, t = GNSolver.pack_ragged([np.asarray(C.A).reshape(-1, n) for C in Cs1], [C.cx for C in Cs1], n=n)
    assert At.shape[1] == t_max
    ds, dsn = np.ones((B, t_max)), np.ones((B, t_max))
    for k, C in enumerate(Cs1):
        (ds if C.scaling else dsn)[k, :Ws1[k].t] = C.diag_scale
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    built = (t_max, up(At.reshape(B, -1)), up(cx), up(ds), up(dsn))
    torch.cuda.synchronize()
    ws.update_working_set_batched_dev(solver, Ws1, rxs1, As1, Cs1, Gs1, Js1, ps1, its1, ws.SQRT_EPS, built=built)
    for k in range(B):
        assert (Ws[k].t, its[k].rankA, its[k].rankJ2, its[k].delete, its[k].index_del) == \
               (Ws1[k].t, its1[k].rankA, its1[k].rankJ2, its1[k].delete, its1[k].index_del), k
        assert np.array_equal(Ws[k].active, Ws1[k].active) and np.array_equal(Ws[k].inactive, Ws1[k].inactive), k
        for a, b in ((ps[k], ps1[k]), (its[k].lam, its1[k].lam), (its[k].b_gn, its1[k].b_gn), (Cs[k].A, Cs1[k].A)):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), k
