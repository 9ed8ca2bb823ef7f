"""The line-search set-up of a batch on device buffers (enlsip_gn_linesearch_setup_batched_dev) and the driver built on it
(linesearch.linesearch_setup_batched_dev): Ap = A * p with the full constraint Jacobian (src/enlsip_functions.jl:2227),
upper_bound_steplength on it (:2149-2178) and the sums dot(Jp,Jp), dot(Jp,rx), dot(rx,rx) (:1561-1584, :2269).

- Ap: bit for bit enlsip_gn_full_constraints_times in the general form; in both forms within 2 n u sum |a||p| of the exact sum
- alpha_upp, index_alpha_upp: exactly the host routine on the downloaded Ap; the oracle's index on the gap-checked cases
  (tests/test_steplength_bound_host.py proves the gaps), alpha_upp within 1e-12 relative
- sums: within 2 m u sum |x||y| of the exact sum; bit for bit the same in another slot, another batch and another call
- nothing outside dAp[k, 0:l) is written, no input is; a negative return writes nothing at all"""
import ctypes as C
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import mpmath as mp
import numpy as np
import pytest

import linesearch_cases as lc

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

ROOT = Path(__file__).resolve().parents[1]
U = lc.U
SENT = -777.25      # what padding, guard slots and untouched outputs hold


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def batches():
    return lc.gpu_batches()


def expected_form(n, l):
    """the predicate of linesearch_wave_form in gn_linesearch_batched.inc, so that the grid follows the library"""
    txt = (ROOT / "enlsip.jl_amd" / "csrc" / "gn_linesearch_batched.inc").read_text()
    mt = re.search(r"linesearch_wave_form\([^)]*\)\s*\{\s*return\s+n\s*<=\s*([0-9]+)\s*&&\s*l\s*<=\s*([0-9]+)\s*;", txt)
    assert mt, "wave-form predicate not found in gn_linesearch_batched.inc"
    return 1 if n <= int(mt.group(1)) and l <= int(mt.group(2)) else 0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def exact_dot(x, y):
    with mp.workdps(60):
        return float(mp.fdot([float(v) for v in x], [float(v) for v in y]))


def host_bound(Ap, cx, inactive, n_inactive, index_del):
    from enlsip_gn import upper_bound_steplength
    return upper_bound_steplength(inactive, int(n_inactive), int(index_del), cx, Ap)


class Call:
    """One call on sentinel-padded device images of a batch {A (B, l, n), p, cx, inactive, n_inactive, index_del, Jp, rx}."""

    def __init__(self, b, pad=True):
        self.b = b
        self.B, self.l, self.n = b["A"].shape
        self.m = b["Jp"].shape[1]
        B, l, n = self.B, self.l, self.n
        self.lda = l + 3 if pad else max(l, 1)
        self.strideA = self.lda * n + (5 if pad else 0)
        A = np.full((B, self.strideA), SENT)
        for k in range(B):
            A[k, :self.lda * n].reshape(n, self.lda)[:, :l] = b["A"][k].T
        self.host = dict(A=A, p=b["p"].copy(), cx=b["cx"].copy(), Jp=b["Jp"].copy(), rx=b["rx"].copy(),
                         Ap=np.full((B + 2, max(l, 1)), SENT))      # slots 0 and B + 1 of Ap are guards

    def run(self, s, sums=True, index_del=True):
        import torch
        dev = {k: torch.from_numpy(v.copy()).to("cuda:0") for k, v in self.host.items()}
        torch.cuda.synchronize()
        b, l = self.b, self.l
        out = s.linesearch_setup_batched_dev(
            self.B, self.m, self.n, l, dev["p"].data_ptr(), dev["A"].data_ptr(), self.lda, self.strideA, dev["cx"].data_ptr(),
            b["inactive"], b["n_inactive"], dev["Ap"].data_ptr() + 8 * max(l, 1), index_del=b["index_del"] if index_del else None,
            dJp=dev["Jp"].data_ptr() if sums else 0, drx=dev["rx"].data_ptr() if sums else 0)
        torch.cuda.synchronize()
        self.form = s.linesearch_form()
        got = {k: v.cpu().numpy() for k, v in dev.items()}
        for k in ("A", "p", "cx", "Jp", "rx"):
            assert got[k].tobytes() == self.host[k].tobytes(), f"input {k} was written"
        assert np.all(got["Ap"][0] == SENT) and np.all(got["Ap"][-1] == SENT), "a guard slot of dAp was written"
        Ap = got["Ap"][1:-1, :l]
        return Ap, out[0], out[1], out[2]


def check_batch(s, name, b, sums_too=True):
    """every assertion of the issue that holds for a random (gap-checked) batch"""
    c = Call(b)
    Ap, alpha, index, sums = c.run(s, sums=sums_too)
    B, l, n, m = c.B, c.l, c.n, c.m
    assert c.form == expected_form(n, l), name
    worst = 0.0
    for k in range(B):
        A, p, cx = b["A"][k], b["p"][k], b["cx"][k]
        if c.form == 0:
            assert same(Ap[k], s.full_constraints_times(A, p)), (name, k, "Ap differs from enlsip_gn_full_constraints_times")
        mag = np.abs(A) @ np.abs(p)
        for j in range(l):
            err = abs(Ap[k, j] - exact_dot(A[j], p))
            assert err <= 2 * n * U * mag[j], (name, k, j, err, 2 * n * U * mag[j])
            worst = max(worst, err / (2 * n * U * mag[j]) if mag[j] else 0.0)
        want = host_bound(Ap[k], cx, b["inactive"][k], b["n_inactive"][k], b["index_del"][k])
        assert same(alpha[k], want[0]) and index[k] == want[1], (name, k, (alpha[k], index[k]), want)
        W = SimpleNamespace(inactive=b["inactive"][k], t=l - int(b["n_inactive"][k]), l=l)
        with np.errstate(all="ignore"):
            oa, oi = lc.eo.upper_bound_steplength(A, cx, p, W, int(b["index_del"][k]))
        print(f"{name} k={k} alpha {alpha[k]!r} oracle {oa!r} index {index[k]} oracle {oi}")
        assert index[k] == oi and abs(alpha[k] - oa) <= 1e-12 * abs(oa), (name, k, alpha[k], oa, index[k], oi)
        if sums_too:
            x, y = b["Jp"][k], b["rx"][k]
            for q, (u, v) in enumerate(((x, x), (x, y), (y, y))):
                ref, bound = exact_dot(u, v), 2 * m * U * float(np.abs(u) @ np.abs(v))
                print(f"{name} k={k} sum {q}: err/bound = {abs(sums[k, q] - ref) / bound:.3f}")
                assert abs(sums[k, q] - ref) <= bound, (name, k, q, sums[k, q], ref, bound)
    print(f"{name}: worst Ap err/bound {worst:.3f}")
    return Ap, alpha, index, sums


@pytest.mark.parametrize("name", [g[0] for g in lc.GPU_SHAPES])
def test_random_batches(solver, batches, name):
    check_batch(solver, name, batches[name])


@pytest.mark.parametrize("name", ["wave_m5000", "gen_l600_list590", "gen_l257", "wave_n63_l64"])
def test_sums_do_not_depend_on_slot_batch_or_call_and_are_optional(solver, batches, name):
    b = batches[name]
    c = Call(b)
    Ap, alpha, index, sums = c.run(solver)
    # the same problems in other slots of a larger batch, in another call
    order = np.array([3, 0, 4, 4, 1, 2, 0])
    b2 = {k: v[order] for k, v in b.items()}
    Ap2, alpha2, index2, sums2 = Call(b2, pad=False).run(solver)
    for i, k in enumerate(order):
        assert same(sums2[i], sums[k]) and same(Ap2[i], Ap[k]) and same(alpha2[i], alpha[k]) and index2[i] == index[k], (name, i, k)
    # a batch of one
    b1 = {k: v[2:3] for k, v in b.items()}
    Ap1, alpha1, index1, sums1 = Call(b1).run(solver)
    assert same(sums1[0], sums[2]) and same(Ap1[0], Ap[2]) and same(alpha1[0], alpha[2]) and index1[0] == index[2]
    # without the sums nothing else changes
    Ap0, alpha0, index0, sums0 = c.run(solver, sums=False)
    assert sums0 is None and same(Ap0, Ap) and same(alpha0, alpha) and np.array_equal(index0, index)
    # index_del = NULL is 0 everywhere
    bz = dict(b, index_del=np.zeros_like(b["index_del"]))
    _, alpha_z, index_z, _ = Call(bz).run(solver)
    _, alpha_n, index_n, _ = Call(b).run(solver, index_del=False)
    assert same(alpha_n, alpha_z) and np.array_equal(index_n, index_z)


@pytest.mark.parametrize("n,l", [(3, 8), (70, 8), (3, 300), (1, 64), (64, 64)])
def test_named_edges_in_both_forms(solver, n, l):
    edges = lc.edge_cases(l)
    rng = np.random.default_rng(5)
    real = [lc.realise(Ap, n, rng) for _, cx, Ap, *_ in edges]
    b = dict(A=np.stack([r[0] for r in real]), p=np.stack([r[1] for r in real]), cx=np.stack([e[1] for e in edges]),
             inactive=np.stack([e[3] for e in edges]), n_inactive=np.array([e[4] for e in edges], dtype=np.int64),
             index_del=np.array([e[5] for e in edges], dtype=np.int64), Jp=np.ones((len(edges), 3)), rx=np.ones((len(edges), 3)))
    c = Call(b)
    Ap, alpha, index, _ = c.run(solver)
    assert c.form == expected_form(n, l)
    for k, (name, cx, Ap_want, lst, ni, idel, want) in enumerate(edges):
        assert np.array_equal(Ap[k], Ap_want, equal_nan=True), name      # the product realises the edge exactly
        got = (float(alpha[k]), int(index[k]))
        host = host_bound(Ap[k], cx, lst, ni, idel)
        oracle = lc.oracle_bound(Ap[k], cx, lst, ni, idel)
        assert same(got[0], host[0]) and got[1] == host[1], (name, got, host)
        assert same(got[0], oracle[0]) and got[1] == oracle[1], (name, got, oracle)
        assert want is None or (same(got[0], want[0]) and got[1] == want[1]), (name, got, want)


@pytest.mark.parametrize("n,l,m", [(2, 3, 2), (65, 3, 2)], ids=["wave", "general"])
def test_batch_beyond_the_grid_y_limit(solver, n, l, m):
    B, distinct = 65537, 7
    base = lc.random_batch(77, distinct, n, l, m)
    slot = np.arange(B) % distinct
    slot[-1] = 3
    b = {k: v[slot] for k, v in base.items()}
    c = Call(b, pad=False)
    Ap, alpha, index, sums = c.run(solver)
    assert c.form == expected_form(n, l)
    for d in range(distinct):
        first = int(np.flatnonzero(slot == d)[0])
        where = slot == d
        assert np.array_equal(bits(Ap[where]), np.broadcast_to(bits(Ap[first]), (where.sum(), l))), d
        assert np.all(bits(alpha[where]) == bits(alpha[first])[0]) and np.all(index[where] == index[first]), d
        assert np.array_equal(bits(sums[where]), np.broadcast_to(bits(sums[first]), (where.sum(), 3))), d
        want = host_bound(Ap[first], base["cx"][d], base["inactive"][d], base["n_inactive"][d], base["index_del"][d])
        assert same(alpha[first], want[0]) and index[first] == want[1]
        mag = np.abs(base["A"][d]) @ np.abs(base["p"][d])
        for j in range(l):
            assert abs(Ap[first, j] - exact_dot(base["A"][d][j], base["p"][d])) <= 2 * n * U * mag[j]
        x, y = base["Jp"][d], base["rx"][d]
        for q, (u, v) in enumerate(((x, x), (x, y), (y, y))):
            assert abs(sums[first, q] - exact_dot(u, v)) <= 2 * m * U * float(np.abs(u) @ np.abs(v))


def test_l_zero_and_empty_lists(solver):
    import torch
    B, n, m = 5, 4, 300
    rng = np.random.default_rng(9)
    Jp, rx = rng.standard_normal((B, m)), rng.standard_normal((B, m))
    dJp, drx, dp = (torch.from_numpy(a).to("cuda:0") for a in (Jp, rx, rng.standard_normal((B, n))))
    for nn in (n, 65):      # both forms
        alpha, index, sums = solver.linesearch_setup_batched_dev(B, m, nn, 0, 0, 0, 1, nn, 0, np.zeros((B, 0), dtype=np.int64),
                                                                 np.zeros(B, dtype=np.int64), 0, dJp=dJp.data_ptr(), drx=drx.data_ptr())
        assert np.all(alpha == 3.0) and not index.any()
        for k in range(B):
            for q, (u, v) in enumerate(((Jp[k], Jp[k]), (Jp[k], rx[k]), (rx[k], rx[k]))):
                assert abs(sums[k, q] - exact_dot(u, v)) <= 2 * m * U * float(np.abs(u) @ np.abs(v))
        alpha, index, sums = solver.linesearch_setup_batched_dev(B, 0, nn, 0, dp.data_ptr(), 0, 1, nn, 0, np.zeros((B, 0), dtype=np.int64),
                                                                 np.zeros(B, dtype=np.int64), 0)
        assert np.all(alpha == 3.0) and not index.any() and sums is None


def test_argument_errors_leave_everything_untouched(solver):
    import torch
    import enlsip_gn._lib as Lm
    L = Lm.load()
    B, m, n, l = 4, 6, 3, 5
    b = lc.random_batch(1, B, n, l, m)
    c = Call(b)
    dev = {k: torch.from_numpy(v.copy()).to("cuda:0") for k, v in c.host.items()}
    torch.cuda.synchronize()
    alpha, index, sums = np.full(B, SENT), np.full(B, -9, dtype=np.int64), np.full((B, 3), SENT)
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    v = lambda nm: C.c_void_p(dev[nm].data_ptr())
    h = solver._h
    good = dict(h=h, batch=B, m=m, n=n, l=l, dp=v("p"), dA=v("A"), lda=c.lda, strideA=c.strideA, dcx=v("cx"),
                inactive=b["inactive"], n_inactive=b["n_inactive"], index_del=b["index_del"], dJp=v("Jp"), drx=v("rx"),
                dAp=C.c_void_p(dev["Ap"].data_ptr() + 8 * l), alpha=alpha, index=index, sums=sums)

    def call(**kw):
        a = dict(good, **kw)
        return L.enlsip_gn_linesearch_setup_batched_dev(
            a["h"], a["batch"], a["m"], a["n"], a["l"], a["dp"], a["dA"], a["lda"], a["strideA"], a["dcx"], hp(a["inactive"]),
            hp(a["n_inactive"]), hp(a["index_del"]), a["dJp"], a["drx"], a["dAp"], hp(a["alpha"]), hp(a["index"]), hp(a["sums"]))

    def edited(name, k, i, value):
        x = b[name].copy()
        if i is None:
            x[k] = value
        else:
            x[k, i] = value
        return x

    ni3 = int(b["n_inactive"][3])
    cases = [
        (-1, dict(h=None), None), (-2, dict(batch=0), None), (-3, dict(n=0), None), (-3, dict(n=1025), None),
        (-3, dict(l=-1), None), (-3, dict(m=0), None),
        (-4, dict(dp=None), None), (-4, dict(dA=None), None), (-4, dict(dcx=None), None), (-4, dict(inactive=None), None),
        (-4, dict(n_inactive=None), None), (-4, dict(dAp=None), None), (-4, dict(alpha=None), None), (-4, dict(index=None), None),
        (-4, dict(dJp=None), None), (-4, dict(drx=None), None), (-4, dict(sums=None), None), (-4, dict(dJp=None, drx=None), None),
        (-5, dict(n_inactive=edited("n_inactive", 2, None, l + 1)), "[2]"), (-5, dict(n_inactive=edited("n_inactive", 1, None, -1)), "[1]"),
        (-6, dict(index_del=edited("index_del", 3, None, l + 1)), "[3]"), (-6, dict(index_del=edited("index_del", 0, None, -1)), "[0]"),
        (-9, dict(lda=l - 1), None), (-10, dict(strideA=c.lda * n - 1), None),
    ]
    # two faults at once: every n_inactive[k] is checked before any index_del[k] or list, the lists before the leading dimension
    kq = int(np.flatnonzero(b["n_inactive"] > 0)[0])
    cases.append((-5, dict(n_inactive=edited("n_inactive", 2, None, l + 1), index_del=edited("index_del", 2, None, l + 1)), "n_inactive[2]"))
    cases.append((-6, dict(inactive=edited("inactive", kq, 0, -1), lda=l - 1), f"inactive[{kq}][0]"))
    if ni3:
        cases.append((-6, dict(inactive=edited("inactive", 3, ni3 - 1, l + 1)), "[3]"))
        cases.append((-6, dict(inactive=edited("inactive", 3, 0, -1)), "[3]"))
    seen = set()
    for want, kw, names in cases:
        got = call(**kw)
        assert got == want, (want, got, list(kw))
        if want != -1:
            msg = L.enlsip_gn_last_error(h).decode()
            assert msg and (names is None or names in msg), (want, msg)
            seen.add(msg)
    assert len(seen) >= 9
    torch.cuda.synchronize()
    assert np.all(alpha == SENT) and np.all(index == -9) and np.all(sums == SENT)
    for k in c.host:
        assert dev[k].cpu().numpy().tobytes() == c.host[k].tobytes(), k
    # a list entry out of range past the used part is not read, m is not read without the sums
    assert call(inactive=edited("inactive", 0, l - 1, l + 7) if b["n_inactive"][0] < l else b["inactive"]) == 0
    assert call(m=0, dJp=None, drx=None, sums=None) == 0


def test_fresh_handle_and_between_factor_and_solve(solver, batches):
    import torch
    from enlsip_gn import GNSolver
    from test_gpu_factored_batched import pack, same as same_any
    from test_gpu_ragged_batch import make_batch
    m, n, t_max, B = 48, 12, 4, 5
    ts = [4, 2, 0, 3, 4]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=19)
    As = [A if tk else np.zeros((0, n)) for A, tk in zip(As, ts)]
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(a).to(dev)
    dJ, drx, dAt, dcx = up(J), up(rx), up(At), up(cx)
    dp, dp_ref = (torch.zeros((B, n), dtype=torch.float64, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    b = batches["wave_n63_l64"]
    want = Call(b).run(solver)
    s, ref = GNSolver(device=0), GNSolver(device=0)
    try:
        def setup():
            got = Call(b).run(s)
            assert same(got[0], want[0]) and same(got[1], want[1]) and np.array_equal(got[2], want[2]) and same(got[3], want[3])
        assert s.linesearch_form() == -1
        setup()                                      # nothing resident at all
        assert s.linesearch_form() == 1
        A_args = (dAt.data_ptr(), n, n * t_max, dcx.data_ptr())
        s.factor_constraints_batched_dev(B, m, n, t_max, t, *A_args)
        setup()                                      # between the factor call and its solve, on other buffers
        s.solve_factored_batched_dev(B, m, n, t_max, t, None, dJ.data_ptr(), m, m * n, drx.data_ptr(), *A_args, dp=dp.data_ptr())
        ref.factor_constraints_batched_dev(B, m, n, t_max, t, *A_args)
        ref.solve_factored_batched_dev(B, m, n, t_max, t, None, dJ.data_ptr(), m, m * n, drx.data_ptr(), *A_args, dp=dp_ref.data_ptr())
        torch.cuda.synchronize()
        assert same_any(dp.cpu().numpy(), dp_ref.cpu().numpy()) and np.isfinite(dp.cpu().numpy()).all()
    finally:
        s.close()
        ref.close()


def test_driver_against_the_oracle(solver):
    """linesearch.linesearch_setup_batched_dev on a small ragged resident batch against oracle/enlsip_outer.py's Jp, Ap, alpha_upp,
    index and dot products.  The device Jp and the oracle's differ by the rounding of two sums of n terms, at most
    d_i = 4 n u (|J||p|)_i per entry, so a dot product of m terms formed from them differs from the oracle's by at most
    2 m u sum |x||y| (its own rounding, twice) plus the first-order effect of d on it."""
    import torch
    from enlsip_gn import GNSolver, linesearch as ls, working_set as ws
    from oracle import synth
    m, n, t_max, l, B, q = 40, 6, 3, 9, 5, 1
    ts = [3, 2, 1, 3, 2]
    Ws, its, Js, rxs, As, cxs, ps = [], [], [], [], [], [], []
    for k, tk in enumerate(ts):
        A = synth.normal_stream(500 + k, 1, l * n).reshape(l, n)
        J = synth.normal_stream(500 + k, 2, m * n).reshape(m, n)
        rx = synth.normal_stream(500 + k, 3, m)
        cx = synth.normal_stream(500 + k, 4, l)
        W = ws.WorkingSet.create(q, l)
        for _ in range(tk - q):
            W.add_constraint(2)      # leaves row q + 1 inactive: active = 1, 3, 4, ...
        it = ws.IterationRecord()
        it.index_del = int(W.inactive[k % (l - tk)]) if k % 2 else 0
        Ws.append(W); its.append(it); Js.append(J); rxs.append(rx); As.append(A); cxs.append(cx)
    act = [W.active[:W.t] - 1 for W in Ws]
    At, cxa, t = GNSolver.pack_ragged([A[a] for A, a in zip(As, act)], [c[a] for c, a in zip(cxs, act)], n=n)
    assert At.shape[1] == t_max
    Jd = np.stack([np.asfortranarray(Jk).T for Jk in Js])
    out = solver.solve_batched_ragged(Jd, np.stack(rxs), At, cxa, t)
    p = np.ascontiguousarray(out[0])
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    dA = up(np.stack([np.asfortranarray(A).T for A in As]))      # (B, n, l): problem k l x n column-major
    got = ls.linesearch_setup_batched_dev(solver, Ws, its, up(p), dA, up(np.stack(cxs)), up(np.stack(rxs)), t_max)
    torch.cuda.synchronize()
    assert solver.linesearch_form() == expected_form(n, l)
    Jp, Ap, actAp = got.Jp.cpu().numpy(), got.Ap.cpu().numpy(), got.active_Ap.cpu().numpy()
    for k in range(B):
        J, A, rx, cx, W = Js[k], As[k], rxs[k], cxs[k], Ws[k]
        oJp, oAp, oact = J @ p[k], A @ p[k], A[act[k]] @ p[k]
        dJ = 4 * n * U * (np.abs(J) @ np.abs(p[k]))
        assert np.all(np.abs(Jp[k] - oJp) <= dJ)
        assert np.all(np.abs(Ap[k] - oAp) <= 4 * n * U * (np.abs(A) @ np.abs(p[k])))
        assert np.all(np.abs(actAp[k, :W.t] - oact) <= 4 * n * U * (np.abs(A[act[k]]) @ np.abs(p[k]))) and not actAp[k, W.t:].any()
        with np.errstate(all="ignore"):
            oa, oi = lc.eo.upper_bound_steplength(A, cx, p[k], W, its[k].index_del)
        gap, margin, cond = lc.gap_report(A, p[k], cx, W.inactive, l - W.t, its[k].index_del)
        assert gap > lc.GAP and margin > lc.GAP and 4 * n * U * cond <= 1e-12
        assert got.index_alpha_upp[k] == oi and abs(got.alpha_upp[k] - oa) <= 1e-12 * abs(oa), (k, got.alpha_upp[k], oa)
        assert (got.alpha_upp[k], got.index_alpha_upp[k]) == ls.upper_bound_steplength(Ap[k], cx, W, its[k].index_del)
        for val, x, y, dx, dy in ((got.JpJp[k], oJp, oJp, dJ, dJ), (got.Jprx[k], oJp, rx, dJ, 0 * dJ), (got.rxrx[k], rx, rx, 0 * dJ, 0 * dJ)):
            tol = 4 * m * U * float(np.abs(x) @ np.abs(y)) + float(dx @ np.abs(y)) + float(np.abs(x) @ dy) + float(dx @ dy)
            assert abs(val - float(x @ y)) <= tol, (k, val, float(x @ y), tol)
