"""The penalty weights and the merit function of a batch on device buffers (enlsip_gn_penalty_weights_batched_dev,
enlsip_gn_merit_batched_dev) and the drivers built on them (linesearch.penalty_weights_batched_dev, linesearch.merit_batched_dev):
penalty_weight_update (src/enlsip_functions.jl:1545-1629), psi(0) (:2243), atwa (:2268) and psi (:1307-1340).

- w, K, scalars and branch of every problem: bit for bit the host routine (enlsip_gn_penalty_weight_update) on the downloaded inputs,
  in both kernel forms, with and without scaling (the host routine is handed active_Ap / diag_scale), with dw == dw_old, in another
  slot and another batch; the host routine itself is held to the oracle by tests/test_penalty_weights_host.py
- sentinel-filled guard slots (around every buffer, past t[k], the whole of a problem not taken) stay untouched, no input changes,
  a negative return writes nothing
- the driver on a solved resident ragged batch against the oracle, with the host test's envelope tolerance and stability check
- psi within (m + l + 4) u * 0.5 * (sum rx^2 + sum |w| cx^2) of the exact value (mpmath, over the entries that enter): the bound of
  any order of a sum of m + l rounded products, two roundings each, and the final add and halving; bit for bit the same in another
  slot, another batch and a second call"""
import ctypes as C
import re
import sys
from pathlib import Path

import mpmath as mp
import numpy as np
import pytest

import penalty_cases as pc

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

ROOT = Path(__file__).resolve().parents[1]
U = pc.U
SENT = -777.25      # what padding, guard slots and untouched outputs hold
same = pc.same_bits


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def expected_form(t_max, l):
    """the predicate of penalty_wave_form in gn_penalty_batched.inc, so that the test follows the library"""
    txt = (ROOT / "enlsip.jl_amd" / "csrc" / "gn_penalty_batched.inc").read_text()
    mt = re.search(r"penalty_wave_form\([^)]*\)\s*\{\s*return\s+t_max\s*<=\s*([0-9]+)\s*&&\s*l\s*<=\s*([0-9]+)\s*;", txt)
    assert mt, "wave-form predicate not found in gn_penalty_batched.inc"
    return 1 if t_max <= int(mt.group(1)) and l <= int(mt.group(2)) else 0


def host(c, Ap, sums):
    """the host routine on one problem: (w, scalars (3,), branch, K)"""
    from enlsip_gn import penalty_weight_update
    w, d, p0, a, br, K = penalty_weight_update(c["w_old"], c["active"], c["t"], c["dimA"], c["norm_code"], Ap, c["cx"], c["K"].copy(), *sums)
    return w, np.array([d, p0, a]), br, K


def host_branch(c):
    return host(c, c["Ap"], pc.exact_sums(c))[2]


class Call:
    """One call on sentinel-guarded device images of `probs` (cases of one norm code, l entries each, t <= t_max).  Slots 0 and
    B + 1 of every buffer are guards."""

    def __init__(self, probs, l, t_max, norm_code, scaling, take=None, seed=3):
        self.probs, self.l, self.t_max, self.norm_code, self.scaling = probs, l, t_max, norm_code, scaling
        B = self.B = len(probs)
        rng = np.random.default_rng(seed)
        assert all(c["l"] == l and c["t"] <= t_max and c["norm_code"] == norm_code for c in probs)
        self.take = None if take is None else np.asarray(take, dtype=np.int64)
        self.t = np.array([c["t"] for c in probs], dtype=np.int64)
        self.dimA = np.array([c["dimA"] for c in probs], dtype=np.int64)
        self.active = np.zeros((B, t_max), dtype=np.int64)
        self.sums = np.array([pc.exact_sums(c) for c in probs]).reshape(B, 3)
        g = lambda *shape: np.full(shape, SENT)
        h = dict(w_old=g(B + 2, max(l, 1)), cx=g(B + 2, max(l, 1)), K=g(B + 2, 4, max(l, 1)), Ap=g(B + 2, max(t_max, 1)),
                 ds=g(B + 2, max(t_max, 1)), w=g(B + 2, max(l, 1)))
        for k, c in enumerate(probs):
            t = c["t"]
            self.active[k, :t] = c["active"][:t]
            h["w_old"][k + 1, :l], h["cx"][k + 1, :l], h["K"][k + 1, :, :l] = c["w_old"], c["cx"], c["K"]
            h["Ap"][k + 1, :t] = c["Ap"]
            h["ds"][k + 1, :t] = 2.0 ** rng.integers(-2, 3, t) * (1.0 + rng.random(t))
        self.host = h

    def reference(self, k):
        c = self.probs[k]
        Ap = self.host["Ap"][k + 1, :c["t"]]
        if self.scaling:
            Ap = Ap / self.host["ds"][k + 1, :c["t"]]
        return host(c, Ap, self.sums[k])

    def run(self, s, alias=False):
        import torch
        dev = {k: torch.from_numpy(v.copy()).to("cuda:0") for k, v in self.host.items()}
        torch.cuda.synchronize()
        l, t_max, B = self.l, self.t_max, self.B
        at = lambda nm, per: dev[nm].data_ptr() + 8 * per
        L1, T1 = max(l, 1), max(t_max, 1)
        dw = at("w_old", L1) if alias else at("w", L1)
        scalars, branch = s.penalty_weights_batched_dev(
            B, l, t_max, self.t, self.dimA, self.active, self.norm_code, self.scaling, at("w_old", L1), at("Ap", T1),
            at("ds", T1) if self.scaling else 0, at("cx", L1), at("K", 4 * L1), self.sums, dw, take=self.take)
        torch.cuda.synchronize()
        self.form = s.penalty_form()
        got = {k: v.cpu().numpy() for k, v in dev.items()}
        for k in ("cx", "Ap", "ds") + (() if alias else ("w_old",)):
            assert got[k].tobytes() == self.host[k].tobytes(), f"input {k} was written"
        for k in ("w", "K", "w_old"):
            assert np.all(got[k][0] == SENT) and np.all(got[k][-1] == SENT), f"a guard slot of {k} was written"
        w = got["w_old" if alias else "w"][1:-1, :l]
        if alias:
            assert np.all(got["w"] == SENT)
        return w, got["K"][1:-1, :, :l], scalars, branch

    def check(self, s, alias=False):
        w, K, scalars, branch = self.run(s, alias)
        assert self.form == expected_form(self.t_max, self.l)
        for k, c in enumerate(self.probs):
            if self.take is not None and self.take[k] == 0:
                untouched = c["w_old"] if alias else np.full(self.l, SENT)
                assert same(w[k], untouched) and same(K[k], c["K"]) and not scalars[k].any() and branch[k] == 0, k
                continue
            hw, hs, hb, hK = self.reference(k)
            assert branch[k] == hb, (k, branch[k], hb)
            assert same(w[k], hw), (k, w[k], hw)
            assert same(K[k], hK), (k, K[k], hK)
            assert same(scalars[k], hs), (k, scalars[k], hs)
        return w, K, scalars, branch


# ---- the problems ------------------------------------------------------------------------------------------------------------------
def small_by_branch(norm_code, l, t_max, count, seed):
    """`count` cases of penalty_cases.host_cases() with this norm code inside problems of l constraints, every branch first"""
    rng = np.random.default_rng(seed)
    pool = [c for c in pc.host_cases() if c["norm_code"] == norm_code and c["l"] <= l and c["t"] <= t_max]
    tagged = [(host_branch(c), c) for c in pool]
    out, seen = [], set()
    for b, c in tagged:                       # one per branch
        if b not in seen:
            seen.add(b)
            out.append(c)
    for b, c in tagged:                       # then whatever comes, named cases first
        if len(out) >= count:
            break
        if all(c is not o for o in out) and not c["name"].startswith("random"):
            out.append(c)
    for b, c in tagged:
        if len(out) >= count:
            break
        if all(c is not o for o in out):
            out.append(c)
    assert seen == ({0} if norm_code == 0 else {0, 1, 2, 3, 4})
    return [pc.padded(c, l, t_max, rng) for c in out[:count]]


@pytest.fixture(scope="module")
def form1():
    return {nc: small_by_branch(nc, 12, 8, 9, 40 + nc) for nc in (0, 2)}


@pytest.fixture(scope="module")
def form0():
    """l = 80, t_max = 70: five problems per norm code; small cases padded up to the strides and cases with t > 64"""
    rng = np.random.default_rng(50)
    small = {nc: small_by_branch(nc, 80, 70, 5, 60 + nc) for nc in (0, 2)}
    by_branch = {host_branch(c): c for c in small[2]}
    big = pc.wanted(host_branch, 2, [1, 3], 80, [70, 66], seed=51)
    big0 = pc.wanted(host_branch, 0, [0, 0], 80, [70, 65], seed=52)
    del rng
    return {2: [by_branch[0], big[0], by_branch[2], big[1], by_branch[4]], 0: small[0][:3] + big0}


@pytest.mark.parametrize("norm_code", [0, 2])
@pytest.mark.parametrize("scaling", [False, True])
def test_form1_nine_problems(solver, form1, norm_code, scaling):
    c = Call(form1[norm_code], 12, 8, norm_code, scaling)
    _, _, _, branch = c.check(solver)
    assert c.form == 1
    if not scaling:      # the problems were picked by their branch on the unscaled active_Ap
        assert set(branch) == ({0} if norm_code == 0 else {0, 1, 2, 3, 4})


@pytest.mark.parametrize("norm_code", [0, 2])
@pytest.mark.parametrize("scaling", [False, True])
def test_form0_five_problems(solver, form0, norm_code, scaling):
    c = Call(form0[norm_code], 80, 70, norm_code, scaling)
    _, _, _, branch = c.check(solver)
    assert c.form == 0 and max(p["t"] for p in c.probs) > 64
    if not scaling:
        assert set(branch) == ({0} if norm_code == 0 else {0, 1, 2, 3, 4})


@pytest.mark.parametrize("which", ["form0", "form1"])
def test_alias_take_slot_and_batch(solver, form0, form1, which):
    probs, l, t_max = (form0[2], 80, 70) if which == "form0" else (form1[2], 12, 8)
    base = Call(probs, l, t_max, 2, True)
    w, K, scalars, branch = base.check(solver)
    # dw == dw_old gives the same bits
    wa, Ka, sa, ba = Call(probs, l, t_max, 2, True).check(solver, alias=True)
    assert same(wa, w) and same(Ka, K) and same(sa, scalars) and np.array_equal(ba, branch)
    # problems not taken: nothing of them is written, with separate buffers and in place
    take = np.ones(len(probs), dtype=np.int64)
    take[[1, len(probs) - 1]] = 0
    for alias in (False, True):
        wt, Kt, st, bt = Call(probs, l, t_max, 2, True, take=take).check(solver, alias=alias)
        for k in np.flatnonzero(take):
            assert same(wt[k], w[k]) and same(Kt[k], K[k]) and same(st[k], scalars[k]) and bt[k] == branch[k]
    # the same problems in other slots of another batch (same scale factors: they are drawn per slot, so reuse the inputs)
    order = [3, 0, 4, 4, 1, 2, 0]
    other = Call([probs[i] for i in order], l, t_max, 2, False)
    plain = Call(probs, l, t_max, 2, False)
    w0, K0, s0, b0 = plain.check(solver)
    w2, K2, s2, b2 = other.check(solver)
    for i, k in enumerate(order):
        assert same(w2[i], w0[k]) and same(K2[i], K0[k]) and same(s2[i], s0[k]) and b2[i] == b0[k], (i, k)
    one = Call(probs[2:3], l, t_max, 2, False).check(solver)
    assert same(one[0][0], w0[2]) and same(one[1][0], K0[2]) and same(one[2][0], s0[2]) and one[3][0] == b0[2]


@pytest.mark.parametrize("norm_code", [0, 2])
def test_batch_beyond_the_grid_y_limit(solver, norm_code):
    B, l, t_max = 70000, 3, 2
    rng = np.random.default_rng(70 + norm_code)
    distinct = []
    while len(distinct) < 7:
        c = pc.random_case(rng, len(distinct) % 6, l=l, t=int(rng.integers(0, 3)), m=4, norm_code=norm_code)
        distinct.append(c)
    slot = np.arange(B) % 7
    slot[-1] = 3
    c = Call([distinct[i] for i in slot], l, t_max, norm_code, False)
    w, K, scalars, branch = c.run(solver)
    assert c.form == expected_form(t_max, l)
    for d in range(7):
        where = slot == d
        first = int(np.flatnonzero(where)[0])
        hw, hs, hb, hK = c.reference(first)
        assert same(w[first], hw) and same(K[first], hK) and same(scalars[first], hs) and branch[first] == hb, d
        n = int(where.sum())
        bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
        assert np.array_equal(bits(w[where]), np.broadcast_to(bits(w[first]), (n, l))), d
        assert np.array_equal(bits(K[where]), np.broadcast_to(bits(K[first]), (n, 4, l))), d
        assert np.array_equal(bits(scalars[where]), np.broadcast_to(bits(scalars[first]), (n, 3))) and np.all(branch[where] == hb), d


def test_no_constraints_and_fresh_handle(solver):
    import torch
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    try:
        assert s.penalty_form() == -1
        sums = np.array([[4.0, 1.0, 9.0], [1.0, -3.0, 16.0]])
        z = np.zeros(2, dtype=np.int64)
        for nc in (0, 2):
            sc, br = s.penalty_weights_batched_dev(2, 0, 0, z, z, np.zeros((2, 0), dtype=np.int64), nc, False, 0, 0, 0, 0, 0, sums, 0)
            assert same(sc, np.array([[1.0, 4.5, 0.0], [-3.0, 8.0, 0.0]])) and not br.any()
        assert s.penalty_form() == 1
        # l > 0 with t_max == 0: the t-strided buffers may be NULL
        c = pc.random_case(np.random.default_rng(1), 0, l=4, t=0, m=3, norm_code=2)
        call = Call([c, c], 4, 0, 2, False)
        call.check(s)
    finally:
        s.close()
    del torch


def test_argument_errors_write_nothing(solver, form1):
    import torch
    import enlsip_gn._lib as Lm
    L = Lm.load()
    probs, l, t_max = form1[2][:4], 12, 8
    B = len(probs)
    c = Call(probs, l, t_max, 2, True)
    dev = {k: torch.from_numpy(v.copy()).to("cuda:0") for k, v in c.host.items()}
    torch.cuda.synchronize()
    scalars, branch = np.full((B, 3), SENT), np.full(B, -9, dtype=np.int32)
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    v = lambda nm, per: C.c_void_p(dev[nm].data_ptr() + 8 * per)
    h = solver._h
    good = dict(h=h, batch=B, l=l, t_max=t_max, t=c.t, dimA=c.dimA, active=c.active, take=None, norm_code=2, scaling=1,
                dw_old=v("w_old", l), dAp=v("Ap", t_max), dds=v("ds", t_max), dcx=v("cx", l), dK=v("K", 4 * l), sums=c.sums,
                dw=v("w", l), scalars=scalars, branch=branch)

    def call(**kw):
        a = dict(good, **kw)
        return L.enlsip_gn_penalty_weights_batched_dev(
            a["h"], a["batch"], a["l"], a["t_max"], hp(a["t"]), hp(a["dimA"]), hp(a["active"]), hp(a["take"]), a["norm_code"],
            a["scaling"], a["dw_old"], a["dAp"], a["dds"], a["dcx"], a["dK"], hp(a["sums"]), a["dw"], hp(a["scalars"]), hp(a["branch"]))

    def edited(x, idx, value):
        x = x.copy()
        x[idx] = value
        return x

    k3 = int(np.flatnonzero(c.t > 0)[-1])
    cases = [
        (-1, dict(h=None), None), (-2, dict(batch=0), None), (-3, dict(l=-1), None), (-3, dict(t_max=1025, l=2000), None),
        (-3, dict(t_max=-1), None), (-3, dict(t_max=l + 1), None), (-3, dict(norm_code=1), None), (-3, dict(l=(1 << 27) + 1), None),
        (-4, dict(t=None), None), (-4, dict(dimA=None), None), (-4, dict(active=None), None), (-4, dict(sums=None), None),
        (-4, dict(scalars=None), None), (-4, dict(branch=None), None), (-4, dict(dw_old=None), None), (-4, dict(dAp=None), None),
        (-4, dict(dds=None), None), (-4, dict(dcx=None), None), (-4, dict(dK=None), None), (-4, dict(dw=None), None),
        (-5, dict(t=edited(c.t, 2, t_max + 1)), "[2]"), (-5, dict(t=edited(c.t, 1, -1)), "[1]"),
        (-6, dict(dimA=edited(c.dimA, 0, int(c.t[0]) + 1)), "[0]"), (-6, dict(dimA=edited(c.dimA, 3, -1)), "[3]"),
        (-6, dict(active=edited(c.active, (k3, 0), 0)), f"[{k3}]"), (-6, dict(active=edited(c.active, (k3, int(c.t[k3]) - 1), l + 1)), f"[{k3}]"),
        # two faults at once: every t[k] is checked before any dimA[k], and dimA[k] before the list of row k and of the rows behind it
        (-5, dict(t=edited(c.t, 2, t_max + 1), dimA=edited(c.dimA, 0, -1)), "t[2]"),
        (-6, dict(dimA=edited(c.dimA, 0, -1), active=edited(c.active, (k3, 0), 0)), "dimA[0]"),
    ]
    for want, kw, names in cases:
        got = call(**kw)
        assert got == want, (want, got, list(kw))
        if want != -1:
            msg = L.enlsip_gn_last_error(h).decode()
            assert msg and (names is None or names in msg), (want, msg)
    torch.cuda.synchronize()
    assert np.all(scalars == SENT) and np.all(branch == -9)
    for k in c.host:
        assert dev[k].cpu().numpy().tobytes() == c.host[k].tobytes(), k
    # ddiag_scale is required only with scaling; an active entry past t[k] is not read
    assert call(dds=None, scaling=0) == 0
    if c.t[0] < t_max:
        assert call(active=edited(c.active, (0, t_max - 1), l + 9)) == 0


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_code", [0, 2])
def test_driver_against_the_oracle(solver, weight_code):
    """jacobian_times_batched_dev, linesearch_setup_batched_dev and penalty_weights_batched_dev on a solved resident ragged batch
    (m = 24, n = 6, l = 5, t from 0 to 4) against the oracle's penalty_weight_update on the downloaded Jp, active_Ap, rx, cx, with
    the tolerance and the stability check of tests/test_penalty_weights_host.py."""
    import torch
    from enlsip_gn import GNSolver, linesearch as ls, working_set as ws
    from oracle import synth
    m, n, l, q = 24, 6, 5, 0
    ts = [0, 1, 2, 3, 4, 4]
    B = len(ts)
    rng = np.random.default_rng(90 + weight_code)
    Ws, its, Js, rxs, As, cxs = [], [], [], [], [], []
    for k, tk in enumerate(ts):
        A = synth.normal_stream(700 + k, 1, l * n).reshape(l, n)
        J = synth.normal_stream(700 + k, 2, m * n).reshape(m, n)
        rx = synth.normal_stream(700 + k, 3, m)
        cx = synth.normal_stream(700 + k, 4, l)
        W = ws.WorkingSet.create(q, l)
        for _ in range(tk):
            W.add_constraint(2 if W.l - W.t > 1 else 1)
        it = ws.IterationRecord()
        it.dimA = [0, tk, tk // 2][k % 3]
        it.code = 2 if k == 3 else 1
        Ws.append(W); its.append(it); Js.append(J); rxs.append(rx); As.append(A); cxs.append(cx)
    act = [W.active[:W.t] - 1 for W in Ws]
    At, cxa, t = GNSolver.pack_ragged([A[a] for A, a in zip(As, act)], [c[a] for c, a in zip(cxs, act)], n=n)
    t_max = At.shape[1]
    assert t_max == 4
    Jd = np.stack([np.asfortranarray(Jk).T for Jk in Js])
    out = solver.solve_batched_ragged(Jd, np.stack(rxs), At, cxa, t)
    p = np.ascontiguousarray(out[0])
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    dA = up(np.stack([np.asfortranarray(A).T for A in As]))
    setup = ls.linesearch_setup_batched_dev(solver, Ws, its, up(p), dA, up(np.stack(cxs)), up(np.stack(rxs)), t_max)
    w_old = 10.0 ** rng.uniform(-1, 1, (B, l))
    K = np.sort(10.0 ** rng.uniform(-1.5, 1.5, (B, 4, l)), axis=1)[:, ::-1].copy()
    ds = 1.0 + rng.random((B, t_max))
    dK = up(K)
    got = ls.penalty_weights_batched_dev(solver, Ws, its, setup, up(w_old), dK, up(np.stack(cxs)), up(ds), weight_code, True)
    torch.cuda.synchronize()
    assert solver.penalty_form() == expected_form(t_max, l)
    Jp, actAp = setup.Jp.cpu().numpy(), setup.active_Ap.cpu().numpy()
    w, K1 = got.w.cpu().numpy(), dK.cpu().numpy()
    for k in range(B):
        tk = ts[k]
        if its[k].code == 2:
            assert same(w[k], w_old[k]) and same(K1[k], K[k]) and got.dpsi0[k] == got.psi0[k] == got.atwa[k] == 0.0 and got.branch[k] == 0
            assert got.predicted_reduction[k] == 0.0
            continue
        c = dict(l=l, t=tk, active=Ws[k].active.astype(np.int64), dimA=its[k].dimA, norm_code=weight_code, w_old=w_old[k], K=K[k],
                 Ap=actAp[k, :tk] / ds[k, :tk], cx=cxs[k], Jp=Jp[k], rx=rxs[k])
        if weight_code == 0 and tk == 0:
            continue      # nrm_Ap = 0: the oracle's Python division raises (tests/test_penalty_weights_host.py checks the IEEE value)
        ref = pc.oracle_run(c)
        env, stable = pc.envelope(c, ref, 2000 + k)
        assert stable, k
        assert got.branch[k] == ref["branch"], (k, got.branch[k], ref["branch"])
        # the device sums are ordered sums of m products, the oracle's inputs the exactly rounded ones: m u sum |x||y| more
        slack = {key: 0.0 for key in ("w", "K", "dpsi0", "psi0", "atwa")}
        for key, val in (("w", w[k]), ("K", K1[k]), ("dpsi0", got.dpsi0[k]), ("psi0", got.psi0[k]), ("atwa", got.atwa[k])):
            print(f"k={k} {key}: got {val!r} oracle {ref[key]!r} envelope {env[key]!r}")
            assert pc.within(val, ref[key], env[key]), (k, key, val, ref[key], env[key], slack[key])
        upp = min(1.0, setup.alpha_upp[k])
        want = upp * (-2.0 * setup.Jprx[k] - upp * setup.JpJp[k] + (2.0 - upp ** 2) * got.atwa[k])
        assert same(got.predicted_reduction[k], want)
    # the merit function at alpha = 0 on the same buffers: psi(0) plus the inactive constraints that are violated
    psi = ls.merit_batched_dev(solver, Ws, up(np.stack(rxs)), up(np.stack(cxs)), got.w)
    for k in range(B):
        b = dict(rx=np.stack(rxs), cx=np.stack(cxs), w=w, t=np.array(ts), n_inactive=l - np.array(ts),
                 active=np.stack([W.active for W in Ws]), inactive=np.stack([np.pad(W.inactive, (0, l - W.inactive.size)) for W in Ws]))
        ref, mag = exact_psi(b, k)
        assert abs(psi[k] - ref) <= (m + l + 4) * U * mag, (k, psi[k], ref)


# ---- the merit function ------------------------------------------------------------------------------------------------------------
def merit_batch(seed, B, m, l, t_max):
    rng = np.random.default_rng(seed)
    b = dict(rx=rng.standard_normal((B, m)) * 10.0 ** rng.uniform(-1, 1, (B, 1)), cx=rng.standard_normal((B, max(l, 1))),
             w=10.0 ** rng.uniform(-1, 1, (B, max(l, 1))), t=np.zeros(B, dtype=np.int64), n_inactive=np.zeros(B, dtype=np.int64),
             active=np.zeros((B, t_max), dtype=np.int64), inactive=np.zeros((B, l), dtype=np.int64))
    for k in range(B):
        t = int(rng.integers(0, t_max + 1))
        perm = rng.permutation(l) + 1
        b["t"][k], b["n_inactive"][k] = t, l - t
        b["active"][k, :t] = perm[:t]
        b["inactive"][k, :l - t] = perm[t:]
    return b


def exact_psi(b, k):
    """(exact psi, the magnitude 0.5 * (sum rx^2 + sum |w| cx^2) over the entries that enter)"""
    with mp.workdps(80):
        f = lambda v: mp.mpf(float(v))
        s = sum((f(v) ** 2 for v in b["rx"][k]), mp.mpf(0))
        mag = s
        for j in b["active"][k, :b["t"][k]]:
            if j:
                term = f(b["w"][k, j - 1]) * f(b["cx"][k, j - 1]) ** 2
                s, mag = s + term, mag + abs(term)
        for j in b["inactive"][k, :b["n_inactive"][k]]:
            if j and b["cx"][k, j - 1] < 0.0:
                term = f(b["w"][k, j - 1]) * f(b["cx"][k, j - 1]) ** 2
                s, mag = s + term, mag + abs(term)
        return float(s / 2), float(mag / 2)


def run_merit(s, b, take=None):
    import torch
    B, m = b["rx"].shape
    l, t_max = b["inactive"].shape[1], b["active"].shape[1]
    host = {k: np.concatenate([np.full((1,) + b[k].shape[1:], SENT), b[k], np.full((1,) + b[k].shape[1:], SENT)]) for k in ("rx", "cx", "w")}
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in host.items()}
    torch.cuda.synchronize()
    psi = s.merit_batched_dev(B, m, l, t_max, b["t"], b["active"], b["inactive"], b["n_inactive"], dev["rx"].data_ptr() + 8 * m,
                              dev["cx"].data_ptr() + 8 * max(l, 1), dev["w"].data_ptr() + 8 * max(l, 1), take=take)
    torch.cuda.synchronize()
    for k in host:
        assert dev[k].cpu().numpy().tobytes() == host[k].tobytes(), f"input {k} was written"
    return psi


@pytest.mark.parametrize("m", [1, 255, 256, 257, 1000])
def test_merit_against_the_exact_value(solver, m):
    B, l, t_max = 6, 12, 8
    b = merit_batch(300 + m, B, m, l, t_max)
    psi = run_merit(solver, b)
    for k in range(B):
        ref, mag = exact_psi(b, k)
        bound = (m + l + 4) * U * mag
        print(f"m={m} k={k} psi {psi[k]!r} exact {ref!r} err/bound {abs(psi[k] - ref) / bound:.3f}")
        assert abs(psi[k] - ref) <= bound, (k, psi[k], ref, bound)
    # a second call, another slot in another batch, a batch of one, and a problem not taken
    assert same(run_merit(solver, b), psi)
    order = np.array([4, 0, 5, 5, 2, 1, 3, 0])
    psi2 = run_merit(solver, {k: v[order] for k, v in b.items()})
    assert same(psi2, psi[order])
    assert same(run_merit(solver, {k: v[3:4] for k, v in b.items()}), psi[3:4])
    take = np.array([1, 0, 1, 1, 0, 1])
    assert same(run_merit(solver, b, take=take), np.where(take != 0, psi, 0.0))


def test_merit_inactive_entries_that_do_not_enter(solver):
    B, m, l, t_max = 5, 7, 6, 2
    b = merit_batch(77, B, m, l, t_max)
    b["t"][:] = 2
    b["n_inactive"][:] = 4
    b["active"][:] = [1, 2]
    b["inactive"][:] = [3, 4, 5, 6, 0, 0]
    b["cx"][:, 2:] = -np.abs(b["cx"][:, 2:]) - 0.5
    base = run_merit(solver, b)
    drop = run_merit(solver, dict(b, n_inactive=np.full(B, 3, dtype=np.int64)))      # without list position 3 (constraint 6)
    for k, value in enumerate([0.0, -0.0, 2.5, np.nan, np.inf]):
        cx = b["cx"].copy()
        cx[k, 5] = value
        got = run_merit(solver, dict(b, cx=cx))
        assert same(got[k], drop[k]), (value, got[k], drop[k])
        assert same(np.delete(got, k), np.delete(base, k))
    # a negative value, -Inf included, does enter; a 0 in the list is padding
    cx = b["cx"].copy()
    cx[0, 5] = -np.inf
    assert run_merit(solver, dict(b, cx=cx))[0] == np.inf
    holes = b["inactive"].copy()
    holes[:, 3] = 0
    assert same(run_merit(solver, dict(b, inactive=holes)), drop)


def test_merit_batch_beyond_the_grid_y_limit_and_edges(solver):
    B, m, l, t_max = 70000, 3, 3, 2
    base = merit_batch(88, 7, m, l, t_max)
    slot = np.arange(B) % 7
    slot[-1] = 3
    psi = run_merit(solver, {k: v[slot] for k, v in base.items()})
    small = run_merit(solver, base)
    assert same(psi, small[slot])
    for k in range(7):
        ref, mag = exact_psi(base, k)
        assert abs(small[k] - ref) <= (m + l + 4) * U * mag
    # no constraint at all, and no residual at all
    rx = np.arange(1.0, 6.0).reshape(1, 5)
    z = np.zeros(1, dtype=np.int64)
    assert solver.merit_batched_dev(1, 5, 0, 0, z, np.zeros((1, 0)), np.zeros((1, 0)), z, _dev(rx), 0, 0)[0] == 27.5
    b = merit_batch(5, 2, 1, 4, 2)
    got = solver.merit_batched_dev(2, 0, 4, 2, b["t"], b["active"], b["inactive"], b["n_inactive"], 0, _dev(b["cx"]), _dev(b["w"]))
    for k in range(2):
        ref, mag = exact_psi(dict(b, rx=np.zeros((2, 0))), k)
        assert abs(got[k] - ref) <= (4 + 4) * U * mag


_keep = []


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    _keep.append(t)
    return t.data_ptr()


def test_merit_argument_errors(solver):
    import enlsip_gn._lib as Lm
    L = Lm.load()
    B, m, l, t_max = 3, 5, 4, 2
    b = merit_batch(9, B, m, l, t_max)
    b["t"][:] = 2
    b["n_inactive"][:] = 2
    b["active"][:] = [1, 2]
    b["inactive"][:] = [3, 4, 0, 0]
    psi = np.full(B, SENT)
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    good = dict(h=solver._h, batch=B, m=m, l=l, t_max=t_max, t=b["t"], active=b["active"], inactive=b["inactive"],
                n_inactive=b["n_inactive"], take=None, drx=C.c_void_p(_dev(b["rx"])), dcx=C.c_void_p(_dev(b["cx"])),
                dw=C.c_void_p(_dev(b["w"])), psi=psi)

    def call(**kw):
        a = dict(good, **kw)
        return L.enlsip_gn_merit_batched_dev(a["h"], a["batch"], a["m"], a["l"], a["t_max"], hp(a["t"]), hp(a["active"]),
                                             hp(a["inactive"]), hp(a["n_inactive"]), hp(a["take"]), a["drx"], a["dcx"], a["dw"],
                                             hp(a["psi"]))

    def edited(x, idx, value):
        x = x.copy()
        x[idx] = value
        return x

    cases = [(-1, dict(h=None)), (-2, dict(batch=0)), (-3, dict(m=-1)), (-3, dict(l=-1)), (-3, dict(t_max=l + 1)), (-3, dict(t_max=-1)),
             (-4, dict(t=None)), (-4, dict(n_inactive=None)), (-4, dict(psi=None)), (-4, dict(active=None)), (-4, dict(inactive=None)),
             (-4, dict(drx=None)), (-4, dict(dcx=None)), (-4, dict(dw=None)),
             (-5, dict(t=edited(b["t"], 1, t_max + 1))), (-5, dict(n_inactive=edited(b["n_inactive"], 2, l + 1))),
             (-5, dict(n_inactive=edited(b["n_inactive"], 0, -1))),
             (-6, dict(active=edited(b["active"], (1, 1), l + 1))), (-6, dict(inactive=edited(b["inactive"], (2, 0), -1)))]
    for want, kw in cases:
        assert call(**kw) == want, (want, list(kw))
    # two faults at once: t[k] and n_inactive[k] are checked problem by problem, then active and inactive row by row
    for want, kw, name in [(-5, dict(t=edited(b["t"], 1, t_max + 1), n_inactive=edited(b["n_inactive"], 0, -1)), "n_inactive[0]"),
                           (-6, dict(active=edited(b["active"], (2, 1), l + 1), inactive=edited(b["inactive"], (1, 0), -1)), "inactive[1]")]:
        assert call(**kw) == want and name in L.enlsip_gn_last_error(solver._h).decode(), (want, name)
    assert np.all(psi == SENT)
    assert call(inactive=edited(b["inactive"], (0, 3), l + 7)) == 0      # past n_inactive: not read
    assert np.all(psi != SENT)
    _keep.clear()
