"""The polynomial fit of the line search for a batch on device buffers (enlsip_gn_linesearch_fit_batched_dev) and the batched line
search built on it (linesearch.linesearch_constrained_batched): coefficients_linesearch! (src/enlsip_functions.jl:1665-1689), the
scaling of v1 (:1986-1998), minrm (:1841-1862) and the choice of :2023-2026.

- the six sums within 2 (m + l) u sum |x||y| of the exactly rounded dot product of elements formed in NumPy with the same IEEE
  operations (the bound of any order of a sum of m + l rounded products, doubled); bit for bit the same in another slot, another
  batch and a second call
- out and arm bit for bit enlsip_gn_linesearch_fit on the returned sums with the record of problem k (a mis-indexed alpha_k, x_min or
  take shows here); the host routine itself is held to the oracle by tests/test_linesearch_fit_host.py
- psi_new bit for bit merit_batched_dev; problems not taken return zeros
- every device buffer, sentinel guard slots around it included, byte-identical after the call; an argument error writes nothing
- a fresh handle, and a call between factor_constraints_batched and its solve
- the driver on the GPU backend against the host-backend driver on the six-terminal batch

Shapes: m at the lane edge (63, 64, 65), the LS_SUM_ROWS edge (1024, 1025) and nblk at LS_MAX_NBLK (65537); l at the wave edge of
the list loop (64, 65); one batch beyond the grid's y limit.  The exact dot product is math.fsum over the error-free products
(Veltkamp / Dekker), checked against mpmath on the first case: mpmath alone takes seconds per sum at m = 65537."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

import linesearch_fit_cases as fc

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

U = fc.U
SENT = -777.25      # what guard slots and untouched outputs hold
same = fc.same_bits
DOUBLES = ("rx", "rx_new", "Jp", "cx", "cx_new", "Ap", "w")


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def exact_dot_fast(x, y):
    """(the exactly rounded dot product, sum |x||y|): x_i y_i = p_i + e_i exactly (Dekker's product on Veltkamp splits; the operands
    here are far from the overflow and underflow thresholds), and math.fsum adds the 2n terms exactly"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    p = x * y
    split = lambda a: ((134217729.0 * a) - ((134217729.0 * a) - a), a - ((134217729.0 * a) - ((134217729.0 * a) - a)))
    (xh, xl), (yh, yl) = split(x), split(y)
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return math.fsum(np.concatenate([p, e]).tolist()), math.fsum(np.abs(p).tolist())


def make_batch(seed, B, m, l, ts):
    """B problems of one shape with t[k] = ts[k]: cases of linesearch_fit_cases.random_case at this size, stacked"""
    rng = np.random.default_rng(seed)
    cs = [fc.random_case(rng, k % 6, m=m, l=l, t=int(ts[k])) for k in range(B)]
    t_max = max(list(ts) + [0])
    b = {k: np.stack([c[k] for c in cs]) for k in DOUBLES}
    b["t"] = np.array(ts, dtype=np.int64)
    b["n_inactive"] = l - b["t"]
    b["active"] = np.stack([c["active"][:t_max] for c in cs])
    b["inactive"] = np.stack([c["inactive"] for c in cs])
    for k in ("alpha_k", "x_min", "a_min", "a_max"):
        b[k] = np.array([c[k] for c in cs])
    b["cases"] = cs
    return b


def pick(b, idx):
    idx = np.asarray(idx)
    return {k: ([v[i] for i in idx] if k == "cases" else v[idx]) for k, v in b.items()}


def run(s, b, take=None, psi=True):
    """One call on sentinel-guarded device images: slots 0 and B + 1 of every buffer are guards.  Every buffer must come back byte
    for byte.  Returns (sums, out, arm, psi_new)."""
    import torch
    B = len(b["t"])
    m, l, t_max = b["rx"].shape[1], b["inactive"].shape[1], b["active"].shape[1]
    guard = lambda a: np.concatenate([np.full((1, max(a.shape[1], 1)), SENT), np.pad(a, ((0, 0), (0, max(a.shape[1], 1) - a.shape[1])),
                                                                                     constant_values=SENT),
                                      np.full((1, max(a.shape[1], 1)), SENT)])
    host = {k: guard(b[k]) for k in DOUBLES}
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in host.items()}
    torch.cuda.synchronize()
    at = lambda k: dev[k].data_ptr() + 8 * host[k].shape[1] if b[k].shape[1] else 0
    got = s.linesearch_fit_batched_dev(B, m, l, t_max, b["t"], b["active"], b["inactive"], b["n_inactive"], b["alpha_k"], b["x_min"],
                                       b["a_min"], b["a_max"], at("rx"), at("rx_new"), at("Jp"), at("cx"), at("cx_new"), at("Ap"), at("w"),
                                       take=take, psi=psi)
    torch.cuda.synchronize()
    for k in host:
        assert dev[k].cpu().numpy().tobytes() == host[k].tobytes(), f"buffer {k} was written"
    return got


def check_values(s, b, got, take=None):
    from enlsip_gn import linesearch_fit
    sums, out, arm, psi = got
    B = len(b["t"])
    m, l = b["rx"].shape[1], b["inactive"].shape[1]
    worst = 0.0
    for k in range(B):
        if take is not None and not take[k]:
            assert not sums[k].any() and not out[k].any() and arm[k] == 0 and (psi is None or psi[k] == 0.0), k
            continue
        c = b["cases"][k]
        v0, v1, v2 = fc.library_order_elements(c)
        for q, (x, y) in enumerate(((v0, v0), (v0, v1), (v0, v2), (v1, v1), (v1, v2), (v2, v2))):
            ref, mag = exact_dot_fast(x, y)
            bound = 2 * (m + l) * U * mag
            worst = max(worst, abs(sums[k, q] - ref) / bound if bound else 0.0)
            assert abs(sums[k, q] - ref) <= bound, (k, q, sums[k, q], ref, bound)
        want, want_arm = linesearch_fit(sums[k], b["alpha_k"][k], b["x_min"][k], b["a_min"][k], b["a_max"][k])
        assert same(out[k], want) and arm[k] == want_arm, (k, out[k], want, arm[k], want_arm)
    print(f"m={m} l={l}: worst |sum - exact| / bound = {worst:.3f}")
    if psi is not None:
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        d = [up(b["rx_new"]), up(b["cx_new"]), up(b["w"])]
        torch.cuda.synchronize()
        ptr = lambda x: x.data_ptr() if x.numel() else 0
        merit = s.merit_batched_dev(B, m, l, b["active"].shape[1], b["t"], b["active"], b["inactive"], b["n_inactive"], ptr(d[0]),
                                    ptr(d[1]), ptr(d[2]), take=take)
        assert same(psi, merit), (psi, merit)


def same_results(a, b):
    return all((x is None and y is None) or same(x, y) for x, y in zip(a[:2] + a[3:], b[:2] + b[3:])) and np.array_equal(a[2], b[2])


def test_the_fast_exact_dot_is_mpmaths():
    rng = np.random.default_rng(1)
    for n in (1, 7, 300):
        x, y = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n), rng.standard_normal(n)
        assert exact_dot_fast(x, y)[0] == fc.exact_dot(x, y)[0]


@pytest.mark.parametrize("l", [0, 1, 64, 65])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1024, 1025, 65537])
def test_shapes(solver, m, l):
    B = 5
    ts = [0, l, l // 2, min(1, l), max(l - 1, 0)]
    b = make_batch(100 * m + l, B, m, l, ts)
    got = run(solver, b)
    check_values(solver, b, got)
    # a second call; other slots of another batch; a batch of one; without psi_new; with problems not taken
    assert same_results(run(solver, b), got)
    order = np.array([3, 0, 4, 4, 1, 2, 0])
    other = run(solver, pick(b, order))
    assert same_results(other, tuple(None if g is None else g[order] for g in got))
    one = run(solver, pick(b, [2]))
    assert same_results(one, tuple(g[2:3] for g in got))
    plain = run(solver, b, psi=False)
    assert plain[3] is None and same_results(plain[:3] + (got[3],), got)
    take = np.array([1, 0, 1, 1, 0], dtype=np.int64)
    part = run(solver, b, take=take)
    check_values(solver, b, part, take=take)
    for k in np.flatnonzero(take):
        assert all(same(p[k], g[k]) for p, g in zip(part, got)), k


def test_every_t_at_l_65(solver):
    l, m = 65, 4
    b = make_batch(7, l + 1, m, l, list(range(l + 1)))
    check_values(solver, b, run(solver, b))


def test_batch_beyond_the_grid_y_limit(solver):
    B, m, l = 65539, 4, 2
    base = make_batch(88, 7, m, l, [0, 1, 2, 1, 2, 0, 1])
    small = run(solver, base)
    check_values(solver, base, small)
    slot = np.arange(B) % 7
    slot[-1] = 3
    big = pick(base, slot)
    big["active"] = np.ascontiguousarray(big["active"])
    got = run(solver, big)
    assert same_results(got, tuple(g[slot] for g in small))


def test_fresh_handle_and_between_factor_and_solve(solver):
    from enlsip_gn import GNSolver
    b = make_batch(3, 3, 5, 3, [1, 0, 3])
    want = run(solver, b)
    s = GNSolver(device=0)
    try:
        assert same_results(run(s, b), want)
        # between the constraint stage of a batch and the solve that goes on with it: the resident factors survive the call
        rng = np.random.default_rng(9)
        Bq, m, n, t_max = 4, 40, 6, 3
        t = np.array([3, 0, 2, 1], dtype=np.int64)
        J, rx = rng.standard_normal((Bq, n, m)), rng.standard_normal((Bq, m))
        At, cx = rng.standard_normal((Bq, t_max, n)), rng.standard_normal((Bq, t_max))
        for k in range(Bq):
            At[k, t[k]:] = 0.0
            cx[k, t[k]:] = 0.0
        ref = solver.solve_batched_ragged(J, rx, At, cx, t)
        s.factor_constraints_batched(m, At, cx, t)
        assert same_results(run(s, b), want)
        got = s.solve_factored_batched(J, rx, At, cx, t)
        for g, r in zip(got[:3], ref[:3]):
            assert same(g, r)
    finally:
        s.close()


def test_argument_errors_write_nothing(solver):
    import torch
    import enlsip_gn._lib as Lm
    L = Lm.load()
    B, m, l = 4, 5, 4
    b = make_batch(21, B, m, l, [2, 0, 4, 1])
    t_max = b["active"].shape[1]
    dev = {k: torch.from_numpy(np.ascontiguousarray(b[k])).to("cuda:0") for k in DOUBLES}
    torch.cuda.synchronize()
    sums, out, arm, psi = np.full((B, 6), SENT), np.full((B, 6), SENT), np.full(B, -9, dtype=np.int32), np.full(B, SENT)
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    v = lambda k: C.c_void_p(dev[k].data_ptr())
    h = solver._h
    good = dict(h=h, batch=B, m=m, l=l, t_max=t_max, t=b["t"], active=b["active"], inactive=b["inactive"], ni=b["n_inactive"],
                take=None, alpha_k=b["alpha_k"], x_min=b["x_min"], a_min=b["a_min"], a_max=b["a_max"], sums=sums, out=out, arm=arm,
                psi=psi, **{k: v(k) for k in DOUBLES})

    def call(**kw):
        a = dict(good, **kw)
        return L.enlsip_gn_linesearch_fit_batched_dev(
            a["h"], a["batch"], a["m"], a["l"], a["t_max"], hp(a["t"]), hp(a["active"]), hp(a["inactive"]), hp(a["ni"]), hp(a["take"]),
            hp(a["alpha_k"]), hp(a["x_min"]), hp(a["a_min"]), hp(a["a_max"]), a["rx"], a["rx_new"], a["Jp"], a["cx"], a["cx_new"],
            a["Ap"], a["w"], hp(a["sums"]), hp(a["out"]), hp(a["arm"]), hp(a["psi"]))

    def edited(x, idx, value):
        x = x.copy()
        x[idx] = value
        return x

    cases = [(-1, dict(h=None), None), (-2, dict(batch=0), None), (-3, dict(m=-1), None), (-3, dict(l=-1), None),
             (-3, dict(t_max=l + 1), None), (-3, dict(t_max=-1), None), (-3, dict(l=(1 << 27) + 1), None),
             (-3, dict(t_max=1025, l=2000), None)]
    cases += [(-4, {k: None}, None) for k in ("t", "ni", "alpha_k", "x_min", "a_min", "a_max", "sums", "out", "arm", "active",
                                              "inactive") + DOUBLES]
    cases += [(-5, dict(t=edited(b["t"], 1, t_max + 1)), "[1]"), (-5, dict(ni=edited(b["n_inactive"], 2, l + 1)), "[2]"),
              (-5, dict(ni=edited(b["n_inactive"], 0, -1)), "[0]"), (-5, dict(ni=edited(b["n_inactive"], 3, l - 2)), "[3]"),
              (-6, dict(active=edited(b["active"], (2, 1), l + 1)), "[2]"), (-6, dict(active=edited(b["active"], (0, 0), 0)), "[0]"),
              (-6, dict(inactive=edited(b["inactive"], (1, 0), -1)), "[1]"), (-6, dict(inactive=edited(b["inactive"], (3, 2), 0)), "[3]")]
    # two faults at once: t[k] and n_inactive[k] are checked problem by problem, then active and inactive row by row
    cases += [(-5, dict(t=edited(b["t"], 1, t_max + 1), ni=edited(b["n_inactive"], 0, -1)), "n_inactive[0]"),
              (-6, dict(active=edited(b["active"], (2, 1), l + 1), inactive=edited(b["inactive"], (1, 0), -1)), "inactive[1]")]
    for want, kw, names in cases:
        got = call(**kw)
        assert got == want, (want, got, list(kw))
        if want != -1:
            msg = L.enlsip_gn_last_error(h).decode()
            assert msg and (names is None or names in msg), (want, msg)
    torch.cuda.synchronize()
    assert np.all(sums == SENT) and np.all(out == SENT) and np.all(arm == -9) and np.all(psi == SENT)
    for k in DOUBLES:
        assert dev[k].cpu().numpy().tobytes() == np.ascontiguousarray(b[k]).tobytes(), k
    # psi_new is optional; an entry past the used part of a list is not read
    assert call(psi=None) == 0 and np.all(sums != SENT) and np.all(psi == SENT)
    assert call(inactive=edited(b["inactive"], (0, l - 1), l + 7)) == 0 and np.all(psi != SENT)


def test_driver_on_the_gpu_backend(solver):
    import torch
    from enlsip_gn import linesearch as ls
    from test_linesearch_fit_host import run_driver
    batch = fc.driver_batch()
    host, host_calls = run_driver(ls.HostLinesearchBackend(), batch)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    got, calls = run_driver(solver, batch, up=up)
    assert got.terminal == host.terminal and np.array_equal(got.n_eval, host.n_eval) and got.rounds == host.rounds
    assert np.array_equal(got.gac_error, host.gac_error) and all(np.array_equal(a, b) for a, b in zip(calls, host_calls))
    assert set(got.terminal) == {"first_fit", "first_fit_minrn", "second_fit", "second_minrn", "armijo", "armijo_error"}
    for k, (pr, run_, env) in enumerate(batch):
        print(f"{got.terminal[k]}: alpha gpu {got.alpha[k]!r} host {host.alpha[k]!r} envelope {env!r}")
        assert abs(got.alpha[k] - host.alpha[k]) <= fc.MARGIN * env + 4.0 * np.spacing(abs(host.alpha[k])), (k, got.alpha[k], host.alpha[k])
