"""The polynomial fit of the line search (linesearch_constrained, src/enlsip_functions.jl:1940-2143) through the library's host entry
points enlsip_gn_linesearch_coefficients, enlsip_gn_linesearch_fit, enlsip_gn_minrn and enlsip_gn_check_reduction, and the batched
driver enlsip_gn.linesearch.linesearch_constrained_batched on the host backend, against oracle.enlsip_outer.  No GPU.

Sums: against the exactly rounded dot product (mpmath) of elements formed in NumPy with the same IEEE operations; the bound is
2 (m + l) u sum |x||y| (a sum of m + l rounded products in any order has (m + l) u; the factor 2 is the issue's).  Dyadic cases are
met bit for bit.

Fit: the oracle runs minrm and the choice on its own vectors; the library gets the exactly rounded dot products of those vectors.
Tolerance, measured from the oracle alone: every case is run 16 more times with each entry of rx_new moved by at most one ulp
(seeded); the envelope of an output is its largest change, and the library must lie within ten times the envelope plus 4 ulp of the
value.  A case whose pattern (arm, clamps, alpha_old == beta_hat, choice) changes under that perturbation sits on a tie and is left
out: at most 2 % of the random cases, none of the named ones.  minrn and check_reduction: scalar in, scalar out, the same rule with
y1 moved by one ulp.

Measured on the CPU: worst |library - oracle| / tolerance 0.50 (fit: pk, s_alpha, s_beta 0.50; alpha_kp1, alpha_hat 0.25;
beta_hat 0.21), 0.00 (minrn: the same bits in all 200 cases); worst |sum - exact| / bound 0.35; 0 of 240 random cases on a tie.
The library's cube root is the libm's with one correction step: glibc's cbrt is an ulp off in every other argument, one_root
cancels, and without the correction a random case missed this tolerance by a factor 2.4 against the oracle's (NumPy's) cbrt.

Mutations of gn_linesearch_fit.hpp, run on the CPU, each failing the tests named:
  - `cx_new[k] > 0` replaced by `cx[k] > 0` in the v_buff test: test_sums_against_the_exact_dot (and the driver test)
  - `<=` for `<` in the choice (`s_beta <= pk`): test_choice_is_strict
  - the last three coefficients of ds instead of the first three: test_fit_against_the_oracle (and test_choice_is_strict, the
    driver test)"""
import collections
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import linesearch_fit_cases as fc


@pytest.fixture(scope="module")
def lib():
    import enlsip_gn._lib as Lm
    return Lm.load()


def lib_sums(c):
    from enlsip_gn import linesearch_coefficients
    return linesearch_coefficients(c["active"], c["t"], c["inactive"], c["l"] - c["t"], c["rx"], c["rx_new"], c["Jp"], c["cx"],
                                   c["cx_new"], c["Ap"], c["w"], c["alpha_k"])


@pytest.fixture(scope="module")
def oracle_side():
    """(case, reference, envelope, stable) per case from the oracle alone: computed once, shared, left unchanged"""
    out = []
    for i, c in enumerate(fc.random_cases() + fc.named_cases() + fc.exact_cases()):
        ref = fc.oracle_run(c)
        env, stable = fc.envelope(c, ref, 1000 + i)
        out.append((c, ref, env, stable))
    return out


def test_ties_stay_under_the_cap(oracle_side):
    """the oracle alone, before the library is involved"""
    rnd = [c["name"] for c, _, _, stable in oracle_side if c["name"].startswith("random") and not stable]
    named = [c["name"] for c, _, _, stable in oracle_side if not c["name"].startswith("random") and not stable]
    print(f"{len(rnd)} of {fc.N_RANDOM} random cases on a tie")
    assert len(rnd) <= 0.02 * fc.N_RANDOM, rnd
    assert not named, named


def test_sums_against_the_exact_dot(oracle_side):
    worst = 0.0
    for c, _, _, _ in oracle_side:
        got = lib_sums(c)
        v0, v1, v2 = fc.library_order_elements(c)
        n = c["m"] + c["l"]
        for q, (a, b) in enumerate(((v0, v0), (v0, v1), (v0, v2), (v1, v1), (v1, v2), (v2, v2))):
            ref, mag = fc.exact_dot(a, b)
            bound = 2 * n * fc.U * mag
            if c["name"].startswith("exact_"):
                assert fc.same_bits(got[q], ref), (c["name"], q, got[q], ref)
            else:
                assert abs(got[q] - ref) <= bound, (c["name"], q, got[q], ref, bound)
                worst = max(worst, abs(got[q] - ref) / bound if bound else 0.0)
    print(f"worst |sum - exact| / bound = {worst:.3f}")


def test_the_library_order_is_the_oracles_vectors(oracle_side):
    """the elements of library_order_elements are the oracle's v0, v1, v2 in another order, bit for bit"""
    for c, ref, _, _ in oracle_side:
        m = c["m"]
        act, inact = fc.lists(c)
        order = np.concatenate([np.arange(m), m + act - 1, m + inact - 1]).astype(np.int64)
        for mine, theirs in zip(fc.library_order_elements(c), ref["vectors"]):
            assert fc.same_bits(mine, theirs[order]), c["name"]


def test_fit_against_the_oracle(oracle_side):
    from enlsip_gn import linesearch_fit
    worst = np.zeros(6)
    for c, ref, env, stable in oracle_side:
        if not stable:
            continue
        out, arm = linesearch_fit(fc.exact_sums(ref["vectors"]), c["alpha_k"], c["x_min"], c["a_min"], c["a_max"])
        assert arm == ref["arm"], (c["name"], arm, ref["arm"])
        tol = fc.tolerance(ref["out"], env)
        with np.errstate(all="ignore"):
            ratio = np.abs(out - ref["out"]) / tol
        worst = np.maximum(worst, ratio)
        assert np.all(ratio <= 1.0), (c["name"], out, ref["out"], env)
        # the discrete outcome is the oracle's: which of the two roots the step is
        assert (out[0] == out[4] and out[0] != out[2]) == ref["pattern"][4], c["name"]
    print(dict(zip(fc.OUT, np.round(worst, 3))), "= worst |library - oracle| / tolerance")


def test_the_case_list_covers_every_path(oracle_side):
    n = collections.Counter()
    for c, ref, _, stable in oracle_side:
        arm, ca, cb, same, choice = ref["pattern"]
        inact = c["inactive"][:c["l"] - c["t"]] - 1
        n["arm", arm] += 1
        n["clamp", ca] += 1
        n["beta_clamp", cb] += arm == 2
        n["alpha_old_is_beta_hat", same] += 1
        n["choice", choice] += 1
        n["choice_open", arm == 2 and not choice] += 1
        n["l0"] += c["l"] == 0
        n["t0"] += c["l"] > 0 and c["t"] == 0
        n["t_eq_l"] += c["l"] > 0 and c["t"] == c["l"]
        n["leaves"] += bool(np.any((c["cx"][inact] > 0) & (c["cx_new"][inact] <= 0)))
        n["enters"] += bool(np.any((c["cx"][inact] <= 0) & (c["cx_new"][inact] > 0)))
        n["x_min_0"] += c["x_min"] == 0.0
    print(dict(n))
    need = [("arm", a) for a in (0, 1, 2)] + [("clamp", k) for k in ("lo", "hi", None)] + [("alpha_old_is_beta_hat", b) for b in (True, False)]
    need += [("choice", True), ("choice", False), ("choice_open", True), "l0", "t0", "t_eq_l", "leaves", "enters", "x_min_0"]
    missing = [k for k in need if n[k] < 1]
    assert not missing, missing
    named = {c["name"] for c, _, _, _ in oracle_side}
    assert {"arm_newton", "arm_one_root", "arm_two_roots", "clamp_high", "clamp_low", "choice_takes_beta", "no_constraints"} <= named


def test_choice_is_strict():
    """alpha_kp1 != beta && p_beta < pk && beta <= alpha_k (:2023-2026) at its edges, on a symmetric quartic: s(a) = 0.5 |v0 + a v1 +
    a^2 v2|^2 with v0.v1 = v1.v2 = 0 is even, its two minima +-sqrt(-s2 / (2 s4)) have the same value bit for bit, so p_beta < pk
    is false by a tie and the step stays alpha_hat."""
    from enlsip_gn import linesearch_fit
    # v0 = (2, 0), v1 = (0, 1), v2 = (-1, 0): s = 2 + (0.5 - 2) a^2 + 0.5 a^4, minima at +-sqrt(1.5)
    sums = np.array([4.0, 0.0, -2.0, 1.0, 0.0, 1.0])
    out, arm = linesearch_fit(sums, 3.0, 1.0, -4.0, 4.0)
    assert arm == 2 and out[2] > 0 > out[4] and out[3] == out[5]
    assert out[0] == out[2] and out[1] == out[3]                 # a tie of the two values keeps alpha_hat: `<`, not `<=`
    # beta <= alpha_k is not strict: beta == alpha_k with a lower value takes beta.  x_min beyond the middle root makes alpha_hat the
    # right minimum; tilt the quartic so that the left one is lower, and put alpha_k on it
    sums = np.array([4.0, 0.5, -2.0, 1.0, 0.0, 1.0])
    probe, arm = linesearch_fit(sums, 3.0, 1.0, -4.0, 4.0)
    assert arm == 2 and probe[4] < 0 < probe[2] and probe[5] < probe[3] and probe[0] == probe[4]
    at, _ = linesearch_fit(sums, probe[4], 1.0, -4.0, 4.0)
    assert at[0] == probe[4]
    below, _ = linesearch_fit(sums, np.nextafter(probe[4], -np.inf), 1.0, -4.0, 4.0)
    assert below[0] == probe[2]


def test_newton_arm_quirks():
    """The d = 1.0 sentinel: on the Newton arm beta_hat = alpha_hat.  A pure parabola s = 1 - 2 a + a^2 (v2 = 0): Dm = 0, so the
    Newton arm, and Newton's method lands on the minimiser 1 in one step and stops after the third (iter < 3)."""
    from enlsip_gn import linesearch_fit
    out, arm = linesearch_fit(np.array([2.0, -2.0, 0.0, 2.0, 0.0, 0.0]), 0.5, 0.5, 0.001, 3.0)
    assert arm == 0 and out[0] == out[2] == out[4] == 1.0 and out[1] == out[3] == out[5] == 0.0
    # a NaN ends the routine
    out, arm = linesearch_fit(np.full(6, np.nan), 0.5, 0.5, 0.001, 3.0)
    assert np.isnan(out[0])


def scalar_envelope(f, args, seed):
    """the envelope rule on a scalar routine: y1 (position 1) moved by one ulp"""
    rng = np.random.default_rng(seed)
    ref = np.asarray(f(*args), dtype=np.float64)
    env = np.zeros_like(ref)
    for _ in range(fc.N_PERTURBED):
        a = list(args)
        a[1] = a[1] * (1.0 + fc.ULP * int(rng.integers(-1, 2)))
        env = np.maximum(env, np.abs(np.asarray(f(*a), dtype=np.float64) - ref))
    return ref, env


def test_minrn_against_the_oracle():
    from enlsip_gn import minrn
    from oracle import enlsip_outer as eo
    rng = np.random.default_rng(5)
    worst, clamped = 0.0, collections.Counter()
    for i in range(200):
        x = np.sort(rng.uniform(0.0, 2.0, 3))[::-1] if i % 2 else rng.uniform(0.0, 2.0, 3)
        y = rng.uniform(0.1, 3.0, 3)
        a_max = float(rng.uniform(0.5, 2.5))
        args = (x[0], y[0], x[1], y[1], x[2], y[2], a_max / 3000.0, a_max, float(rng.uniform(0.1, 10.0)))
        ref, env = scalar_envelope(eo.minrn, args, i)
        got = np.array(minrn(*args))
        tol = fc.tolerance(ref, env)
        worst = max(worst, float(np.max(np.abs(got - ref) / tol)))
        assert np.all(np.abs(got - ref) <= tol), (args, got, ref, env)
        clamped["hi" if ref[0] == a_max else "lo" if ref[0] == a_max / 3000.0 else None] += 1
    print(f"worst |library - oracle| / tolerance = {worst:.3f}", dict(clamped))
    assert all(clamped[k] for k in ("hi", "lo", None))
    # the three closeness tests of :1719
    eps = eo.SQRT_EPS / 2.0
    for x1, x2, x3 in ((1.0, 1.0 + 0.5 * eps, 3.0), (1.0, 3.0, 1.0 - 0.5 * eps), (0.0, 1.0, 1.0 + 0.25 * eps)):
        args = (x1, 2.0, x2, 1.0, x3, 3.0, 0.001, 3.0, 2.0)
        assert minrn(*args) == (0.0, 0.0) == tuple(eo.minrn(*args))
    args = (1.0, 2.0, 1.0 + 2.0 * eps, 1.0, 3.0, 3.0, 0.001, 3.0, 2.0)
    assert minrn(*args) != (0.0, 0.0)


def test_check_reduction_against_the_oracle():
    from enlsip_gn import check_reduction
    from oracle import enlsip_outer as eo
    rng = np.random.default_rng(6)
    seen = collections.Counter()
    for _ in range(400):
        a = [float(v) for v in rng.uniform(0.0, 2.0, 3)] + [0.3, float(rng.uniform(-1.0, 1.0))]
        want = eo.check_reduction(*a)
        first = a[0] - a[2] >= a[3] * a[4]
        seen[first, bool(want)] += 1
        assert check_reduction(*a) is bool(want), a
    assert all(seen[k] for k in ((True, True), (True, False), (False, False)))
    # the comparisons at their edges: >= on the first, strict < and > inside
    assert check_reduction(2.0, 0.5, 1.0, 0.5, 2.0) is True            # psi_a - approx == eta diff: enters; psi_a - psi_k < eta diff fails
    assert check_reduction(2.0, 1.5, 1.0, 0.5, 2.0) is False           # 0.5 < 1 and 1.5 > 0.4
    assert check_reduction(2.0, 0.4, 1.0, 0.5, 4.0) is False           # 1 < 2: the first test fails
    assert check_reduction(5.0, 1.0, 4.0, 0.5, 2.0) is True            # psi_k == delta psi_a: `>` fails, so a reduction is likely


def test_return_codes(lib):
    c = fc.exact_cases()[0]
    m, l, t = c["m"], c["l"], c["t"]
    SENT = -777.25
    sums = np.full(6, SENT)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    good = dict(m=m, l=l, t=t, active=c["active"], inactive=c["inactive"], ni=l - t, rx=c["rx"], rx_new=c["rx_new"], Jp=c["Jp"],
                cx=c["cx"], cx_new=c["cx_new"], Ap=c["Ap"], w=c["w"], sums=sums)

    def call(**kw):
        a = dict(good, **kw)
        return lib.enlsip_gn_linesearch_coefficients(a["m"], a["l"], a["t"], p(a["active"]), p(a["inactive"]), a["ni"], p(a["rx"]),
                                                     p(a["rx_new"]), p(a["Jp"]), p(a["cx"]), p(a["cx_new"]), p(a["Ap"]), p(a["w"]), 0.5,
                                                     p(a["sums"]))

    def edited(x, i, v):
        x = x.copy()
        x[i] = v
        return x

    cases = [(-2, dict(sums=None)), (-2, dict(m=-1)), (-2, dict(l=-1)), (-2, dict(t=-1)), (-2, dict(t=l + 1)), (-2, dict(ni=-1)),
             (-2, dict(ni=l + 1))]
    cases += [(-4, {k: None}) for k in ("active", "inactive", "rx", "rx_new", "Jp", "cx", "cx_new", "Ap", "w")]
    cases += [(-5, dict(t=t - 1)), (-5, dict(ni=l - t + 1)), (-6, dict(active=edited(c["active"], 0, 0))),
              (-6, dict(active=edited(c["active"], t - 1, l + 1))), (-6, dict(inactive=edited(c["inactive"], 0, -2))),
              (-6, dict(inactive=edited(c["inactive"], l - t - 1, l + 1)))]
    for want, kw in cases:
        assert call(**kw) == want, (want, list(kw))
    assert np.all(sums == SENT)
    # an entry past the used part of a list is not read; with m == 0 or l == 0 the vectors of that part may be NULL
    assert call(active=edited(c["active"], t, l + 5)) == 0 and np.all(sums != SENT)
    assert call(m=0, rx=None, rx_new=None, Jp=None) == 0
    assert call(l=0, t=0, ni=0, active=None, inactive=None, cx=None, cx_new=None, Ap=None, w=None) == 0
    out, arm = np.full(6, SENT), C.c_int(-9)
    fit = lambda s, o, a: lib.enlsip_gn_linesearch_fit(p(s), 0.5, 0.5, 0.001, 2.0, p(o), a)
    assert fit(sums, None, C.byref(arm)) == -2 and fit(sums, out, None) == -2 and fit(None, out, C.byref(arm)) == -4
    assert np.all(out == SENT) and arm.value == -9
    assert fit(sums, out, C.byref(arm)) == 0
    a, pa = C.c_double(SENT), C.c_double(SENT)
    args = (1.0, 2.0, 2.0, 1.0, 3.0, 3.0, 0.001, 3.0, 2.0)
    assert lib.enlsip_gn_minrn(*args, None, C.byref(pa)) == -2 and lib.enlsip_gn_minrn(*args, C.byref(a), None) == -2
    assert a.value == SENT and pa.value == SENT
    assert lib.enlsip_gn_check_reduction(1.0, 1.0, 1.0, 0.3, 1.0, None) == -2


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
def run_driver(backend, batch, up=lambda a: a, down=lambda a: a):
    """linesearch_constrained_batched on the six-terminal batch.  up / down move an array to the backend's memory and back."""
    from enlsip_gn import linesearch as ls
    probs = [pr for pr, _, _ in batch]
    B = len(probs)
    m, l = probs[0]["m"], probs[0]["l"]
    Ws = [pr["W"] for pr in probs]
    stack = lambda key: np.stack([pr[key] for pr in probs])
    setup = SimpleNamespace(Jp=up(stack("Jp")), Ap=up(stack("Ap")))
    rx_new, cx_new = np.zeros((B, m)), np.zeros((B, l))
    bufs = [up(rx_new), up(cx_new)]
    calls = []

    def evaluate(alpha, take):
        calls.append(take.copy())
        for k in np.flatnonzero(take):
            rx_new[k], cx_new[k] = probs[k]["r"].at(alpha[k]), probs[k]["c"].at(alpha[k])
        for buf, host in zip(bufs, (rx_new, cx_new)):
            buf[...] = up(host)
        return bufs

    vec = lambda key: np.array([pr[key] for pr in probs])
    res = ls.linesearch_constrained_batched(backend, Ws, evaluate, setup, up(stack("rx")), up(stack("cx")), up(stack("w")), vec("a0"),
                                            vec("psi0"), vec("dpsi0"), vec("a_low"), vec("a_upp"), p_max=np.ones(B))
    return res, calls


@pytest.fixture(scope="module")
def batch():
    return fc.driver_batch()


def check_driver(res, calls, batch):
    wanted = {"armijo_two_halvings": "armijo"}
    for k, (pr, run, env) in enumerate(batch):
        print(f"{fc.TERMINALS[k]}: alpha {res.alpha[k]!r} oracle {run['alpha']!r} envelope {env!r} psi calls {res.n_eval[k]} / {run['n_psi']}")
        assert res.terminal[k] == wanted.get(fc.TERMINALS[k], fc.TERMINALS[k]) == run["terminal"], (k, res.terminal[k], run["terminal"])
        assert res.n_eval[k] == run["n_psi"], (k, res.n_eval[k], run["n_psi"])
        assert bool(res.gac_error[k]) == run["gac_error"], k
        assert abs(res.alpha[k] - run["alpha"]) <= fc.MARGIN * env + 4.0 * np.spacing(abs(run["alpha"])), (k, res.alpha[k], run["alpha"], env)
    # the masks: a round evaluates only the problems still running, and every problem takes part in as many rounds as it counts
    assert res.rounds == len(calls) == int(max(res.n_eval))
    assert np.array_equal(np.sum(calls, axis=0), res.n_eval)
    assert len(set(int(v) for v in res.n_eval)) > 1 and any(0 < int(c.sum()) < len(batch) for c in calls)


def test_driver_reaches_every_terminal_in_one_batch(batch):
    from enlsip_gn import linesearch as ls
    assert [run["terminal"] for _, run, _ in batch] == ["first_fit", "first_fit_minrn", "second_fit", "second_minrn", "armijo", "armijo_error"]
    assert batch[1][1]["rec"]["minrn"] >= 1 and batch[4][1]["n_psi"] - 3 >= 2 and batch[5][1]["gac_error"]
    res, calls = run_driver(ls.HostLinesearchBackend(), batch)
    check_driver(res, calls, batch)
