"""penalty_weight_update (src/enlsip_functions.jl:1545-1629, with :1504-1539, :1429-1497, :1374-1423, :1344-1360) through the
library's host entry point enlsip_gn_penalty_weight_update, the routine the batched kernels run, against
oracle.enlsip_outer.penalty_weight_update.  No GPU.

The oracle runs on the vectors Jp, rx with copies of K; the library gets the exactly rounded sums of the same vectors (mpmath).
Tolerance, measured from the oracle alone: every case is run 16 more times with each entry of Jp and rx moved by at most one ulp
(seeded); the envelope of an output is its largest change, and the library must lie within ten times the envelope plus 4 ulp of the
value.  A case whose discrete pattern (branch, which entries of w differ from w_old and from the old K[4], which entries of K
moved) changes under that perturbation sits on a tie; none is allowed.  The hand-made dyadic cases are compared bit for bit.

The oracle's Python division raises where Julia's `rmy / nrm_Ap` (:1514) gives +-Inf, so the maximum-norm arm with nrm_Ap = 0 is
put to the oracle only with alpha_w = 1 (the arm that does not divide); the division by zero itself is checked against the value
the IEEE rule gives.

One-line mutations of the routine, run on the CPU: `w[:] = K[4]` (:1383) replaced by previous_w makes
test_every_case_against_the_oracle and test_exact_cases_bit_for_bit fail.  `buff >= w_old[i]` turned into `>` (:1405) is met by no
assertion, and cannot be by values: at a tie buff == w_old[i] the entry holds the same weight whether it is kept or dropped, and
the next pass's c is the same number in exact arithmetic (tau - w_i y_i over y_sum - y_i^2 equals tau / y_sum when
c y_i == w_i), so the two arms differ by roundings only."""
import collections
import ctypes as C

import numpy as np
import pytest

import penalty_cases as pc


@pytest.fixture(scope="module")
def lib():
    import enlsip_gn._lib as Lm
    return Lm.load()


@pytest.fixture(scope="module")
def results():
    """(case, oracle reference, envelope, stable, library outputs) per case: computed once, shared, left unchanged"""
    from enlsip_gn import penalty_weight_update
    out = []
    for i, c in enumerate(pc.host_cases()):
        ref = pc.oracle_run(c)
        env, stable = pc.envelope(c, ref, 1000 + i)
        K = c["K"].copy()
        w, dpsi0, psi0, atwa, branch, K = penalty_weight_update(c["w_old"], c["active"], c["t"], c["dimA"], c["norm_code"], c["Ap"],
                                                                c["cx"], K, *pc.exact_sums(c))
        out.append((c, ref, env, stable, dict(w=w, K=K, dpsi0=dpsi0, psi0=psi0, atwa=atwa, branch=branch)))
    return out


def test_no_case_sits_on_a_tie(results):
    unstable = [c["name"] for c, _, _, stable, _ in results if not stable]
    assert not unstable, unstable


def test_every_case_against_the_oracle(results):
    worst = collections.defaultdict(float)
    for c, ref, env, _, got in results:
        assert got["branch"] == ref["branch"], (c["name"], got["branch"], ref["branch"])
        for key in ("w", "K", "dpsi0", "psi0", "atwa"):
            g, r, e = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (got[key], ref[key], env[key]))
            with np.errstate(all="ignore"):
                tol = pc.MARGIN * e + 4.0 * np.spacing(np.abs(r))
                ratio = np.where(np.isfinite(r) & (tol > 0), np.abs(g - r) / np.where(tol > 0, tol, 1.0), 0.0)
            worst[key] = max(worst[key], float(np.nanmax(ratio)))
            assert pc.within(g, r, e), (c["name"], key, g, r, e)
        # the discrete pattern of the library's outputs is the oracle's
        assert tuple((got["w"] != c["w_old"]).tolist()) == ref["pattern"][1], c["name"]
        assert tuple((got["w"] != c["K"][3]).tolist()) == ref["pattern"][2], c["name"]
    print({k: round(v, 3) for k, v in worst.items()}, "= worst |got - ref| / tolerance per output")


def test_exact_cases_bit_for_bit(results):
    seen = set()
    for c, ref, _, _, got in results:
        if not c["name"].startswith("exact_"):
            continue
        seen.add(c["norm_code"])
        assert got["branch"] == ref["branch"]
        for key in ("w", "K", "dpsi0", "psi0", "atwa"):
            assert pc.same_bits(got[key], ref[key]), (c["name"], key, got[key], ref[key])
    assert seen == {0, 2}


def first_moved_row(K0, K1, k):
    return next((ii for ii in range(4) if not pc.same_bits(K0[ii, k], K1[ii, k])), None)


def test_the_case_list_covers_every_path(results):
    n = collections.Counter()
    for c, ref, _, _, got in results:
        rec, t, dimA = ref["rec"], c["t"], c["dimA"]
        n["branch", got["branch"]] += 1
        n["t0"] += t == 0
        n["dimA0"] += t > 0 and dimA == 0
        n["dimA_mid"] += 0 < dimA < t
        n["dimA_t"] += t > 0 and dimA == t
        n["not_ascending"] += bool(np.any(np.diff(c["active"][:t]) < 0))
        if c["norm_code"] == 0:
            n["mu_arm", rec["mu_zero_arm"]] += 1
            n["mu_place", rec["mu_place"]] += 1
            # the library placed mu where the oracle did
            assert first_moved_row(c["K"], got["K"], 0) == rec["mu_place"], c["name"]
        elif t:
            for k in c["active"][:t] - 1:
                n["assort", first_moved_row(c["K"], ref["K"], k)] += 1
        if "ctrl" in rec:
            n["nb_pos0"] += rec["nb_pos"] == 0
            if rec["nb_pos"] > 0:
                d = rec["drops"]
                n["no_drop"] += sum(d) == 0
                n["one_pass_drop"] += sum(1 for x in d if x) == 1
                n["ctrl1_two_pass_drop"] += rec["ctrl"] == 1 and sum(1 for x in d if x) >= 2
                n["emptied"] += sum(d) == rec["nb_pos"]
                n["c_is_1"] += rec["c_is_1"]
        with np.errstate(all="ignore"):
            act = c["active"][:dimA] - 1
            n["nrm_Ap0"] += t > 0 and not np.any(c["Ap"])
            n["nrm_cx0"] += dimA > 0 and not np.any(c["cx"][act])
            n["JpJp0"] += not np.any(c["Jp"])
    print(dict(n))
    need = [("branch", b) for b in range(5)] + [("mu_arm", True), ("mu_arm", False)] + [("mu_place", p) for p in (0, 1, 2, 3, None)]
    need += [("assort", p) for p in (0, 1, 2, 3)]
    need += ["t0", "dimA0", "dimA_mid", "dimA_t", "not_ascending", "nb_pos0", "no_drop", "one_pass_drop", "ctrl1_two_pass_drop",
             "emptied", "c_is_1", "nrm_Ap0", "nrm_cx0", "JpJp0"]
    missing = [k for k in need if n[k] < 1]
    assert not missing, missing


def test_division_by_a_zero_norm_is_ieee(lib):
    """:1514 with nrm_Ap = 0 outside the alpha_w = 1 arm: mu = rmy / 0 = +Inf (rmy > 0 here).  t = 0: no weight changes, mu > w[1] is
    placed at the top of K[.][1] (:1515-1537, active[1] == 0 read as 1).  t > 0 with Ap = 0: the active weights become +Inf."""
    from enlsip_gn import penalty_weight_update
    w_old = np.array([1.0, 2.0, 3.0])
    K = np.array([[8.0, 9.0, 9.0], [4.0, 9.0, 9.0], [2.0, 9.0, 9.0], [1.0, 9.0, 9.0]])
    JpJp, Jprx, rxrx = 4.0, 1.0, 9.0            # alpha_w = -1 / 4, rmy = 5 / 0.25 - 4 = 16
    w, dpsi0, psi0, atwa, branch, K1 = penalty_weight_update(w_old, np.zeros(3, dtype=np.int64), 0, 0, 0, np.zeros(0), np.zeros(3),
                                                             K.copy(), JpJp, Jprx, rxrx)
    assert branch == 0 and pc.same_bits(w, w_old) and (dpsi0, psi0, atwa) == (1.0, 4.5, 0.0)
    assert pc.same_bits(K1, np.array([[np.inf, 9.0, 9.0], [8.0, 9.0, 9.0], [4.0, 9.0, 9.0], [2.0, 9.0, 9.0]]))
    w, dpsi0, psi0, atwa, branch, K1 = penalty_weight_update(w_old, np.array([3, 2, 0]), 2, 1, 0, np.zeros(2), np.array([1.0, 1.0, 1.0]),
                                                             K.copy(), JpJp, Jprx, rxrx)
    assert branch == 0 and pc.same_bits(w, np.array([1.0, np.inf, np.inf])) and psi0 == np.inf and np.isnan(atwa) and np.isnan(dpsi0)
    assert pc.same_bits(K1[:, 0], np.array([np.inf, 8.0, 4.0, 2.0])) and pc.same_bits(K1[:, 1:], K[:, 1:])
    # norm_code 0 with l == 0, where the Julia would throw: w stays empty, K untouched, the scalars are those of no constraint
    w, dpsi0, psi0, atwa, branch, _ = penalty_weight_update(np.zeros(0), np.zeros(0, dtype=np.int64), 0, 0, 0, np.zeros(0), np.zeros(0),
                                                            np.zeros((4, 0)), JpJp, Jprx, rxrx)
    assert w.size == 0 and branch == 0 and (dpsi0, psi0, atwa) == (1.0, 4.5, 0.0)


def test_w_may_be_w_old(lib):
    for c in pc.exact_cases() + pc.special_cases():
        l, t = c["l"], c["t"]
        s = pc.exact_sums(c)
        outs = []
        for alias in (False, True):
            w_old, K = c["w_old"].copy(), c["K"].copy()
            w = w_old if alias else np.zeros(l)
            sc, br = np.zeros(3), C.c_int(-1)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            rc = lib.enlsip_gn_penalty_weight_update(l, t, p(c["active"]), c["dimA"], c["norm_code"], p(w_old), p(c["Ap"]), p(c["cx"]),
                                                     *s, p(K), p(w), p(sc), C.byref(br))
            assert rc == 0
            outs.append((w.copy(), K, sc, br.value))
        assert all(pc.same_bits(a, b) for a, b in zip(outs[0][:3], outs[1][:3])) and outs[0][3] == outs[1][3], c["name"]


def test_argument_errors_leave_K_and_w_untouched(lib):
    c = pc.exact_cases()[1]
    l, t = c["l"], c["t"]
    SENT = -777.25
    K, w, sc = c["K"].copy(), np.full(l, SENT), np.full(3, SENT)
    br = C.c_int(-9)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    good = dict(l=l, t=t, active=c["active"], dimA=c["dimA"], norm_code=2, w_old=c["w_old"], Ap=c["Ap"], cx=c["cx"], K=K, w=w, sc=sc,
                br=C.byref(br))

    def call(**kw):
        a = dict(good, **kw)
        return lib.enlsip_gn_penalty_weight_update(a["l"], a["t"], p(a["active"]), a["dimA"], a["norm_code"], p(a["w_old"]), p(a["Ap"]),
                                                   p(a["cx"]), 4.0, 4.0, 16.0, p(a["K"]), p(a["w"]), p(a["sc"]), a["br"])

    def bad_active(i, v):
        a = c["active"].copy()
        a[i] = v
        return a

    cases = [(-2, dict(K=None)), (-2, dict(w=None)), (-2, dict(sc=None)), (-2, dict(br=None)), (-2, dict(l=-1)), (-2, dict(t=-1)),
             (-2, dict(t=l + 1)), (-2, dict(dimA=-1)), (-2, dict(dimA=t + 1)), (-2, dict(norm_code=1)), (-2, dict(norm_code=3)),
             (-4, dict(active=None)), (-4, dict(w_old=None)), (-4, dict(Ap=None)), (-4, dict(cx=None)),
             (-5, dict(active=bad_active(0, 0))), (-5, dict(active=bad_active(t - 1, l + 1))), (-5, dict(active=bad_active(1, -3)))]
    for want, kw in cases:
        assert call(**kw) == want, (want, list(kw))
    assert pc.same_bits(K, c["K"]) and np.all(w == SENT) and np.all(sc == SENT) and br.value == -9
    # an entry past t is not read; with t == 0 the t-vectors may be NULL
    assert call(active=bad_active(t, l + 5)) == 0
    assert call(t=0, dimA=0, active=None, Ap=None, cx=None) == 0
