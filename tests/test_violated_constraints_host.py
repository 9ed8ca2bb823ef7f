"""The host walk enlsip_gn_evaluate_violated_constraints (csrc/gn_violated_constraints.hpp, the routine the batched kernels run)
against the literal restatement oracle.enlsip_outer.evaluate_violated_constraints.  The oracle runs with a ws_mod proxy that
raises on the first repeated (active, inactive, t, i) state, the technique of tests/test_hs_set.py: where the oracle ends, t, the
lists and `added` are identical and status is 0; where it repeats, status is 1 and the lists are those of the repeated state at
the start of the pass.  Status 2 (the pass cap) must never occur.  No GPU."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))


class _Cycle(Exception):
    pass


def oracle_walk(l, n, q, t, active, inactive, cx, iau, walk=None):
    """(t, active (l,), inactive (l,), added, status) of the oracle; status 1 with the state the repeated pass starts from"""
    from oracle import enlsip_outer as eo
    from oracle import gn_oracle as go
    W = go.WorkingSet(q, t, l, np.array(active, dtype=np.int64), np.array(inactive, dtype=np.int64))
    seen, start, added = set(), {}, {"v": False}

    class Proxy:
        @staticmethod
        def remove_constraint(Wx, s):
            start["lists"] = (Wx.active.copy(), Wx.inactive.copy(), Wx.t, added["v"])      # the state the pass starts from
            go.remove_constraint(Wx, s)

        @staticmethod
        def add_constraint(Wx, s):
            state = (tuple(int(v) for v in Wx.active), tuple(int(v) for v in Wx.inactive), int(Wx.t), int(s))
            if state in seen:
                raise _Cycle()
            seen.add(state)
            go.add_constraint(Wx, s)
            added["v"] = True

    try:
        add = (walk or eo.evaluate_violated_constraints)(np.asarray(cx), W, iau, n, Proxy)
        return W.t, W.active.copy(), W.inactive.copy(), bool(add), 0
    except _Cycle:
        a, i, tt, _ = start["lists"]
        return tt, a, i, None, 1


def random_case(rng):
    l, n = int(rng.integers(1, 71)), int(rng.integers(1, 71))
    bnd = min(l, n)
    q = int(rng.integers(0, bnd + 1))
    t = int(rng.integers(q, bnd + 1))
    extra = np.sort(rng.choice(np.arange(q + 1, l + 1), size=t - q, replace=False)) if t > q else np.zeros(0, dtype=np.int64)
    active = np.zeros(l, dtype=np.int64)
    active[:t] = np.concatenate([np.arange(1, q + 1), extra])
    rest = np.setdiff1d(np.arange(1, l + 1), active[:t])
    inactive = np.zeros(l, dtype=np.int64)
    inactive[:l - t] = rest
    cx = rng.standard_normal(l) + float(rng.integers(-1, 2))
    if rng.random() < 0.3 and l >= 2:      # ties
        cx[rng.integers(0, l, size=max(1, l // 3))] = cx[0]
    iau = int(rng.integers(0, l + 1))
    return l, n, q, t, active, inactive, cx, iau


def hand_cases():
    nan = float("nan")
    full = lambda l: (np.arange(1, l + 1), np.zeros(l, dtype=np.int64))
    cases = {}
    a, i = full(4)
    cases["l_equals_t"] = (4, 6, 1, 4, a, i, np.array([-1.0, -1.0, -1.0, -1.0]), 0)
    a, i = full(3)
    cases["q_equals_l"] = (3, 3, 3, 3, a, i, np.array([0.5, -2.0, 0.0]), 2)
    cases["nan_is_never_violated"] = (4, 4, 0, 1, np.array([2, 0, 0, 0]), np.array([1, 3, 4, 0]), np.array([nan, 1.0, nan, -1.0]), 3)
    # capacity 2, both active inequalities hold the same worst value: the FIRST one (position 1) leaves
    cases["ties_first_maximum"] = (5, 2, 0, 2, np.array([4, 5, 0, 0, 0]), np.array([1, 2, 3, 0, 0]),
                                   np.array([1.0, 2.0, -3.0, 0.5, 0.5]), 0)
    # a NaN among the active values never wins the search; with only NaN / -Inf nothing is swapped
    cases["nan_active_no_swap"] = (3, 1, 0, 1, np.array([1, 0, 0]), np.array([2, 3, 0]), np.array([nan, -1.0, -2.0]), 0)
    cases["delta_arm"] = (3, 3, 0, 0, np.zeros(3, dtype=np.int64), np.array([1, 2, 3]), np.array([0.05, 0.05, 0.2]), 2)
    cases["delta_arm_not_reached"] = (3, 3, 0, 0, np.zeros(3, dtype=np.int64), np.array([1, 2, 3]), np.array([0.05, 0.1, 0.2]), 2)
    # at capacity the removed constraint 1 sorts in front of the candidate 2 and would come straight back: the reference spins
    cases["one_pass_cycle"] = (3, 1, 0, 1, np.array([1, 0, 0]), np.array([2, 3, 0]), np.array([0.5, -1.0, 2.0]), 0)
    # the same values, but the removed constraint 3 sorts behind the candidate: a true swap
    cases["swap"] = (3, 1, 0, 1, np.array([3, 0, 0]), np.array([1, 2, 0]), np.array([-1.0, 3.0, 0.5]), 0)
    # after the removal another constraint than the candidate sits at position i and is the one added (the quirk of :642)
    cases["quirk_adds_whatever_sits_at_i"] = (4, 1, 0, 1, np.array([1, 0, 0, 0]), np.array([2, 3, 4, 0]),
                                              np.array([0.5, 1.0, -1.0, 2.0]), 0)
    return cases


def host_walk(l, n, q, t, active, inactive, cx, iau):
    from enlsip_gn import evaluate_violated_constraints
    return evaluate_violated_constraints(l, n, q, t, active, inactive, cx, iau)


def same(got, want, tag):
    t, a, i, added, status = got
    wt, wa, wi, wadded, wstatus = want
    l = a.size
    assert status == wstatus, (tag, status, wstatus)
    assert status != 2, tag
    assert t == wt and np.array_equal(a, wa), tag
    assert np.array_equal(i[:l - t], wi[:l - t]) and not i[l - t:].any() and not wi[l - t:].any(), tag
    if wadded is not None:
        assert added == wadded, tag


def test_random_walks_match_the_oracle():
    rng = np.random.default_rng(20251019)
    stat, add, kinds = set(), set(), {"none": 0, "add": 0, "cycle": 0}
    for it in range(3000):
        case = random_case(rng)
        want = oracle_walk(*case)
        got = host_walk(*case)
        same(got, want, ("random", it))
        stat.add(got[4])
        add.add(got[3])
        kinds["cycle" if got[4] == 1 else ("add" if got[3] else "none")] += 1
    assert stat == {0, 1} and add == {False, True}, (stat, add)
    assert min(kinds.values()) >= 300, kinds      # every kind of walk is well represented


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(name):
    case = hand_cases()[name]
    want = oracle_walk(*case)
    got = host_walk(*case)
    same(got, want, name)
    expect = {"one_pass_cycle": (1, False), "swap": (0, True), "ties_first_maximum": (0, True), "nan_active_no_swap": (0, False),
              "l_equals_t": (0, False), "q_equals_l": (0, False), "delta_arm": (0, True), "delta_arm_not_reached": (0, False),
              "nan_is_never_violated": (0, True), "quirk_adds_whatever_sits_at_i": (1, True)}[name]
    assert (got[4], got[3]) == expect, (name, got)
    if name == "ties_first_maximum":
        assert list(got[1][:2]) == [3, 5] and 4 in got[2]
    if name == "delta_arm":
        assert list(got[1][:got[0]]) == [2]
    if name == "delta_arm_not_reached":
        assert got[0] == 0
    if name == "quirk_adds_whatever_sits_at_i":      # the violated 3 stays out, 2 went in; the next pass would spin
        assert list(got[1][:got[0]]) == [2]


@pytest.mark.parametrize("name", ["hs20", "hs23"])
def test_the_state_hs20_and_hs23_reach(name, monkeypatch):
    """the call inside which the restated outer iteration spins (tests/test_hs_set.py): the host walk stops it with status 1 in
    the state the repeated pass starts from"""
    import hs_problems as hp
    from oracle import enlsip_outer as eo
    key = [k for k in hp.CYCLING if name in k.lower()]
    assert key, list(hp.CYCLING)
    orig = eo.evaluate_violated_constraints
    caught = {}

    def watched(cx, W, index_alpha_upp, n, ws_mod):
        inact = np.zeros(W.l, dtype=np.int64)
        inact[:W.inactive.size] = W.inactive
        case = (W.l, n, W.q, W.t, W.active.copy(), inact, np.array(cx, dtype=np.float64), int(index_alpha_upp))
        want = oracle_walk(*case, walk=orig)
        if want[4] == 1:
            caught["case"], caught["want"] = case, want
            raise _Cycle()
        return orig(cx, W, index_alpha_upp, n, ws_mod)

    monkeypatch.setattr(eo, "evaluate_violated_constraints", watched)
    P = dict(hp.CYCLING[key[0]]())
    kw = dict(P.pop("kw"))
    P.pop("x_star"); P.pop("f_star")
    with pytest.raises(_Cycle):
        eo.solve(P.pop("r"), P.pop("jac_r"), P.pop("n"), P.pop("m"), P.pop("x0"), backend=eo.OracleBackend(), time_limit=30.0, **P, **kw)
    case, want = caught["case"], caught["want"]
    got = host_walk(*case)
    same(got, want, name)
    assert got[4] == 1 and got[0] == min(case[0], case[1])      # stopped at capacity, where the reference spins


def test_error_codes():
    import enlsip_gn._lib as L
    lib = L.load()
    l, n = 4, 3
    act = np.array([1, 2, 0, 0], dtype=np.int64)
    ina = np.array([3, 4, 0, 0], dtype=np.int64)
    cx = np.ones(l)      # nothing is violated: a call that passes the checks changes nothing
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(l=l, n=n, q=1, t=2, act=act, ina=ina, cx=cx, iau=0, t_null=False, added_null=False, status_null=False):
        tt, ad, st = C.c_int64(t), C.c_int64(-9), C.c_int64(-9)
        return lib.enlsip_gn_evaluate_violated_constraints(l, n, q, None if t_null else C.byref(tt), p(act), p(ina), p(cx), iau,
                                                           None if added_null else C.byref(ad), None if status_null else C.byref(st))

    bad = lambda v, k, x: np.concatenate([v[:k], [x], v[k + 1:]]).astype(np.int64)
    assert call() == 0
    for kw in (dict(t_null=True), dict(added_null=True), dict(status_null=True), dict(l=-1), dict(n=-1), dict(q=-1), dict(q=3),
               dict(t=5)):
        assert call(**kw) == -2, kw
    for kw in (dict(act=None), dict(ina=None), dict(cx=None)):
        assert call(**kw) == -4, kw
    for kw in (dict(act=bad(act, 0, 5)), dict(act=bad(act, 1, -1)), dict(ina=bad(ina, 1, 5)), dict(ina=bad(ina, 0, -1)), dict(iau=5),
               dict(iau=-1)):
        assert call(**kw) == -5, kw
    assert np.array_equal(act, [1, 2, 0, 0]) and np.array_equal(ina, [3, 4, 0, 0])
    assert call(l=0, t=0, q=0, act=None, ina=None, cx=None) == 0      # no constraint at all
