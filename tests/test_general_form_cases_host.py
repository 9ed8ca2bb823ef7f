"""Certification, without a GPU, of the case tables of tests/general_form_cases.py: every table is built, the conditions its GPU
test relies on are asserted on the inputs and the host routines' answers, and the time the expected values take to build is
recorded (record_property, and printed)."""
import time

import numpy as np
import pytest

import general_form_cases as G
from general_form_cases import A, D, lc, pc

STRIDE = G.STRIDE


def timed(record_property, name, build):
    t0 = time.perf_counter()
    out = build()
    dt = time.perf_counter() - t0
    record_property(f"build_seconds[{name}]", round(dt, 3))
    print(f"expected values of {name}: {dt:.2f} s")
    return out


# ---- deletion / restore ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t_max", G.DELETE_SHAPES)
def test_delete_tables(record_property, n, t_max):
    cases = timed(record_property, f"delete {n}x{t_max}", lambda: G.delete_cases(n, t_max, True))
    assert len(cases) == 3 and [c["record"] for c in cases] == [True, True, False] and {c["scaling"] for c in cases} == {True, False}
    for c in cases:
        t, s = c["t"], c["s"]
        assert 5 <= len(t) <= 9 and t.min() == 0 and t.max() == t_max
        assert s.any() and not s.all() and np.all(s <= t)
        if c["take"] is not None:
            assert (c["take"] == 0).any() and not s[c["take"] == 0].any()
        if t_max > STRIDE:      # entries behind the first stride are shifted (a shift of MORE than a stride: the designed tables)
            assert t[s > 0].max() > STRIDE
        if c["back"] is not None:
            hit, back = s != 0, c["back"] != 0
            assert back.any() and (hit & ~back).any() and not (back & ~hit).any()      # a proper subset of the deleted rows
    assert cases[0]["back"] is not None


@pytest.mark.parametrize("t", G.DESIGNED_T)
def test_designed_delete_tables(record_property, t):
    c = timed(record_property, f"designed delete t={t}", lambda: G.designed_delete_case(t, True))      # asserts the designed s itself
    rows = G.designed_rows(t)
    assert set(rows) >= {1, 256, 257, t - 1, t} and all(s <= t for s in rows)
    assert (t < 513) or {258, 512, 513} <= set(rows)
    assert np.array_equal(c["s"][:len(rows)], rows)
    for k, pos in enumerate(c["ties"], start=len(rows)):
        assert c["s"][k] == pos[-1] and all(c["buf"].lam[k, p - 1] == c["buf"].lam[k, pos[-1] - 1] for p in pos)
        assert len({(p - 1) // STRIDE for p in pos}) > 1 or pos == [255, 256, 257][:len(pos)]
    assert any((p[0] - 1) // STRIDE != (p[-1] - 1) // STRIDE for p in c["ties"])
    back = c["back"]
    assert back.any() and ((c["s"] != 0) & (back == 0)).any()
    assert (c["t"] - c["s"]).max() == t - 1 and (c["t"] - c["s"])[back != 0].max() >= STRIDE      # every trip of the vector loops, both ways


# ---- additions / rebuild ---------------------------------------------------------------------------------------------------------------
def check_add(cases, n, l):
    seen_status, seen_added, ins, rem = set(), set(), -1, -1
    for c in cases:
        assert not (c["wst"] == 2).any()
        seen_status |= set(c["wst"].tolist())
        seen_added |= set(c["wadd"].tolist())
        i, r = G.add_positions(c)      # asserts that the restated walk and the host routine agree
        ins, rem = max(ins, i), max(rem, r)
    if n < l:
        assert seen_status == {0, 1} and seen_added == {0, 1}, (seen_status, seen_added)
    # the lists are long enough for a second stride only here: active holds at most min(n, l) entries, inactive at most l
    if min(n, l) > STRIDE:
        assert ins >= STRIDE, ins
    if l > STRIDE:
        assert rem >= STRIDE, rem
    return ins, rem


@pytest.mark.parametrize("n,l", G.ADD_SHAPES)
def test_add_tables(record_property, n, l):
    cases = timed(record_property, f"add {n}x{l}", lambda: G.add_shape_cases(n, l, True))
    assert [c["scaling"] for c in cases] == [False, True] and cases[0]["take"] is None
    assert set(cases[1]["take"].tolist()) == {0, 1, 2}
    check_add(cases, n, l)


def test_add_full_and_capped_tables(record_property):
    c = timed(record_property, "add 1024x1024", G.add_full_case)
    assert (c["n"], c["l"], c["t_max"], c["B"], c["scaling"]) == (1024, 1024, 1024, 3, True)
    ins, rem = check_add([c], 1024, 1024)
    assert c["wt"].max() > 3 * STRIDE or ins >= STRIDE
    c = timed(record_property, "add capped", G.add_capped_case)
    assert c["t_max"] < min(c["n"], c["l"]) and c["t_max"] % 64 != 0 and c["wt"].max() == c["t_max"] and c["wt"].min() < c["t_max"]
    assert not c["wadd"].any() and np.array_equal(c["wt"], c["t"])      # rebuild only


# ---- line-search set-up ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in G.LS_SHAPES])
def test_linesearch_tables(record_property, name):
    b = timed(record_property, f"linesearch {name}", lambda: G.ls_batch(name))
    B, l, n = b["A"].shape
    for k in range(B):      # the input conditions check_batch's index and alpha comparisons rest on
        assert G.ls_conditions(b, k), (name, k, lc.gap_report(b["A"][k], b["p"][k], b["cx"][k], b["inactive"][k], b["n_inactive"][k], b["index_del"][k]))
    if l > STRIDE:
        assert b["n_inactive"].max() > STRIDE


def test_linesearch_designed_ties():
    from enlsip_gn import upper_bound_steplength
    same, two = G.ls_designed_ties()
    for name, cx, Ap, lst, ni, idel, want in (same, two):
        pos = [int(np.flatnonzero(lst == r + 1)[0]) for r in np.flatnonzero(Ap == -2.0)]
        assert len(pos) == 2 and want[1] == lst[min(pos)] and want[1] != min(lst[pos])      # the first position, not the lowest row
        got = upper_bound_steplength(lst, ni, idel, cx, Ap)
        assert (float(got[0]), int(got[1])) == want == lc.oracle_bound(Ap, cx, lst, ni, idel), name
    pos = sorted(int(np.flatnonzero(same[3] == r + 1)[0]) for r in np.flatnonzero(same[2] == -2.0))
    assert pos[1] - pos[0] == STRIDE                                   # one thread of k_ls_bound sees both
    pos = sorted(int(np.flatnonzero(two[3] == r + 1)[0]) for r in np.flatnonzero(two[2] == -2.0))
    assert pos == [40, 300] and (pos[1] - pos[0]) % STRIDE != 0        # two threads


def test_linesearch_edges_at_the_cap():
    edges = lc.edge_cases(G.CAP)
    assert all(e[1].size == G.CAP for e in edges)
    far = next(e for e in edges if e[0] == "tie_far_end_first_wins")
    assert int(np.flatnonzero(far[3] == 5)[0]) > 3 * STRIDE      # the winning tie sits in the list's fourth stride


# ---- penalty weights -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,t_max", G.PENALTY_SHAPES)
def test_penalty_tables(record_property, l, t_max):
    for norm_code in (0, 2):
        probs = timed(record_property, f"penalty {l}x{t_max} norm {norm_code} (search)", lambda: G.penalty_problems(l, t_max, norm_code))
        ts = [c["t"] for c in probs]
        assert len(probs) == G.PENALTY_BATCH and max(ts) == t_max and min(ts) == 0 and ts.count(t_max) >= 2
        for scaling in (False, True):
            call = G.penalty_call(probs, l, t_max, norm_code, scaling)
            timed(record_property, f"penalty {l}x{t_max} norm {norm_code} scaling {scaling}",
                  lambda: [call.reference(k) for k in range(len(probs))])
            far_moves, first_moved = G.penalty_coverage(probs, l, t_max, norm_code, scaling)
            if norm_code and t_max > STRIDE:
                assert far_moves > 0, (l, t_max, scaling)      # an active entry at list position >= 256 moves an entry of K
            if not norm_code:
                assert first_moved > 0, (l, t_max, scaling)    # a problem takes the `moved` branch of the max norm
