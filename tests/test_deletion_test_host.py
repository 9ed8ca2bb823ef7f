"""The constraint deletion test on the CPU: enlsip_gn_check_constraint_deletion (the host instantiation of
enlsip.jl_amd/csrc/gn_deletion_test.hpp, the routine the batched kernels run) against oracle.gn_oracle.check_constraint_deletion
(src/enlsip_functions.jl:574-603).  Every comparison is exact: the result is an index."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import gn_oracle as go

ROOT = Path(__file__).resolve().parents[1]
T_MAXES = (1, 2, 4, 8, 64, 65, 130)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import enlsip_gn._lib as L
    return L.load()


def oracle_s(q, lam, scaling, ds, grad_res):
    with np.errstate(all="ignore"):
        return go.check_constraint_deletion(q, np.zeros((len(lam), 1)), lam, scaling, ds, grad_res)


def random_cases(count=4000):
    """(q, lam, scaling, diag_scale, grad_res) as the issue sets them, from one generator"""
    rng = np.random.default_rng(0)
    cases = []
    for i in range(count):
        t_max = T_MAXES[int(rng.integers(len(T_MAXES)))]
        t = int(rng.integers(0, t_max + 1))
        q = int(rng.integers(0, t + 1))
        lam = rng.standard_normal(t)
        if i % 5 == 0 and t - q >= 2:      # a tie among the candidates
            a, b = rng.choice(np.arange(q, t), size=2, replace=False)
            lam[b] = lam[a]
        scaling = bool(i % 2)
        ds = np.ones(t) if i % 3 == 0 else rng.uniform(0.5, 2.0, t)
        if i % 5 == 0 and t - q >= 2:
            ds[b] = ds[a]
        grad_res = (0.0, 10.0 * abs(rng.standard_normal()), 1e-3)[i % 3]
        cases.append((q, lam, scaling, ds, grad_res))
    return cases


def edge_cases():
    """named edges: (name, q, lam, scaling, diag_scale, grad_res)"""
    nan, inf = np.nan, np.inf
    one = lambda t: np.ones(t)
    return [
        ("tie_last_wins", 0, np.array([1.0, -2.0, -2.0, 3.0]), False, one(4), 0.0),
        ("tie_last_wins_scaled", 1, np.array([1.0, -2.0, -1.0, -4.0]), True, np.array([1.0, 1.0, 0.5, 2.0]), 0.0),
        ("nan_candidate", 1, np.array([1.0, nan, -2.0]), False, one(3), 0.0),
        ("nan_below_q", 2, np.array([nan, 1.0, -2.0, -3.0]), False, one(4), 0.0),
        ("nan_last", 0, np.array([-1.0, -2.0, nan]), True, one(3), 0.0),
        ("all_zero", 1, np.zeros(5), False, one(5), 0.0),
        ("all_zero_scaled", 0, np.zeros(3), True, np.array([0.5, 2.0, 1.5]), 0.0),
        ("t_equals_q", 3, np.array([-1.0, -2.0, -3.0]), False, one(3), 0.0),
        ("t_zero", 0, np.zeros(0), False, one(0), 0.0),
        ("q_is_t_minus_1", 3, np.array([-5.0, -6.0, -7.0, -1.0]), False, one(4), 0.0),
        ("q_is_t_minus_1_positive", 3, np.array([-5.0, -6.0, -7.0, 1.0]), False, one(4), 0.0),
        ("minus_zero", 0, np.array([-0.0, 0.0, -0.0, 0.0]), False, one(4), 0.0),
        ("minus_zero_first", 0, np.array([0.0, -0.0]), True, np.array([2.0, 0.5]), 0.0),
        ("minus_inf", 0, np.array([1.0, -inf, -3.0]), False, one(3), 0.0),
        ("plus_inf", 0, np.array([inf, -1.0, -3.0]), False, one(3), 0.0),
        ("both_inf", 1, np.array([-inf, -inf, inf, -inf]), False, one(4), 0.0),
        ("inf_gated", 0, np.array([1.0, -inf]), False, one(2), inf),
        ("gate_closes", 0, np.array([1.0, -1.0]), False, one(2), 10.0 + 1e-9),
        ("gate_equal_keeps", 0, np.array([1.0, -1.0]), False, one(2), 10.0),
        ("nan_grad_res", 0, np.array([1.0, -1.0]), False, one(2), nan),
    ]


def lib_s(lib, q, lam, scaling, ds, grad_res):
    lam, ds = np.ascontiguousarray(lam, dtype=np.float64), np.ascontiguousarray(ds, dtype=np.float64)
    s = C.c_int64(-9)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = lib.enlsip_gn_check_constraint_deletion(q, lam.size, p(lam), p(ds), int(scaling), grad_res, C.byref(s))
    assert rc == 0
    return int(s.value)


def test_random_cases_against_the_oracle(lib):
    cases = random_cases()
    want = [oracle_s(*c) for c in cases]
    # on the oracle alone: both outcomes are well populated, and the grad_res gate turns many a non-zero s into 0
    zero = sum(1 for s in want if s == 0)
    gated = sum(1 for c, s in zip(cases, want) if s == 0 and oracle_s(c[0], c[1], c[2], c[3], -np.inf) != 0)
    print(f"oracle: {zero} cases with s = 0, {len(want) - zero} with s != 0, {gated} closed by the gate")
    assert zero >= 0.4 * len(want) and len(want) - zero >= 0.4 * len(want) and gated >= 100
    got = [lib_s(lib, *c) for c in cases]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (bad[:5], [(got[i], want[i]) for i in bad[:5]])


@pytest.mark.parametrize("case", edge_cases(), ids=lambda c: c[0])
def test_named_edges_against_the_oracle(lib, case):
    name, q, lam, scaling, ds, grad_res = case
    want = oracle_s(q, lam, scaling, ds, grad_res)
    assert lib_s(lib, q, lam, scaling, ds, grad_res) == want, name
    # what the issue states about them, on the oracle
    if name.startswith("tie_last_wins"):
        assert want == (3 if not scaling else 4)
    if name.startswith("nan") and name != "nan_grad_res":
        assert want == 0
    if name.startswith("all_zero"):
        assert want == len(lam)
    if name in ("t_equals_q", "t_zero"):
        assert want == 0


def test_python_mirrors_agree(lib):
    """working_set.check_constraint_deletion (the host mirror the drivers use) and the module-level wrapper of the library"""
    from enlsip_gn import check_constraint_deletion, working_set as ws
    cases = random_cases(600) + [c[1:] for c in edge_cases()]
    for q, lam, scaling, ds, grad_res in cases:
        want = oracle_s(q, lam, scaling, ds, grad_res)
        with np.errstate(all="ignore"):
            assert ws.check_constraint_deletion(q, np.zeros((len(lam), 1)), lam, scaling, ds, grad_res) == want
        assert check_constraint_deletion(q, lam, scaling, ds, grad_res) == want


def test_argument_errors(lib):
    s = C.c_int64(7)
    x = np.ones(4)
    p = x.ctypes.data_as(C.c_void_p)
    f = lib.enlsip_gn_check_constraint_deletion
    assert f(0, -1, p, p, 0, 0.0, C.byref(s)) < 0          # t < 0
    assert f(-1, 4, p, p, 0, 0.0, C.byref(s)) < 0          # q < 0
    assert f(5, 4, p, p, 0, 0.0, C.byref(s)) < 0           # q > t
    assert f(0, 4, p, p, 0, 0.0, None) < 0                 # s NULL
    assert f(1, 4, None, p, 0, 0.0, C.byref(s)) < 0        # lambda NULL while t > q
    assert f(1, 4, p, None, 0, 0.0, C.byref(s)) < 0        # diag_scale NULL while t > q
    assert s.value == 7                                    # nothing written on an error
    assert f(4, 4, None, None, 0, 0.0, C.byref(s)) == 0 and s.value == 0      # t == q: neither array is read
    assert f(0, 0, None, None, 1, 0.0, C.byref(s)) == 0 and s.value == 0


def test_header_binding_and_glue_declare_the_entry_points():
    import enlsip_gn._lib as L
    hdr = (ROOT / "include" / "enlsip_gn.h").read_text()
    glue = (ROOT / "enlsip.jl_amd" / "julia" / "EnlsipHIP.jl").read_text()
    for name, nargs in (("enlsip_gn_check_constraint_deletion", 7), ("enlsip_gn_delete_constraints_batched_dev", 17),
                        ("enlsip_gn_restore_constraints_batched_dev", 13), ("enlsip_gn_get_deletion_form", 2)):
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S).group(1)
        assert len(args.split(",")) == nargs == len(L.PROTOTYPES[name][1]), name
        assert f"(:{name}, LIB)" in glue, name
    assert "src/enlsip_functions.jl:574-603" in hdr
