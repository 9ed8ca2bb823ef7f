"""The upper bound of the steplength on the CPU: enlsip_gn_upper_bound_steplength (the host instantiation of
enlsip.jl_amd/csrc/gn_steplength_bound.hpp, the routine the batched kernels run) against
oracle/enlsip_outer.py::upper_bound_steplength (src/enlsip_functions.jl:2149-2178) on the same Ap.  alpha_upp and the index are
compared exactly: the inputs and the IEEE operations are the same.  The file also proves, from float64 products alone, the input
conditions the device cases rely on (tests/test_gpu_linesearch_setup_batched.py)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import linesearch_cases as lc

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import enlsip_gn._lib as L
    return L.load()


def lib_bound(lib, Ap, cx, inactive, n_inactive, index_del):
    Ap, cx = np.ascontiguousarray(Ap, dtype=np.float64), np.ascontiguousarray(cx, dtype=np.float64)
    lst = np.ascontiguousarray(inactive, dtype=np.int64)
    a, idx = C.c_double(-9.0), C.c_int64(-9)
    p = lambda x: x.ctypes.data_as(C.c_void_p) if x.size else None
    rc = lib.enlsip_gn_upper_bound_steplength(Ap.size, int(n_inactive), p(lst), int(index_del), p(cx), p(Ap), C.byref(a), C.byref(idx))
    assert rc == 0
    return float(a.value), int(idx.value)


def same_answer(got, want):
    return got[1] == want[1] and np.float64(got[0]).view(np.uint64) == np.float64(want[0]).view(np.uint64)


def test_random_cases_against_the_oracle(lib):
    rng = np.random.default_rng(0)
    cases = [lc.random_case(rng, tie=(i % 5 == 0)) for i in range(600)]
    want, got = [], []
    for c in cases:
        Ap = c["A"] @ c["p"]
        want.append(lc.oracle_bound(Ap, c["cx"], c["inactive"], c["n_inactive"], c["index_del"]))
        got.append(lib_bound(lib, Ap, c["cx"], c["inactive"], c["n_inactive"], c["index_del"]))
    # on the oracle alone: every outcome is well populated
    none = sum(1 for a, i in want if i == 0)
    capped = sum(1 for a, i in want if i != 0 and a == 3.0)
    below = sum(1 for a, i in want if i != 0 and a < 3.0)
    print(f"oracle: {none} cases without a row, {capped} capped at 3.0 with a row, {below} below 3.0")
    assert min(none, capped, below) >= 50
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if not same_answer(g, w)]
    assert not bad, (bad[:5], [(got[i], want[i]) for i in bad[:5]])


@pytest.mark.parametrize("l", (8, 300))
@pytest.mark.parametrize("case", lc.edge_cases(), ids=lambda c: c[0])
def test_named_edges(lib, case, l):
    name = case[0]
    _, cx, Ap, lst, ni, idel, want = next(c for c in lc.edge_cases(l) if c[0] == name)
    oracle = lc.oracle_bound(Ap, cx, lst, ni, idel)
    got = lib_bound(lib, Ap, cx, lst, ni, idel)
    assert same_answer(got, oracle), (name, got, oracle)
    assert want is None or same_answer(got, want), (name, got, want)
    if name == "all_alpha_above_3":      # the reference keeps the minimising row although the bound is the cap
        assert got[0] == 3.0 and got[1] != 0


def test_l_equal_1(lib):
    one = np.array([1], dtype=np.int64)
    for cx, Ap, idel, want in ((2.0, -4.0, 0, (0.5, 1)), (2.0, -4.0, 1, (3.0, 0)), (8.0, -1.0, 0, (3.0, 1)), (-2.0, -4.0, 0, (3.0, 0)),
                               (2.0, 4.0, 0, (3.0, 0)), (2.0, -0.0, 0, (3.0, 0)), (np.nan, -1.0, 0, (3.0, 0))):
        got = lib_bound(lib, np.array([Ap]), np.array([cx]), one, 1, idel)
        assert same_answer(got, want) and same_answer(got, lc.oracle_bound(np.array([Ap]), np.array([cx]), one, 1, idel)), (cx, Ap)
    assert lib_bound(lib, np.array([-4.0]), np.array([2.0]), one, 0, 0) == (3.0, 0)
    assert lib_bound(lib, np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int64), 0, 0) == (3.0, 0)      # l = 0


def test_python_wrappers_agree(lib):
    from enlsip_gn import linesearch as ls, upper_bound_steplength, working_set as ws
    rng = np.random.default_rng(3)
    for i in range(100):
        c = lc.random_case(rng, tie=(i % 4 == 0))
        Ap = c["A"] @ c["p"]
        want = lc.oracle_bound(Ap, c["cx"], c["inactive"], c["n_inactive"], c["index_del"])
        assert same_answer(upper_bound_steplength(c["inactive"], c["n_inactive"], c["index_del"], c["cx"], Ap), want)
        l = Ap.size
        W = ws.WorkingSet(0, l - c["n_inactive"], l, np.zeros(l, dtype=np.int64), c["inactive"])
        assert same_answer(ls.upper_bound_steplength(Ap, c["cx"], W, c["index_del"]), want)


def test_argument_errors(lib):
    f = lib.enlsip_gn_upper_bound_steplength
    x = np.ones(4)
    lst = np.array([1, 2, 3, 4], dtype=np.int64)
    p, q = x.ctypes.data_as(C.c_void_p), lst.ctypes.data_as(C.c_void_p)
    a, i = C.c_double(7.0), C.c_int64(7)
    A, I = C.byref(a), C.byref(i)
    assert f(4, 4, q, 0, p, p, None, I) == -2               # an output pointer NULL
    assert f(4, 4, q, 0, p, p, A, None) == -2
    assert f(-1, 0, q, 0, p, p, A, I) == -2                 # l < 0
    assert f(4, -1, q, 0, p, p, A, I) == -2                 # n_inactive outside 0..l
    assert f(4, 5, q, 0, p, p, A, I) == -2
    assert f(4, 4, None, 0, p, p, A, I) == -4               # an input NULL while n_inactive > 0
    assert f(4, 4, q, 0, None, p, A, I) == -4
    assert f(4, 4, q, 0, p, None, A, I) == -4
    for bad in (5, -1):                                     # a list entry outside 0..l
        lst2 = np.array([1, 2, bad, 4], dtype=np.int64)
        assert f(4, 4, lst2.ctypes.data_as(C.c_void_p), 0, p, p, A, I) == -5
        assert f(4, 2, lst2.ctypes.data_as(C.c_void_p), 0, p, p, A, I) == 0      # ... but not past the used part
        a.value, i.value = 7.0, 7
    assert (a.value, i.value) == (7.0, 7)                   # nothing written on an error
    assert f(4, 0, None, 0, None, None, A, I) == 0 and (a.value, i.value) == (3.0, 0)      # n_inactive = 0: no array is read


def test_header_binding_and_glue_declare_the_entry_points():
    import enlsip_gn._lib as L
    hdr = (ROOT / "include" / "enlsip_gn.h").read_text()
    glue = (ROOT / "enlsip.jl_amd" / "julia" / "EnlsipHIP.jl").read_text()
    for name, nargs in (("enlsip_gn_upper_bound_steplength", 8), ("enlsip_gn_linesearch_setup_batched_dev", 19),
                        ("enlsip_gn_get_linesearch_form", 2)):
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S).group(1)
        assert len(args.split(",")) == nargs == len(L.PROTOTYPES[name][1]), name
        assert f"(:{name}, LIB)" in glue, name
    for cite in ("src/enlsip_functions.jl:2149-2178", ":2226-2229", ":1561-1584", ":2269"):
        assert cite in hdr, cite


# ---- the input conditions of the device cases, from the oracle side alone ------------------------------------------------------
def test_device_cases_have_a_gap():
    """For every problem of the device test's random batches: the two smallest qualifying alpha_j differ by more than 1e-9
    relative and every |Ap_j| that decides a sign exceeds 1e-9 sum |a||p|, so the index cannot depend on the summation order; and
    the winning row is conditioned well enough that two roundings of its dot product keep alpha_upp within 1e-12 relative."""
    worst_gap, worst_margin, worst_alpha, deciding = np.inf, np.inf, 0.0, 0
    for name, b in lc.gpu_batches().items():
        for k in range(b["A"].shape[0]):
            gap, margin, cond = lc.gap_report(b["A"][k], b["p"][k], b["cx"][k], b["inactive"][k], b["n_inactive"][k],
                                              b["index_del"][k])
            n = b["A"].shape[2]
            assert gap > lc.GAP and margin > lc.GAP and 4 * n * lc.U * cond <= 1e-12, (name, k, gap, margin, cond)
            worst_gap, worst_margin, worst_alpha = min(worst_gap, gap), min(worst_margin, margin), max(worst_alpha, 4 * n * lc.U * cond)
            deciding += np.isfinite(gap)
    print(f"device cases: smallest gap {worst_gap:.3e}, smallest sign margin {worst_margin:.3e}, largest alpha_upp spread "
          f"{worst_alpha:.3e}, {deciding} problems with two candidates")
    assert deciding >= 50
