"""The termination test on the CPU: enlsip_gn_minmax_lagrangian_mult and enlsip_gn_check_termination_criteria (the host routines of
enlsip.jl_amd/csrc/gn_termination.hpp; the second is the one the batched call runs on the downloaded sums) against
oracle/enlsip_outer.py (src/enlsip_functions.jl:540-564, :2399-2517), exactly: same inputs, same IEEE operations.  The decision is
handed the scalars formed by the SAME NumPy expressions the oracle uses, so nothing is rounded in between.
enlsip_gn_termination_sums, whose summation orders the kernels follow, is checked against mpmath inside the bound
2 k u sum|x_i||y_i| of tests/test_gpu_linesearch_setup_batched.py.  The file also shows, on the oracle alone, that the cases of
tests/termination_cases.py stay clear of their thresholds (the cap the GPU test relies on)."""
import ctypes as C
import math
import re
import types
from pathlib import Path

import numpy as np
import pytest

import termination_cases as tc
from oracle import enlsip_outer as eo

ROOT = Path(__file__).resolve().parents[1]
U = 2.0 ** -53
SQRT_EPS = math.sqrt(float(np.finfo(np.float64).eps))


@pytest.fixture(scope="module")
def T():
    import __graft_entry__ as ge
    ge.build()
    from enlsip_gn import termination
    return termination


def bits(x):
    return np.float64(x).view(np.uint64)


def oracle_minmax(lam, q, t, ds, scaling):
    W = types.SimpleNamespace(q=q, t=t)
    aC = types.SimpleNamespace(scaling=scaling, diag_scale=np.asarray(ds, dtype=np.float64))
    return eo.minmax_lagrangian_mult(np.asarray(lam, dtype=np.float64), W, aC)


def same_pair(got, want):
    return all(bits(g) == bits(w) or (math.isnan(g) and math.isnan(w)) for g, w in zip(got, want))


# ---- minmax_lagrangian_mult ---------------------------------------------------------------------------------------------------------
def test_minmax_random_cases_against_the_oracle(T):
    rng = np.random.default_rng(0)
    finite = 0
    for i in range(400):
        t = int(rng.integers(0, 12))
        q = int(rng.integers(0, t + 1))
        scaling = bool(i % 2)
        lam = rng.standard_normal(t) * 10.0 ** rng.integers(-9, 2, size=t)
        ds = rng.random(t) * 10.0 ** rng.integers(-2, 3, size=t) + 1e-3
        want = oracle_minmax(lam, q, t, ds, scaling)
        got = T.minmax_lagrangian_mult(lam, q, t, ds, scaling)
        assert same_pair(got, want), (i, got, want)
        finite += math.isfinite(want[0])
    assert 100 <= finite <= 350      # both outcomes of the product test are well populated


@pytest.mark.parametrize("scaling", (False, True))
def test_minmax_named_edges(T, scaling):
    one = np.ones(4)
    cases = {
        "t == q": ([-1.0, -2.0, -3.0], 3, 3, one),
        "t == 0": ([], 0, 0, []),
        "product exactly -sqrt(eps)": ([5.0, -SQRT_EPS, 7.0], 1, 3, one),
        "product just above -sqrt(eps)": ([5.0, np.nextafter(-SQRT_EPS, 0.0), 7.0], 1, 3, one),
        "equal minima": ([1.0, -2.0, -2.0, -1.0], 0, 4, one),
        "minimum among the equalities is not looked at": ([-9.0, -2.0, -3.0], 1, 3, one),
        "NaN multiplier": ([1.0, float("nan"), -3.0], 0, 3, one),
        "NaN among the equalities": ([float("nan"), -1.0, -3.0], 1, 3, one),
    }
    for name, (lam, q, t, ds) in cases.items():
        want = oracle_minmax(lam, q, t, ds[:t], scaling)
        got = T.minmax_lagrangian_mult(lam, q, t, ds[:t], scaling)
        assert same_pair(got, want), (name, got, want)
    assert T.minmax_lagrangian_mult([-1.0], 1, 1, [1.0], scaling) == (math.inf, 0.0)
    assert T.minmax_lagrangian_mult([5.0, -SQRT_EPS], 1, 2, [1.0, 1.0], scaling)[0] == -SQRT_EPS      # <= : the edge passes
    # the pinned NaN behaviour: lambda_abs_max is the quiet NaN, sigma_min ignores the NaN entry
    smin, lmax = T.minmax_lagrangian_mult([1.0, float("nan"), -3.0], 0, 3, [1.0, 1.0, 1.0], scaling)
    assert smin == -3.0 and bits(lmax) == 0x7FF8000000000000


# ---- check_termination_criteria -----------------------------------------------------------------------------------------------------
def lib_decision(T, c, scalars=None, tol=tc.TOL):
    s = tc.numpy_scalars(c) if scalars is None else scalars
    rec = np.zeros((), dtype=T.SUMS_DTYPE)
    for k, v in s.items():
        rec[k] = v
    st = c["state"]
    state = T.make_state(restart=st["restart"], code=st["code"], delete=st["delete"], grad_res=st["grad_res"], nb_iter=st["nb_iter"],
                         nb_newton_steps=st["nb_newton_steps"], error_code=st["error_code"], psi_error=st["psi_error"],
                         delta_time=st["delta_time"], q=c["q"], t=c["t"], l=c["l"], dimJ2=c["dimJ2"], psi0=st["psi0"])
    return T.check_termination_criteria(state, rec, T.make_tol(**tol))


def all_cases(seed=1, reps=6):
    rng = np.random.default_rng(seed)
    shapes = [(40, 5, 7), (70, 9, 12), (33, 3, 4), (65, 8, 8)]
    out = []
    for arm in tc.ARMS:
        for r in range(reps):
            m, n, l = shapes[r % len(shapes)]
            t = l if (r == 3 and arm not in ("inactive_nonpos", "sigma_small_t1")) else None      # l == t
            out.append(tc.make_case(rng, arm, m, n, l, t=t, scaling=bool(r % 2)))
    return out


def test_decision_against_the_oracle_on_every_arm(T):
    cases = all_cases()
    want = [tc.oracle_exit(c) for c in cases]
    got = [lib_decision(T, c) for c in cases]
    bad = [(c["arm"], g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, bad[:5]
    # coverage, on the oracle alone: every arm gives its code, so every reachable statement of the chain is walked
    off = [(c["arm"], w, tc.expected_code(c)) for c, w in zip(cases, want) if w != tc.expected_code(c)]
    assert not off, off[:5]
    assert set(want) >= {10000, 2000, 300, 40, 12000, 10300, 12340, -2, -3, -4, -5, -9, -6, -10, -11, 0}
    assert any(c["t"] == 1 and c["t"] > c["q"] for c in cases) and any(c["t"] > 1 and c["t"] > c["q"] for c in cases)
    assert any(c["l"] == c["t"] for c in cases) and any(c["t"] == 0 for c in cases)


def test_cases_stay_clear_of_their_thresholds():
    """On the oracle alone: at most 5 % of the random cases have a compared quantity within its rounding bound of its threshold
    (the cap of the GPU comparison against the oracle); by construction it is none."""
    cases = all_cases(seed=2)
    near = sum(tc.on_a_threshold(c) for c in cases)
    print(f"{near} of {len(cases)} cases on a threshold")
    assert near <= 0.05 * len(cases)


def test_decision_on_thresholds_and_the_feas_negation(T):
    """Cases that sit ON a threshold by construction, and the unreachable negation: the host routine alone, statement by statement."""
    rng = np.random.default_rng(3)
    c = tc.make_case(rng, "c4567", 40, 5, 7, t=3)
    s = tc.numpy_scalars(c)
    assert lib_decision(T, c, s) == 12340
    edge = dict(s, d1_sq=s["rx_sum"] * (tc.TOL["eps_rel"] * tc.TOL["eps_rel"]))            # <= holds on the edge
    assert lib_decision(T, c, edge) == 12340
    edge = dict(s, d1_sq=np.nextafter(s["rx_sum"] * (tc.TOL["eps_rel"] * tc.TOL["eps_rel"]), np.inf))
    assert lib_decision(T, c, edge) == 2340
    edge = dict(s, rx_sum=tc.TOL["eps_abs"] * tc.TOL["eps_abs"], d1_sq=0.0)                # <=
    assert lib_decision(T, c, edge) == 12340
    edge = dict(s, x_diff=tc.TOL["eps_x"] * s["x_nrm"])                                     # strict <
    assert lib_decision(T, c, edge) == 12040
    edge = dict(s, active_cx_nrm=tc.TOL["eps_c"])                                           # strict <: necessary fails
    assert lib_decision(T, c, edge) == 0
    eps = float(np.finfo(np.float64).eps)
    edge = dict(s, p_nrm=3.0 * eps)                                                         # alfnoi == 0.25: not > 0.25
    assert lib_decision(T, c, edge) == 12300
    # feas = -1: n_inactive_le0 > 0 while n_inactive_nonpos == 0 cannot come from data; the routine negates all the same
    assert lib_decision(T, c, dict(s, n_inactive_le0=1)) == -12340
    # a NaN among the inactive cx: not > 0, so the necessary condition fails; it is not <= 0
    assert lib_decision(T, c, dict(s, n_inactive_nonpos=1)) == 0
    # abnormal chain on its edges: x_diff == 10 eps_x, Atcx == 10 eps_c, penalty sum == 1.0 all pass (<=, <=, >=)
    c = tc.make_case(rng, "infeasible", 40, 5, 7, t=2)
    s = tc.numpy_scalars(c)
    edge = dict(s, x_diff=10.0 * tc.TOL["eps_x"], Atcx_nrm=10.0 * tc.TOL["eps_c"], active_penalty_sum=1.0)
    assert lib_decision(T, c, edge) == -10
    assert lib_decision(T, c, dict(edge, active_penalty_sum=np.nextafter(1.0, 0.0))) == 0
    c["state"]["delta_time"] = 0.0                                                          # strict >
    assert lib_decision(T, c, dict(edge, active_penalty_sum=0.5)) == 0


# ---- termination_sums against mpmath ------------------------------------------------------------------------------------------------
def mp_reference(c):
    import mpmath as mp
    mp.mp.prec = 400
    f = lambda v: [mp.mpf(float(x)) for x in v]
    dot = lambda a, b: mp.fsum(x * y for x, y in zip(a, b))
    t, l, n, m = c["t"], c["l"], c["n"], c["m"]
    act = [int(i) - 1 for i in c["active"][:t]]
    rx, x, xp, p = f(c["rx"]), f(c["x"]), f(c["x_prev"]), f(c["p"])
    grad = [dot(f(c["J"][:, j]), rx) for j in range(n)]
    cxa = f(c["cx_active"])
    atcx = [dot(f(c["At"][j, :t]), cxa) for j in range(n)]
    w, cx = f(c["w"]), f(c["cx_all"])
    d1 = f(c["d_gn"][: c["dimJ2"]])
    return dict(grad=grad, rx_sum=dot(rx, rx), grad_nrm=mp.sqrt(dot(grad, grad)), p_nrm=mp.sqrt(dot(p, p)),
                active_cx_nrm=mp.sqrt(dot(cxa, cxa)), d1_sq=dot(d1, d1), x_diff=mp.sqrt(mp.fsum((a - b) ** 2 for a, b in zip(xp, x))),
                x_nrm=mp.sqrt(dot(x, x)), Atcx_nrm=mp.sqrt(dot(atcx, atcx)), active_penalty_sum=mp.fsum(w[i] ** 2 for i in act),
                whsum=mp.fsum(w[i] * cx[i] ** 2 for i in act))


@pytest.mark.parametrize("shape", [(1, 1, 0, 0), (63, 5, 7, 3), (130, 64, 64, 64), (257, 65, 70, 9), (1025, 130, 200, 40)],
                         ids=lambda s: "m%d_n%d_l%d_t%d" % s)
def test_sums_against_mpmath(T, shape):
    m, n, l, t = shape
    rng = np.random.default_rng(m + n)
    c = tc.make_case(rng, "none", m, n, l, t=t, q=t // 2, scaling=True)
    c["lam"][: t // 3] *= -1.0
    c["cx_all"][::3] *= -1.0
    got, grad = T.termination_sums(J=c["J"], rx=c["rx"], cx_all=c["cx_all"], x=c["x"], x_prev=c["x_prev"], p=c["p"], d_gn=c["d_gn"],
                                   dimJ2=c["dimJ2"], lam=c["lam"], cx_active=c["cx_active"], diag_scale=c["diag_scale"], At=c["At"],
                                   w=c["w"], active=c["active"], inactive=c["inactive"], q=c["q"], t=t, scaling=True,
                                   psi0=c["state"]["psi0"])
    ref, bound, s = mp_reference(c), tc.rounding_bounds(c), tc.numpy_scalars(c)
    g_bound = 2.0 * m * U * (np.abs(c["J"]).T @ np.abs(c["rx"]))
    for j in range(n):
        assert abs(float(grad[j] - ref["grad"][j])) <= g_bound[j], ("grad", j)
    for name in ("rx_sum", "grad_nrm", "p_nrm", "active_cx_nrm", "d1_sq", "x_diff", "x_nrm", "Atcx_nrm", "active_penalty_sum", "whsum"):
        err = abs(float(got[name] - ref[name]))
        print(f"{name}: error {err:.3e}, bound {bound[name]:.3e}")
        assert err <= bound[name], name
    # exact: the counts, the multiplier pair, and progress from the fields as formed
    for name in ("n_inactive_nonpos", "n_inactive_le0"):
        assert got[name] == s[name], name
    assert same_pair((got["sigma_min"], got["lambda_abs_max"]), (s["sigma_min"], s["lambda_abs_max"]))
    assert got["progress"] == (2 * c["state"]["psi0"] - got["rx_sum"]) - got["whsum"]
    # given the gradient and rx_sum formed elsewhere, the routine takes them as they are
    got2, grad2 = T.termination_sums(J=c["J"], rx=c["rx"], cx_all=c["cx_all"], x=c["x"], x_prev=c["x_prev"], p=c["p"], d_gn=c["d_gn"],
                                     dimJ2=c["dimJ2"], lam=c["lam"], cx_active=c["cx_active"], diag_scale=c["diag_scale"],
                                     At=c["At"], w=c["w"], active=c["active"], inactive=c["inactive"], q=c["q"], t=t, scaling=True,
                                     psi0=c["state"]["psi0"], grad_in=2.0 * grad, rx_sum_in=7.0)
    assert got2["rx_sum"] == 7.0 and np.array_equal(grad2, 2.0 * grad) and got2["grad_nrm"] == 2.0 * got["grad_nrm"]
    assert got2["Atcx_nrm"] == got["Atcx_nrm"] and got2["progress"] == (2 * c["state"]["psi0"] - 7.0) - got["whsum"]


def test_sums_order_is_the_documented_one(T):
    """The strided partials and the butterfly, restated in NumPy: a sum depends on its length and operands alone."""
    def ordered(terms):
        x = np.zeros(64)
        for j, v in enumerate(terms):
            x[j & 63] = x[j & 63] + v
        for mk in (1, 2, 7, 15, 16, 32):
            y = x.copy()
            for s in range(64):
                y[s] = x[s] + x[s ^ mk] if s < (s ^ mk) else x[s ^ mk] + x[s]
            x = y
        return x[0]
    rng = np.random.default_rng(5)
    c = tc.make_case(rng, "none", 200, 130, 9, t=4, q=1)
    got, grad = T.termination_sums(J=c["J"], rx=c["rx"], cx_all=c["cx_all"], x=c["x"], x_prev=c["x_prev"], p=c["p"], d_gn=c["d_gn"],
                                   dimJ2=c["dimJ2"], lam=c["lam"], cx_active=c["cx_active"], diag_scale=c["diag_scale"], At=c["At"],
                                   w=c["w"], active=c["active"], inactive=c["inactive"], q=1, t=4, scaling=False)
    assert got["p_nrm"] == math.sqrt(ordered(c["p"] * c["p"]))
    assert got["x_diff"] == math.sqrt(ordered((c["x_prev"] - c["x"]) ** 2))
    assert got["rx_sum"] == ordered(c["rx"] * c["rx"])
    v = np.zeros(130)
    for col in range(4):
        v = v + c["At"][:, col] * c["cx_active"][col]
    assert got["Atcx_nrm"] == math.sqrt(ordered(v * v))
    assert got["grad_nrm"] == math.sqrt(ordered(grad * grad))


# ---- the prototypes -----------------------------------------------------------------------------------------------------------------
def test_prototypes_and_struct_mirrors():
    import enlsip_gn._lib as L
    hdr = (ROOT / "include" / "enlsip_gn.h").read_text()
    glue = (ROOT / "enlsip.jl_amd" / "julia" / "EnlsipHIP.jl").read_text()
    for name, nargs in (("enlsip_gn_minmax_lagrangian_mult", 7), ("enlsip_gn_check_termination_criteria", 4),
                        ("enlsip_gn_termination_sums", 28), ("enlsip_gn_termination_batched_dev", 31),
                        ("enlsip_gn_get_termination_form", 2)):
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S).group(1)
        assert len(args.split(",")) == nargs, name
        assert len(L.PROTOTYPES[name][1]) == nargs, name
    ctype = {"int64_t": C.c_int64, "double": C.c_double}
    jtype = {"int64_t": "Int64", "double": "Float64"}
    for cname, mirror, jname in (("enlsip_gn_term_state", L.TermState, "TermState"), ("enlsip_gn_term_tol", L.TermTol, "TermTol"),
                                 ("enlsip_gn_term_sums", L.TermSums, "TermSums")):
        body = re.search(r"typedef struct " + cname + r"\s*\{(.*?)\}\s*" + cname + r"\s*;", hdr, flags=re.S).group(1)
        lines = [ln for ln in body.splitlines() if ln.strip()]
        assert all(re.search(r"/\* :\d+", ln) for ln in lines), cname      # every field cites its line
        fields = re.findall(r"(\w+)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert [(f, ctype[t]) for t, f in fields] == list(mirror._fields_), cname
        jbody = re.search(r"^struct " + jname + r"\n(.*?)^end", glue, flags=re.S | re.M).group(1)
        assert re.findall(r"^\s*(\w+)::(\w+)", jbody, flags=re.M) == [(f, jtype[t]) for t, f in fields], jname
    assert L.load().enlsip_gn_version() >= 202


def test_argument_checks_and_scratch_layout_on_the_cpu(tmp_path):
    """check_termination and TerminationScratch (gn_batch_records.hpp) in a stand-alone host program, tests/termination_check.cpp:
    every numbered argument error of the batched call without a GPU."""
    import os
    import shutil
    import subprocess
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    clang = clang if os.path.exists(clang) else shutil.which("clang++") or shutil.which("g++")
    assert clang, "no C++ compiler"
    exe = tmp_path / "termination_check"
    subprocess.run([clang, "-std=c++17", "-O1", "-g", str(ROOT / "tests" / "termination_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and "FAILED" not in out.stdout and out.stdout.count("ok ") >= 30, out.stdout + out.stderr
