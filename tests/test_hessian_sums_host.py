"""The finite-difference Hessian sums of the Newton branch on the CPU: enlsip_gn_hessian_points and enlsip_gn_hessian_sums (the
host routines of enlsip.jl_amd/csrc/gn_hessian_sums.hpp whose bytes the kernels give) against oracle/enlsip_outer.py::hessian_res
and hessian_cons (src/enlsip_functions.jl:243-328).  The points are the reference's bit for bit.  The sums are byte-identical to a
restatement of the documented order (tests/hessian_cases.py), lie within (ceil(k / 64) + 6) u sum|terms| of the exact sum of the
same rounded terms, and agree with the reference's left-to-right sums on the same recorded evaluations within the bound between
two summation orders, entry by entry.  The argument checks of the batched calls, the pair decode and the host routines on buffers
of exactly their used size run in a stand-alone program, tests/hessian_sums_check.cpp, under the host sanitizers where no GPU is
present."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import hessian_cases as hc

ROOT = Path(__file__).resolve().parents[1]
U = hc.U


@pytest.fixture(scope="module")
def D():
    import __graft_entry__ as ge
    ge.build()
    from enlsip_gn import direction
    return direction


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- the points -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 5))
def test_points_are_the_reference_s_bit_for_bit(D, n):
    seen = set()
    for shift in range(len(hc.X_SPECIAL)):
        x = hc.special_x(n, shift)
        seen.update(float(v).hex() for v in x)
        want = hc.reference_points(x)
        got = D.hessian_points(x)
        assert got.shape == want.shape == (n * (n + 1) // 2, 4, n)
        assert same_bytes(got, want), (n, shift)
    assert seen == {float(v).hex() for v in hc.X_SPECIAL}      # -0.0 and 0.0 both


def test_points_of_a_range_that_starts_and_ends_inside_a_row(D):
    x = hc.special_x(5, 3)
    want = hc.reference_points(x)
    for pair0, npairs in ((7, 2), (4, 5), (11, 3), (0, 1), (14, 1), (8, 1)):      # row k = 3 is pairs 6..9, row 4 pairs 10..14
        assert same_bytes(D.hessian_points(x, pair0, npairs), want[pair0: pair0 + npairs]), (pair0, npairs)


def test_the_diagonal_keeps_its_two_roundings(D):
    x = hc.X_ROUNDTRIP
    e = hc.step(x)
    assert hc.find_roundtrip() == x and (x - e) + e != x                  # the kept value is what the search finds
    got = D.hessian_points(np.array([x]))[0, :, 0]
    assert same_bytes(got, np.array([(x + e) + e, (x - e) + e, (x + e) - e, (x - e) - e]))
    assert got[1] != x
    big = 2.0 ** 60                                                       # the step is relative: eps = 2^60 eps1, far above ulp(x) = 256
    eb = hc.step(big)
    assert eb == big * hc.EPS1 and big + eb != big
    assert same_bytes(D.hessian_points(np.array([big]))[0, :, 0], np.array([(big + eb) + eb, (big - eb) + eb, (big + eb) - eb, (big - eb) - eb]))


def test_eps1_is_the_reference_s(D):
    """eps_k = max(|0.0|, 1.0) * eps1 = eps1, and 0.0 + eps1 = eps1: point f1 of the pair (1, 0) of x = 0 IS eps1"""
    got = D.hessian_points(np.zeros(2), 1, 1)[0]
    assert same_bytes(got[0], np.array([hc.EPS1, hc.EPS1])) and same_bytes(got[3], np.array([-hc.EPS1, -hc.EPS1]))
    assert hc.EPS1 == float(np.finfo(np.float64).eps) ** (1.0 / 3.0)


# ---- the sums -------------------------------------------------------------------------------------------------------------------------
SUM_SHAPES = [(m, l, t) for m in (0, 1, 63, 64, 65, 129) for l in (0, 1, 65) for t in sorted({0, min(1, l), l})]


@pytest.mark.parametrize("m,l,t", SUM_SHAPES)
def test_sums_bytes_bounds_and_the_reference(D, m, l, t):
    n = 3
    rng = np.random.default_rng(7000 + 100 * m + 3 * l + t)
    # bytes and the derived bound, with a padding 0 inside a shuffled active list
    P = hc.random_problem(rng, m, n, l, t)
    got = D.hessian_sums(P["x"], P["F"], P["rx"], P["G"], P["lam"], P["active"], t)
    rest = hc.restated(P["x"], P["F"], P["rx"], P["G"], P["lam"], P["active"], t)
    assert same_bytes(got, hc.restated_gamma(P["x"], P["F"], P["rx"], P["G"], P["lam"], P["active"], t))
    assert same_bytes(got, got.T)
    worst = 0.0
    for e in rest:
        for name, tm, cnt in (("s_r", e["u"], m), ("s_c", e["v"], t)):
            bound = Fraction((math.ceil(cnt / 64) + 6) * U) * hc.exact(np.abs(tm))
            err = abs(Fraction(e[name]) - hc.exact(tm))
            assert err <= bound, (name, e["k"], e["j"], float(err), float(bound))
            worst = max(worst, float(err / bound)) if bound else worst
    print(f"m={m} l={l} t={t}: largest error / bound of a sum {worst:.3f}")
    # the reference on the same recorded evaluations (it has no padding entries: a 0 would index its last constraint)
    P = hc.random_problem(rng, m, n, l, t, pad=False)
    got = D.hessian_sums(P["x"], P["F"], P["rx"], P["G"], P["lam"], P["active"], t)
    want = hc.reference_gamma(P["x"], P["F"], P["rx"], P["G"], P["lam"], P["active"], t)
    worst = 0.0
    for e in hc.restated(P["x"], P["F"], P["rx"], P["G"], P["lam"], P["active"], t):
        k, j = e["k"], e["j"]
        tol = hc.entry_bound(e, m, t)
        for a, b in ((k, j), (j, k)):
            diff = abs(got[a, b] - want[a, b])
            assert diff <= tol, (a, b, got[a, b], want[a, b], diff, tol)
            worst = max(worst, diff / tol) if tol else worst
    print(f"m={m} l={l} t={t}: largest difference / tolerance against the reference {worst:.3f}")


def test_a_pair_range_writes_its_own_entries_only(D):
    rng = np.random.default_rng(11)
    n, m, l, t = 5, 70, 4, 3
    P = hc.random_problem(rng, m, n, l, t)
    whole = D.hessian_sums(P["x"], P["F"], P["rx"], P["G"], P["lam"], P["active"], t)
    for pair0, npairs in ((0, 1), (14, 1), (7, 2), (4, 5), (0, 15)):
        G0 = np.full((n, n), -7.25e33)
        got = D.hessian_sums(P["x"], P["F"][pair0: pair0 + npairs], P["rx"], P["G"][pair0: pair0 + npairs], P["lam"], P["active"], t,
                             pair0=pair0, Gamma=G0.copy())
        want = G0.copy()
        for k, j in hc.pairs(n)[pair0: pair0 + npairs]:
            want[k, j] = want[j, k] = whole[k, j]
        assert same_bytes(got, want), (pair0, npairs)


def test_the_two_divisor_forms_coincide_in_double_precision(D):
    """(4 eps_j) eps_k and (4.0 eps_k) eps_j: the factor 4 is exact (eps >= eps1, and 4 eps <= 4 * 1.8e308 * 6.1e-6 is finite) and
    a power of two commutes with rounding, so both are fl(4 eps_j eps_k); where that product overflows both are +Inf, and no
    step is small enough for an underflow.  The search finds no x that separates them; DESIGN.md 5.15 says so, and both forms
    stay in the code as the reference writes them."""
    rng = np.random.default_rng(3)
    xs = np.concatenate([hc.X_SPECIAL, rng.standard_normal(20000) * 10.0 ** rng.integers(-300, 300, size=20000),
                         [np.finfo(np.float64).max, np.finfo(np.float64).tiny, 5e-324]])
    e = np.maximum(np.abs(xs), 1.0) * hc.EPS1
    ej, ek = e[:, None], e[None, ::37]
    with np.errstate(over="ignore"):
        assert np.isfinite(4 * e).all() and np.array_equal((4 * ej) * ek, (4.0 * ek) * ej)
    # and the routine's bytes are those of the restatement, which writes each divisor in its own association
    P = hc.random_problem(rng, 40, 4, 5, 3, x=[3.7e5, -0.2, 1.0 + 2.0 ** -30, -8.1e-3])
    got = D.hessian_sums(P["x"], P["F"], P["rx"], P["G"], P["lam"], P["active"], 3)
    assert same_bytes(got, hc.restated_gamma(P["x"], P["F"], P["rx"], P["G"], P["lam"], P["active"], 3))


def test_a_nan_or_inf_reaches_its_own_pair_only(D):
    rng = np.random.default_rng(12)
    n, m, l, t = 4, 66, 3, 2
    P = hc.random_problem(rng, m, n, l, t, pad=False)
    clean = D.hessian_sums(P["x"], P["F"], P["rx"], P["G"], P["lam"], P["active"], t)
    for bad in (math.nan, math.inf):
        for where in ("F", "G"):
            q = 4                                                         # pair (2, 1)
            Q = dict(P, F=P["F"].copy(), G=P["G"].copy())
            if where == "F":
                Q["F"][q, 2, 65] = bad
            else:
                Q["G"][q, 1, int(P["active"][1]) - 1] = bad
            got = D.hessian_sums(Q["x"], Q["F"], Q["rx"], Q["G"], Q["lam"], Q["active"], t)
            k, j = hc.pairs(n)[q]
            assert not np.isfinite(got[k, j]) and not np.isfinite(got[j, k])
            mask = np.ones((n, n), dtype=bool)
            mask[k, j] = mask[j, k] = False
            assert same_bytes(got[mask], clean[mask])


# ---- the arguments --------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_host_routines(D):
    import enlsip_gn._lib as L
    lib = L.load()
    n, m, l, t = 3, 4, 2, 2
    x, rx, lam = np.ones(n), np.ones(m), np.ones(t)
    X = np.zeros((6, 4, n))
    F, G, Gam = np.zeros((6, 4, m)), np.zeros((6, 4, l)), np.zeros((n, n))
    act = np.array([2, 1], dtype=np.int64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    pts = lambda n_=n, pair0=0, npairs=6, x_=x, X_=X: lib.enlsip_gn_hessian_points(n_, pair0, npairs, p(x_), p(X_))
    assert pts() == 0
    assert pts(n_=0) == -2 and pts(npairs=0) == -2 and pts(pair0=-1) == -2 and pts(pair0=1) == -2 and pts(pair0=6, npairs=1) == -2
    assert pts(pair0=5, npairs=1) == 0
    assert pts(x_=None) == -4 and pts(X_=None) == -4

    def sums(m_=m, n_=n, l_=l, t_=t, pair0=0, npairs=6, act_=act, x_=x, F_=F, rx_=rx, G_=G, lam_=lam, Gam_=Gam, ldg=n):
        return lib.enlsip_gn_hessian_sums(m_, n_, l_, t_, pair0, npairs, p(act_), p(x_), p(F_), p(rx_), p(G_), p(lam_), p(Gam_), ldg)
    assert sums() == 0
    assert sums(m_=-1) == -2 and sums(n_=0) == -2 and sums(l_=-1) == -2
    assert sums(npairs=0) == -2 and sums(pair0=-1) == -2 and sums(pair0=1) == -2 and sums(pair0=6, npairs=1) == -2
    assert sums(x_=None) == -4 and sums(Gam_=None) == -4 and sums(F_=None) == -4 and sums(rx_=None) == -4
    assert sums(act_=None) == -4 and sums(G_=None) == -4 and sums(lam_=None) == -4
    assert sums(m_=0, F_=None, rx_=None) == 0                             # nothing of F or rx is read when m == 0
    assert sums(t_=0, act_=None, G_=None, lam_=None) == 0                 # nor of the constraint side when t == 0
    assert sums(l_=0, t_=0, act_=None, G_=None, lam_=None) == 0
    assert sums(t_=3) == -5 and sums(t_=-1) == -5 and sums(ldg=n - 1) == -5
    assert sums(act_=np.array([3, 1], dtype=np.int64)) == -5 and sums(act_=np.array([1, -1], dtype=np.int64)) == -5
    assert sums(act_=np.array([0, 1], dtype=np.int64)) == 0
    with pytest.raises(D.GNError):
        D.hessian_points(np.ones(2), 2, 2)


# ---- the prototypes -------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_ccalls():
    import enlsip_gn._lib as L
    hdr = (ROOT / "include" / "enlsip_gn.h").read_text()
    glue = (ROOT / "enlsip.jl_amd" / "julia" / "EnlsipHIP.jl").read_text()
    jarg = {"int64_t": "Int64", "double": "Float64", "int": "Cint", "enlsip_gn_handle": "Ptr{Cvoid}", "int64_t*": "Ptr{Int64}",
            "double*": "Ptr{Float64}"}
    carg = {"int64_t": C.c_int64, "enlsip_gn_handle": C.c_void_p, "int64_t*": C.c_void_p, "double*": C.c_void_p}
    for name, nargs in (("enlsip_gn_hessian_points", 5), ("enlsip_gn_hessian_points_batched_dev", 7), ("enlsip_gn_hessian_sums", 14),
                        ("enlsip_gn_hessian_sums_batched_dev", 19)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert decl, name
        ctypes_ = [re.sub(r"\s*\w+$", "", re.sub(r"\bconst\b", "", a).strip()).replace(" ", "") for a in decl.group(1).split(",")]
        assert len(ctypes_) == nargs, name
        assert L.PROTOTYPES[name] == (C.c_int, [carg[t] for t in ctypes_]), name
        call = re.search(r"@ccall LIB\." + name + r"\((.*?)\)::Cint", glue, flags=re.S)
        assert call, f"{name}: no @ccall in EnlsipHIP.jl"
        jtypes = re.findall(r"::((?:Ptr\{\w+\})|\w+)\s*(?:,|$)", call.group(1).strip())
        assert jtypes == [jarg[t] for t in ctypes_], (name, jtypes, ctypes_)
    section = hdr[hdr.index("the finite-difference Hessian sums of the Newton branch"):hdr.index("int enlsip_gn_hessian_points(")]
    for cite in ("src/enlsip_functions.jl:243-328", ":259-265", ":268-271", ":272", ":317-321", ":322", ":393"):
        assert cite in section, cite
    for fn in ("hessian_points_hip", "hessian_points_batched_dev_hip", "hessian_sums_hip!", "hessian_sums_batched_dev_hip"):
        assert re.search(r"^function " + re.escape(fn) + r"\(", glue, flags=re.M), fn
    assert L.load().enlsip_gn_version() >= 204


def test_the_analysis_refuses_both_hessian_sources(D):
    with pytest.raises(ValueError):
        D.search_direction_analys_batched_dev(None, [], [], [], {}, m=1, n=1, t_max=0, iter_number=0, scaling=False, rx_sum=0.0,
                                              hessians=lambda k: None, hessian_evals=(None, None))


def test_argument_checks_decode_and_host_routines_in_a_stand_alone_program(tmp_path):
    """tests/hessian_sums_check.cpp: every argument error of the two batched calls, pair ranges at both ends of the index, the
    pair decode for every pair of n = 1..64 and the last pairs of n = 46341, and the host routines on buffers of exactly their
    used size, with -fsanitize=address,undefined where no GPU is present (the sanitizers run on CPU-only machines).  Nothing is
    loaded into Python."""
    import torch
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    clang = clang if os.path.exists(clang) else shutil.which("clang++") or shutil.which("g++")
    assert clang, "no C++ compiler"
    exe = tmp_path / "hessian_sums_check"
    san = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([clang, "-std=c++17", "-O1", "-g", *san, str(ROOT / "tests" / "hessian_sums_check.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    print(out.stdout)
    assert "AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    assert out.returncode == 0 and "FAILED" not in out.stdout and out.stdout.count("ok ") >= 40, out.stdout + out.stderr
