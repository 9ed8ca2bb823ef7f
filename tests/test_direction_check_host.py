"""The Gauss-Newton direction check on the CPU: enlsip_gn_check_gn_direction (the host routine of
enlsip.jl_amd/csrc/gn_direction_check.hpp that the batched call runs on the downloaded sums) against
oracle/enlsip_outer.py::check_gn_direction (src/enlsip_functions.jl:943-1030), exactly: method_code and the bytes of beta, on a
table (tests/direction_cases.py) that reaches all three codes and every named condition in both states.
enlsip_gn_direction_sums, whose summation order the kernels follow, is checked against exact rational arithmetic inside
2 k u sum|x_i||y_i|, its counts exactly.  The argument checks of the batched call and the host routines on buffers of exactly
their used size run in a stand-alone program, tests/direction_check.cpp, under the host sanitizers where no GPU is present."""
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

import direction_cases as dc

ROOT = Path(__file__).resolve().parents[1]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def D():
    import __graft_entry__ as ge
    ge.build()
    from enlsip_gn import direction
    return direction


def bits(x):
    return np.float64(x).view(np.uint64)


def lib_state(D, c, **over):
    f = dict(iter_number=c["iter_number"], restart=c["restart"], add=c["add"], delete=c["delete"], q=c["q"], t=c["t"], l=c["l"],
             rankA=c["rankA"], prev_code=c["prev_code"], prev_beta=c["prev_beta"], prev_progress=c["prev_progress"],
             prev_predicted_reduction=c["prev_predicted_reduction"], prev_alpha=c["prev_alpha"])
    f.update(over)
    return D.make_state(**f)


def lib_decision(D, c):
    ge, neg, lt = dc.counts(c)
    rec = np.zeros((), dtype=D.SUMS_DTYPE)
    for k in ("b1_sq", "d_sq", "d1_sq", "d1_asprev_sq", "active_c_sum"):
        rec[k] = c[k]
    rec["n_lm_ge"], rec["n_lm_neg"], rec["n_inactive_lt_delta"] = ge, neg, lt
    return D.check_gn_direction(lib_state(D, c), rec, c["m"], c["n"])


# ---- the decision ---------------------------------------------------------------------------------------------------------------------
def test_decision_against_the_oracle_on_the_whole_table(D):
    cases = dc.table()
    seen = {name: set() for name in dc.CONDITIONS}
    codes = set()
    worst = math.inf
    for i, c in enumerate(cases):
        want_code, want_beta = dc.oracle_decision(c)
        got_code, got_beta = lib_decision(D, c)
        assert got_code == want_code and bits(got_beta) == bits(want_beta), (i, got_code, want_code, got_beta, want_beta)
        r, code, margin = dc.reached(c)
        assert code == want_code, (i, "the restatement of the test module disagrees with the oracle", code, want_code)
        for name, state in r.items():
            seen[name].add(bool(state))
        codes.add(want_code)
        worst = min(worst, margin)
    print(f"{len(cases)} cases, smallest relative distance of a compared pair from equality: {worst:.3e}")
    assert codes == {1, -1, 2}
    assert all(s == {False, True} for s in seen.values()), {k: v for k, v in seen.items() if v != {False, True}}
    assert worst >= 1e-6
    assert any(c["m"] == c["n"] - c["t"] for c in cases) and any(c["l"] == c["q"] for c in cases)
    assert any(c["t"] == c["n"] == c["rankA"] for c in cases) and any(c["q"] == c["t"] and c["l"] == c["t"] for c in cases)


def test_decision_on_its_thresholds(D):
    """Cases that sit ON a threshold by construction: the host routine alone, statement by statement."""
    c = dc.make_case(prev_code=1, beta_ratio=2.0, progress=(0.01, 1.0))          # beta == c1 * prev_beta: strict <, so not lower
    assert lib_decision(D, c)[0] == -1
    c = dc.make_case(prev_code=1, beta_ratio=0.5, progress=(0.1 * 1.0, 1.0))     # progress == c2 * predicted: strict >
    assert lib_decision(D, c)[0] == -1
    c = dc.make_case(prev_code=1, beta_ratio=0.5, progress=(1.0, 1.0), b1_sq=0.0, d1_sq=1.0, d_factor=16.0)      # dnrm == c3 beta: <=
    assert lib_decision(D, c)[0] == 1
    base = dict(prev_code=-1, t=2, q=2, l=2, n=6, rankA=2)                       # nothing to reduce, cond4..cond6 false
    c = dc.make_case(**base, b1_sq=0.0, d1_sq=1.0, d_factor=100.0)               # dnrm == c4 beta: cond8 false
    assert lib_decision(D, c)[0] == -1
    c = dc.make_case(**base, b1_sq=0.0, d1_sq=1.0, d_factor=100.0)
    c["d_sq"] = math.nextafter(10.0, math.inf) ** 2
    assert math.sqrt(c["d_sq"]) > 10.0 and lib_decision(D, c)[0] == 2
    c = dc.make_case(**base, m=4)                                                # m == n - t: cond7
    assert lib_decision(D, c)[0] == 2
    assert lib_decision(D, dc.make_case(**base, m=4, active_c_sum=0.1))[0] == 2                            # cond4 is strict
    assert lib_decision(D, dc.make_case(**base, m=4, active_c_sum=math.nextafter(0.1, 1.0)))[0] == -1


# ---- the sums -------------------------------------------------------------------------------------------------------------------------
def exact_sums(st, a, m):
    fr = lambda v: [Fraction(float(x)) for x in v]
    sq = lambda v: sum(x * x for x in v)
    d = fr(a["d"])
    kp = max(st["prev_dimJ2"] + st["prev_t"] - st["t"] - 1, 0)
    act = [int(i) - 1 for i in a["active"][: st["t"]] if i]
    cx = fr(np.nan_to_num(a["cx_all"]))
    return dict(b1_sq=(sq(fr(a["b"][: st["dimA"]])), st["dimA"]), d_sq=(sq(d), m), d1_sq=(sq(d[: st["dimJ2"]]), st["dimJ2"]),
                d1_asprev_sq=(sq(d[:kp]), kp), active_c_sum=(sq([cx[i] for i in act]), st["t"]))


def check_sums(D, st, a, m, n, want_status=None):
    state = D.make_state(**st)
    got, status = D.direction_sums(state, m=m, n=n, **a)
    if want_status is not None:
        assert status == want_status
    if status == 1:
        return got, status
    for name, (ref, k) in exact_sums(st, a, m).items():
        err = abs(Fraction(float(got[name])) - ref)
        assert err <= Fraction(2 * k * U) * ref, (name, float(err), k)      # sum|x_i||x_i| is the sum itself
    c = dict(q=st["q"], t=st["t"], l=st["l"], lam=a["lam"], diag_scale=a["diag_scale"], cx_all=a["cx_all"], inactive=a["inactive"],
             scaling=a["scaling"])
    assert (got["n_lm_ge"], got["n_lm_neg"], got["n_inactive_lt_delta"]) == dc.counts(c)
    return got, status


@pytest.mark.parametrize("length", (1, 63, 64, 65, 130))
@pytest.mark.parametrize("which", ("m", "t", "l"))
def test_sums_against_exact_arithmetic_at_every_length(D, which, length):
    m, t, l = 7, 3, 5
    if which == "m":
        m = length
    elif which == "t":
        t, l = length, length + 2
    else:
        l, t = length, min(3, length)
    rng = np.random.default_rng(1000 * length + ord(which))
    for scaling in (False, True):
        st, a = dc.random_problem(rng, m, 6, l, t, t // 2, scaling=scaling)
        check_sums(D, st, a, m, 6)
        st, a = dc.random_problem(rng, m, 6, l, t, 0, dimA=t, dimJ2=m, k_prev=m, scaling=scaling)
        check_sums(D, st, a, m, 6)


def test_sums_at_the_named_edges(D):
    rng = np.random.default_rng(7)
    m, n, l, t = 40, 30, 9, 4
    for k_prev, status in ((-3, 0), (0, 0), (1, 0), (5, 0), (m, 2), (m + 1, 1)):
        st, a = dc.random_problem(rng, m, n, l, t, 1, dimJ2=5, k_prev=k_prev)
        got, _ = check_sums(D, st, a, m, n, want_status=status)
        if k_prev <= 0:
            assert bits(got["d1_asprev_sq"]) == bits(0.0)
        if k_prev == 5:
            assert bits(got["d1_asprev_sq"]) == bits(got["d1_sq"])
        if k_prev == m:
            assert bits(got["d1_asprev_sq"]) == bits(got["d_sq"])
    for dimA in (0, t):
        st, a = dc.random_problem(rng, m, n, l, t, 1, dimA=dimA)
        got, _ = check_sums(D, st, a, m, n)
        assert (got["b1_sq"] == 0.0) == (dimA == 0)
    st, a = dc.random_problem(rng, m, n, l, t, t)                       # t == q: no multiplier is looked at
    got, _ = check_sums(D, st, a, m, n)
    assert got["n_lm_ge"] == 0 and got["n_lm_neg"] == 0
    st, a = dc.random_problem(rng, m, n, t, t, 1)                       # l == t: no inactive constraint
    assert check_sums(D, st, a, m, n)[0]["n_inactive_lt_delta"] == 0
    st, a = dc.random_problem(rng, 0, n, l, t, 1, dimJ2=0, k_prev=-1)   # m == 0
    got, _ = check_sums(D, st, a, 0, n)
    assert got["d_sq"] == 0.0 and got["d1_sq"] == 0.0
    st, a = dc.random_problem(rng, m, n, l, t, 1)                       # a list entry 0 contributes nothing
    a["active"][1] = 0
    a["inactive"][0] = 0
    got, _ = check_sums(D, st, a, m, n)


def test_a_nan_passes_no_comparison(D):
    rng = np.random.default_rng(8)
    m, n, l, t, q = 10, 8, 9, 5, 1
    for scaling in (False, True):
        st, a = dc.random_problem(rng, m, n, l, t, q, scaling=scaling)
        a["lam"][:] = -1.0
        a["diag_scale"][:] = 1.0
        a["cx_all"][:] = 0.01
        base, _ = check_sums(D, st, a, m, n)
        assert (base["n_lm_ge"], base["n_lm_neg"], base["n_inactive_lt_delta"]) == (0, t - q, l - t)
        a["lam"][2] = math.nan
        got, _ = check_sums(D, st, a, m, n)
        assert (got["n_lm_ge"], got["n_lm_neg"]) == (0, t - q - 1)
        a["lam"][:] = 1.0
        a["diag_scale"][3] = math.nan
        got, _ = check_sums(D, st, a, m, n)
        assert (got["n_lm_ge"], got["n_lm_neg"]) == (t - q - 1, 0)
        a["cx_all"][int(a["inactive"][0]) - 1] = math.nan
        got, _ = check_sums(D, st, a, m, n)
        assert got["n_inactive_lt_delta"] == l - t - 1


def test_sums_order_is_the_documented_one(D):
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
    st, a = dc.random_problem(rng, 200, 150, 140, 130, 3, dimA=100, dimJ2=77, k_prev=70)
    got, _ = D.direction_sums(D.make_state(**st), m=200, n=150, **a)
    d = a["d"]
    assert got["d_sq"] == ordered(d * d) and got["d1_sq"] == ordered(d[:77] * d[:77]) and got["d1_asprev_sq"] == ordered(d[:70] * d[:70])
    assert got["b1_sq"] == ordered(a["b"][:100] ** 2)
    assert got["active_c_sum"] == ordered(a["cx_all"][a["active"][:130] - 1] ** 2)


def test_sums_argument_errors(D):
    import enlsip_gn._lib as L
    lib = L.load()
    st = D.make_state(t=2, q=1, l=3, dimA=2, dimJ2=2)
    out, status = L.DirSums(), C.c_int64(0)
    arr = np.ones(4)
    idx = np.array([1, 2, 3], dtype=np.int64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    call = lambda s, m=4, n=3, l=3, act=idx, d=arr: lib.enlsip_gn_direction_sums(
        m, n, l, C.byref(s), p(act), p(idx), p(arr), None if d is None else p(d), p(arr), p(arr), p(arr), 0, C.byref(out), C.byref(status))
    assert call(st) == 0
    assert call(st, l=4) == -2 and call(st, n=0) == -2 and call(D.make_state(t=2, q=1, l=3, dimA=3)) == -2
    assert call(D.make_state(t=2, q=1, l=3, dimJ2=5)) == -2 and call(D.make_state(t=2, q=3, l=3)) == -2
    assert call(st, d=None) == -4
    assert call(st, act=np.array([1, 4, 0], dtype=np.int64)) == -5


# ---- the prototypes -------------------------------------------------------------------------------------------------------------------
def test_prototypes_struct_mirrors_and_ccalls():
    import enlsip_gn._lib as L
    hdr = (ROOT / "include" / "enlsip_gn.h").read_text()
    glue = (ROOT / "enlsip.jl_amd" / "julia" / "EnlsipHIP.jl").read_text()
    jarg = {"int64_t": "Int64", "double": "Float64", "int": "Cint", "enlsip_gn_handle": "Ptr{Cvoid}", "int64_t*": "Ptr{Int64}",
            "double*": "Ptr{Float64}", "int*": "Ptr{Cint}", "enlsip_gn_dir_state*": "Ptr{DirState}", "enlsip_gn_dir_sums*": "Ptr{DirSums}"}
    for name, nargs in (("enlsip_gn_check_gn_direction", 6), ("enlsip_gn_direction_sums", 14),
                        ("enlsip_gn_direction_check_batched_dev", 20), ("enlsip_gn_get_direction_form", 2)):
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S).group(1)
        ctypes_ = [re.sub(r"\s*\w+$", "", re.sub(r"\bconst\b", "", a).strip()).replace(" ", "") for a in args.split(",")]
        assert len(ctypes_) == nargs and len(L.PROTOTYPES[name][1]) == nargs, name
        # the glue's @ccall of the entry point: one argument per parameter, of the matching Julia type
        call = re.search(r"@ccall LIB\." + name + r"\((.*?)\)::Cint", glue, flags=re.S)
        assert call, f"{name}: no @ccall in EnlsipHIP.jl"
        jtypes = re.findall(r"::((?:Ptr\{\w+\})|\w+)\s*(?:,|$)", call.group(1).strip())
        assert jtypes == [jarg[t] for t in ctypes_], (name, jtypes, ctypes_)
    ctype = {"int64_t": C.c_int64, "double": C.c_double}
    jtype = {"int64_t": "Int64", "double": "Float64"}
    for cname, mirror, jname in (("enlsip_gn_dir_state", L.DirState, "DirState"), ("enlsip_gn_dir_sums", L.DirSums, "DirSums")):
        body = re.search(r"typedef struct " + cname + r"\s*\{(.*?)\}\s*" + cname + r"\s*;", hdr, flags=re.S).group(1)
        lines = [ln for ln in body.splitlines() if ln.strip()]
        assert all(re.search(r"/\* :\d+", ln) for ln in lines), cname      # every field cites its line
        fields = re.findall(r"(\w+)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert [(f, ctype[t]) for t, f in fields] == list(mirror._fields_), cname
        jbody = re.search(r"^struct " + jname + r"\n(.*?)^end", glue, flags=re.S | re.M).group(1)
        assert re.findall(r"^\s*(\w+)::(\w+)", jbody, flags=re.M) == [(f, jtype[t]) for t, f in fields], jname
    for fn in ("check_gn_direction_hip", "direction_sums_hip", "direction_check_batched_dev_hip", "direction_form_hip"):
        assert re.search(r"^function " + fn + r"\(", glue, flags=re.M), fn
    assert L.load().enlsip_gn_version() >= 203
    assert "oracle" not in (ROOT / "enlsip.jl_amd" / "python" / "enlsip_gn" / "direction.py").read_text()


def test_argument_checks_and_host_routines_in_a_stand_alone_program(tmp_path):
    """tests/direction_check.cpp: every numbered argument error of the batched call, the scratch layout and the host routines on
    buffers of exactly their used size, with -fsanitize=address,undefined where no GPU is present (the sanitizers run on
    CPU-only machines).  Nothing is loaded into Python."""
    import torch
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    clang = clang if os.path.exists(clang) else shutil.which("clang++") or shutil.which("g++")
    assert clang, "no C++ compiler"
    exe = tmp_path / "direction_check"
    san = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([clang, "-std=c++17", "-O1", "-g", *san, str(ROOT / "tests" / "direction_check.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    print(out.stdout)
    assert "AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    assert out.returncode == 0 and "FAILED" not in out.stdout and out.stdout.count("ok ") >= 35, out.stdout + out.stderr


def test_the_end_to_end_batch_forces_its_outcomes_away_from_every_threshold():
    """On the oracle alone, before the GPU is consulted (tests/test_gpu_direction_check_batched.py runs the same batch there): the
    seven problems give the outcomes they are named after, and no comparison of check_gn_direction is decided within a relative
    1e-6 of its threshold."""
    want = {"code 1": (1, 0), "code -1, smaller dimensions": (-1, 0), "code -1 back to 1": (1, 0), "code 2 with hessians": (2, 0),
            "code 2 without hessians": (2, -4)}
    for P in dc.e2e_problems():
        assert dc.e2e_margin(P) >= 1e-6, P["kind"]
        if P["kind"] not in want:
            continue
        err, cur = dc.e2e_oracle(P)
        assert (cur.code, err) == want[P["kind"]], (P["kind"], cur.code, err)
        ranks = (cur.rankA, cur.rankJ2)
        if "smaller" in P["kind"]:
            assert (cur.dimA, cur.dimJ2) == (ranks[0] - 1, ranks[1] - 1)
        elif P["kind"] == "code 2 with hessians":
            assert (cur.dimA, cur.dimJ2, cur.nb_newton_steps) == (-P["t"], P["t"] - 6, 1)
        else:
            assert (cur.dimA, cur.dimJ2) == ranks and cur.nb_newton_steps == 0
