"""Cases of the line search's polynomial fit shared by tests/test_linesearch_fit_host.py and tests/test_gpu_linesearch_fit_batched.py:
coefficients_linesearch! / minrm / the choice of :2023-2026 (src/enlsip_functions.jl:1665-1689, :1841-1862) through
oracle/enlsip_outer.py, a record of what the oracle did inside (the arm of parameters_rm, the clamps of bounds, alpha_old == beta_hat,
the outcome of the choice), the perturbation envelope of its outputs, the one-variable problems of the driver test and a
reference driver run.

Sizes: m <= 16, l <= 12."""
import contextlib
from types import SimpleNamespace

import mpmath as mp
import numpy as np

from oracle import enlsip_outer as eo

U = np.finfo(np.float64).eps / 2
ULP = 2.0 ** -52
N_PERTURBED = 16        # oracle runs per case with rx_new moved by at most one ulp
MARGIN = 10.0           # the margin the project gives a 1-ulp envelope (alpha_tolerance of tests/test_reference_problems.py)
OUT = ("alpha_kp1", "pk", "alpha_hat", "s_alpha", "beta_hat", "s_beta")


def exact_dot(x, y):
    """(the exactly rounded dot product, sum |x||y|)"""
    with mp.workdps(100):
        xs, ys = [mp.mpf(float(v)) for v in x], [mp.mpf(float(v)) for v in y]
        return float(mp.fdot(xs, ys)), float(mp.fsum(abs(a * b) for a, b in zip(xs, ys)))


def same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the oracle, with a record of what it did ---------------------------------------------------------------------------------------
@contextlib.contextmanager
def traced_oracle(rec):
    """oracle.enlsip_outer with newton_raphson, one_root, two_roots and parameters_rm wrapped so that the arm taken and the
    unclamped roots are recorded in `rec`; the functions themselves run unchanged."""
    nr, one, two, prm = eo.newton_raphson, eo.one_root, eo.two_roots, eo.parameters_rm

    def nr_w(*a):
        rec["arm"] = 0
        return nr(*a)

    def one_w(*a):
        rec["arm"] = 1
        return one(*a)

    def two_w(*a):
        rec["arm"] = 2
        return two(*a)

    def prm_w(*a):
        ah, bh = prm(*a)
        rec["raw"] = (float(ah), float(bh))
        return ah, bh

    eo.newton_raphson, eo.one_root, eo.two_roots, eo.parameters_rm = nr_w, one_w, two_w, prm_w
    try:
        yield
    finally:
        eo.newton_raphson, eo.one_root, eo.two_roots, eo.parameters_rm = nr, one, two, prm


def lists(c):
    return c["active"][:c["t"]], c["inactive"][:c["l"] - c["t"]]


def oracle_vectors(c, rx_new=None):
    """v0, v1, v2 as linesearch_constrained builds them (oracle/enlsip_outer.py:791-805) at the trial point of the case"""
    m, l, t = c["m"], c["l"], c["t"]
    act, inact = lists(c)
    w, cx = c["w"], c["cx"]
    v1 = np.concatenate([c["Jp"], c["Ap"]]).astype(np.float64)
    for k in act - 1:                                                            # :1986-1998
        v1[m + k] = np.sqrt(w[k]) * v1[m + k]
    for k in inact - 1:
        v1[m + k] = 0.0 if cx[k] > 0 else np.sqrt(w[k]) * v1[m + k]
    v0, v2 = np.zeros(m + l), np.zeros(m + l)
    with np.errstate(all="ignore"):
        eo.coefficients_linesearch(v0, v1, v2, c["alpha_k"], c["rx"], cx, c["rx_new"] if rx_new is None else rx_new, c["cx_new"], w,
                                   m, t, l, c["active"], c["inactive"])
    return v0, v1, v2


def oracle_run(c, rx_new=None):
    """The oracle on a case (rx_new: a perturbed copy).  Returns dict(out (6,), arm, pattern, vectors)."""
    v0, v1, v2 = oracle_vectors(c, rx_new)
    rec = {}
    with traced_oracle(rec), np.errstate(all="ignore"):
        a_hat, sa, b_hat, sb = eo.minrm(v0, v1, v2, c["x_min"], c["a_min"], c["a_max"])
    a_kp1, pk = a_hat, sa
    choice = bool(a_kp1 != b_hat and sb < pk and b_hat <= c["alpha_k"])          # :2023-2026
    if choice:
        a_kp1, pk = b_hat, sb
    clamp = lambda raw: "hi" if raw > c["a_max"] else ("lo" if min(raw, c["a_max"]) < c["a_min"] else None)
    raw_a, raw_b = rec["raw"]
    pattern = (rec["arm"], clamp(raw_a), clamp(raw_b), raw_a == raw_b, choice)
    return dict(out=np.array([a_kp1, pk, a_hat, sa, b_hat, sb], dtype=np.float64), arm=rec["arm"], pattern=pattern, vectors=(v0, v1, v2))


def exact_sums(vectors):
    v0, v1, v2 = vectors
    return np.array([exact_dot(a, b)[0] for a, b in ((v0, v0), (v0, v1), (v0, v2), (v1, v1), (v1, v2), (v2, v2))])


def envelope(c, ref, seed):
    """N_PERTURBED oracle runs with every entry of rx_new moved by at most one ulp (seeded).  Returns (env (6,), stable)."""
    rng = np.random.default_rng(seed)
    env = np.zeros(6)
    stable = True
    for _ in range(N_PERTURBED):
        got = oracle_run(c, c["rx_new"] * (1.0 + ULP * rng.integers(-1, 2, size=c["rx_new"].shape)))
        stable = stable and got["pattern"] == ref["pattern"]
        with np.errstate(all="ignore"):
            d = np.abs(got["out"] - ref["out"])
        env = np.maximum(env, np.where(np.isnan(d), 0.0, d))
    return env, stable


def tolerance(ref, env):
    return MARGIN * np.asarray(env) + 4.0 * np.spacing(np.abs(np.asarray(ref, dtype=np.float64)))


# ---- the elements in NumPy, in the library's order ----------------------------------------------------------------------------------
def library_order_elements(c):
    """v0, v1, v2 formed with the same IEEE operations, in the order the library adds them: the m residuals, the active list, the
    inactive list"""
    act, inact = lists(c)
    w, cx, cxn, Ap, al = c["w"], c["cx"], c["cx_new"], c["Ap"], c["alpha_k"]
    with np.errstate(all="ignore"):
        sa, si = np.sqrt(w[act - 1]), np.sqrt(w[inact - 1])
        out_old, out_new = cx[inact - 1] > 0, cxn[inact - 1] > 0
        v0 = np.concatenate([c["rx"], sa * cx[act - 1], np.where(out_old, 0.0, si * cx[inact - 1])])
        v1 = np.concatenate([c["Jp"], sa * Ap[act - 1], np.where(out_old, 0.0, si * Ap[inact - 1])])
        vb = np.concatenate([c["rx_new"], sa * cxn[act - 1], np.where(out_new, 0.0, si * cxn[inact - 1])])
        v2 = ((vb - v0) / al - v1) / al
    return v0, v1, v2


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def random_case(rng, kind, m=None, l=None, t=None):
    """One case: a trial point of a smooth problem, rx_new = rx + alpha Jp + alpha^2 q with the size of q (the curvature) set by
    kind: 0 nearly linear (the Newton arm), 1-2 moderate, 3-5 strong curvature (the analytic arms, two minima among them)."""
    m = int(rng.integers(1, 17)) if m is None else m
    l = int(rng.integers(0, 13)) if l is None else l
    t = int(rng.integers(0, l + 1)) if t is None else t
    perm = rng.permutation(l) + 1
    active, inactive = np.zeros(l, dtype=np.int64), np.zeros(l, dtype=np.int64)
    active[:t] = perm[:t] if rng.integers(3) else np.sort(perm[:t])
    inactive[:l - t] = perm[t:] if rng.integers(3) else np.sort(perm[t:])
    curv = (1e-3, 0.3, 1.0, 4.0, 12.0, 40.0)[kind % 6]
    alpha_k = float(10.0 ** rng.uniform(-1.0, 0.0))
    rx, Jp = rng.standard_normal(m), rng.standard_normal(m)
    cx, Ap = rng.standard_normal(l), rng.standard_normal(l)
    rx_new = rx + alpha_k * Jp + alpha_k ** 2 * curv * rng.standard_normal(m)
    cx_new = cx + alpha_k * Ap + alpha_k ** 2 * curv * rng.standard_normal(l)
    w = 10.0 ** rng.uniform(-1, 1, l)
    a_max = float(10.0 ** rng.uniform(-0.5, 0.5))
    x_min = alpha_k if rng.integers(4) else 0.0
    return dict(m=m, l=l, t=t, active=active, inactive=inactive, rx=rx, rx_new=rx_new, Jp=Jp, cx=cx, cx_new=cx_new, Ap=Ap, w=w,
                alpha_k=min(alpha_k, a_max), x_min=min(x_min, a_max), a_min=a_max / 3000.0, a_max=a_max)


def found(name, want, seed, **size):
    """The first case of a seeded search that the ORACLE's record puts where `want(case, reference)` says, and that is on no tie"""
    rng = np.random.default_rng(seed)
    for i in range(4000):
        c = random_case(rng, i % 6, **size)
        try:
            ref = oracle_run(c)
        except (ZeroDivisionError, ValueError):
            continue
        if want(c, ref) and envelope(c, ref, seed)[1]:
            c["name"] = name
            return c
    raise AssertionError(f"no case for {name}")


def named_cases():
    """The cases the issue names, each found by the oracle's own record"""
    inact = lambda c: c["inactive"][:c["l"] - c["t"]] - 1
    leaves = lambda c, r: bool(np.any((c["cx"][inact(c)] > 0) & (c["cx_new"][inact(c)] <= 0)))
    enters = lambda c, r: bool(np.any((c["cx"][inact(c)] <= 0) & (c["cx_new"][inact(c)] > 0)))
    P = lambda r: r["pattern"]
    spec = [
        ("arm_newton", lambda c, r: P(r)[0] == 0, {}), ("arm_one_root", lambda c, r: P(r)[0] == 1, {}),
        ("arm_two_roots", lambda c, r: P(r)[0] == 2, {}),
        ("clamp_high", lambda c, r: P(r)[1] == "hi", {}), ("clamp_low", lambda c, r: P(r)[1] == "lo", {}),
        ("beta_clamp_high", lambda c, r: P(r)[0] == 2 and P(r)[2] == "hi", {}),
        ("beta_clamp_low", lambda c, r: P(r)[0] == 2 and P(r)[2] == "lo", {}),
        ("alpha_old_is_beta_hat_clamped", lambda c, r: P(r)[3] and P(r)[1] is not None, {}),
        ("choice_takes_beta", lambda c, r: P(r)[4], {}), ("choice_keeps_alpha_two_roots", lambda c, r: P(r)[0] == 2 and not P(r)[4], {}),
        ("no_constraints", lambda c, r: True, dict(l=0)), ("none_active", lambda c, r: True, dict(l=5, t=0)),
        ("all_active", lambda c, r: True, dict(l=5, t=5)),
        ("inactive_row_turns_violated", leaves, dict(l=6, t=2)), ("inactive_row_turns_satisfied", enters, dict(l=6, t=2)),
    ]
    return [found(name, want, 500 + i, **size) for i, (name, want, size) in enumerate(spec)]


def exact_cases():
    """Hand-made dyadic cases: every element, product and sum is exact, so the sums must be met bit for bit in any order"""
    base = dict(m=4, l=4, t=2, active=np.array([3, 1, 0, 0], dtype=np.int64), inactive=np.array([4, 2, 0, 0], dtype=np.int64),
                rx=np.array([1.0, -2.0, 0.5, 4.0]), Jp=np.array([2.0, 1.0, -1.0, 0.5]), rx_new=np.array([3.0, -1.5, 0.25, 2.0]),
                cx=np.array([1.0, -2.0, 0.5, 3.0]), Ap=np.array([-1.0, 2.0, 4.0, 1.0]), cx_new=np.array([0.5, 1.0, -1.0, -2.0]),
                w=np.array([4.0, 0.25, 16.0, 1.0]), alpha_k=0.5, x_min=0.5, a_min=2.0 ** -10, a_max=2.0)
    return [dict(base, name="exact_half_step"), dict(base, name="exact_quarter_step", alpha_k=0.25, x_min=0.0)]


SEED = 20261019
N_RANDOM = 240


def random_cases():
    rng = np.random.default_rng(SEED)
    out = []
    while len(out) < N_RANDOM:
        c = random_case(rng, len(out) % 6)
        c["name"] = f"random_{len(out)}_kind{len(out) % 6}"
        out.append(c)
    return out


# ---- the driver's problems: one variable, every terminal of linesearch_constrained ----------------------------------------------------
class Line:
    """r(x) and c(x) of one variable as the oracle's callbacks, x = 0, p = 1: r_i = a_i + b_i x + q_i x^2 + e_i sin(f x),
    c_j likewise"""

    def __init__(self, coef, f):
        self.coef, self.f = np.asarray(coef, dtype=np.float64), f

    def at(self, x):
        a, b, q, e = self.coef.T
        return a + b * x + q * x * x + e * np.sin(self.f * x)

    def eval_into(self, x, out):
        out[:] = self.at(float(np.asarray(x).ravel()[0]))


def driver_problem(rng, style):
    m, l, t = 3, 2, 1
    scale = (0.05, 1.0, 4.0, 12.0, 40.0, 120.0)[style % 6]
    r = Line(np.column_stack([rng.standard_normal(m), rng.standard_normal(m), scale * rng.standard_normal(m),
                              scale * rng.standard_normal(m)]), float(rng.uniform(2.0, 25.0)))
    c = Line(np.column_stack([rng.standard_normal(l), rng.standard_normal(l), scale * rng.standard_normal(l),
                              0.3 * scale * rng.standard_normal(l)]), float(rng.uniform(2.0, 25.0)))
    W = SimpleNamespace(l=l, t=t, active=np.array([1, 0], dtype=np.int64), inactive=np.array([2, 0], dtype=np.int64))
    w = 10.0 ** rng.uniform(-0.5, 0.5, l)
    rx, cx = r.at(0.0), c.at(0.0)
    Jp, Ap = r.coef[:, 1] + r.coef[:, 3] * r.f, c.coef[:, 1] + c.coef[:, 3] * c.f
    psi0 = eo.psi(np.zeros(1), 0.0, np.ones(1), r, c, w, m, l, t, W.active, W.inactive)
    dpsi0 = float(Jp @ rx) + float(w[0] * Ap[0] * cx[0])
    if dpsi0 >= 0:
        r.coef[:, 1] *= -1.0
        r.coef[:, 3] *= -1.0
        c.coef[:, 1] *= -1.0
        c.coef[:, 3] *= -1.0
        Jp, Ap = -Jp, -Ap
        dpsi0 = -dpsi0
    a_upp = float(10.0 ** rng.uniform(-0.3, 0.5))
    return dict(r=r, c=c, W=W, w=w, rx=rx, cx=cx, Jp=Jp, Ap=Ap, psi0=float(psi0), dpsi0=dpsi0, a_upp=a_upp, a_low=a_upp / 3000.0,
                a0=min(1.0, a_upp), m=m, l=l, t=t)


def oracle_linesearch(pr, jiggle=None):
    """eo.linesearch_constrained on a driver problem with a record of its path: the terminal (by the calls it makes: minrm count,
    minrn count, goldstein_armijo_step) and the number of psi evaluations.  jiggle: a generator that perturbs every evaluated
    residual vector by at most one ulp."""
    rec = dict(minrm=0, minrn=0, psi=0, gac=False, psis=[])
    minrm, minrn, psi, gac = eo.minrm, eo.minrn, eo.psi, eo.goldstein_armijo_step

    def minrm_w(*a):
        rec["minrm"] += 1
        return minrm(*a)

    def minrn_w(*a):
        rec["minrn"] += 1
        return minrn(*a)

    def psi_w(*a):
        rec["psi"] += 1
        rec["psis"].append(float(psi(*a)))
        return rec["psis"][-1]

    def gac_w(*a):
        rec["gac"] = True
        return gac(*a)

    r = pr["r"]
    if jiggle is not None:
        base = pr["r"]
        r = SimpleNamespace(eval_into=lambda x, out: out.__setitem__(slice(None), base.at(float(np.asarray(x).ravel()[0]))
                                                                      * (1.0 + ULP * jiggle.integers(-1, 2, size=out.shape))))
    eo.minrm, eo.minrn, eo.psi, eo.goldstein_armijo_step = minrm_w, minrn_w, psi_w, gac_w
    try:
        with np.errstate(all="ignore"):
            alpha, err = eo.linesearch_constrained(np.zeros(1), pr["a0"], np.ones(1), r, pr["c"], pr["rx"].copy(), pr["cx"].copy(),
                                                   np.concatenate([pr["Jp"], pr["Ap"]]), pr["w"], pr["W"], pr["psi0"], pr["dpsi0"],
                                                   pr["a_low"], pr["a_upp"])
    finally:
        eo.minrm, eo.minrn, eo.psi, eo.goldstein_armijo_step = minrm, minrn, psi, gac
    return dict(alpha=float(alpha), gac_error=bool(err), n_psi=rec["psi"], rec=rec, terminal=oracle_terminal(pr, rec, bool(err)))


def oracle_terminal(pr, rec, err):
    """The terminal of a recorded oracle run, in the names of enlsip_gn.linesearch: by the routines it called and, between the two
    arms that call the same ones, by the oracle's own test of :2036 on its first psi"""
    if rec["gac"]:
        return "armijo_error" if err else "armijo"
    if rec["minrm"] == 2:
        return "second_fit"
    a1, psi1 = min(pr["a0"], pr["a_upp"]), rec["psis"][0]
    if (-(pr["psi0"] - psi1) <= 0.25 * pr["dpsi0"] * a1) or (psi1 < 0.4 * pr["psi0"]):
        return "first_fit_minrn" if rec["minrn"] else "first_fit"
    return "second_minrn"


TERMINALS = ("first_fit", "first_fit_minrn", "second_fit", "second_minrn", "armijo_two_halvings", "armijo_error")


def driver_envelope(pr, ref, seed):
    """N_PERTURBED oracle runs with every evaluated residual moved by at most one ulp: (largest change of alpha, same path)"""
    env, stable = 0.0, True
    for i in range(N_PERTURBED):
        got = oracle_linesearch(pr, jiggle=np.random.default_rng(seed * 100 + i))
        stable = stable and (got["terminal"], got["n_psi"], got["gac_error"]) == (ref["terminal"], ref["n_psi"], ref["gac_error"])
        env = max(env, abs(got["alpha"] - ref["alpha"]))
    return env, stable


def driver_batch(seed=11):
    """One batch holding every terminal of linesearch_constrained, by the oracle's trace: the first problem of a seeded search per
    terminal whose path survives the one-ulp perturbation.  Returns [(problem, oracle run, alpha envelope)] in TERMINALS order."""
    rng = np.random.default_rng(seed)
    got = {}
    for i in range(20000):
        pr = driver_problem(rng, i % 6)
        try:
            run = oracle_linesearch(pr)
        except (ZeroDivisionError, ValueError):
            continue
        key = run["terminal"]
        if key == "armijo":
            key = "armijo_two_halvings" if run["n_psi"] - 3 >= 2 else None      # psi calls: two before the arm, one at its start
        if key is None or key in got:
            continue
        env, stable = driver_envelope(pr, run, i)
        if stable:
            got[key] = (pr, run, env)
        if len(got) == len(TERMINALS):
            return [got[k] for k in TERMINALS]
    raise AssertionError(f"terminals not reached: {set(TERMINALS) - set(got)}")
