"""Cases of the Gauss-Newton direction check shared by tests/test_direction_check_host.py and
tests/test_gpu_direction_check_batched.py: a table of scalar cases that drives every named condition of check_gn_direction
(src/enlsip_functions.jl:943-1030) both ways, the reference objects of oracle/enlsip_outer.py made from a case, a restatement of
the conditions (for the coverage assertion only: the product is never compared with it), and random array data of one problem
for the sums.

A case holds the SUMS (b1_sq, d_sq, ...); the oracle is handed their square roots, so both sides start from the same bits.  The
quantities are drawn far from the thresholds (a factor 1.04 or more), although with equal inputs and equal IEEE operations no
threshold can be decided by rounding anyway.

One thing about the oracle's arithmetic: the reference writes d1nrm^2, which Julia evaluates as d1nrm * d1nrm.  The oracle
writes d1nrm ** 2, which CPython hands to libm's pow, and pow(x, 2.0) is one ulp off x * x for about one x in 1200.  The table
keeps to sums whose roots square the same both ways (settle() below moves a sum to the next float until they do: a property of
the platform's libm, looked at before anything of the library runs), so that the oracle computes what the reference computes."""
import itertools
import math
import types

import numpy as np

from oracle import enlsip_outer as eo

SQRT_EPS = math.sqrt(float(np.finfo(np.float64).eps))
CONDITIONS = ("newton_or_restart", "first_iter", "submin_prev_iter", "add_or_del", "convergence_lower_c1", "progress_not_close",
              "lagrange_mult_cond", "inactive_lt_delta", "newton_previously", "cond4", "cond5", "cond6", "cond7", "cond8")


def settle(s):
    """the next float at or above s whose square root r has r ** 2 == r * r in this interpreter"""
    s = float(s)
    while True:
        r = math.sqrt(s)
        if r ** 2 == r * r:
            return s
        s = math.nextafter(s, math.inf)


def make_case(*, n=6, t=2, q=1, l=4, rankA=None, m=None, iter_number=3, restart=False, add=False, delete=False, prev_code=1,
              b1_sq=1.0, d1_sq=1.0, d_factor=1.0, asprev_factor=1.0, active_c_sum=0.0, beta_ratio=4.0, progress=(1.0, 1.0),
              prev_alpha=1.0, lam_kind="pos", inactive_small=False, scaling=False, nan_in=None):
    """d_sq = d_factor * (d1_sq + b1_sq), d1_asprev_sq = asprev_factor * d1_sq, prev_beta = beta_ratio * beta.
    lam_kind: "pos" every multiplier of q+1..t positive, "neg" every one below -1, "mixed" both, "tiny_neg" in (-sqrt(eps), 0)."""
    rankA = t if rankA is None else rankA
    m = n - t + 5 if m is None else m
    b1_sq, d1_sq = settle(b1_sq), settle(d1_sq)
    b1, d1 = math.sqrt(b1_sq), math.sqrt(d1_sq)
    beta = math.sqrt(d1 * d1 + b1 * b1)
    lam = np.full(t, 3.0)
    ds = np.full(t, 2.0)
    k = t - q
    if lam_kind == "neg":
        lam[q:] = -5.0
    elif lam_kind == "mixed":
        lam[q:] = np.where(np.arange(k) % 2 == 0, -5.0, 4.0)
    elif lam_kind == "tiny_neg":
        lam[q:] = -1e-12
    lam[:q] = -7.0                                        # the equalities are not looked at
    cx = np.full(l, 2.0)
    inactive = np.zeros(l, dtype=np.int64)
    active = np.zeros(l, dtype=np.int64)
    active[:t] = np.arange(1, t + 1)
    inactive[: l - t] = np.arange(t + 1, l + 1)
    if inactive_small and l - t > 0:
        cx[l - 1] = 0.05
    if nan_in == "lam" and k > 0:
        lam[t - 1] = math.nan
    if nan_in == "diag_scale" and k > 0:
        ds[t - 1] = math.nan
    if nan_in == "cx" and l - t > 0:
        cx[t] = math.nan
    return dict(n=n, m=m, t=t, q=q, l=l, rankA=rankA, iter_number=iter_number, restart=restart, add=add, delete=delete,
                prev_code=prev_code, b1_sq=b1_sq, d1_sq=d1_sq, d_sq=d_factor * (d1_sq + b1_sq), d1_asprev_sq=asprev_factor * d1_sq,
                active_c_sum=active_c_sum, prev_beta=beta_ratio * beta, prev_progress=progress[0],
                prev_predicted_reduction=progress[1], prev_alpha=prev_alpha, lam=lam, diag_scale=ds, cx_all=cx, active=active,
                inactive=inactive, scaling=scaling)


def counts(c):
    """the three counts by the oracle's own NumPy expressions (:1004, :1009)"""
    q, t, l = c["q"], c["t"], c["l"]
    rows = np.array([(1.0 / c["diag_scale"][i]) if c["scaling"] else c["diag_scale"][i] for i in range(q, t)])
    lw = c["lam"][q:t]
    with np.errstate(invalid="ignore"):
        ge = int(np.sum(lw * rows >= -SQRT_EPS)) if t > q else 0
        neg = int(np.sum(lw < 0)) if t > q else 0
        lt = int(sum(c["cx_all"][int(c["inactive"][j]) - 1] < 0.1 for j in range(l - t) if c["inactive"][j]))      # 0: padding
    return ge, neg, lt


def norms(c):
    return tuple(math.sqrt(c[k]) for k in ("b1_sq", "d1_sq", "d1_asprev_sq", "d_sq"))


def oracle_decision(c):
    b1, d1, dprev, dn = norms(c)
    W = types.SimpleNamespace(q=c["q"], t=c["t"], l=c["l"], inactive=c["inactive"])
    km1 = types.SimpleNamespace(code=c["prev_code"], beta=c["prev_beta"], progress=c["prev_progress"],
                                predicted_reduction=c["prev_predicted_reduction"], alpha=c["prev_alpha"])
    with np.errstate(invalid="ignore"):
        return eo.check_gn_direction(b1, d1, dprev, dn, c["active_c_sum"], c["iter_number"], c["rankA"], c["n"], c["m"], c["restart"],
                                     c["add"], c["delete"], W, c["cx_all"], c["lam"], km1, c["scaling"], c["diag_scale"])


def reached(c):
    """{condition: state} of every named condition the reference EVALUATES on this case (a restatement for the coverage assertion
    and the margin; short-circuit order is not modelled: a condition counts as reached when its statement is executed), and the
    smallest relative distance of a compared pair from equality"""
    b1, d1, dprev, dn = norms(c)
    beta = math.sqrt(d1 * d1 + b1 * b1)
    ge, neg, lt = counts(c)
    margin = [math.inf]

    def cmp(a, b):      # records how far a is from b; returns a < b
        if a != b or a != 0:
            margin[0] = min(margin[0], abs(a - b) / max(abs(a), abs(b)))
        return a < b
    r = dict(newton_or_restart=c["prev_code"] == 2 or c["restart"], first_iter=c["iter_number"] == 0,
             submin_prev_iter=c["prev_code"] == -1, add_or_del=c["add"] or c["delete"],
             convergence_lower_c1=cmp(beta, 0.5 * c["prev_beta"]),
             progress_not_close=cmp(0.1 * c["prev_predicted_reduction"], c["prev_progress"]) and not cmp(4.0 * beta, dn))
    enter = r["newton_or_restart"] or (not r["first_iter"] and (r["submin_prev_iter"] or not (
        r["add_or_del"] or r["convergence_lower_c1"] or r["progress_not_close"])))
    if not enter:
        return r, 1, margin[0]
    nl_k = math.sqrt(d1 * d1 + c["active_c_sum"])
    nl_km1 = math.sqrt(dprev * dprev + c["active_c_sum"])
    to_reduce = False
    if c["q"] < c["t"]:
        r["lagrange_mult_cond"] = ge > 0 and neg > 0
        to_reduce = r["lagrange_mult_cond"]
    if c["l"] - c["t"] > 0:
        r["inactive_lt_delta"] = lt > 0
        to_reduce = to_reduce or r["inactive_lt_delta"]
    r["newton_previously"] = c["prev_code"] == 2 and not c["delete"]
    r["cond4"] = cmp(0.1, c["active_c_sum"])
    r["cond5"] = c["delete"] or c["add"] or to_reduce or (c["t"] == c["n"] and c["t"] == c["rankA"])
    eps = 1e-2
    r["cond6"] = (not (c["l"] == c["q"] or c["rankA"] <= c["t"])) and not (cmp(beta, eps * dn) or (cmp(b1, eps) and c["m"] == c["n"] - c["t"]))
    code = -1
    if r["newton_previously"] or not (r["cond4"] or r["cond5"] or r["cond6"]):
        r["cond7"] = (cmp(c["prev_alpha"], 0.05) and cmp(nl_km1, 0.1 * nl_k)) or c["m"] == c["n"] - c["t"]
        r["cond8"] = cmp(10.0 * beta, dn)
        if r["newton_previously"] or r["cond7"] or r["cond8"]:
            code = 2
    return r, code, margin[0]


def table():
    """the explicit edges, then a product over the drivers of every condition"""
    out = [
        make_case(),                                                         # code 1: convergence_lower_c1
        make_case(iter_number=0, beta_ratio=0.5, progress=(0.01, 1.0)),      # first iteration
        make_case(m=4, n=6, t=2),                                            # m == n - t
        make_case(l=3, t=3, q=3, n=6),                                       # l == q, q == t, l == t
        make_case(n=3, t=3, q=1, l=5, rankA=3),                              # t == n == rankA
        make_case(t=2, q=2, l=2),                                            # q == t with l == t
        make_case(t=0, q=0, l=0, rankA=0),
    ]
    for nan_in in ("lam", "diag_scale", "cx"):
        for kind in ("neg", "mixed"):
            out.append(make_case(prev_code=-1, lam_kind=kind, nan_in=nan_in, scaling=nan_in == "diag_scale"))
    shapes = [dict(n=6, t=2, q=1, l=4), dict(n=6, t=2, q=1, l=4, m=4), dict(n=6, t=2, q=1, l=4, rankA=3), dict(n=6, t=2, q=2, l=2),
              dict(n=3, t=3, q=1, l=5), dict(n=5, t=1, q=1, l=1, rankA=0, m=4), dict(n=6, t=2, q=0, l=2, rankA=4)]
    first = itertools.product(shapes, (1, -1, 2), (False, True), ("none", "add", "del"), (0, 3), (4.0, 0.5), ((1.0, 1.0), (0.01, 1.0)))
    for shape, prev_code, restart, ad, it, ratio, prog in first:
        out.append(make_case(**shape, prev_code=prev_code, restart=restart, add=ad == "add", delete=ad == "del", iter_number=it,
                             beta_ratio=ratio, progress=prog, d_factor=9.0))
    # inside the branch: prev_code -1 enters it whatever the rest
    second = itertools.product(shapes, (-1, 2), ("pos", "neg", "mixed", "tiny_neg"), (False, True), (0.0, 0.01, 1.0),
                               (1.0, 9.0, 49.0, 400.0, 1e6), (0.0, 1e-3, 1.0), (0.01, 1.0), (1e-6, 1.0))
    for i, (shape, prev_code, kind, small, csum, dfac, afac, alpha, b1) in enumerate(second):
        out.append(make_case(**shape, prev_code=prev_code, lam_kind=kind, inactive_small=small, active_c_sum=csum, d_factor=dfac,
                             asprev_factor=afac, prev_alpha=alpha, b1_sq=b1, d1_sq=(1e-8, 1.0, 100.0)[i % 3], scaling=bool(i % 2),
                             delete=(i % 7 == 0)))
    return out


def random_problem(rng, m, n, l, t, q, *, dimA=None, dimJ2=None, k_prev=None, scaling=False):
    """array data of one problem for the sums: (state fields as a dict, arrays)"""
    dimA = int(rng.integers(0, t + 1)) if dimA is None else dimA
    dimJ2 = int(rng.integers(0, m + 1)) if dimJ2 is None else dimJ2
    k_prev = int(rng.integers(-2, m + 1)) if k_prev is None else k_prev
    perm = rng.permutation(l) + 1
    active, inactive = np.zeros(l, dtype=np.int64), np.zeros(l, dtype=np.int64)
    active[:t] = perm[:t]
    inactive[: l - t] = perm[t:]
    lam = rng.standard_normal(t) * 10.0 ** rng.integers(-10, 2, size=t)
    ds = rng.random(t) + 0.5
    cx = rng.standard_normal(l) * 0.2
    st = dict(iter_number=3, q=q, t=t, l=l, rankA=min(t, n), dimA=dimA, dimJ2=dimJ2, prev_code=-1, prev_t=t, prev_dimJ2=k_prev + 1,
              prev_beta=1.0, prev_progress=1.0, prev_predicted_reduction=1.0, prev_alpha=1.0)
    return st, dict(active=active, inactive=inactive, b=rng.standard_normal(t), d=rng.standard_normal(m) * 10.0 ** rng.integers(-3, 3, size=m),
                    lam=lam, diag_scale=ds, cx_all=cx, scaling=scaling)


# ---- the end-to-end batch: search_direction_analys over seven small problems ---------------------------------------------------------
E2E_SHAPE = (12, 6, 4)      # m, n, l
E2E_KINDS = ("code 1", "code -1, smaller dimensions", "code -1 back to 1", "code 2 with hessians", "code 2 without hessians",
             "not taken", "status 1")


def _iteration(**kw):
    z = np.zeros(0)
    f = dict(x=z, p=z, rx=z, cx=z, t=0, alpha=1.0, index_alpha_upp=0, lam=z, w=z, rankA=0, rankJ2=0, dimA=0, dimJ2=0, b_gn=z, d_gn=z,
             predicted_reduction=1.0, progress=1.0, grad_res=0.0, speed=0.0, beta=1.0, restart=False, first=False, add=False,
             delete=False, index_del=0, code=1, nb_newton_steps=0)
    f.update(kw)
    return eo.Iteration(**f)


def e2e_problems():
    """Seven problems (E2E_KINDS, in that order) with m = 12, n = 6, l = 4 and ragged t: the data, the oracle's Gauss-Newton
    solve, the current and previous records that force each outcome, and residual / constraint functions whose Jacobians at x
    are J and A (a quadratic term gives the Newton branch its Hessian sums).  Computed on the CPU."""
    from oracle import gn_oracle as go
    m, n, l = E2E_SHAPE
    ts, qs = (2, 2, 1, 2, 3, 2, 2), (1, 0, 1, 1, 1, 0, 1)
    out = []
    for k, kind in enumerate(E2E_KINDS):
        rng = np.random.default_rng(4100 + k)
        t, q = ts[k], qs[k]
        J, A = rng.standard_normal((m, n)), rng.standard_normal((l, n))
        x, rx = rng.standard_normal(n), rng.standard_normal(m)
        cx = np.concatenate([0.05 * rng.standard_normal(t), 1.0 + rng.random(l - t)])      # active small, inactive well above delta
        s, u = 0.05 * rng.standard_normal(m), 0.05 * rng.standard_normal(l)
        r = eo.EvalFunction(lambda y, rx=rx, J=J, s=s, x=x: rx + J @ (y - x) + 0.5 * s * float((y - x) @ (y - x)), None)
        c = eo.EvalFunction(lambda y, cx=cx, A=A, u=u, x=x: cx + A @ (y - x) + 0.5 * u * float((y - x) @ (y - x)), None)
        W = go.WorkingSet(q, t, l, np.concatenate([np.arange(1, t + 1), np.zeros(l - t, dtype=np.int64)]),
                          np.concatenate([np.arange(t + 1, l + 1), np.zeros(t - q, dtype=np.int64)]))
        aC = go.Constraint(cx[:t].copy(), A[:t].copy(), False, np.zeros(t))
        go.evaluate_scaling(aC)
        ref = go.gn_subproblem(J, rx, aC.A, aC.cx)
        rec = go.IterationRecord()
        lam = go.first_lagrange_mult_estimate(aC.A, J.T @ rx, aC.cx, False, aC.diag_scale, ref.F_A, rec, go.SQRT_EPS)
        beta0 = math.sqrt(float(np.linalg.norm(ref.d[:ref.rankJ2])) ** 2 + float(np.linalg.norm(ref.b[:ref.rankA])) ** 2)
        cur = _iteration(x=x, p=ref.p.copy(), rx=rx, cx=cx, t=t, lam=lam, rankA=ref.rankA, rankJ2=ref.rankJ2, dimA=ref.rankA,
                         dimJ2=ref.rankJ2, b_gn=ref.b.copy(), d_gn=ref.d.copy())
        prev = _iteration(rx=1.1 * rx, cx=1.1 * cx, t=t, dimA=ref.rankA, dimJ2=ref.rankJ2, beta=4.0 * beta0, alpha=0.5)
        second = True
        if kind.startswith("code -1"):
            cur.restart, cur.add, prev.code = True, True, -1
            if "smaller" in kind:
                prev.dimA, prev.dimJ2 = ref.rankA - 1, ref.rankJ2 - 1
        elif kind.startswith("code 2"):
            prev.code, prev.dimA, prev.dimJ2 = 2, -t, t - n
            second = "without" not in kind
        elif kind == "status 1":
            prev.dimJ2 = m + 2
        out.append(dict(kind=kind, J=J, A=A, x=x, rx=rx, cx=cx, r=r, c=c, W=W, aC=aC, ref=ref, lam=lam, cur=cur, prev=prev, t=t, q=q,
                        second=second, iter_number=3, take=int(kind != "not taken")))
    return out


def e2e_hessians(P):
    """Gamma = r_mat - c_mat of :391-396 for one problem, by the reference's own finite differences on the problem's functions"""
    m, n, l = E2E_SHAPE
    return eo.hessian_res(P["r"], P["x"], P["rx"], n, m) - eo.hessian_cons(P["c"], P["x"], P["lam"], P["W"].active, n, l, P["t"])


def e2e_oracle(P):
    """oracle.enlsip_outer.search_direction_analys on a copy of the problem's current record: (error_code, record)"""
    cur = P["cur"].copy()
    ref = P["ref"]
    err = eo.search_direction_analys(P["prev"], cur, P["iter_number"], P["x"], P["c"], P["r"], P["rx"], P["cx"], P["aC"],
                                     float(P["aC"].cx @ P["aC"].cx), ref.p.copy(), P["J"], P["W"], ref.F_A, ref.F_L11, ref.F_J2,
                                     P["second"], eo.OracleBackend())
    return err, cur


def e2e_case(P):
    """the problem as a case of reached(): the sums are the squares of the oracle's own norms"""
    cur, prev, W = P["cur"], P["prev"], P["W"]
    kp = max(prev.dimJ2 + prev.t - W.t - 1, 0)
    sq = lambda v: float(np.linalg.norm(v)) ** 2
    return dict(n=E2E_SHAPE[1], m=E2E_SHAPE[0], t=W.t, q=W.q, l=W.l, rankA=cur.rankA, iter_number=P["iter_number"], restart=cur.restart,
                add=cur.add, delete=cur.delete, prev_code=prev.code, b1_sq=sq(cur.b_gn[:cur.dimA]), d1_sq=sq(cur.d_gn[:cur.dimJ2]),
                d_sq=sq(cur.d_gn), d1_asprev_sq=sq(cur.d_gn[:kp]), active_c_sum=float(P["aC"].cx @ P["aC"].cx), prev_beta=prev.beta,
                prev_progress=prev.progress, prev_predicted_reduction=prev.predicted_reduction, prev_alpha=prev.alpha, lam=P["lam"],
                diag_scale=P["aC"].diag_scale, cx_all=P["cx"], active=W.active, inactive=W.inactive, scaling=False)


def e2e_margin(P):
    """smallest relative distance from equality of every comparison check_gn_direction makes on this problem, the two elementwise
    ones (:1004, :1009) included"""
    _, _, margin = reached(e2e_case(P))
    W = P["W"]
    for i in range(W.q, W.t):
        prod = P["lam"][i] * P["aC"].diag_scale[i]
        margin = min(margin, abs(prod + SQRT_EPS) / max(abs(prod), SQRT_EPS), 1.0 if P["lam"][i] != 0 else 0.0)
    for j in range(W.l - W.t):
        v = P["cx"][int(W.inactive[j]) - 1]
        margin = min(margin, abs(v - 0.1) / max(abs(v), 0.1))
    return margin
