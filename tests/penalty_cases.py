"""Cases of the penalty-weight update shared by tests/test_penalty_weights_host.py and tests/test_gpu_penalty_weights_batched.py:
penalty_weight_update (src/enlsip_functions.jl:1545-1629) through oracle/enlsip_outer.py, a record of what the oracle did inside
(the arguments of its own inner calls; the drops per pass of min_norm_w come from a counting copy of its loop that only classifies
cases), the perturbation envelope of its outputs, and the problems of the device test.

Sizes: l <= 12, t <= 8, m <= 16, the smallest at which every loop of the routine still takes all its paths."""
import contextlib
from types import SimpleNamespace

import mpmath as mp
import numpy as np

from oracle import enlsip_outer as eo

U = np.finfo(np.float64).eps / 2
ULP = 2.0 ** -52
N_PERTURBED = 16        # oracle runs per case with Jp, rx moved by at most one ulp
MARGIN = 10.0           # the margin the project gives a 1-ulp envelope (alpha_tolerance of tests/test_reference_problems.py)


def exact_dot(x, y):
    """the exactly rounded dot product"""
    with mp.workdps(80):
        return float(mp.fdot([mp.mpf(float(v)) for v in x], [mp.mpf(float(v)) for v in y]))


def exact_sums(c):
    return exact_dot(c["Jp"], c["Jp"]), exact_dot(c["Jp"], c["rx"]), exact_dot(c["rx"], c["rx"])


# ---- the oracle, with a record of what it did ---------------------------------------------------------------------------------------
@contextlib.contextmanager
def traced_oracle(rec):
    """oracle.enlsip_outer with its euclidean_norm_weight_update, min_norm_w and max_norm_weight_update wrapped so that their
    arguments and what they left are recorded in `rec`; the functions themselves run unchanged."""
    eu, mn, mx = eo.euclidean_norm_weight_update, eo.min_norm_w, eo.max_norm_weight_update

    def eu_w(vA, cx, active, t, mu, dimA, previous_w, K):
        if t:
            act = np.asarray(active[:t], dtype=np.int64) - 1
            rec["ztw_ge_mu"] = bool(float((vA ** 2) @ K[3][act]) >= mu)       # the oracle's own expression for :1453
            rec["ztw_lt_mu"] = bool(float((vA ** 2) @ K[3][act]) < mu)
        return eu(vA, cx, active, t, mu, dimA, previous_w, K)

    def mn_w(ctrl, w, w_old, y, tau, pos_index, nb_pos):
        rec["ctrl"], rec["nb_pos"] = ctrl, nb_pos
        rec["pos0"] = [int(v) for v in pos_index[:nb_pos]]
        if nb_pos > 0:
            yn = float(np.linalg.norm(y))
            rec["c_is_1"] = bool(np.max(np.abs(y / yn if yn != 0.0 else y)) <= eo.EPS)      # the first pass's test of :1398
            rec["drops"] = drops_per_pass(ctrl, w_old, y, tau, rec["pos0"], nb_pos)
        mn(ctrl, w, w_old, y, tau, pos_index, nb_pos)

    def mx_w(nrm_Ap, rmy, alpha_w, delta, w, active, t, K):
        rec["mu_zero_arm"] = bool(abs(alpha_w - 1.0) <= delta)
        col = [float(K[i][0]) for i in range(4)]
        mx(nrm_Ap, rmy, alpha_w, delta, w, active, t, K)
        after = [float(K[i][0]) for i in range(4)]
        rec["mu_place"] = next((i for i in range(4) if not same_bits(col[i], after[i])), None)

    eo.euclidean_norm_weight_update, eo.min_norm_w, eo.max_norm_weight_update = eu_w, mn_w, mx_w
    try:
        yield
    finally:
        eo.euclidean_norm_weight_update, eo.min_norm_w, eo.max_norm_weight_update = eu, mn, mx


def same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def oracle_run(c, Jp=None, rx=None):
    """The oracle on a case (Jp, rx: perturbed copies).  Returns dict(w, K (4, l), dpsi0, psi0, atwa, branch, rec, pattern)."""
    l, t = c["l"], c["t"]
    W = SimpleNamespace(active=c["active"].copy(), t=t, l=l)
    K = [c["K"][i].copy() for i in range(4)]
    Jp = c["Jp"] if Jp is None else Jp
    rx = c["rx"] if rx is None else rx
    rec = {}
    with traced_oracle(rec), np.errstate(all="ignore"):
        w, dpsi0 = eo.penalty_weight_update(c["w_old"].copy(), Jp.copy(), c["Ap"].copy(), K, rx.copy(), c["cx"].copy(), W, c["dimA"],
                                            c["norm_code"])
    act = c["active"][:t] - 1
    with np.errstate(all="ignore"):
        psi0 = 0.5 * (float(rx @ rx) + float(w[act] @ c["cx"][act] ** 2))          # :2243
        atwa = float(w[act] @ c["Ap"] ** 2)                                       # :2268
    K = np.stack(K)
    if c["norm_code"] == 0 or t == 0:
        branch = 0
    elif "ctrl" not in rec:
        branch = 4
    elif rec["ctrl"] == 1:
        branch = 3
    else:
        branch = 1 if rec["ztw_ge_mu"] else 2
    pattern = (branch, tuple((w != c["w_old"]).tolist()), tuple((w != c["K"][3]).tolist()),
               tuple((~((K == c["K"]) | (np.isnan(K) & np.isnan(c["K"])))).ravel().tolist()))
    return dict(w=np.asarray(w, dtype=np.float64), K=K, dpsi0=float(dpsi0), psi0=psi0, atwa=atwa, branch=branch, rec=rec,
                pattern=pattern)


def drops_per_pass(ctrl, w_old, y, tau, pos, nb_pos):
    """The number of entries each pass of min_norm_w (:1396-1420) drops: the loop of oracle/enlsip_outer.py:495-527 with a counter.
    Used only to CLASSIFY cases for the coverage assertions, never to judge a value."""
    y = np.array(y, dtype=np.float64)
    pos = list(pos) + [0]
    y_sum = float(y @ y)
    y_norm = float(np.linalg.norm(y))
    if y_norm != 0.0:
        y = y / y_norm
    y = np.append(y, 0.0)
    tau_new, s, n_runch, out = tau, 0.0, nb_pos, []
    while True:
        tau_new -= s
        with np.errstate(all="ignore"):
            cc = 1.0 if np.max(np.abs(y[:-1])) <= eo.EPS else tau_new / y_sum
        y_sum, s, i_stop, k, dropped = 0.0, 0.0, n_runch, 1, 0
        while k <= n_runch:
            i = pos[k - 1] - 1
            with np.errstate(all="ignore"):
                buff = cc * y[k - 1] * y_norm
            if buff >= w_old[i]:
                y_sum += y[k - 1] ** 2
                k += 1
            else:
                s += w_old[i] * y[k - 1] * y_norm
                n_runch -= 1
                dropped += 1
                for j in range(k, n_runch + 1):
                    pos[j - 1] = pos[j]
                    y[j - 1] = y[j]
        y_sum *= y_norm * y_norm
        out.append(dropped)
        if n_runch <= 0 or ctrl == 2 or i_stop == n_runch:
            return out


# ---- the envelope --------------------------------------------------------------------------------------------------------------------
def envelope(c, ref, seed):
    """N_PERTURBED oracle runs with every entry of Jp and rx moved by at most one ulp (seeded).  Returns (env, stable): env = the
    largest change of each output, stable = the discrete pattern never changed."""
    rng = np.random.default_rng(seed)
    env = dict(w=np.zeros(c["l"]), K=np.zeros((4, c["l"])), dpsi0=0.0, psi0=0.0, atwa=0.0)
    stable = True
    for _ in range(N_PERTURBED):
        Jp = c["Jp"] * (1.0 + ULP * rng.integers(-1, 2, size=c["Jp"].shape))
        rx = c["rx"] * (1.0 + ULP * rng.integers(-1, 2, size=c["rx"].shape))
        got = oracle_run(c, Jp, rx)
        stable = stable and got["pattern"] == ref["pattern"]
        with np.errstate(all="ignore"):
            for key in env:
                d = np.abs(np.asarray(got[key]) - np.asarray(ref[key]))
                d = np.where(np.isnan(d), 0.0, d)          # inf - inf, nan - nan: the value itself is compared exactly
                env[key] = np.maximum(env[key], d)
    return env, stable


def within(got, ref, env):
    """|got - ref| <= MARGIN * env + 4 ulp(ref), entry by entry; a non-finite reference must be met exactly"""
    got, ref, env = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (got, ref, env))
    fin = np.isfinite(ref)
    exact = (got == ref) | (np.isnan(got) & np.isnan(ref))
    with np.errstate(all="ignore"):
        close = np.abs(got - ref) <= MARGIN * env + 4.0 * np.spacing(np.abs(ref))
    return bool(np.all(np.where(fin, close, exact)))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def random_case(rng, kind, l=None, t=None, m=None, norm_code=None):
    """One case.  kind (0..5) picks what is biased: the scale of Jp against Ap (which side of mu ztw falls on), signs, spreads."""
    l = int(rng.integers(1, 13)) if l is None else l
    t = int(rng.integers(0, min(8, l) + 1)) if t is None else t
    m = int(rng.integers(1, 17)) if m is None else m
    norm_code = (0, 2)[int(rng.integers(2))] if norm_code is None else norm_code
    active = np.zeros(l, dtype=np.int64)
    perm = rng.permutation(l)[:t] + 1
    active[:t] = perm if rng.integers(3) else np.sort(perm)
    dimA = [0, t, int(rng.integers(0, t + 1)), t][int(rng.integers(4))] if t else 0
    w_old = 10.0 ** rng.uniform(-1, 1, l)
    K = np.sort(10.0 ** rng.uniform(-1.5, 1.5, (4, l)), axis=0)[::-1].copy()
    Ap = rng.standard_normal(t) * 10.0 ** rng.uniform(-1, 1)
    cx = rng.standard_normal(l) * 10.0 ** rng.uniform(-1, 1)
    Jp = rng.standard_normal(m) * 10.0 ** rng.uniform(-1.5, 1.5)
    rx = rng.standard_normal(m) * 10.0 ** rng.uniform(-1, 1)
    sub = kind % 6
    if sub == 1:                                  # alpha_w near 1: rx close to -Jp, small weights
        rx = -Jp * (1.0 + 0.05 * rng.standard_normal(m))
        w_old *= 1e-3
    elif sub == 2 and t:                          # the e of :1479 all <= 0: nb_pos = 0 in branch 2
        cx[active[:t] - 1] = np.abs(cx[active[:t] - 1]) * np.sign(Ap)
        Jp *= 30.0
    elif sub == 3:                                # a large mu
        Jp *= 100.0
    elif sub == 4 and t:                          # weights with a wide spread: the ctrl = 1 arm drops entries pass after pass
        K[3, active[:t] - 1] = 10.0 ** rng.uniform(-3, 3, t)
        K[:] = np.sort(K, axis=0)[::-1]
        Jp *= 10.0
    elif sub == 5:                                # a small history: assort! inserts high up
        K *= 10.0 ** rng.uniform(-3, -1)
    if norm_code == 0 and t == 0:
        # nrm_Ap = 0: the oracle's Python division of :1514 raises where Julia's gives +-Inf, so the oracle can only be asked with
        # alpha_w = 1, the arm that does not divide (the host test checks the division by zero against its stated value instead)
        rx = -Jp
    return dict(l=l, t=t, m=m, active=active, dimA=dimA, norm_code=norm_code, w_old=w_old, K=K, Ap=Ap, cx=cx, Jp=Jp, rx=rx)


def special_cases():
    """The named degenerate cases of the issue: nrm_Ap = 0, nrm_cx = 0, JpJp = 0, each under both norm codes"""
    out = []
    rng = np.random.default_rng(4242)
    for norm_kind in (0, 1):
        for what in ("Ap0", "cx0", "Jp0", "Ap0_dimA_t"):
            c = random_case(rng, 0, l=6, t=3, m=5, norm_code=2 * norm_kind)
            c["name"] = f"{what}_norm{c['norm_code']}"
            if what.startswith("Ap0"):
                c["Ap"] = np.zeros(3)
                c["dimA"] = 3 if what.endswith("dimA_t") else 1
                if c["norm_code"] == 0:
                    c["rx"] = -c["Jp"]          # see random_case: the oracle cannot divide by nrm_Ap = 0
            elif what == "cx0":
                c["dimA"] = 2
                c["cx"][c["active"][:2] - 1] = 0.0
            else:
                c["Jp"] = np.zeros(5)
            out.append(c)
    return out


def two_pass_case():
    """The ctrl = 1 arm dropping entries in two passes.  z = (4, 1, 1), mu = 3 * Jp.Jp = 18 (Jp.rx = 0), K[4] = (1, 1.5, 0.99) on the
    active entries: ztw = 6.49 < mu.  Pass 1 has buff = 18 z_i / 18 = (4, 1, 1) and drops the second entry (1 < 1.5); pass 2 has
    buff = 16.5 z_i / 17 and drops the third (0.97 < 0.99); pass 3 drops nothing."""
    K = np.array([[9.0, 8.0, 7.0, 6.0], [5.0, 4.0, 3.0, 4.0], [3.0, 2.0, 2.0, 3.0], [1.5, 1.0, 0.99, 2.0]])
    return dict(name="ctrl1_two_passes", l=4, t=3, m=3, active=np.array([2, 1, 3, 0], dtype=np.int64), dimA=3, norm_code=2,
                w_old=np.array([0.5, 0.25, 2.0, 1.0]), K=K, Ap=np.array([2.0, -1.0, 1.0]), cx=np.array([0.3, -0.7, 1.1, 0.2]),
                Jp=np.array([1.0, 1.0, 2.0]), rx=np.array([1.0, 1.0, -1.0]))


def exact_cases():
    """Hand-made dyadic cases, one per norm_code: every sum, product, square root and normalisation is exact (the one quotient that
    is not, 20 / 3, is a single IEEE division on both sides), so the oracle must be met bit for bit."""
    base = dict(l=5, t=4, m=4, active=np.array([2, 5, 1, 4, 0], dtype=np.int64), dimA=4,
                w_old=np.array([1.0, 2.0, 64.0, 0.5, 4.0]), Ap=np.array([1.0, -1.0, 1.0, 1.0]),      # nrm_Ap = 2
                cx=np.array([0.5, 2.0, 3.0, 2.0, -1.0]),                                            # nrm_cx = 2 over the active
                Jp=np.array([1.0, 1.0, 1.0, 1.0]), rx=np.array([2.0, -2.0, 2.0, 2.0]))              # Jp.Jp = 4, Jp.rx = 4, rx.rx = 16
    K = np.array([[64.0, 32.0, 32.0, 64.0, 16.0], [32.0, 16.0, 16.0, 32.0, 8.0], [16.0, 8.0, 8.0, 16.0, 4.0],
                  [4.0, 1.0, 2.0, 8.0, 2.0]])
    # rmy = |4 + 4| / 0.25 - 4 = 28.  Euclidean: z = 1, ztw = 1 + 2 + 4 + 8 = 15 < 28 with dimA == t: ctrl = 1; pass 1 has c = 7, buff = 7
    # and drops the entry with K[4] = 8; pass 2 has c = (28 - 8) / 3.  Maximum norm: mu = 28 / 2 = 14 goes to the third place of K[.][1].
    return [dict(base, name="exact_max_norm", norm_code=0, K=K.copy()), dict(base, name="exact_euclidean", norm_code=2, K=K.copy())]


SEED = 20261019
N_RANDOM = 240


def host_cases():
    """The case list of the host test: random cases of every kind, the named degenerate ones and the exact ones."""
    rng = np.random.default_rng(SEED)
    cases = []
    for i in range(N_RANDOM):
        c = random_case(rng, i % 6)
        c["name"] = f"random_{i}_kind{i % 6}"
        cases.append(c)
    return cases + special_cases() + [two_pass_case()] + exact_cases()


# ---- the device test's problems ---------------------------------------------------------------------------------------------------
def padded(c, l, t_max, rng):
    """The case inside a problem of l constraints and a t_max-strided active part: the extra entries are live data of the larger
    problem (the l-wide copies move them)"""
    out = dict(c)
    grow = lambda v, fill: np.concatenate([v, fill])
    extra = l - c["l"]
    out["l"] = l
    out["w_old"] = grow(c["w_old"], 10.0 ** rng.uniform(-1, 1, extra))
    out["cx"] = grow(c["cx"], rng.standard_normal(extra))
    out["K"] = np.concatenate([c["K"], np.sort(10.0 ** rng.uniform(-1.5, 1.5, (4, extra)), axis=0)[::-1]], axis=1)
    out["active"] = grow(c["active"], np.zeros(extra, dtype=np.int64))
    return out


def wanted(host_branch, norm_code, branches, l, t_choices, seed, m=8):
    """One case per wanted branch at the given sizes, found by a seeded search judged by `host_branch(case) -> int`"""
    rng = np.random.default_rng(seed)
    out = []
    for b, t in zip(branches, t_choices):
        for _ in range(4000):
            c = random_case(rng, int(rng.integers(6)), l=l, t=t, m=m, norm_code=norm_code)
            if host_branch(c) == b:
                out.append(c)
                break
        else:
            raise AssertionError(f"no case for branch {b} with t = {t}, l = {l}")
    return out
