"""Cases of the termination test shared by tests/test_termination_host.py and tests/test_gpu_termination_batched.py: random data
of one problem built to reach a named arm of check_termination_criteria (src/enlsip_functions.jl:2399-2517), the reference
objects of oracle/enlsip_outer.py made from it, the scalars of the decision by the reference's own NumPy expressions, and the
rounding bounds inside which a compared quantity counts as sitting on its threshold.

Thresholds are drawn far from the data: a quantity that must pass lies a factor 10 or more inside its threshold, one that must
fail a factor 10 outside, so that rounding decides nothing except where a case is built ON a threshold."""
import math
import types

import numpy as np

from oracle import enlsip_outer as eo

U = 2.0 ** -53
TOL = dict(max_iter=100, eps_abs=1e-10, eps_rel=1e-5, eps_x=1e-3, eps_c=1e-4)

# the arms: convergence codes alone and summed, each abnormal code in its elseif position, the failing preliminary conditions
CONVERGED = {"c4": 10000, "c5": 2000, "c6": 300, "c7": 40, "c45": 12000, "c46": 10300, "c4567": 12340}
ABNORMAL = {"max_iter": -2, "max_iter_beats_error_code": -2, "err-3": -3, "err-4": -4, "err-5": -5, "err_beats_newton": -4,
            "newton": -9, "newton_beats_psi": -9, "psi": -6, "psi_beats_infeasible": -6, "infeasible": -10,
            "infeasible_beats_time": -10, "time": -11, "none": 0}
PRELIM = {"restart": 0, "code-1_long_step": 0, "restart_then_time": -11}
NECESSARY_FAILS = {"del": 0, "cx_active_large": 0, "grad_res_large": 0, "inactive_nonpos": 0, "sigma_small_t1": 0,
                   "sigma_small_t2": 0}
ARMS = {**CONVERGED, **ABNORMAL, **PRELIM, **NECESSARY_FAILS}


def make_case(rng, arm, m, n, l, t=None, q=None, scaling=False):
    """One problem.  t, q default to random values that fit the arm."""
    if t is None:
        t = int(rng.integers(0, min(l, 6) + 1))
    if arm == "sigma_small_t1":
        t = 1
    if arm == "sigma_small_t2":
        t = max(t, 2)
    if arm in ("infeasible", "infeasible_beats_time", "psi_beats_infeasible", "cx_active_large"):
        t = max(t, 1)
    t = min(t, l)
    if arm == "inactive_nonpos":
        t = min(t, l - 1)
    if q is None:
        q = int(rng.integers(0, t + 1))
    if arm.startswith("sigma_small"):
        q = 0
        if t < (2 if arm == "sigma_small_t2" else 1):
            raise ValueError("arm needs more constraints")
    perm = rng.permutation(l) + 1
    active = np.zeros(l, dtype=np.int64)
    inactive = np.zeros(l, dtype=np.int64)
    active[:t] = np.sort(perm[:t])
    inactive[:l - t] = np.sort(perm[t:])
    c = dict(arm=arm, m=m, n=n, l=l, t=t, q=q, scaling=bool(scaling), active=active, inactive=inactive)
    c["J"] = np.asfortranarray(rng.standard_normal((m, n)))
    c["rx"] = rng.standard_normal(m)
    c["x"] = rng.standard_normal(n) + 2.0
    c["x_prev"] = c["x"] + 0.5 * rng.standard_normal(n)                 # x_diff ~ 0.5 sqrt(n) against eps_x |x| ~ 2e-3 sqrt(n)
    c["p"] = rng.standard_normal(n)
    c["dimJ2"] = int(rng.integers(0, n + 1))
    c["d_gn"] = rng.standard_normal(n)
    c["lam"] = np.abs(rng.standard_normal(t)) + 0.5                     # no negative multiplier: sigma_min = +Inf
    c["diag_scale"] = rng.random(t) + 0.5
    c["At"] = np.asfortranarray(rng.standard_normal((n, t)))
    c["cx_active"] = 1e-7 * rng.standard_normal(t)                      # ||.|| < eps_c by a factor 100 or more
    c["cx_all"] = np.abs(rng.standard_normal(l)) + 0.1                  # every inactive constraint satisfied
    c["w"] = 0.1 * rng.random(l) / max(math.sqrt(t), 1.0)               # dot(w[active], w[active]) <= 0.01
    st = dict(restart=False, code=1, delete=False, grad_res=1e-9, nb_iter=3, nb_newton_steps=0, error_code=0, psi_error=0,
              delta_time=-1.0, psi0=float(rng.random()) + 1.0)
    c["state"] = st

    def converge(crit4, crit5, crit6, crit7):
        # rx_sum ~ m, d1.d1 ~ dimJ2: criterion 4 holds when d1 is scaled to 1e-9 (1e-18 dimJ2 <= 1e-10 m) or empty
        if crit5:
            c["rx"] *= 1e-13                                            # rx_sum ~ 1e-26 m <= 1e-20
            c["d_gn"] *= 1e-20 if crit4 else 1.0                        # against rx_sum eps_rel^2 ~ 1e-36 m
        else:
            c["d_gn"] *= 1e-9 if crit4 else 1.0
        if not crit4:
            c["dimJ2"] = max(c["dimJ2"], 1)
        if crit6:
            c["x_prev"] = c["x"] + 1e-6 * rng.standard_normal(n)
        if crit7:
            c["p"] = np.zeros(n)                                        # alfnoi = 1

    if arm in CONVERGED:
        converge("4" in arm, "5" in arm, "6" in arm, "7" in arm)
    elif arm in NECESSARY_FAILS:
        converge(True, False, True, False)                              # would give 10300 if the necessary conditions held
        if arm == "del":
            st["delete"] = True
        elif arm == "cx_active_large":
            if t == 0:
                raise ValueError("arm needs t > 0")
            c["cx_active"] = rng.standard_normal(t) + 3.0
        elif arm == "grad_res_large":
            st["grad_res"] = 1e3 * (1.0 + float(np.linalg.norm(c["J"].T @ c["rx"])))
        elif arm == "inactive_nonpos":
            if l - t == 0:
                raise ValueError("arm needs an inactive constraint")
            c["cx_all"][inactive[int(rng.integers(0, l - t))] - 1] = -0.5
        else:
            c["lam"][t - 1] = -1e-6 if arm == "sigma_small_t2" else -1.0     # passes the product test, below eps_rel * factor
            c["lam"][: t - 1] = 10.0
    elif arm in ABNORMAL:
        c["cx_active"] = rng.standard_normal(t) + 3.0 if t else c["cx_active"]     # necessary conditions fail (t > 0) ...
        st["grad_res"] = 1e3 * (1.0 + float(np.linalg.norm(c["J"].T @ c["rx"])))   # ... and for every t
        infeasible = arm in ("infeasible", "infeasible_beats_time", "psi_beats_infeasible")
        if infeasible:
            c["x_prev"] = c["x"] + 1e-6 * rng.standard_normal(n)        # x_diff <= 10 eps_x
            c["cx_active"] = 1e-7 * rng.standard_normal(t)              # ||At cx|| <= 10 eps_c
            c["w"][active[:t] - 1] = 2.0                                # penalty sum >= 1
        if arm in ("max_iter", "max_iter_beats_error_code"):
            st["nb_iter"] = TOL["max_iter"] + int(rng.integers(0, 3))
        if arm in ("max_iter_beats_error_code", "err_beats_newton"):
            st["error_code"] = -4
        if arm.startswith("err-"):
            st["error_code"] = int(arm[3:])
        if arm in ("err_beats_newton", "newton", "newton_beats_psi"):
            st["nb_newton_steps"] = 6
        if arm in ("newton_beats_psi", "psi", "psi_beats_infeasible"):
            st["psi_error"] = -1
        if arm in ("infeasible_beats_time", "time"):
            st["delta_time"] = 0.5
    else:
        converge(True, False, True, False)
        if arm.startswith("restart"):
            st["restart"] = True
        else:
            st["code"] = -1                                             # alfnoi <= 0.25: p is a long step
        if arm == "restart_then_time":
            st["delta_time"] = 2.0
    return c


def expected_code(c):
    return ARMS[c["arm"]]


def oracle_objects(c):
    """(it, prev_iter, W, active_C) of oracle/enlsip_outer.py from a case"""
    st = c["state"]
    it = types.SimpleNamespace(p=c["p"], restart=st["restart"], code=st["code"], delete=st["delete"], grad_res=st["grad_res"],
                               d_gn=c["d_gn"], dimJ2=c["dimJ2"], w=c["w"], nb_newton_steps=st["nb_newton_steps"], lam=c["lam"])
    prev = types.SimpleNamespace(x=c["x_prev"])
    W = types.SimpleNamespace(q=c["q"], t=c["t"], l=c["l"], active=c["active"], inactive=c["inactive"])
    aC = types.SimpleNamespace(cx=c["cx_active"], A=np.ascontiguousarray(c["At"].T), scaling=c["scaling"], diag_scale=c["diag_scale"])
    return it, prev, W, aC


def oracle_exit(c, tol=TOL):
    it, prev, W, aC = oracle_objects(c)
    st = c["state"]
    rx_sum = float(c["rx"] @ c["rx"])
    grad = c["J"].T @ c["rx"]
    smin, lmax = eo.minmax_lagrangian_mult(c["lam"], W, aC)
    return eo.check_termination_criteria(it, prev, W, aC, c["x"], c["cx_all"], rx_sum, grad, tol["max_iter"], st["nb_iter"],
                                         tol["eps_abs"], tol["eps_rel"], tol["eps_x"], tol["eps_c"], st["error_code"],
                                         st["delta_time"], smin, lmax, st["psi_error"])


def numpy_scalars(c):
    """the fields of enlsip_gn_term_sums by the SAME NumPy expressions oracle/enlsip_outer.py uses"""
    it, prev, W, aC = oracle_objects(c)
    t, l = c["t"], c["l"]
    act = np.asarray(c["active"][:t], dtype=np.int64) - 1
    inact = np.asarray(c["inactive"][: l - t], dtype=np.int64) - 1
    smin, lmax = eo.minmax_lagrangian_mult(c["lam"], W, aC)
    d1 = c["d_gn"][: max(c["dimJ2"], 0)]
    rx_sum = float(c["rx"] @ c["rx"])
    whsum = float(c["w"][act] @ (c["cx_all"][act] ** 2))
    return dict(rx_sum=rx_sum, grad_nrm=float(np.linalg.norm(c["J"].T @ c["rx"])), p_nrm=float(np.linalg.norm(c["p"])),
                active_cx_nrm=float(np.linalg.norm(c["cx_active"])), n_inactive_nonpos=int(np.sum(~(c["cx_all"][inact] > 0))),
                n_inactive_le0=int(np.sum(c["cx_all"][inact] <= 0.0)), sigma_min=smin, lambda_abs_max=lmax, d1_sq=float(d1 @ d1),
                x_diff=float(np.linalg.norm(c["x_prev"] - c["x"])), x_nrm=float(np.linalg.norm(c["x"])),
                Atcx_nrm=float(np.linalg.norm(aC.A.T @ aC.cx)), active_penalty_sum=0.0 if t == 0 else float(c["w"][act] @ c["w"][act]),
                whsum=whsum, progress=2 * c["state"]["psi0"] - rx_sum - whsum)


def rounding_bounds(c):
    """ABSOLUTE bounds on the error of each computed field against the exact value on the same float64 inputs.
    - A plain sum of k products (rx_sum, d1_sq, active_penalty_sum): 2 k u sum|x_i||y_i|, the bound of
      tests/test_gpu_linesearch_setup_batched.py (k roundings at most lie on any path: one product, at most k - 1 additions that
      are not additions of an exact zero).
    - A norm of k entries (p_nrm, x_nrm, active_cx_nrm): the corresponding bound after the square root, which halves the relative
      error of the sum, plus one ulp for the root: (k + 1) u times the norm.
    - whsum: every term w c^2 carries two product roundings, one more than a plain product: 2 (k + 1) u sum|w| c^2.
    - x_diff: every term carries the rounding of the difference twice (it is squared) and of the square, two more than a plain
      product, and no cancellation is hidden (the inputs are exact, the bound is relative to the difference): 2 (k + 2) u on the
      sum, so (k + 2) u + u on the norm.
    - grad_nrm, Atcx_nrm: entry j of the inner product has the plain-sum bound e_j = 2 k u (|M| |v|)_j with k = m / t; the norm of
      the computed vector differs from the exact one by at most ||e||, and forming it adds (n + 1) u times itself."""
    m, n, t = c["m"], c["n"], c["t"]
    s = numpy_scalars(c)
    plain = lambda k: 2.0 * k * U
    norm = lambda k: (k + 1.0) * U
    g_err = float(np.linalg.norm(plain(m) * (np.abs(c["J"]).T @ np.abs(c["rx"]))))
    a_err = float(np.linalg.norm(plain(t) * (np.abs(c["At"]) @ np.abs(c["cx_active"])))) if t else 0.0
    return dict(rx_sum=plain(m) * s["rx_sum"], grad_nrm=g_err + norm(n) * (s["grad_nrm"] + g_err), p_nrm=norm(n) * s["p_nrm"],
                active_cx_nrm=norm(t) * s["active_cx_nrm"], d1_sq=plain(c["dimJ2"]) * s["d1_sq"], x_diff=(n + 3.0) * U * s["x_diff"],
                x_nrm=norm(n) * s["x_nrm"], Atcx_nrm=a_err + norm(n) * (s["Atcx_nrm"] + a_err),
                active_penalty_sum=plain(t) * s["active_penalty_sum"], whsum=plain(t + 1) * abs(s["whsum"]))


def on_a_threshold(c, tol=TOL):
    """True when some quantity the decision compares lies within its rounding bound of its threshold.  Where the threshold is itself
    computed (sqrt(eps_rel) (1 + grad_nrm), rx_sum eps_rel^2, eps_x x_nrm, eps_rel factor) the bound of the field inside it is
    carried through and 4 u of the threshold's magnitude covers the at most three roundings of forming it."""
    s, b = numpy_scalars(c), rounding_bounds(c)
    eps = float(np.finfo(np.float64).eps)
    near = lambda value, thr, err: abs(value - thr) <= err
    checks = [near(s["p_nrm"], 3.0 * eps, b["p_nrm"] + 4 * U * eps),
              near(s["active_cx_nrm"], tol["eps_c"], b["active_cx_nrm"]),
              near(math.sqrt(tol["eps_rel"]) * (1 + s["grad_nrm"]), c["state"]["grad_res"],
                   math.sqrt(tol["eps_rel"]) * b["grad_nrm"] + 4 * U * (1 + s["grad_nrm"])),
              near(s["d1_sq"], s["rx_sum"] * tol["eps_rel"] ** 2, b["d1_sq"] + (b["rx_sum"] + 4 * U * s["rx_sum"]) * tol["eps_rel"] ** 2),
              near(s["rx_sum"], tol["eps_abs"] ** 2, b["rx_sum"]),
              near(s["x_diff"], tol["eps_x"] * s["x_nrm"], b["x_diff"] + tol["eps_x"] * (b["x_nrm"] + 4 * U * s["x_nrm"])),
              near(s["x_diff"], 10.0 * tol["eps_x"], b["x_diff"]),
              near(s["Atcx_nrm"], 10.0 * tol["eps_c"], b["Atcx_nrm"]),
              near(s["active_penalty_sum"], 1.0, b["active_penalty_sum"])]
    if c["t"] > c["q"] and math.isfinite(s["sigma_min"]):
        factor = 1 + s["rx_sum"] if c["t"] == 1 else s["lambda_abs_max"]
        checks.append(near(s["sigma_min"], tol["eps_rel"] * factor, tol["eps_rel"] * (b["rx_sum"] + 4 * U * abs(factor))))
    return any(checks)
