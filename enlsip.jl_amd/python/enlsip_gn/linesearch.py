"""The set-up of the line search (``compute_steplength``, src/enlsip_functions.jl:2197-2293) before the line search itself, over
the HIP library: the products ``Jp = J * p``, ``Ap = A * p`` and ``active_Ap = C.A * p`` (:2226-2229), ``upper_bound_steplength``
(:2149-2178, called at :2252) and the three sums through which ``Jp`` enters ``penalty_weight_update`` (:1561-1584) and the predicted
reduction (:2269); then the penalty weights (``penalty_weight_update``, :2238, :1545-1629) with ``psi(0)`` (:2243), ``atwa`` and the
predicted reduction (:2267-2269), and the merit function ``psi`` (:1307-1340) of evaluated trial points.  The division ``active_Ap
./ diag_scale`` (:2231-2233) happens inside the penalty-weight call.  Then the line search itself: the polynomial fit of
``linesearch_constrained`` (:1940-2143: ``coefficients_linesearch!`` :1665-1689, ``minrm`` :1841-1862 and the choice of :2023-2026) as
one call per batch, and ``linesearch_constrained_batched``, the whole state machine of :1940-2143 over a batch with the callbacks
as the only thing left to the caller.  ``check_derivatives`` and the first guess ``alpha0`` stay with the caller.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import api as _api
from .api import GNSolver, upper_bound_steplength as _upper_bound_steplength


def upper_bound_steplength(Ap, cx, W, index_del: int):
    """``upper_bound_steplength(A, cx, p, work_set, index_del)`` (:2149-2178) with ``Ap = A * p`` already formed, through the library's
    host routine (no GPU): ``(alpha_upp, index_alpha_upp)``.  W: a ``WorkingSet`` (``inactive``, ``t``, ``l``)."""
    return _upper_bound_steplength(W.inactive, W.l - W.t, index_del, cx, Ap)


def pack_inactive(Ws, its=None):
    """The host records of the batched call: ``inactive`` (B, l) zero padded, ``n_inactive`` = l - t and ``index_del`` per problem
    (0 without iteration records).  All problems share l."""
    B = len(Ws)
    l = Ws[0].l
    if any(W.l != l for W in Ws):
        raise ValueError("the problems of a batch share l")
    inactive = np.zeros((B, l), dtype=np.int64)
    n_inactive = np.zeros(B, dtype=np.int64)
    index_del = np.zeros(B, dtype=np.int64)
    for k, W in enumerate(Ws):
        n_inactive[k] = l - W.t
        inactive[k, :l - W.t] = np.asarray(W.inactive[:l - W.t], dtype=np.int64)
        if its is not None:
            index_del[k] = its[k].index_del
    return inactive, n_inactive, index_del


@dataclass
class LinesearchSetup:
    Jp: object                  # device (B, m):      J * p                       :2226
    Ap: object                  # device (B, l):      A * p, all constraints      :2227
    active_Ap: object           # device (B, t_max):  C.A * p, 0 past t[k]        :2229 (before the division of :2231-2233)
    alpha_upp: np.ndarray       # (B,)                                            :2252
    index_alpha_upp: np.ndarray     # (B,) int64, 1-based, 0 for none             :2252
    JpJp: np.ndarray            # (B,) dot(Jp, Jp)                                :2269, :1561-1584
    Jprx: np.ndarray            # (B,) dot(Jp, rx)
    rxrx: np.ndarray            # (B,) dot(rx, rx)


def linesearch_setup_batched_dev(solver: GNSolver, Ws, its, dp, dA, dcx, drx, t_max: int, lda: int = 0, strideA: int = 0,
                                 prob0: int = 0) -> LinesearchSetup:
    """The set-up for problems prob0 .. prob0 + len(Ws) - 1 of the resident batch, everything in device buffers (torch tensors):
    dp (B, n) the directions, dA the full constraint Jacobians (problem k: l x n column-major at k * strideA, lda >= l; default
    packed), dcx (B, l) ALL constraint values, drx (B, m) the residuals.  ``jacobian_times_batched_dev`` forms Jp and active_Ap on
    the resident J and A' (t_max: the resident batch's), then one ``linesearch_setup_batched_dev`` call forms Ap, the bound and the
    sums.  Only the five scalars per problem come down."""
    import torch
    B = len(Ws)
    n = dp.shape[-1]
    m = drx.shape[-1]
    l = Ws[0].l
    inactive, n_inactive, index_del = pack_inactive(Ws, its)
    new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dp.device)
    dJp, dAp, dact = new(B, m), new(B, max(l, 1)), new(B, max(t_max, 1))
    solver.jacobian_times_batched_dev(prob0, B, dp.data_ptr(), dJp=dJp.data_ptr(), dAp=dact.data_ptr() if t_max else 0)
    lda = lda or max(l, 1)
    strideA = strideA or lda * n
    alpha, index, sums = solver.linesearch_setup_batched_dev(
        B, m, n, l, dp.data_ptr(), dA.data_ptr() if l else 0, lda, strideA, dcx.data_ptr() if l else 0, inactive, n_inactive,
        dAp.data_ptr() if l else 0, index_del=index_del, dJp=dJp.data_ptr(), drx=drx.data_ptr())
    return LinesearchSetup(dJp, dAp[:, :l], dact[:, :t_max], alpha, index, sums[:, 0].copy(), sums[:, 1].copy(), sums[:, 2].copy())


def pack_active(Ws, t_max: int):
    """The host records of the penalty-weight and merit calls: ``active`` (B, t_max) zero padded and ``t`` per problem."""
    B = len(Ws)
    active = np.zeros((B, t_max), dtype=np.int64)
    t = np.zeros(B, dtype=np.int64)
    for k, W in enumerate(Ws):
        t[k] = W.t
        active[k, :W.t] = np.asarray(W.active[:W.t], dtype=np.int64)
    return active, t


def pack_working_sets(Ws, t_max=None):
    """The host records of a batch of working sets: ``(B, l, t_max, active, t, inactive, n_inactive)``; t_max None: the largest t."""
    if t_max is None:
        t_max = max([W.t for W in Ws] + [0])
    inactive, n_inactive, _ = pack_inactive(Ws)
    return (len(Ws), Ws[0].l, t_max) + pack_active(Ws, t_max) + (inactive, n_inactive)


@dataclass
class PenaltyWeights:
    w: object                           # device (B, l): the new weights; w_old where the problem is not taken     :2238 / :2286
    dpsi0: np.ndarray                   # (B,) psi'(0)                                                            :1628
    psi0: np.ndarray                    # (B,) psi(0)                                                             :2243
    atwa: np.ndarray                    # (B,)                                                                    :2268
    branch: np.ndarray                  # (B,) int32: the arm of the weight update taken (include/enlsip_gn.h)
    predicted_reduction: np.ndarray     # (B,)                                                                    :2267-2269


def penalty_weights_batched_dev(solver: GNSolver, Ws, its, setup: LinesearchSetup, dw_old, dK, dcx, ddiag_scale, weight_code: int,
                                scaling: bool) -> PenaltyWeights:
    """``penalty_weight_update`` (:2238) for the problems of a ``LinesearchSetup``, everything in device buffers (torch tensors):
    dw_old (B, l) the previous weights, dK (B, 4, l) the weight histories (updated in place), dcx (B, l) ALL constraint values,
    ddiag_scale (B, t_max) (None without scaling).  its[k].dimA is the dimension the direction was computed with; problems with
    its[k].code == 2 are not taken (:2284-2290): their w is w_old and their scalars are 0.  Only the scalars come down."""
    B, l, t_max, active, t, _, _ = pack_working_sets(Ws, setup.active_Ap.shape[-1])
    dimA = np.array([it.dimA for it in its], dtype=np.int64)
    take = np.array([0 if it.code == 2 else 1 for it in its], dtype=np.int64)
    sums = np.stack([setup.JpJp, setup.Jprx, setup.rxrx], axis=1)
    dw = dw_old.clone()
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else 0
    act_Ap = setup.active_Ap if setup.active_Ap.is_contiguous() else setup.active_Ap.contiguous()
    scalars, branch = solver.penalty_weights_batched_dev(
        B, l, t_max, t, dimA, active, weight_code, scaling, ptr(dw_old), ptr(act_Ap), ptr(ddiag_scale) if scaling else 0, ptr(dcx),
        ptr(dK), sums, ptr(dw), take=take)
    upp = np.minimum(1.0, setup.alpha_upp)                                                       # :2267
    pred = upp * (-2.0 * setup.Jprx - upp * setup.JpJp + (2.0 - upp ** 2) * scalars[:, 2])       # :2269
    pred = np.where(take != 0, pred, 0.0)
    return PenaltyWeights(dw, scalars[:, 0].copy(), scalars[:, 1].copy(), scalars[:, 2].copy(), branch, pred)


def merit_batched_dev(solver: GNSolver, Ws, drx, dcx, dw, take=None) -> np.ndarray:
    """``psi`` (:1307-1340) of one trial point per problem: drx (B, m) and dcx (B, l) the residuals and ALL constraint values at the
    trial points, dw (B, l) the weights (device tensors).  Returns psi (B,)."""
    B, l, t_max, active, t, inactive, n_inactive = pack_working_sets(Ws)
    ptr = lambda x: x.data_ptr() if x.numel() else 0
    return solver.merit_batched_dev(B, drx.shape[-1], l, t_max, t, active, inactive, n_inactive, ptr(drx), ptr(dcx), ptr(dw), take=take)


# ---- the polynomial fit and the line search itself (src/enlsip_functions.jl:1940-2143) ---------------------------------------------
@dataclass
class LinesearchFit:
    sums: np.ndarray            # (B, 6) v0.v0, v0.v1, v0.v2, v1.v1, v1.v2, v2.v2                      :1849, :1749-1751
    out: np.ndarray             # (B, 6) alpha_kp1, pk (after the choice of :2023-2026), alpha_hat, s_alpha, beta_hat, s_beta
    arm: np.ndarray             # (B,) int32: 0 Newton-Raphson, 1 one root, 2 two roots                :1754-1778
    psi: object                 # (B,) psi of the trial point, or None                                 :2000


def linesearch_fit_batched_dev(solver: GNSolver, Ws, setup: LinesearchSetup, drx, dcx, drx_new, dcx_new, dw, alpha_k, x_min,
                               alpha_min, alpha_max, take=None, psi=False) -> LinesearchFit:
    """``coefficients_linesearch!`` and ``minrm`` with the choice (:2010-2026) for the problems of a ``LinesearchSetup``: drx, drx_new
    (B, m) the residuals at x and at the trial point, dcx, dcx_new (B, l) ALL constraint values there, dw (B, l) the weights (device
    tensors); setup.Jp and setup.Ap are the UNSCALED products (nothing is written).  alpha_k, x_min, alpha_min, alpha_max: (B,)
    host arrays.  With psi the merit function of the trial point comes back from the same call."""
    B, l, t_max, active, t, inactive, n_inactive = pack_working_sets(Ws)
    # contiguous views, kept alive until the call has returned
    bufs = [x if x.is_contiguous() else x.contiguous() for x in (drx, drx_new, setup.Jp, dcx, dcx_new, setup.Ap, dw)]
    sums, out, arm, psi_new = solver.linesearch_fit_batched_dev(
        B, drx.shape[-1], l, t_max, t, active, inactive, n_inactive, alpha_k, x_min, alpha_min, alpha_max,
        *[x.data_ptr() if x.numel() else 0 for x in bufs], take=take, psi=psi)
    return LinesearchFit(sums, out, arm, psi_new)


class HostLinesearchBackend:
    """The two calls the batched line search needs, on host arrays (NumPy in place of device tensors) through the library's host
    routines, no GPU: the merit function as a plain ordered sum (residuals in index order, the active list, the inactive list,
    :1322-1339) and the fit as ``linesearch_coefficients`` + ``linesearch_fit`` per problem."""

    @staticmethod
    def _psi(W, rx, cx, w) -> float:
        s = 0.0
        for v in rx:
            s += float(v) * float(v)
        c = 0.0
        for j in W.active[:W.t]:
            c += float(w[j - 1]) * (float(cx[j - 1]) * float(cx[j - 1]))
        for j in W.inactive[:W.l - W.t]:
            if cx[j - 1] < 0.0:
                c += float(w[j - 1]) * (float(cx[j - 1]) * float(cx[j - 1]))
        return 0.5 * (s + c)

    def merit(self, Ws, rx, cx, w, take=None) -> np.ndarray:
        return np.array([self._psi(W, rx[k], cx[k], w[k]) if take is None or take[k] else 0.0 for k, W in enumerate(Ws)])

    def fit(self, Ws, setup, rx, cx, rx_new, cx_new, w, alpha_k, x_min, alpha_min, alpha_max, take=None, psi=False) -> LinesearchFit:
        B = len(Ws)
        sums, out, arm = np.zeros((B, 6)), np.zeros((B, 6)), np.zeros(B, dtype=np.int32)
        for k, W in enumerate(Ws):
            if take is not None and not take[k]:
                continue
            sums[k] = _api.linesearch_coefficients(W.active, W.t, W.inactive, W.l - W.t, rx[k], rx_new[k], setup.Jp[k], cx[k],
                                                   cx_new[k], setup.Ap[k], w[k], alpha_k[k])
            out[k], arm[k] = _api.linesearch_fit(sums[k], alpha_k[k], x_min[k], alpha_min[k], alpha_max[k])
        return LinesearchFit(sums, out, arm, self.merit(Ws, rx_new, cx_new, w, take) if psi else None)


class _DeviceLinesearchBackend:
    """the same two calls on device tensors through a GNSolver"""

    def __init__(self, solver):
        self.solver = solver

    def merit(self, Ws, drx, dcx, dw, take=None):
        return merit_batched_dev(self.solver, Ws, drx, dcx, dw, take=take)

    def fit(self, Ws, setup, *args, **kw):
        return linesearch_fit_batched_dev(self.solver, Ws, setup, *args, **kw)


# the terminals of linesearch_constrained, as LinesearchResult.terminal names them
FIRST_FIT = "first_fit"                 # :2036-2062 accepted after the first minrm, the reduce loop never entered
FIRST_FIT_MINRN = "first_fit_minrn"     # :2036-2062 the same arm after at least one minrn round
SECOND_FIT = "second_fit"               # :2078-2092 the second minrm at the new point
SECOND_MINRN = "second_minrn"           # :2094-2096 minrn at the new point
ARMIJO = "armijo"                       # :2133-2137 goldstein_armijo_step, left by its sufficient-decrease test
ARMIJO_ERROR = "armijo_error"           # the same, left with gac_error


@dataclass
class LinesearchResult:
    alpha: np.ndarray           # (B,) the step lengths                                                :2142
    gac_error: np.ndarray       # (B,) bool
    rounds: int                 # calls of `evaluate`
    terminal: list              # per problem, one of the names above
    n_eval: np.ndarray          # (B,) int64: evaluations (psi calls of the reference) per problem


def _one_linesearch(alpha0, psi0, dpsi0, alpha_min, alpha_max, p_max):
    """linesearch_constrained (:1940-2143) for one problem as a generator.  It yields what it needs next and is sent the answer:
    ("fit", alpha_k, x_min, evaluate) -> (psi or None, sums, out); ("psi", alpha) -> psi.  Returns (alpha, gac_error, terminal)."""
    eta, tau, gamma = 0.3, 0.25, 0.4                                            # :1965-1967
    a_k = min(alpha0, alpha_max)                                                # :1974
    a_km1, psi_km1 = 0.0, psi0
    # :2000-2026.  The fit's x_min depends on the psi the same call returns (:2019): the call is made with x_min = alpha_k, the
    # value of the usual case diff_psi >= 0, and otherwise the scalar stage is redone on the returned sums by the host routine,
    # which is what the call runs
    psi_k, sums, out = yield ("fit", a_k, a_k, True)
    diff_psi = psi0 - psi_k
    if not diff_psi >= 0:
        out, _ = _api.linesearch_fit(sums, a_k, 0.0, alpha_min, alpha_max)
    a_kp1, pk = float(out[0]), float(out[1])
    a_km2, psi_km2 = a_km1, psi_km1
    a_km1, psi_km1 = a_k, psi_k
    a_k = a_kp1
    psi_k = yield ("psi", a_k)                                                  # :2033
    refresh = False
    if (-diff_psi <= tau * dpsi0 * a_km1) or (psi_km1 < gamma * psi0):          # :2036
        diff_psi = psi0 - psi_k
        refresh = True                                                          # this arm's loop refreshes diff_psi (:2055)
        terminal = FIRST_FIT
    else:
        diff_psi = psi0 - psi_k                                                 # :2068
        if (-diff_psi <= tau * dpsi0 * a_k) or (psi_k < gamma * psi0):          # :2071
            if psi0 <= psi_km1:                                                 # :2075: a second minrm at the point just evaluated
                _, sums, out = yield ("fit", a_k, a_k, False)
                a_kp1, pk = float(out[0]), float(out[1])
                a_km1, psi_km1 = 0.0, psi0
                terminal = SECOND_FIT
            else:
                a_kp1, pk = _api.minrn(a_k, psi_k, a_km1, psi_km1, a_km2, psi_km2, alpha_min, alpha_max, p_max)
                terminal = SECOND_MINRN
            a_km2, psi_km2 = a_km1, psi_km1
            a_km1, psi_km1 = a_k, psi_k
            a_k = a_kp1
            psi_k = yield ("psi", a_k)                                          # :2107
        else:                                                                   # goldstein_armijo_step (:1893-1923) from alpha_k
            u = a_k
            ex = (p_max * u < _api.SQRT_EPS) or (u <= alpha_min)
            psi_u = yield ("psi", u)
            while (not ex) and (psi_u > psi0 + tau * u * dpsi0):
                u *= 0.5
                psi_u = yield ("psi", u)
                ex = (p_max * u < _api.SQRT_EPS) or (u <= alpha_min)
            return u, bool(ex), ARMIJO_ERROR if ex else ARMIJO
    # the reduce loop of both arms (:2043-2062, :2111-2130).  The second arm does NOT refresh diff_psi: :2100 assigns `diff`,
    # :2111 reads `diff_psi`, the value of :2068
    while _api.check_reduction(psi_km1, psi_k, pk, eta, diff_psi):
        a_kp1, pk = _api.minrn(a_k, psi_k, a_km1, psi_km1, a_km2, psi_km2, alpha_min, alpha_max, p_max)
        a_km2, psi_km2 = a_km1, psi_km1
        a_km1, psi_km1 = a_k, psi_k
        a_k = a_kp1
        psi_k = yield ("psi", a_k)
        if refresh:
            diff_psi = psi0 - psi_k
            terminal = FIRST_FIT_MINRN
    if (psi_km1 - pk >= eta * diff_psi) and (psi_k < psi_km1):                  # :2058, :2126
        a_km1, psi_km1 = a_k, psi_k
    return a_km1, False, terminal


def linesearch_constrained_batched(backend, Ws, evaluate, setup: LinesearchSetup, drx, dcx, dw, alpha0, psi0, dpsi0, alpha_low,
                                   alpha_upp, p_max) -> LinesearchResult:
    """``linesearch_constrained`` (:1940-2143) for every problem of a batch, each with its own state; a round evaluates only the
    problems still running.

    backend: a ``GNSolver`` (drx, dcx, dw and the buffers of ``evaluate`` are device tensors) or a ``HostLinesearchBackend`` (NumPy
    arrays).  Every psi goes through the backend's merit call, every minrm through its fit call; minrn and check_reduction are the
    library's host routines.  ``evaluate(alpha, take) -> (drx_new, dcx_new)``: the caller's callback.  It evaluates the residuals
    and ALL constraints at x_k + alpha[k] p_k for the problems with take[k] != 0 into its two buffers ((B, m) and (B, l), the same
    two at every call), leaves the rows of the other problems as they are, and returns the buffers.  setup: Jp and Ap as the set-up
    call left them (unscaled); alpha0, psi0, dpsi0, alpha_low, alpha_upp, p_max (= max |p_k|, :1979): (B,) host arrays.

    The Goldstein-Armijo arm runs as rounds of halving with its own exit test, its first round at the step it starts from, as
    :1911 evaluates it.  Returns a ``LinesearchResult``."""
    B = len(Ws)
    be = _DeviceLinesearchBackend(backend) if isinstance(backend, GNSolver) else backend
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(B)
    alpha0, psi0, dpsi0, alpha_low, alpha_upp, p_max = (f(a) for a in (alpha0, psi0, dpsi0, alpha_low, alpha_upp, p_max))
    gens = [_one_linesearch(alpha0[k], psi0[k], dpsi0[k], alpha_low[k], alpha_upp[k], p_max[k]) for k in range(B)]
    req = [next(g) for g in gens]
    alpha, gac = np.zeros(B), np.zeros(B, dtype=bool)
    terminal = [None] * B
    n_eval = np.zeros(B, dtype=np.int64)
    rounds = 0
    point = np.zeros(B)                 # the step every problem was last evaluated at
    bufs = None
    while any(r is not None for r in req):
        answer = [None] * B
        ev = np.array([1 if r is not None and (r[0] == "psi" or r[3]) else 0 for r in req], dtype=np.int64)
        if ev.any():
            for k in np.flatnonzero(ev):
                point[k] = req[k][1]
            bufs = evaluate(point.copy(), ev.copy())
            rounds += 1
            n_eval += ev
        for with_psi in (True, False):      # the fits of this pass: with the evaluation (and psi) first, then those without
            fk = np.array([1 if r is not None and r[0] == "fit" and bool(r[3]) == with_psi else 0 for r in req], dtype=np.int64)
            if fk.any():
                a_k = np.array([r[1] if fk[k] else 0.0 for k, r in enumerate(req)])
                x_min = np.array([r[2] if fk[k] else 0.0 for k, r in enumerate(req)])
                got = be.fit(Ws, setup, drx, dcx, bufs[0], bufs[1], dw, a_k, x_min, alpha_low, alpha_upp, take=fk, psi=with_psi)
                for k in np.flatnonzero(fk):
                    answer[k] = (float(got.psi[k]) if with_psi else None, got.sums[k].copy(), got.out[k].copy())
        pk = np.array([1 if r is not None and r[0] == "psi" else 0 for r in req], dtype=np.int64)
        if pk.any():
            psi = be.merit(Ws, bufs[0], bufs[1], dw, take=pk)
            for k in np.flatnonzero(pk):
                answer[k] = float(psi[k])
        for k in range(B):
            if req[k] is None:
                continue
            try:
                req[k] = gens[k].send(answer[k])
            except StopIteration as done:
                alpha[k], gac[k], terminal[k] = done.value
                req[k] = None
    return LinesearchResult(alpha, gac, rounds, terminal, n_eval)
