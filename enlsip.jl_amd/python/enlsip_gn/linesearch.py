"""The set-up of the line search (``compute_steplength``, src/enlsip_functions.jl:2197-2293) before the line search itself, over
the HIP library: the products ``Jp = J * p``, ``Ap = A * p`` and ``active_Ap = C.A * p`` (:2226-2229), ``upper_bound_steplength``
(:2149-2178, called at :2252) and the three sums through which ``Jp`` enters ``penalty_weight_update`` (:1561-1584) and the predicted
reduction (:2269); then the penalty weights (``penalty_weight_update``, :2238, :1545-1629) with ``psi(0)`` (:2243), ``atwa`` and the
predicted reduction (:2267-2269), and the merit function ``psi`` (:1307-1340) of evaluated trial points.  The division ``active_Ap
./ diag_scale`` (:2231-2233) happens inside the penalty-weight call.  The polynomial fit, ``check_derivatives``, the first guess
``alpha0`` and the callbacks stay with the caller.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

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
    B = len(Ws)
    l = Ws[0].l
    t_max = setup.active_Ap.shape[-1]
    active, t = pack_active(Ws, t_max)
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
    B = len(Ws)
    l = Ws[0].l
    t_max = max([W.t for W in Ws] + [0])
    active, t = pack_active(Ws, t_max)
    inactive, n_inactive, _ = pack_inactive(Ws)
    ptr = lambda x: x.data_ptr() if x.numel() else 0
    return solver.merit_batched_dev(B, drx.shape[-1], l, t_max, t, active, inactive, n_inactive, ptr(drx), ptr(dcx), ptr(dw), take=take)
