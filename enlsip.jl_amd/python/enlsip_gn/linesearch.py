"""The set-up of the line search (``compute_steplength``, src/enlsip_functions.jl:2197-2293) before the line search itself, over
the HIP library: the products ``Jp = J * p``, ``Ap = A * p`` and ``active_Ap = C.A * p`` (:2226-2229), ``upper_bound_steplength``
(:2149-2178, called at :2252) and the three sums through which ``Jp`` enters ``penalty_weight_update`` (:1561-1584) and the predicted
reduction (:2269).  The penalty weights, the merit function, the polynomial fit and the callbacks stay with the caller, and so does
the division ``active_Ap ./ diag_scale`` (:2231-2233).
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
