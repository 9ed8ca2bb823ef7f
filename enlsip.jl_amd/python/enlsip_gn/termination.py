"""The termination test of the outer iteration (src/enlsip_functions.jl:2828-2839) over the HIP library: ``minmax_lagrangian_mult``
(:540-564), ``check_termination_criteria`` (:2399-2517) and the sums they read as host wrappers of the library's host entry points
(no GPU), and ``termination_batched_dev``, which runs the whole stage for a batch on the caller's device buffers from
``WorkingSet`` / ``IterationRecord`` objects.  Delta_time, max_iter and the error_code / Psi_error bookkeeping stay with the caller
and come in as inputs.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from ._lib import TermState, TermSums, TermTol
from .api import GNError, GNSolver, _dptr, _fptr

_CT = {C.c_int64: np.int64, C.c_double: np.float64}
SUMS_DTYPE = np.dtype([(name, _CT[ct]) for name, ct in TermSums._fields_])
STATE_DTYPE = np.dtype([(name, _CT[ct]) for name, ct in TermState._fields_])
assert SUMS_DTYPE.itemsize == C.sizeof(TermSums) and STATE_DTYPE.itemsize == C.sizeof(TermState)


def _f64(x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.float64)


def make_tol(max_iter: int, eps_abs: float, eps_rel: float, eps_x: float, eps_c: float) -> TermTol:
    return TermTol(int(max_iter), float(eps_abs), float(eps_rel), float(eps_x), float(eps_c))


def make_state(*, restart=False, code=0, delete=False, grad_res=0.0, nb_iter=0, nb_newton_steps=0, error_code=0, psi_error=0,
               delta_time=0.0, q=0, t=0, l=0, dimJ2=0, psi0=0.0) -> TermState:
    """One problem's enlsip_gn_term_state (``delete`` is the header's ``del``)."""
    return TermState(int(bool(restart)), int(code), int(bool(delete)), float(grad_res), int(nb_iter), int(nb_newton_steps),
                     int(error_code), int(psi_error), float(delta_time), int(q), int(t), int(l), int(dimJ2), float(psi0))


def minmax_lagrangian_mult(lam, q: int, t: int, diag_scale, scaling: bool):
    """``minmax_lagrangian_mult`` (:540-564) on host data: (sigma_min, lambda_abs_max).  A NaN among the t multipliers makes
    lambda_abs_max NaN, as the reference's ``maximum``."""
    lam, ds = _f64(lam), _f64(diag_scale)
    if t > q and (lam.size < t or ds.size < t):
        raise ValueError("lambda and diag_scale need t entries")
    smin, lmax = C.c_double(0.0), C.c_double(0.0)
    rc = L.load().enlsip_gn_minmax_lagrangian_mult(q, t, _fptr(lam), _fptr(ds), int(bool(scaling)), C.byref(smin), C.byref(lmax))
    if rc != 0:
        raise GNError(f"enlsip_gn_minmax_lagrangian_mult returned {rc}")
    return float(smin.value), float(lmax.value)


def check_termination_criteria(state: TermState, sums, tol: TermTol) -> int:
    """The decision of :2420-2516 on scalars.  ``sums``: a TermSums or one record of SUMS_DTYPE."""
    if not isinstance(sums, TermSums):
        sums = TermSums.from_buffer_copy(np.asarray(sums, dtype=SUMS_DTYPE).tobytes())
    code = C.c_int64(0)
    rc = L.load().enlsip_gn_check_termination_criteria(C.byref(state), C.byref(sums), C.byref(tol), C.byref(code))
    if rc != 0:
        raise GNError(f"enlsip_gn_check_termination_criteria returned {rc}")
    return int(code.value)


def termination_sums(*, J, rx, cx_all, x, x_prev, p, d_gn, dimJ2: int, lam, cx_active, diag_scale, At, w, active, inactive,
                     q: int, t: int, scaling: bool, psi0: float = 0.0, grad_in=None, rx_sum_in: Optional[float] = None):
    """enlsip_gn_termination_sums on the host arrays of one problem: (sums, grad) with sums one record of SUMS_DTYPE.  J: (m, n);
    At: (n, >= t), the OLD active slot as lam, cx_active, diag_scale; active / inactive: 1-based, the first t / l - t entries
    used.  grad_in / rx_sum_in: the gradient / rx_sum as formed elsewhere (the device's), taken as given."""
    J = np.asfortranarray(J, dtype=np.float64)
    m, n = J.shape
    At = np.asfortranarray(np.asarray(At, dtype=np.float64).reshape(n, -1))
    cx_all = _f64(cx_all)
    l = cx_all.size
    act = np.ascontiguousarray(np.asarray(active).astype(np.int64))
    ina = np.ascontiguousarray(np.asarray(inactive).astype(np.int64))
    vec = [_f64(v) for v in (rx, cx_all, x, x_prev, p, d_gn, lam, cx_active, diag_scale)]
    if act.size < t or ina.size < l - t or At.shape[1] < t or any(v.size < t for v in vec[6:]):
        raise ValueError("the lists and the active slot need t (inactive: l - t) entries")
    if vec[0].size != m or any(v.size != n for v in vec[2:5]) or vec[5].size < dimJ2 or _f64(w).size != l:
        raise ValueError("rx needs m, x, x_prev, p n, d_gn dimJ2 and w l entries")
    w = _f64(w)
    g_in = _f64(grad_in)
    rs_in = None if rx_sum_in is None else np.array([rx_sum_in], dtype=np.float64)
    grad = np.zeros(n)
    out = TermSums()
    rc = L.load().enlsip_gn_termination_sums(
        m, n, l, t, q, dimJ2, float(psi0), _fptr(act), _fptr(ina), _fptr(J), max(m, 1), *[_fptr(v) for v in vec], _fptr(At), max(n, 1),
        _fptr(w), int(bool(scaling)), _fptr(g_in), _fptr(rs_in), _fptr(grad), C.byref(out))
    if rc != 0:
        raise GNError(f"enlsip_gn_termination_sums returned {rc}")
    return np.frombuffer(bytes(out), dtype=SUMS_DTYPE)[0].copy(), grad


@dataclass
class TerminationBuffers:
    """Raw device pointers of one call (0 = NULL).  The NEW point: dJ (m x n column-major per problem), drx (m), dcx_all (l), dx
    (n).  The iteration that just ended: dx_prev, dp, dd_gn (n each), dlambda, dcx_active, ddiag_scale (t_max each) and dAt (n x
    t_max), the OLD active slot, dw (l).  Output: dgrad (n per problem).  dx_prev is ``prev_iter.x`` as the reference holds it
    at :2838: ``previous_iter`` is copied before ``iter.x`` is advanced (:2858-2860), so it is the point the PREVIOUS iteration
    started from, two steps behind ``dx``."""
    dJ: int = 0
    drx: int = 0
    dcx_all: int = 0
    dx: int = 0
    dx_prev: int = 0
    dp: int = 0
    dd_gn: int = 0
    dlambda: int = 0
    dcx_active: int = 0
    ddiag_scale: int = 0
    dAt: int = 0
    dw: int = 0
    dgrad: int = 0


@dataclass
class Termination:
    exit_code: np.ndarray       # (batch,) int64; 0: the problem goes on
    sums: np.ndarray            # (batch,) SUMS_DTYPE
    progress: np.ndarray        # (batch,) iter.progress of :2280

    @property
    def go_on(self) -> np.ndarray:
        """the take mask of the next iteration's batched calls"""
        return (self.exit_code == 0).astype(np.int64)


def termination_raw(solver: GNSolver, batch: int, m: int, n: int, l: int, t_max: int, states, tol: TermTol, active, inactive,
                    bufs: TerminationBuffers, scaling: bool, take=None, ldj=None, strideJ=None, ldat=None, strideAt=None,
                    sums=None, exit_code=None):
    """enlsip_gn_termination_batched_dev as it stands: ``states`` a ctypes array of TermState (or a sequence of them), active /
    inactive (batch, l) host lists.  Returns (sums (batch,) SUMS_DTYPE, exit_code (batch,) int64); the entries of problems with
    take 0 keep what the optional ``sums`` / ``exit_code`` arrays held (zeros by default)."""
    if not isinstance(states, C.Array):
        states = (TermState * batch)(*states)
    act = np.ascontiguousarray(np.asarray(active).astype(np.int64))
    ina = np.ascontiguousarray(np.asarray(inactive).astype(np.int64))
    if act.size != batch * l or ina.size != batch * l:
        raise ValueError(f"active and inactive must have {batch} x {l} entries")
    tk = None if take is None else GNSolver._host_i64(take, batch, "take")
    ldj = max(m, 1) if ldj is None else ldj
    ldat = max(n, 1) if ldat is None else ldat
    strideJ = ldj * n if strideJ is None else strideJ
    strideAt = ldat * t_max if strideAt is None else strideAt
    sums = np.zeros(batch, dtype=SUMS_DTYPE) if sums is None else sums
    exit_code = np.zeros(batch, dtype=np.int64) if exit_code is None else exit_code
    b = bufs
    solver._chk(solver._lib.enlsip_gn_termination_batched_dev(
        solver._h, batch, m, n, l, t_max, C.cast(states, C.c_void_p), C.byref(tol), _fptr(act) if act.size else None,
        _fptr(ina) if ina.size else None, _fptr(tk), int(bool(scaling)), _dptr(b.dJ), ldj, strideJ, _dptr(b.drx), _dptr(b.dcx_all),
        _dptr(b.dx), _dptr(b.dx_prev), _dptr(b.dp), _dptr(b.dd_gn), _dptr(b.dlambda), _dptr(b.dcx_active), _dptr(b.ddiag_scale),
        _dptr(b.dAt), ldat, strideAt, _dptr(b.dw), _dptr(b.dgrad), _fptr(sums), _fptr(exit_code)))
    return sums, exit_code


def termination_form(solver: GNSolver) -> int:
    """Kernel form of the last termination call on the solver's handle: 0 general, 1 one wave per problem, -1 none yet."""
    return solver._form("enlsip_gn_get_termination_form")


def termination_batched_dev(solver: GNSolver, Ws, its, bufs: TerminationBuffers, tol: TermTol, *, m: int, n: int, t_max: int,
                            scaling: bool, nb_iter, error_code=0, psi_error=0, delta_time=0.0, psi0=0.0, take=None, ldj=None,
                            strideJ=None, ldat=None, strideAt=None) -> Termination:
    """The stage between ``new_point!`` and ``evaluate_violated_constraints`` (:2828-2839) for B problems of one shape in one
    call.  ``Ws``: the working sets as they stood during the iteration (``W.q``, ``W.t``, the lists); ``its``: the iteration
    records, of which ``restart``, ``code``, ``delete``, ``grad_res``, ``nb_newton_steps`` and ``dimJ2`` are read (an absent
    attribute is 0 / False).  ``nb_iter``, ``error_code``, ``psi_error``, ``delta_time`` and ``psi0``: one value or one per
    problem, the caller's bookkeeping.  ``bufs``: the device buffers; ``bufs.dgrad`` receives grad_fx for the next first
    multiplier estimate.  Returns the exit codes, the sums and iter.progress; ``Termination.go_on`` is the next take mask."""
    B = len(Ws)
    l = Ws[0].l
    if any(W.l != l for W in Ws) or len(its) != B:
        raise ValueError("one shape per batch: every problem needs the same l, and one iteration record per problem")
    per = {k: np.broadcast_to(np.asarray(v), (B,)) for k, v in
           dict(nb_iter=nb_iter, error_code=error_code, psi_error=psi_error, delta_time=delta_time, psi0=psi0).items()}
    states = (TermState * B)()
    act, ina = np.zeros((B, l), dtype=np.int64), np.zeros((B, l), dtype=np.int64)
    for k, (W, it) in enumerate(zip(Ws, its)):      # the reference's inactive has l - q entries: zero-padded to l for the call
        act[k, :] = W.active
        ina[k, :l - W.q] = W.inactive
        states[k] = make_state(restart=getattr(it, "restart", False), code=getattr(it, "code", 0), delete=getattr(it, "delete", False),
                               grad_res=getattr(it, "grad_res", 0.0), nb_iter=per["nb_iter"][k],
                               nb_newton_steps=getattr(it, "nb_newton_steps", 0), error_code=per["error_code"][k],
                               psi_error=per["psi_error"][k], delta_time=per["delta_time"][k], q=W.q, t=W.t, l=l,
                               dimJ2=max(int(getattr(it, "dimJ2", 0)), 0), psi0=per["psi0"][k])
    sums, code = termination_raw(solver, B, m, n, l, t_max, states, tol, act, ina, bufs, scaling, take, ldj, strideJ, ldat, strideAt)
    return Termination(code, sums, sums["progress"].copy())
