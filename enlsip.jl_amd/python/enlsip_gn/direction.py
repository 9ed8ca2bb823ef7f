"""The analysis of the Gauss-Newton direction (src/enlsip_functions.jl:1191-1291) over the HIP library: ``check_gn_direction``
(:943-1030) and the sums it reads as host wrappers of the library's host entry points (no GPU), and
``GNSolver.direction_check_batched_dev``, which forms the sums of a batch on the caller's device buffers and returns the method
codes: -1 is the take of ``subspace_direction_batched_dev``, 2 the take of ``newton_direction_batched_dev``.
``search_direction_analys_batched_dev`` is the whole of :1237-1290 over a batch: the check, then one call for each of the two
branches.  The Hessian sums of the Newton branch (:243-328) are the caller's ``hessians`` callback, or, where the residuals and
constraints are batched device functions (``hessian_evals``), ``hessian_sums_batched_dev``: stencil points and sums on the device
around the caller's evaluations, Gamma written where the batched Newton call reads it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._lib import DirState, DirSums
from .api import GNError, GNSolver, _dptr, _fptr

_CT = {C.c_int64: np.int64, C.c_double: np.float64}
SUMS_DTYPE = np.dtype([(name, _CT[ct]) for name, ct in DirSums._fields_])
STATE_DTYPE = np.dtype([(name, _CT[ct]) for name, ct in DirState._fields_])
assert SUMS_DTYPE.itemsize == C.sizeof(DirSums) and STATE_DTYPE.itemsize == C.sizeof(DirState)


def _f64(x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.float64)


def make_state(*, iter_number=0, restart=False, add=False, delete=False, q=0, t=0, l=0, rankA=0, dimA=0, dimJ2=0, prev_code=1,
               prev_dimJ2=0, prev_t=0, prev_beta=0.0, prev_progress=0.0, prev_predicted_reduction=0.0, prev_alpha=1.0) -> DirState:
    """One problem's enlsip_gn_dir_state (``delete`` is the header's ``del``)."""
    return DirState(int(iter_number), int(bool(restart)), int(bool(add)), int(bool(delete)), int(q), int(t), int(l), int(rankA),
                    int(dimA), int(dimJ2), int(prev_code), int(prev_dimJ2), int(prev_t), float(prev_beta), float(prev_progress),
                    float(prev_predicted_reduction), float(prev_alpha))


def _as_sums(sums) -> DirSums:
    if isinstance(sums, DirSums):
        return sums
    return DirSums.from_buffer_copy(np.asarray(sums, dtype=SUMS_DTYPE).tobytes())


def check_gn_direction(state: DirState, sums, m: int, n: int):
    """The decision of :943-1030 on scalars: (method_code, beta).  ``sums``: a DirSums or one record of SUMS_DTYPE."""
    sums = _as_sums(sums)
    code, beta = C.c_int64(0), C.c_double(0.0)
    rc = L.load().enlsip_gn_check_gn_direction(C.byref(state), C.byref(sums), m, n, C.byref(code), C.byref(beta))
    if rc != 0:
        raise GNError(f"enlsip_gn_check_gn_direction returned {rc}")
    return int(code.value), float(beta.value)


def direction_sums(state: DirState, *, m: int, n: int, active, inactive, b, d, lam, diag_scale, cx_all, scaling: bool):
    """enlsip_gn_direction_sums on the host arrays of one problem: (sums, status) with sums one record of SUMS_DTYPE (zeros when
    status is 1).  b: >= dimA entries, d: m, lam and diag_scale: t, cx_all: l; active / inactive: 1-based, the first t / l - t
    entries used."""
    l, t = int(state.l), int(state.t)
    act = np.ascontiguousarray(np.asarray(active).astype(np.int64))
    ina = np.ascontiguousarray(np.asarray(inactive).astype(np.int64))
    b, d, lam, ds, cx = (_f64(v) for v in (b, d, lam, diag_scale, cx_all))
    if act.size < t or ina.size < l - t or lam.size < t or ds.size < t or b.size < state.dimA or d.size != m or cx.size != l:
        raise ValueError("the lists, lam and diag_scale need t (inactive: l - t) entries, b dimA, d m and cx_all l")
    out, status = DirSums(), C.c_int64(0)
    rc = L.load().enlsip_gn_direction_sums(m, n, l, C.byref(state), _fptr(act), _fptr(ina), _fptr(b), _fptr(d), _fptr(lam), _fptr(ds),
                                           _fptr(cx), int(bool(scaling)), C.byref(out), C.byref(status))
    if rc != 0:
        raise GNError(f"enlsip_gn_direction_sums returned {rc}")
    return np.frombuffer(bytes(out), dtype=SUMS_DTYPE)[0].copy(), int(status.value)


@dataclass
class DirectionCheck:
    method_code: np.ndarray     # (batch,) int64: 1 Gauss-Newton accepted, -1 subspace minimisation, 2 Newton
    beta: np.ndarray            # (batch,) float64
    status: np.ndarray          # (batch,) int64: 0, 1 the reference would throw (no code), 2 a prefix of d past n - rankA
    sums: np.ndarray            # (batch,) SUMS_DTYPE

    def take(self, code: int) -> np.ndarray:
        """the take mask of the call that serves ``code`` (-1: subspace_direction_batched_dev, 2: newton_direction_batched_dev)"""
        return ((self.method_code == code) & (self.status != 1)).astype(np.int64)


def direction_check_batched_dev(solver: GNSolver, batch: int, m: int, n: int, l: int, t_max: int, states, active, inactive, scaling: bool,
                                db: int, dd: int, dlambda: int, ddiag_scale: int, dcx_all: int, take=None, out: DirectionCheck = None
                                ) -> DirectionCheck:
    """enlsip_gn_direction_check_batched_dev: ``states`` a ctypes array of DirState (or a sequence of them), active / inactive
    (batch, l) host lists, the rest raw device pointers (0 = NULL) where the solve and the multiplier calls left them.  The entries
    of problems with take 0 keep what ``out`` held (method_code 0, beta NaN, status -1 and zero sums by default)."""
    if not isinstance(states, C.Array):
        states = (DirState * batch)(*states)
    act = np.ascontiguousarray(np.asarray(active).astype(np.int64))
    ina = np.ascontiguousarray(np.asarray(inactive).astype(np.int64))
    if act.size != batch * l or ina.size != batch * l:
        raise ValueError(f"active and inactive must have {batch} x {l} entries")
    tk = None if take is None else GNSolver._host_i64(take, batch, "take")
    if out is None:
        out = DirectionCheck(np.zeros(batch, dtype=np.int64), np.full(batch, np.nan), np.full(batch, -1, dtype=np.int64),
                             np.zeros(batch, dtype=SUMS_DTYPE))
    solver._chk(solver._lib.enlsip_gn_direction_check_batched_dev(
        solver._h, batch, m, n, l, t_max, C.cast(states, C.c_void_p), _fptr(act) if act.size else None,
        _fptr(ina) if ina.size else None, _fptr(tk), int(bool(scaling)), _dptr(db), _dptr(dd), _dptr(dlambda), _dptr(ddiag_scale),
        _dptr(dcx_all), _fptr(out.sums), _fptr(out.method_code), _fptr(out.beta), _fptr(out.status)))
    return out


# ---- the finite-difference Hessian sums of the Newton branch (:243-328) around the caller's evaluations ------------------------------
def hessian_pairs(n: int) -> int:
    """pairs (k, j), 0 <= j <= k < n, of the lower triangle; pair index P = k (k + 1) / 2 + j"""
    return n * (n + 1) // 2


def hessian_points(x, pair0: int = 0, npairs: int = None) -> np.ndarray:
    """enlsip_gn_hessian_points on the host (no GPU): the stencil points of pairs pair0 .. pair0 + npairs - 1 (default: all of
    them) around x, (npairs, 4, n); slot s of a pair is x_work before evaluation f_{s+1} of :259-265, bit for bit."""
    x = _f64(x).reshape(-1)
    n = x.size
    npairs = hessian_pairs(n) - pair0 if npairs is None else npairs
    X = np.zeros((max(npairs, 0), 4, n))
    rc = L.load().enlsip_gn_hessian_points(n, pair0, npairs, _fptr(x), _fptr(X))
    if rc != 0:
        raise GNError(f"enlsip_gn_hessian_points returned {rc}")
    return X


def hessian_sums(x, F, rx, G, lam, active, t: int, *, pair0: int = 0, Gamma=None) -> np.ndarray:
    """enlsip_gn_hessian_sums on the host (no GPU): Gamma[k, j] = Gamma[j, k] = r - c (:268-272, :317-322, :393) of the pairs
    pair0 .. pair0 + npairs - 1 from F (npairs, 4, m), the residuals, and G (npairs, 4, l), all constraints, at the points of
    ``hessian_points``.  rx: m, lam: t, active: the first t entries used, 1-based.  ``Gamma``: an (n, n) array whose other entries
    are kept (Gamma is symmetric in what is written, so its memory order does not matter), default zeros.  Returns it."""
    x, rx = _f64(x).reshape(-1), _f64(rx).reshape(-1)
    n, m = x.size, rx.size
    F = _f64(F)
    npairs = F.shape[0]
    G = np.zeros((npairs, 4, 0)) if G is None else _f64(G)
    l = G.shape[-1]
    if F.shape != (npairs, 4, m) or G.shape != (npairs, 4, l):
        raise ValueError("F must be (npairs, 4, m) and G (npairs, 4, l)")
    lam = np.zeros(0) if lam is None else _f64(lam).reshape(-1)
    act = np.zeros(0, dtype=np.int64) if active is None else np.ascontiguousarray(np.asarray(active).astype(np.int64)).reshape(-1)
    if lam.size < t or act.size < t:
        raise ValueError("lam and active need t entries")
    Gamma = np.zeros((n, n)) if Gamma is None else Gamma
    if Gamma.shape != (n, n) or Gamma.dtype != np.float64 or not (Gamma.flags.c_contiguous or Gamma.flags.f_contiguous):
        raise ValueError("Gamma must be a contiguous (n, n) float64 array")
    ptr = lambda a: _fptr(a) if a.size else None
    rc = L.load().enlsip_gn_hessian_sums(m, n, l, t, pair0, npairs, ptr(act), _fptr(x), ptr(F), ptr(rx), ptr(G), ptr(lam),
                                         _fptr(Gamma), n)
    if rc != 0:
        raise GNError(f"enlsip_gn_hessian_sums returned {rc}")
    return Gamma


def hessian_points_dev(solver: GNSolver, count: int, n: int, pair0: int, npairs: int, dx: int, dX: int) -> None:
    """enlsip_gn_hessian_points_batched_dev on raw device pointers: dx (count, n) in, dX (count, npairs, 4, n) out"""
    solver._chk(solver._lib.enlsip_gn_hessian_points_batched_dev(solver._h, count, n, pair0, npairs, _dptr(dx), _dptr(dX)))


def hessian_sums_dev(solver: GNSolver, count: int, m: int, n: int, l: int, t_max: int, pair0: int, npairs: int, t, active, slot,
                     dx: int, dF: int, drx: int, dG: int, dlambda: int, dGamma: int, ldg: int, strideG: int) -> None:
    """enlsip_gn_hessian_sums_batched_dev: t (count), active (count, l) and slot (count, or None for the identity) are host
    arrays, the rest raw device pointers (0 = NULL)."""
    tt = GNSolver._host_i64(t, count, "t")
    act = np.ascontiguousarray(np.asarray(active).astype(np.int64)) if active is not None else np.zeros(0, dtype=np.int64)
    if active is not None and act.size != count * l:
        raise ValueError(f"active must have {count} x {l} entries")
    sl = None if slot is None else GNSolver._host_i64(slot, count, "slot")
    solver._chk(solver._lib.enlsip_gn_hessian_sums_batched_dev(
        solver._h, count, m, n, l, t_max, pair0, npairs, _fptr(tt), _fptr(act) if act.size else None, _fptr(sl), _dptr(dx),
        _dptr(dF), _dptr(drx), _dptr(dG), _dptr(dlambda), _dptr(dGamma), ldg, strideG))


HESSIAN_BUFFER_DOUBLES = 1 << 25      # default bound of one point or evaluation buffer of the driver below: 256 MiB


def hessian_sums_batched_dev(solver: GNSolver, Ws, dx, drx, dlam, residuals, constraints, dGamma, *, slot=None,
                             pairs_per_call: int = None) -> None:
    """``hessian_res!`` and ``hessian_cons!`` (:243-328) and Gamma = r_mat - c_mat (:393) for N problems of one shape whose
    residuals and constraints are batched device functions.  ``Ws``: the N working sets; dx (N, n), drx (N, m), dlam (N, t_max):
    contiguous float64 device tensors of the same N problems in order.  ``residuals(X)`` / ``constraints(X)``: the caller's
    callbacks; X is (N, 4 npairs, n), the stencil points of npairs pairs of every problem, and they return (N, 4 npairs, m) and
    (N, 4 npairs, l), ALL l constraints, as float64 device tensors (``constraints`` may be None when l == 0).  ``dGamma``: a device
    tensor (S, n, ldg) with unit stride along its last axis; Gamma of problem k goes column-major to slot ``slot[k]`` of it (None:
    slot k), slot[k] < 0 leaves problem k alone.  Only the entries of Gamma are written, rows >= n of a column and other slots are
    kept.

    The driver allocates one point buffer and walks the triangle in ranges of ``pairs_per_call`` pairs (default: all of them, or as
    many as keep a buffer inside HESSIAN_BUFFER_DOUBLES): points, the two callbacks, sums.  A callback's result is read where it
    is when it is contiguous, and copied into a buffer of the driver (allocated once) when it is not.  The library runs on its own
    stream and every call returns after synchronising it; torch's current stream is synchronised before the library reads what a
    callback wrote.  Nothing of Gamma, the points or the evaluations crosses PCIe."""
    import torch
    N = len(Ws)
    if N < 1:
        return
    n, m, l = int(dx.shape[1]), int(drx.shape[1]), int(Ws[0].l)
    t_max = int(dlam.shape[1]) if dlam is not None else 0
    if any(W.l != l for W in Ws) or dx.shape[0] != N or drx.shape[0] != N or (dlam is not None and dlam.shape[0] != N):
        raise ValueError("one shape per batch: every problem needs the same l, and dx, drx, dlam one row per problem")
    for name, v in (("dx", dx), ("drx", drx), ("dlam", dlam)):
        if v is not None and (v.dtype != torch.float64 or not v.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float64 tensor")
    if dGamma.dim() != 3 or dGamma.dtype != torch.float64 or dGamma.stride(2) != 1 or dGamma.shape[1] < n or dGamma.shape[2] < n:
        raise ValueError("dGamma must be a float64 tensor (S, >= n, >= n) with unit stride along its last axis")
    if l > 0 and t_max > 0 and constraints is None:
        raise ValueError("constraints is required when l > 0")
    dev = dx.device
    pairs = hessian_pairs(n)
    if pairs_per_call is None:
        pairs_per_call = max(1, min(pairs, HESSIAN_BUFFER_DOUBLES // (N * 4 * max(m, n, l, 1))))
    ppc = max(1, min(int(pairs_per_call), pairs))
    t = [int(W.t) for W in Ws]
    act = np.zeros((N, l), dtype=np.int64)
    for k, W in enumerate(Ws):
        act[k, :] = W.active
    with_c = l > 0 and t_max > 0 and any(t)
    cur = torch.cuda.current_stream(dev)
    Xbuf = torch.empty(N * ppc * 4 * n, dtype=torch.float64, device=dev)
    own = {}                                    # the driver's evaluation buffers, allocated at the first result that needs one

    def resident(name, v, cols, npr):
        if tuple(v.shape) != (N, 4 * npr, cols) or v.dtype != torch.float64 or v.device != dev:
            raise ValueError(f"{name} must return a float64 tensor ({N}, {4 * npr}, {cols}) on {dev}")
        if v.is_contiguous():
            return v
        if name not in own:
            own[name] = torch.empty(N * ppc * 4 * cols, dtype=torch.float64, device=dev)
        out = own[name][: N * npr * 4 * cols].view(N, 4 * npr, cols)
        out.copy_(v)
        return out
    ptr = lambda v: v.data_ptr() if v is not None and v.numel() else 0
    for pair0 in range(0, pairs, ppc):
        npr = min(ppc, pairs - pair0)
        X = Xbuf[: N * npr * 4 * n].view(N, 4 * npr, n)
        cur.synchronize()                       # dx (and the last round's use of X) are complete before the library writes X
        hessian_points_dev(solver, N, n, pair0, npr, dx.data_ptr(), X.data_ptr())
        F = resident("residuals", residuals(X), m, npr) if m > 0 else None
        G = resident("constraints", constraints(X), l, npr) if with_c else None
        cur.synchronize()                       # the evaluations are complete before the library reads them
        hessian_sums_dev(solver, N, m, n, l, t_max, pair0, npr, t, act, slot, dx.data_ptr(), ptr(F), drx.data_ptr() if m else 0,
                         ptr(G), ptr(dlam), dGamma.data_ptr(), int(dGamma.stride(1)), int(dGamma.stride(0)))


def direction_form(solver: GNSolver) -> int:
    """Kernel form of the last direction check on the solver's handle: 0 general, 1 one wave per problem, -1 none yet."""
    return solver._form("enlsip_gn_get_direction_form")


@dataclass
class DirectionRecord:
    """what search_direction_analys leaves in current_iter (:1282-1289) and returns, for one problem"""
    code: int = 0               # method code after :1254-1256; 0: no code was formed (status 1) or the problem was not taken
    dimA: int = 0
    dimJ2: int = 0
    beta: float = float("nan")
    speed: float = float("nan")
    error_code: int = 0         # 0, -3 the Newton step failed (:1268), -4 Newton wanted but no second derivatives (:1276)
    status: int = -1            # of the direction check: 0, 1, 2; -1 not taken
    nb_newton_steps: int = 0    # current_iter.nb_newton_steps after :1266
    taken: bool = False
    subspace_status: int = 0    # status of subspace_direction_batched_dev for this problem
    newton_status: int = 0      # status of newton_direction_batched_dev for this problem


def search_direction_analys_batched_dev(solver: GNSolver, Ws, iters, prevs, bufs, *, m: int, n: int, t_max: int, iter_number,
                                        scaling: bool, rx_sum, hessians=None, hessian_evals=None, take=None, prob0: int = 0):
    """``search_direction_analys`` (:1237-1290) for B problems of one shape whose solve is resident on ``solver`` (problems prob0 ..
    prob0 + B - 1) and whose vectors are in torch device buffers: ``bufs`` maps "p" (B, n), "b" (B, t_max), "d" (B, m), "lam",
    "diag_scale" (B, t_max) and "cx_all" (B, l) to contiguous float64 tensors, as the solve and the multiplier calls left them.
    ``Ws``: the working sets; ``iters``: the current records (restart, add, delete, rankA, rankJ2, dimA, dimJ2,
    nb_newton_steps); ``prevs``: the previous records (code, dimA, dimJ2, t, beta, progress, predicted_reduction, alpha, rx, cx);
    ``iter_number`` and ``rx_sum`` (dot(rx, rx) of the current point): one value or one per problem.
    The check runs first.  Code 1 keeps p, b, d with the ranks as dimensions.  The code -1 problems are the take mask and the
    enlsip_gn_subspace_prev records of ONE subspace_direction_batched_dev call, which overwrites their slots of p, b, d; the code
    goes back to 1 where both chosen dimensions are the ranks (:1254-1256).  The code 2 problems get Gamma = ``hessians(k)`` (n x n,
    r_mat - c_mat; the callback is the caller's) and ONE newton_direction_batched_dev call, which overwrites their slots of p,
    with dimA = -t, dimJ2 = t - n and one more Newton step counted; a Newton status of 1 gives error_code -3.  With ``hessians``
    None, or returning None for a problem, that problem gets error_code -4 and the Gauss-Newton values (:1270-1276).  A problem
    with status 1 (the reference throws at :1231) and one with take 0 are left alone.  Returns one DirectionRecord per problem.
    ``hessian_evals`` = (residuals, constraints), the batched device callbacks of ``hessian_sums_batched_dev``, instead of
    ``hessians``: Gamma of the code 2 problems is formed by that driver from ``bufs["x"]`` (B, n), ``bufs["rx"]`` (B, m) and
    ``bufs["lam"]``, directly in the device tensor the Newton call takes (``bufs["Gamma"]``, (B, n, n), when the caller wants to
    keep it; a buffer of the call otherwise), and nothing of it crosses PCIe.  Passing both is a ValueError."""
    import torch
    if hessians is not None and hessian_evals is not None:
        raise ValueError("hessians and hessian_evals exclude each other")
    B = len(Ws)
    l = Ws[0].l
    if any(W.l != l for W in Ws) or len(iters) != B or len(prevs) != B:
        raise ValueError("one shape per batch: every problem needs the same l, and one current and one previous record per problem")
    itn = np.broadcast_to(np.asarray(iter_number), (B,))
    rxs = np.broadcast_to(np.asarray(rx_sum, dtype=np.float64), (B,))
    tk = np.ones(B, dtype=np.int64) if take is None else GNSolver._host_i64(take, B, "take")
    states = (DirState * B)()
    act, ina = np.zeros((B, l), dtype=np.int64), np.zeros((B, l), dtype=np.int64)
    for k, (W, it, pv) in enumerate(zip(Ws, iters, prevs)):
        act[k, :] = W.active
        ina[k, :len(W.inactive)] = W.inactive
        states[k] = make_state(iter_number=itn[k], restart=it.restart, add=it.add, delete=it.delete, q=W.q, t=W.t, l=l, rankA=it.rankA,
                               dimA=it.dimA, dimJ2=it.dimJ2, prev_code=pv.code, prev_dimJ2=pv.dimJ2, prev_t=pv.t, prev_beta=pv.beta,
                               prev_progress=pv.progress, prev_predicted_reduction=pv.predicted_reduction, prev_alpha=pv.alpha)
    ptr = lambda name: bufs[name].data_ptr() if bufs.get(name) is not None and bufs[name].numel() else 0
    chk = direction_check_batched_dev(solver, B, m, n, l, t_max, states, act, ina, scaling, ptr("b"), ptr("d"), ptr("lam"),
                                      ptr("diag_scale"), ptr("cx_all"), take=tk)
    out = [DirectionRecord() for _ in range(B)]
    for k, (W, it, pv) in enumerate(zip(Ws, iters, prevs)):
        r = out[k]
        r.taken, r.nb_newton_steps = bool(tk[k]), int(it.nb_newton_steps)
        if not tk[k]:
            continue
        r.status = int(chk.status[k])
        if r.status == 1:
            continue
        r.code, r.beta = int(chk.method_code[k]), float(chk.beta[k])
        r.dimA, r.dimJ2 = int(it.rankA), int(it.rankJ2)                                          # :1242-1243, :1275
        with np.errstate(divide="ignore", invalid="ignore"):
            r.speed = float(np.float64(r.beta) / np.float64(pv.beta))                           # :1287
    dev = bufs["p"].device
    sub = chk.take(-1) * tk
    if sub.any():                                                                                # :1249-1256
        prev = GNSolver.pack_subspace_prev(
            B, [abs(pv.dimA) + W.t - pv.t for W, pv in zip(Ws, prevs)], [abs(pv.dimJ2) + pv.t - W.t for W, pv in zip(Ws, prevs)],
            [int(bool(it.restart)) for it in iters], [pv.alpha for pv in prevs],
            [float(np.dot(pv.cx, pv.cx)) - float(chk.sums["active_c_sum"][k]) if sub[k] else 0.0 for k, pv in enumerate(prevs)],
            [float(np.dot(pv.rx, pv.rx)) - float(rxs[k]) if sub[k] else 0.0 for k, pv in enumerate(prevs)])
        dinfo = torch.zeros((B, 6), dtype=torch.int64, device=dev)
        dst = torch.zeros(B, dtype=torch.int32, device=dev)
        solver.subspace_direction_batched_dev(prob0, B, prev, take=sub, dp=ptr("p"), db=ptr("b"), dd=ptr("d"), dinfo=dinfo.data_ptr(),
                                              dstatus=dst.data_ptr())
        info, st = dinfo.cpu().numpy(), dst.cpu().numpy()
        for k in np.nonzero(sub)[0]:
            r = out[k]
            r.subspace_status = int(st[k])
            if st[k] == 5:      # the reference would index out of bounds in choose_subspace_dimensions: nothing was written
                continue
            r.dimA, r.dimJ2 = int(info[k, 3]), int(info[k, 4])
            if r.dimA == iters[k].rankA and r.dimJ2 == iters[k].rankJ2:
                r.code = 1                                                                       # :1254-1256
    newton = chk.take(2) * tk
    dG = None
    if newton.any() and hessian_evals is not None:                                               # :390-393 on the device
        idx = np.nonzero(newton)[0]
        dG = bufs.get("Gamma")
        if dG is None:
            dG = torch.zeros((B, n, n), dtype=torch.float64, device=dev)
        elif tuple(dG.shape) != (B, n, n) or dG.dtype != torch.float64 or not dG.is_contiguous():
            raise ValueError('bufs["Gamma"] must be a contiguous float64 (B, n, n) tensor')
        on = torch.from_numpy(idx).to(dev)
        pick = lambda name: bufs[name].index_select(0, on) if bufs.get(name) is not None and bufs[name].numel() else None
        hessian_sums_batched_dev(solver, [Ws[k] for k in idx], bufs["x"].index_select(0, on), bufs["rx"].index_select(0, on),
                                 pick("lam"), hessian_evals[0], hessian_evals[1], dG, slot=idx)
    elif newton.any():                                                                           # :1259-1277
        G = np.zeros((B, n, n))
        for k in np.nonzero(newton)[0]:
            gam = None if hessians is None else hessians(int(k))
            if gam is None:
                out[k].error_code = -4                                                           # :1270-1276
                newton[k] = 0
                continue
            G[k] = np.asarray(gam, dtype=np.float64).reshape(n, n).T                             # column-major per slot
        if newton.any():
            dG = torch.from_numpy(G).to(dev)
    if newton.any():
        dst = torch.zeros(B, dtype=torch.int32, device=dev)
        solver.newton_direction_batched_dev(prob0, B, dG.data_ptr(), n, n * n, ptr("p"), dst.data_ptr(), take=newton)
        st = dst.cpu().numpy()
        for k in np.nonzero(newton)[0]:
            r = out[k]
            r.newton_status = int(st[k])
            r.dimA, r.dimJ2 = -Ws[k].t, Ws[k].t - n                                              # :1264-1265
            r.nb_newton_steps += 1                                                               # :1266
            if st[k] == 1:
                r.error_code = -3                                                                # :1267-1269
    return out


GNSolver.direction_check_batched_dev = direction_check_batched_dev
GNSolver.direction_form = direction_form
GNSolver.hessian_points_dev = hessian_points_dev
GNSolver.hessian_sums_dev = hessian_sums_dev
GNSolver.hessian_sums_batched_dev = hessian_sums_batched_dev
