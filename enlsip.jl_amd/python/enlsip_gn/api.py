"""Host-side mirror of the reference's interface for the GN subproblem, over the C ABI.

``GNSolver.solve`` has the argument meaning of the reference's
``gn_search_direction(J, rx, cx, F_A, F_L11, rankA, t, ε_rank, iter)`` preceded by the QR lines
of ``update_working_set`` (src/enlsip_functions.jl:206-234, :700, :768-769) and returns the
quantities those lines write into ``Iteration`` (rankA, rankJ2, dimA, dimJ2, b_gn, d_gn) plus the
three ``QRPivoted``-like factor views whose accessors (``.R``, ``.p``, ``Qt_mul``, ``Q_mul``) are
backed by the device-resident factors.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L

SQRT_EPS = math.sqrt(np.finfo(np.float64).eps)


class GNError(RuntimeError):
    pass


def route_names(lib=None) -> list:
    """Every route bit the library knows, in bit order (enlsip_gn_route_name)."""
    lib = lib or L.load()
    names, bit = [], 0
    while True:
        nm = lib.enlsip_gn_route_name(bit)
        if nm is None:
            return names
        names.append(nm.decode())
        bit += 1


def _fptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dptr(x: int):
    """a raw device pointer for the device forms; 0 is NULL"""
    return C.c_void_p(x) if x else None


def determine_solving_dim(previous_dimR: int, rankR: int, predicted_linear_progress: float, obj_progress: float,
                          prelin_previous_dim: float, diagR, y, previous_alpha: float, restart: bool) -> int:
    """determine_solving_dim (src/enlsip_functions.jl:1041-1113) on host data, through the library's host entry point (no GPU):
    the dimension it picks.  Raises IndexError where the reference would index out of bounds (return 5)."""
    dg = np.ascontiguousarray(diagR, dtype=np.float64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    if dg.size < rankR or yv.size < rankR:
        raise ValueError("diagR and y need rankR entries")
    nd = C.c_int64(0)
    rc = L.load().enlsip_gn_determine_solving_dim(int(previous_dimR), int(rankR), float(predicted_linear_progress), float(obj_progress),
                                                  float(prelin_previous_dim), _fptr(dg), _fptr(yv), float(previous_alpha),
                                                  int(bool(restart)), C.byref(nd))
    if rc == 5:
        raise IndexError("determine_solving_dim: the reference indexes tau / rho out of bounds (previous_dimR > rankR)")
    if rc:
        raise GNError(f"enlsip_gn_determine_solving_dim returned {rc}")
    return int(nd.value)


def check_constraint_deletion(q: int, lam, scaling: bool, diag_scale, grad_res: float) -> int:
    """check_constraint_deletion (src/enlsip_functions.jl:574-603) on host data, through the library's host entry point (no GPU):
    the 1-based index of the constraint to delete, 0 for none.  t = len(lam); the routine the batched kernels run."""
    lv = np.ascontiguousarray(lam, dtype=np.float64)
    dv = np.ascontiguousarray(diag_scale, dtype=np.float64)
    t = lv.size
    if dv.size < t:
        raise ValueError("diag_scale needs one entry per multiplier")
    s = C.c_int64(0)
    rc = L.load().enlsip_gn_check_constraint_deletion(int(q), t, _fptr(lv) if t else None, _fptr(dv) if t else None,
                                                      int(bool(scaling)), float(grad_res), C.byref(s))
    if rc:
        raise GNError(f"enlsip_gn_check_constraint_deletion returned {rc}")
    return int(s.value)


def evaluate_violated_constraints(l: int, n: int, q: int, t: int, active, inactive, cx, index_alpha_upp: int):
    """evaluate_violated_constraints (src/enlsip_functions.jl:608-650) on host data, through the library's host entry point (no
    GPU): the routine the batched kernels run.  active / inactive: 1-based, the first t / l - t entries used; shorter arrays
    (the reference's inactive has l - q entries) are zero-padded to l.  Returns (t, active (l,), inactive (l,), added, status);
    status 1: the reference would repeat a swap pass for ever, the lists are in that unchanged state; 2: the pass cap."""
    def padded(x, name):
        a = np.asarray(x).astype(np.int64).ravel()
        if a.size > l:
            raise ValueError(f"{name} has more than l entries")
        return np.ascontiguousarray(np.concatenate([a, np.zeros(l - a.size, dtype=np.int64)]))
    av, iv = padded(active, "active"), padded(inactive, "inactive")
    cv = np.ascontiguousarray(cx, dtype=np.float64)
    if cv.size != l:
        raise ValueError("cx needs l entries")
    tt, added, status = C.c_int64(int(t)), C.c_int64(0), C.c_int64(0)
    p = lambda a: _fptr(a) if a.size else None
    rc = L.load().enlsip_gn_evaluate_violated_constraints(int(l), int(n), int(q), C.byref(tt), p(av), p(iv), p(cv),
                                                          int(index_alpha_upp), C.byref(added), C.byref(status))
    if rc:
        raise GNError(f"enlsip_gn_evaluate_violated_constraints returned {rc}")
    return int(tt.value), av, iv, bool(added.value), int(status.value)


def gather_active_constraints(active, t: int, A, cx, scaling: bool, ldat: Optional[int] = None, out=None):
    """active_C.cx / active_C.A of src/enlsip_functions.jl:2854-2855 with evaluate_scaling! (src/structures.jl:160-178) on host
    data, through the library's host entry point (no GPU): the routine the batched kernels run.  A: (l, n); active: 1-based, the
    first t entries count.  Returns (At (t, ldat): row c is column c of the n x t column-major A' block, cx_active (t,),
    diag_scale (t,)); `out` = (At, cx_active, diag_scale) is written in place (only rows 0..n-1 of a column)."""
    Af = np.asfortranarray(A, dtype=np.float64)
    l, n = Af.shape
    cv = np.ascontiguousarray(cx, dtype=np.float64)
    av = np.ascontiguousarray(np.asarray(active).astype(np.int64))
    if cv.size != l or av.size < t:
        raise ValueError("cx needs l entries and active t")
    ldat = n if ldat is None else int(ldat)
    At, ca, ds = out if out is not None else (np.zeros((t, ldat)), np.zeros(t), np.zeros(t))
    if not (At.flags.c_contiguous and At.dtype == np.float64 and At.shape == (t, ldat)) or ca.size < t or ds.size < t:
        raise ValueError("out must be (At (t, ldat) C-contiguous float64, cx_active (t,), diag_scale (t,))")
    p = lambda a: _fptr(a) if a.size else None
    rc = L.load().enlsip_gn_gather_active_constraints(l, n, int(t), p(av), p(Af), max(l, 1), p(cv), int(bool(scaling)), p(At), ldat,
                                                      p(ca), p(ds))
    if rc:
        raise GNError(f"enlsip_gn_gather_active_constraints returned {rc}")
    return At, ca, ds


def upper_bound_steplength(inactive, n_inactive: int, index_del: int, cx, Ap):
    """upper_bound_steplength (src/enlsip_functions.jl:2149-2178) on host data with Ap = A * p already formed, through the
    library's host entry point (no GPU): (alpha_upp, index_alpha_upp).  inactive: 1-based rows, 0 padding, of which the first
    n_inactive are walked; l = len(cx); the routine the batched kernels run."""
    iv = np.ascontiguousarray(np.asarray(inactive).astype(np.int64))
    cv = np.ascontiguousarray(cx, dtype=np.float64)
    av = np.ascontiguousarray(Ap, dtype=np.float64)
    l = cv.size
    if av.size != l:
        raise ValueError("cx and Ap need l entries each")
    if iv.size < n_inactive:
        raise ValueError("inactive needs n_inactive entries")
    alpha, idx = C.c_double(0.0), C.c_int64(0)
    rc = L.load().enlsip_gn_upper_bound_steplength(l, int(n_inactive), _fptr(iv) if iv.size else None, int(index_del),
                                                   _fptr(cv) if l else None, _fptr(av) if l else None, C.byref(alpha),
                                                   C.byref(idx))
    if rc:
        raise GNError(f"enlsip_gn_upper_bound_steplength returned {rc}")
    return float(alpha.value), int(idx.value)


def penalty_weight_update(w_old, active, t: int, dimA: int, norm_code: int, active_Ap, cx, K, JpJp: float, Jprx: float, rxrx: float):
    """penalty_weight_update (src/enlsip_functions.jl:1545-1629) with psi(0) of :2243 and atwa of :2268 on host data, through the
    library's host entry point (no GPU): the routine the batched kernels run.  active: 1-based constraints of which the first t
    count; active_Ap: t entries of C.A * p (already divided by diag_scale where scaling is on); K: (4, l), updated IN PLACE when it
    is a C-contiguous float64 array (else a copy is updated and returned); Jp and rx enter through the three sums.  Returns
    (w (l,), dpsi0, psi0, atwa, branch, K)."""
    wo = np.ascontiguousarray(w_old, dtype=np.float64)
    l = wo.size
    av = np.ascontiguousarray(np.asarray(active).astype(np.int64))
    ap = np.ascontiguousarray(active_Ap, dtype=np.float64)
    cv = np.ascontiguousarray(cx, dtype=np.float64)
    Kv = K if isinstance(K, np.ndarray) and K.dtype == np.float64 and K.flags.c_contiguous else np.array(K, dtype=np.float64, order="C")
    if Kv.shape != (4, l) or cv.size != l:
        raise ValueError("K must be (4, l) and cx (l,)")
    if av.size < t or ap.size < t:
        raise ValueError("active and active_Ap need t entries")
    w = np.zeros(l)
    sc = np.zeros(3)
    br = C.c_int(0)
    rc = L.load().enlsip_gn_penalty_weight_update(l, int(t), _fptr(av) if av.size else None, int(dimA), int(norm_code),
                                                  _fptr(wo) if l else None, _fptr(ap) if ap.size else None, _fptr(cv) if l else None,
                                                  float(JpJp), float(Jprx), float(rxrx), _fptr(Kv) if l else None,
                                                  _fptr(w) if l else None, _fptr(sc), C.byref(br))
    if rc:
        raise GNError(f"enlsip_gn_penalty_weight_update returned {rc}")
    return w, float(sc[0]), float(sc[1]), float(sc[2]), int(br.value), Kv


def linesearch_coefficients(active, t: int, inactive, n_inactive: int, rx, rx_new, Jp, cx, cx_new, Ap, w, alpha_k: float) -> np.ndarray:
    """The six dot products v0.v0, v0.v1, v0.v2, v1.v1, v1.v2, v2.v2 of coefficients_linesearch! (src/enlsip_functions.jl:1665-1689)
    with the scaling of v1 = [Jp; Ap] (:1986-1998) on host data, through the library's host entry point (no GPU).  active / inactive:
    1-based constraints of which the first t / n_inactive count (t + n_inactive == l); Ap is the UNSCALED A * p.  No vector is
    built and nothing is written; the terms are added in the order residuals, active list, inactive list."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    rx, rx_new, Jp, cx, cx_new, Ap, w = (f(a) for a in (rx, rx_new, Jp, cx, cx_new, Ap, w))
    m, l = rx.size, cx.size
    if rx_new.size != m or Jp.size != m or cx_new.size != l or Ap.size != l or w.size != l:
        raise ValueError("rx, rx_new, Jp need m entries each and cx, cx_new, Ap, w l entries each")
    av = np.ascontiguousarray(np.asarray(active).astype(np.int64))
    iv = np.ascontiguousarray(np.asarray(inactive).astype(np.int64))
    if av.size < t or iv.size < n_inactive:
        raise ValueError("active needs t entries and inactive n_inactive")
    sums = np.zeros(6)
    p = lambda a: _fptr(a) if a.size else None
    rc = L.load().enlsip_gn_linesearch_coefficients(m, l, int(t), p(av), p(iv), int(n_inactive), p(rx), p(rx_new), p(Jp), p(cx),
                                                    p(cx_new), p(Ap), p(w), float(alpha_k), _fptr(sums))
    if rc:
        raise GNError(f"enlsip_gn_linesearch_coefficients returned {rc}")
    return sums


def linesearch_fit(sums, alpha_k: float, x_min: float, alpha_min: float, alpha_max: float):
    """minrm (src/enlsip_functions.jl:1841-1862) on the six sums and the choice of :2023-2026, through the library's host entry
    point (no GPU).  Returns (out (6,): alpha_kp1, pk, alpha_hat, s_alpha, beta_hat, s_beta; arm: 0 Newton-Raphson, 1 one root,
    2 two roots)."""
    sv = np.ascontiguousarray(sums, dtype=np.float64)
    if sv.size != 6:
        raise ValueError("sums needs 6 entries")
    out = np.zeros(6)
    arm = C.c_int(0)
    rc = L.load().enlsip_gn_linesearch_fit(_fptr(sv), float(alpha_k), float(x_min), float(alpha_min), float(alpha_max), _fptr(out),
                                           C.byref(arm))
    if rc:
        raise GNError(f"enlsip_gn_linesearch_fit returned {rc}")
    return out, int(arm.value)


def minrn(x1, y1, x2, y2, x3, y3, alpha_min, alpha_max, p_max):
    """minrn (src/enlsip_functions.jl:1708-1735) through the library's host entry point (no GPU): (alpha, p_alpha)."""
    a, pa = C.c_double(0.0), C.c_double(0.0)
    rc = L.load().enlsip_gn_minrn(float(x1), float(y1), float(x2), float(y2), float(x3), float(y3), float(alpha_min),
                                  float(alpha_max), float(p_max), C.byref(a), C.byref(pa))
    if rc:
        raise GNError(f"enlsip_gn_minrn returned {rc}")
    return float(a.value), float(pa.value)


def check_reduction(psi_alpha, psi_k, approx_k, eta, diff_psi) -> bool:
    """check_reduction (src/enlsip_functions.jl:1870-1886) through the library's host entry point (no GPU)."""
    likely = C.c_int(0)
    rc = L.load().enlsip_gn_check_reduction(float(psi_alpha), float(psi_k), float(approx_k), float(eta), float(diff_psi),
                                            C.byref(likely))
    if rc:
        raise GNError(f"enlsip_gn_check_reduction returned {rc}")
    return bool(likely.value)


@dataclass
class GNResult:
    p: np.ndarray
    b: np.ndarray
    d: np.ndarray
    rankA: int
    rankJ2: int
    code: int
    dimA: int
    dimJ2: int
    status: int
    jpvtA: np.ndarray
    jpvtL: np.ndarray
    jpvtJ2: np.ndarray


class FactorView:
    """QRPivoted-like view of one resident factorisation (valid until the next solve)."""

    def __init__(self, solver: "GNSolver", which: int, prob: int = 0):
        self._s, self._which, self._prob = solver, which, prob

    @property
    def shape(self):
        r, c = C.c_int64(), C.c_int64()
        self._s._chk(self._s._lib.enlsip_gn_factor_shape(self._s._h, self._which, self._prob, C.byref(r), C.byref(c)))
        return int(r.value), int(c.value)

    @property
    def R(self) -> np.ndarray:
        r, c = self.shape
        out = np.zeros((max(r, 1), c), order="F")
        self._s._chk(self._s._lib.enlsip_gn_get_R(self._s._h, self._which, self._prob, _fptr(out), max(r, 1)))
        return out[:r, :]

    def diagR(self) -> np.ndarray:
        r, c = self.shape
        out = np.zeros(min(r, c))
        if out.size:
            self._s._chk(self._s._lib.enlsip_gn_get_diagR(self._s._h, self._which, self._prob, _fptr(out)))
        return out

    @property
    def p(self) -> np.ndarray:
        _, c = self.shape
        out = np.zeros(c, dtype=np.int64)
        if c:
            self._s._chk(self._s._lib.enlsip_gn_get_jpvt(self._s._h, self._which, self._prob, _fptr(out)))
        return out

    def Qt_mul(self, v: np.ndarray) -> np.ndarray:
        out = np.array(v, dtype=np.float64, copy=True)
        self._s._chk(self._s._lib.enlsip_gn_apply_qt(self._s._h, self._which, self._prob, _fptr(out)))
        return out

    def Q_mul(self, v: np.ndarray) -> np.ndarray:
        out = np.array(v, dtype=np.float64, copy=True)
        self._s._chk(self._s._lib.enlsip_gn_apply_q(self._s._h, self._which, self._prob, _fptr(out)))
        return out


class GNSolver:
    """One handle = one HIP stream + device workspace (not thread-safe)."""

    def __init__(self, device: int = -1, flags: int = 0, tile_rows: int = 0, stream: int = 0):
        self._lib = L.load()
        self._h = C.c_void_p()
        self._device = device       # -1: the current device
        self._resident_m = None     # rows of the last ragged host-form solve made through this object (solve_changed_batched)
        opts = L.Opts(device=device, flags=flags, panel_width=0, tile_rows=tile_rows,
                      stream=C.c_void_p(stream) if stream else None)
        rc = self._lib.enlsip_gn_create(C.byref(self._h), C.byref(opts))
        if rc != 0:
            msg = self._lib.enlsip_gn_last_error(None)
            raise GNError(f"enlsip_gn_create failed with code {rc}: {msg.decode() if msg else 'no usable HIP device?'}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.enlsip_gn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != 0:
            msg = self._lib.enlsip_gn_last_error(self._h)
            raise GNError(f"libenlsip_gn error {rc}: {msg.decode() if msg else ''}")

    # ---- single problem, host buffers -------------------------------------------------------
    def solve(self, J: np.ndarray, rx: np.ndarray, A_active: np.ndarray, cx: np.ndarray,
              eps_rank: float = SQRT_EPS, dimA: int = -1, dimJ2: int = -1) -> GNResult:
        """A_active is the t x n active-constraint Jacobian (the reference's ``C.A``)."""
        J = np.asfortranarray(J, dtype=np.float64)
        m, n = J.shape
        A_active = np.asarray(A_active, dtype=np.float64).reshape(-1, n)
        t = A_active.shape[0]
        At = np.asfortranarray(A_active.T)                  # n x t column-major
        rx = np.ascontiguousarray(rx, dtype=np.float64)
        cx = np.ascontiguousarray(cx, dtype=np.float64)
        kA = min(n, t)
        p, b, d = np.zeros(n), np.zeros(t), np.zeros(m)
        jA, jL, jJ = np.zeros(t, np.int64), np.zeros(kA, np.int64), np.zeros(n, np.int64)
        info = L.Info()
        self._chk(self._lib.enlsip_gn_solve(self._h, m, n, t, _fptr(J), m, _fptr(rx), _fptr(At) if t else None,
                                            max(n, 1), _fptr(cx) if t else None, eps_rank, dimA, dimJ2,
                                            _fptr(p), _fptr(b), _fptr(d), C.byref(info),
                                            _fptr(jA), _fptr(jL), _fptr(jJ)))
        n2 = n - int(info.rankA)
        return GNResult(p, b, d, int(info.rankA), int(info.rankJ2), int(info.code), int(info.dimA),
                        int(info.dimJ2), int(info.status), jA, jL, jJ[:n2].copy())

    # ---- batch, host buffers ----------------------------------------------------------------
    def factor_constraints(self, m: int, A: np.ndarray, cx: np.ndarray, eps_rank: float = SQRT_EPS):
        """Constraint stage alone (src/enlsip_functions.jl:700, :768-769): F_A, rankA, F_L11 left resident for
        first_lagrange (pass grad_fx) and the F_A / F_L11 accessors.  A: (t, n) active constraint Jacobian; m: rows of the
        solve that follows.  Returns (rankA, code, dimA)."""
        A = np.asarray(A, dtype=np.float64)
        t, n = (A.shape if A.size else (0, A.shape[1] if A.ndim == 2 else 0))
        At = np.ascontiguousarray(A) if t else None          # (t, n) C-order == column-major n x t
        cxv = np.ascontiguousarray(cx, dtype=np.float64) if t else None
        info = L.Info()
        self._chk(self._lib.enlsip_gn_factor_constraints(self._h, m, n, t, _fptr(At) if t else None, max(n, 1),
                                                         _fptr(cxv) if t else None, eps_rank, C.byref(info)))
        return int(info.rankA), int(info.code), int(info.dimA)

    def solve_factored(self, J: np.ndarray, rx: np.ndarray, t: int, eps_rank: float = SQRT_EPS, dimJ2: int = -1) -> GNResult:
        """The solve right after factor_constraints with an unchanged working set (src/enlsip_functions.jl:768-771 reuses the
        F_A of :700): only J and rx go in."""
        J = np.asfortranarray(J, dtype=np.float64)
        m, n = J.shape
        rx = np.ascontiguousarray(rx, dtype=np.float64)
        kA = min(n, t)
        p, b, d = np.zeros(n), np.zeros(t), np.zeros(m)
        jA, jL, jJ = np.zeros(t, np.int64), np.zeros(kA, np.int64), np.zeros(n, np.int64)
        info = L.Info()
        self._chk(self._lib.enlsip_gn_solve_factored(self._h, m, n, t, _fptr(J), m, _fptr(rx), eps_rank, dimJ2,
                                                     _fptr(p), _fptr(b), _fptr(d), C.byref(info), _fptr(jA), _fptr(jL), _fptr(jJ)))
        n2 = n - int(info.rankA)
        return GNResult(p, b, d, int(info.rankA), int(info.rankJ2), int(info.code), int(info.dimA),
                        int(info.dimJ2), int(info.status), jA, jL, jJ[:n2].copy())

    def solve_batched(self, J: np.ndarray, rx: np.ndarray, At: np.ndarray, cx: np.ndarray,
                      eps_rank: float = SQRT_EPS):
        """J: (batch, n, m) C-order array holding each m x n problem column-major (i.e. J[k].T is
        the matrix), rx: (batch, m), At: (batch, t, n) C-order = column-major n x t, cx: (batch, t)."""
        batch, n, m = J.shape
        t = At.shape[1] if At is not None and At.size else 0
        kA = min(n, t)
        J = np.ascontiguousarray(J, dtype=np.float64)
        rx = np.ascontiguousarray(rx, dtype=np.float64)
        p, b, d = np.zeros((batch, n)), np.zeros((batch, t)), np.zeros((batch, m))
        jA = np.zeros((batch, t), np.int64)
        jL = np.zeros((batch, kA), np.int64)
        jJ = np.zeros((batch, n), np.int64)
        info = (L.Info * batch)()
        if t:
            At = np.ascontiguousarray(At, dtype=np.float64)
            cx = np.ascontiguousarray(cx, dtype=np.float64)
        self._chk(self._lib.enlsip_gn_solve_batched(
            self._h, batch, m, n, t, _fptr(J), m, m * n, _fptr(rx), _fptr(At) if t else None, max(n, 1), n * t,
            _fptr(cx) if t else None, eps_rank, _fptr(p), _fptr(b), _fptr(d),
            C.cast(info, C.c_void_p), _fptr(jA), _fptr(jL), _fptr(jJ)))
        infos = [(int(i.rankA), int(i.rankJ2), int(i.code), int(i.dimA), int(i.dimJ2), int(i.status)) for i in info]
        return p, b, d, infos, jA, jL, jJ

    # ---- ragged batch: one working-set size per problem (src/enlsip_functions.jl:686-795) ---------
    @staticmethod
    def pack_ragged(As, cxs, n: Optional[int] = None):
        """Each problem's own active Jacobian A_k (t_k x n) and cx_k (t_k) -> the padded layout of solve_batched_ragged:
        At (batch, t_max, n), cx (batch, t_max) with zeros past t_k, and t (int64).  n is taken from the 2-D A_k; pass it when
        no A_k carries it (an empty batch, or every A_k empty and 1-D)."""
        As = [np.asarray(A, dtype=np.float64) for A in As]
        if len(As) != len(cxs):
            raise ValueError(f"pack_ragged: {len(As)} matrices but {len(cxs)} cx vectors")
        widths = {A.shape[1] for A in As if A.ndim == 2}
        if n is None:
            if not widths:
                raise ValueError("pack_ragged: n cannot be inferred (no 2-D A_k); pass n")
            if len(widths) > 1:
                raise ValueError(f"pack_ragged: the A_k have different column counts {sorted(widths)}")
            n = widths.pop()
        elif widths - {n}:
            raise ValueError(f"pack_ragged: A_k with {sorted(widths - {n})} columns, n = {n}")
        for A in As:
            if A.size and A.ndim != 2:
                raise ValueError("pack_ragged: every non-empty A_k must be a t_k x n matrix")
        t = np.array([A.shape[0] if A.size else 0 for A in As], dtype=np.int64)
        t_max = int(t.max()) if len(t) else 0
        At = np.zeros((len(As), t_max, n))
        cx = np.zeros((len(As), t_max))
        for k, (A, c) in enumerate(zip(As, cxs)):
            if t[k]:
                At[k, :t[k]] = A
                cx[k, :t[k]] = np.asarray(c, dtype=np.float64)
        return At, cx, t

    def solve_batched_ragged(self, J: np.ndarray, rx: np.ndarray, At: np.ndarray, cx: np.ndarray, t,
                             eps_rank: float = SQRT_EPS):
        """Like solve_batched, with problem k's own t[k] <= t_max: At (batch, t_max, n) and cx (batch, t_max) are padded
        (pack_ragged builds them); rows past t[k] are not read.  Outputs have the t_max layout with zeros past t[k]."""
        batch, n, m = J.shape
        self._resident_m = m
        t = np.ascontiguousarray(t, dtype=np.int64)
        t_max = At.shape[1] if At is not None and At.ndim == 3 else 0
        kA = min(n, t_max)
        J = np.ascontiguousarray(J, dtype=np.float64)
        rx = np.ascontiguousarray(rx, dtype=np.float64)
        p, b, d = np.zeros((batch, n)), np.zeros((batch, t_max)), np.zeros((batch, m))
        jA = np.zeros((batch, t_max), np.int64)
        jL = np.zeros((batch, kA), np.int64)
        jJ = np.zeros((batch, n), np.int64)
        info = (L.Info * batch)()
        if t_max:
            At = np.ascontiguousarray(At, dtype=np.float64)
            cx = np.ascontiguousarray(cx, dtype=np.float64)
        self._chk(self._lib.enlsip_gn_solve_batched_ragged(
            self._h, batch, m, n, t_max, t.ctypes.data_as(C.c_void_p), _fptr(J), m, m * n, _fptr(rx),
            _fptr(At) if t_max else None, max(n, 1), n * t_max, _fptr(cx) if t_max else None, eps_rank,
            _fptr(p), _fptr(b), _fptr(d), C.cast(info, C.c_void_p), _fptr(jA), _fptr(jL), _fptr(jJ)))
        infos = [(int(i.rankA), int(i.rankJ2), int(i.code), int(i.dimA), int(i.dimJ2), int(i.status)) for i in info]
        return p, b, d, infos, jA, jL, jJ

    def solve_batched_ragged_dev(self, batch, m, n, t_max, t, dJ, ldj, strideJ, drx, dAt, ldat, strideAt, dcx,
                                 eps_rank=SQRT_EPS, dp=0, db=0, dd=0, dinfo=0, djA=0, djL=0, djJ=0):
        """Device pointers as solve_batched_dev; t stays a host array of batch entries."""
        t = np.ascontiguousarray(t, dtype=np.int64)
        self._chk(self._lib.enlsip_gn_solve_batched_ragged_dev(
            self._h, batch, m, n, t_max, t.ctypes.data_as(C.c_void_p), _dptr(dJ), ldj, strideJ, _dptr(drx), _dptr(dAt), ldat,
            strideAt, _dptr(dcx), eps_rank, _dptr(dp), _dptr(db), _dptr(dd), _dptr(dinfo), _dptr(djA), _dptr(djL), _dptr(djJ)))

    # ---- batched constraint stage and the solve that goes on with it (src/enlsip_functions.jl:700-704, then :725 / :771) ----------
    @staticmethod
    def _ragged_A(At, cx, t, n: Optional[int] = None):
        """Checked (At (batch, t_max, n) float64 C-order, cx (batch, t_max), t int64 (batch,)) of the padded ragged layout."""
        At = np.asarray(At, dtype=np.float64)
        if At.ndim != 3:
            raise ValueError("At must be (batch, t_max, n) (pack_ragged builds it)")
        batch, t_max, nn = At.shape
        if n is not None and nn != n:
            raise ValueError(f"At has {nn} columns per constraint, J has n = {n}")
        cx = np.asarray(cx, dtype=np.float64)
        if cx.shape != (batch, t_max):
            raise ValueError(f"cx must be ({batch}, {t_max}), got {cx.shape}")
        t = np.full(batch, t_max, dtype=np.int64) if t is None else np.ascontiguousarray(t, dtype=np.int64)
        if t.shape != (batch,):
            raise ValueError(f"t must have {batch} entries")
        if np.any(t < 0) or np.any(t > t_max):
            raise ValueError(f"every t[k] must lie in 0..t_max = {t_max}")
        return np.ascontiguousarray(At), np.ascontiguousarray(cx), t

    @staticmethod
    def _refactor_mask(refactor, batch: int):
        if refactor is None:
            return None
        r = np.ascontiguousarray(np.asarray(refactor).astype(np.int64))
        if r.shape != (batch,):
            raise ValueError(f"refactor must have {batch} entries")
        return r

    @staticmethod
    def _changed_mask(changed, batch: int):
        c = None if changed is None else np.ascontiguousarray(np.asarray(changed).astype(np.int64))
        if c is None or c.shape != (batch,):
            raise ValueError(f"changed must have {batch} entries")
        return c

    def factor_constraints_batched(self, m: int, At: np.ndarray, cx: np.ndarray, t=None, eps_rank: float = SQRT_EPS):
        """Constraint stage of a whole ragged batch, nothing about J: At (batch, t_max, n), cx (batch, t_max), t (batch,) or None
        (all t_max), m: rows of the solve that follows.  Leaves F_A, F_L11 of every problem resident (first_lagrange_batched with
        grad_fx, the F_A / F_L11 accessors).  Returns [(rankA, code, dimA), ...]."""
        At, cx, t = self._ragged_A(At, cx, t)
        batch, t_max, n = At.shape
        if batch < 1:
            raise ValueError("batch must be >= 1")
        info = (L.Info * batch)()
        self._chk(self._lib.enlsip_gn_factor_constraints_batched(
            self._h, batch, m, n, t_max, _fptr(t), _fptr(At) if t_max else None, max(n, 1), n * t_max,
            _fptr(cx) if t_max else None, eps_rank, C.cast(info, C.c_void_p)))
        return [(int(i.rankA), int(i.code), int(i.dimA)) for i in info]

    def factor_constraints_batched_dev(self, batch, m, n, t_max, t, dAt, ldat, strideAt, dcx, eps_rank=SQRT_EPS, dinfo=0):
        """Device pointers; t stays a host array of batch entries (None: all t_max)."""
        if t is not None:
            t = np.ascontiguousarray(t, dtype=np.int64)
            if t.shape != (batch,):
                raise ValueError(f"t must have {batch} entries")
        self._chk(self._lib.enlsip_gn_factor_constraints_batched_dev(
            self._h, batch, m, n, t_max, _fptr(t), _dptr(dAt), ldat, strideAt, _dptr(dcx), eps_rank, _dptr(dinfo)))

    def solve_factored_batched(self, J: np.ndarray, rx: np.ndarray, At: np.ndarray, cx: np.ndarray, t=None, refactor=None,
                               eps_rank: float = SQRT_EPS):
        """The Jacobian side right after factor_constraints_batched: arguments and results as solve_batched_ragged, plus
        refactor (batch,) flags or None.  A problem without a flag keeps its constraint stage (its t[k] must be the factored
        one, its At / cx rows are not read); a flagged problem gets its stage again from its At / cx rows and t[k]."""
        J = np.asarray(J, dtype=np.float64)
        if J.ndim != 3:
            raise ValueError("J must be (batch, n, m)")
        batch, n, m = J.shape
        At, cx, t = self._ragged_A(At, cx, t, n)
        if At.shape[0] != batch:
            raise ValueError(f"At holds {At.shape[0]} problems, J {batch}")
        rx = np.ascontiguousarray(rx, dtype=np.float64)
        if rx.shape != (batch, m):
            raise ValueError(f"rx must be ({batch}, {m})")
        r = self._refactor_mask(refactor, batch)
        self._resident_m = m
        t_max = At.shape[1]
        kA = min(n, t_max)
        J = np.ascontiguousarray(J)
        p, b, d = np.zeros((batch, n)), np.zeros((batch, t_max)), np.zeros((batch, m))
        jA = np.zeros((batch, t_max), np.int64)
        jL = np.zeros((batch, kA), np.int64)
        jJ = np.zeros((batch, n), np.int64)
        info = (L.Info * batch)()
        self._chk(self._lib.enlsip_gn_solve_factored_batched(
            self._h, batch, m, n, t_max, _fptr(t), _fptr(r), _fptr(J), m, m * n, _fptr(rx),
            _fptr(At) if t_max else None, max(n, 1), n * t_max, _fptr(cx) if t_max else None, eps_rank,
            _fptr(p), _fptr(b), _fptr(d), C.cast(info, C.c_void_p), _fptr(jA), _fptr(jL), _fptr(jJ)))
        infos = [(int(i.rankA), int(i.rankJ2), int(i.code), int(i.dimA), int(i.dimJ2), int(i.status)) for i in info]
        return p, b, d, infos, jA, jL, jJ

    def solve_factored_batched_dev(self, batch, m, n, t_max, t, refactor, dJ, ldj, strideJ, drx, dAt, ldat, strideAt, dcx,
                                   eps_rank=SQRT_EPS, dp=0, db=0, dd=0, dinfo=0, djA=0, djL=0, djJ=0):
        """Device pointers as solve_batched_ragged_dev; t and refactor stay host arrays.  dAt, ldat, strideAt, dcx are those of
        factor_constraints_batched_dev, the flagged problems' slots rewritten in place."""
        if t is not None:
            t = np.ascontiguousarray(t, dtype=np.int64)
            if t.shape != (batch,):
                raise ValueError(f"t must have {batch} entries")
        r = self._refactor_mask(refactor, batch)
        self._chk(self._lib.enlsip_gn_solve_factored_batched_dev(
            self._h, batch, m, n, t_max, _fptr(t), _fptr(r), _dptr(dJ), ldj, strideJ, _dptr(drx), _dptr(dAt), ldat, strideAt,
            _dptr(dcx), eps_rank, _dptr(dp), _dptr(db), _dptr(dd), _dptr(dinfo), _dptr(djA), _dptr(djL), _dptr(djJ)))

    def constraint_refactored(self) -> int:
        """Problems the constraint kernels of the last factor_constraints_batched / solve_factored_batched were launched over."""
        c = C.c_int64(0)
        self._chk(self._lib.enlsip_gn_get_constraint_refactored(self._h, C.byref(c)))
        return int(c.value)

    # ---- only the problems whose working set changed, in place (src/enlsip_functions.jl:728-743, :745-762, :773-790) -------------
    def solve_changed_batched(self, At: np.ndarray, cx: np.ndarray, t, changed, eps_rank: float = SQRT_EPS, m: Optional[int] = None):
        """On the fully solved ragged batch this solver's last host-form solve left resident (solve_batched_ragged,
        solve_factored_batched, or this call): the problems with a changed flag again, constraint stage and Jacobian side, from
        the resident J, rx and their At / cx rows and t[k]; nothing of another problem is touched.  At (batch, t_max, n) and
        cx (batch, t_max) in the resident layout (rows of unflagged problems are not read), t (batch,), changed (batch,) flags.
        Returns the tuple of solve_batched_ragged; the slots of unflagged problems are left as they are made here: NaN in p, b, d,
        zero in the pivots and the info records.  m: rows of the resident problems; needed only when they were not solved
        through this object's solve_batched_ragged / solve_factored_batched (which remember it)."""
        At, cx, t = self._ragged_A(At, cx, t)
        batch, t_max, n = At.shape
        if batch < 1:
            raise ValueError("batch must be >= 1")
        ch = self._changed_mask(changed, batch)
        m = m if m is not None else self._resident_m
        if m is None:
            raise ValueError("solve_changed_batched: no ragged host-form solve was made through this object: pass m= (the rows "
                             "of the resident problems)")
        kA = min(n, t_max)
        p, b, d = np.full((batch, n), np.nan), np.full((batch, t_max), np.nan), np.full((batch, m), np.nan)
        jA = np.zeros((batch, t_max), np.int64)
        jL = np.zeros((batch, kA), np.int64)
        jJ = np.zeros((batch, n), np.int64)
        info = (L.Info * batch)()
        self._chk(self._lib.enlsip_gn_solve_changed_batched(
            self._h, batch, m, n, t_max, _fptr(t), _fptr(ch), _fptr(At) if t_max else None, max(n, 1), n * t_max,
            _fptr(cx) if t_max else None, eps_rank, _fptr(p), _fptr(b), _fptr(d), C.cast(info, C.c_void_p), _fptr(jA), _fptr(jL),
            _fptr(jJ)))
        infos = [(int(i.rankA), int(i.rankJ2), int(i.code), int(i.dimA), int(i.dimJ2), int(i.status)) for i in info]
        return p, b, d, infos, jA, jL, jJ

    def solve_changed_batched_dev(self, batch, m, n, t_max, t, changed, dAt, ldat, strideAt, dcx, eps_rank=SQRT_EPS, dp=0, db=0, dd=0,
                                  dinfo=0, djA=0, djL=0, djJ=0):
        """Device pointers; t and changed stay host arrays.  dAt, ldat, strideAt, dcx are the buffers of the resident solve, the
        flagged problems' slots rewritten in place; only the flagged problems' output slots are written."""
        t = np.ascontiguousarray(t, dtype=np.int64)
        if t.shape != (batch,):
            raise ValueError(f"t must have {batch} entries")
        ch = self._changed_mask(changed, batch)
        self._chk(self._lib.enlsip_gn_solve_changed_batched_dev(
            self._h, batch, m, n, t_max, _fptr(t), _fptr(ch), _dptr(dAt), ldat, strideAt, _dptr(dcx), eps_rank, _dptr(dp), _dptr(db),
            _dptr(dd), _dptr(dinfo), _dptr(djA), _dptr(djL), _dptr(djJ)))

    def jacobian_resolved(self) -> int:
        """Problems the Jacobian-side kernels of the last solve were launched over (both pipelined halves): batch after a
        whole-batch solve, the number of flags after solve_changed_batched."""
        c = C.c_int64(0)
        self._chk(self._lib.enlsip_gn_get_jacobian_resolved(self._h, C.byref(c)))
        return int(c.value)

    # ---- batch, device buffers (raw pointers, e.g. torch tensor .data_ptr()) ------------------
    def solve_batched_dev(self, batch, m, n, t, dJ, ldj, strideJ, drx, dAt, ldat, strideAt, dcx,
                          eps_rank=SQRT_EPS, dp=0, db=0, dd=0, dinfo=0, djA=0, djL=0, djJ=0):
        self._chk(self._lib.enlsip_gn_solve_batched_dev(
            self._h, batch, m, n, t, _dptr(dJ), ldj, strideJ, _dptr(drx), _dptr(dAt), ldat, strideAt, _dptr(dcx), eps_rank,
            _dptr(dp), _dptr(db), _dptr(dd), _dptr(dinfo), _dptr(djA), _dptr(djL), _dptr(djJ)))

    # ---- resident factors ---------------------------------------------------------------------
    def factor(self, which: int, prob: int = 0) -> FactorView:
        return FactorView(self, which, prob)

    def JQ1(self, m: int, n: int, prob: int = 0) -> np.ndarray:
        out = np.zeros((m, n), order="F")
        self._chk(self._lib.enlsip_gn_get_JQ1(self._h, prob, _fptr(out), m))
        return out

    def resolve(self, m: int, n: int, t: int, dimA: int, dimJ2: int, code: int = -1, prob: int = 0):
        """sub_search_direction re-entry on the resident factors (src/enlsip_functions.jl:1253)."""
        p, b, d = np.zeros(n), np.zeros(t), np.zeros(m)
        self._chk(self._lib.enlsip_gn_resolve(self._h, prob, dimA, dimJ2, code, _fptr(p), _fptr(b), _fptr(d)))
        return p, b, d

    # ---- multiplier estimates on the resident data (src/enlsip_functions.jl:461-537, :2690) -----------
    def gradient(self, n: int, prob: int = 0) -> np.ndarray:
        g = np.zeros(n)
        self._chk(self._lib.enlsip_gn_gradient(self._h, prob, _fptr(g)))
        return g

    def jacobian_times(self, m: int, t: int, p: np.ndarray, prob: int = 0):
        """(J p, A_active p) of the last solve's J and A (src/enlsip_functions.jl:2226-2229)."""
        pv = np.ascontiguousarray(p, dtype=np.float64)
        Jp, Ap = np.zeros(m), np.zeros(t)
        self._chk(self._lib.enlsip_gn_jacobian_times(self._h, prob, _fptr(pv), _fptr(Jp), _fptr(Ap) if t else None))
        return Jp, Ap

    def full_constraints_times(self, A: np.ndarray, p: np.ndarray) -> np.ndarray:
        """A p with the FULL constraint Jacobian (l x n), src/enlsip_functions.jl:2227."""
        Af = np.asfortranarray(A, dtype=np.float64)
        l, n = Af.shape
        pv = np.ascontiguousarray(p, dtype=np.float64)
        Ap = np.zeros(l)
        if l:
            self._chk(self._lib.enlsip_gn_full_constraints_times(self._h, l, n, _fptr(Af), l, _fptr(pv), _fptr(Ap)))
        return Ap

    def matrix_times_QA(self, M: np.ndarray, prob: int = 0) -> np.ndarray:
        """M * F_A.Q for a host matrix with the row count of the last solve (`J * F_A.Q`, src/enlsip_functions.jl:526, :1249)."""
        Mf = np.asfortranarray(M, dtype=np.float64)
        rows, n = Mf.shape
        out = np.zeros((rows, n), order="F")
        self._chk(self._lib.enlsip_gn_matrix_times_QA(self._h, prob, rows, _fptr(Mf), max(rows, 1), _fptr(out), max(rows, 1)))
        return out

    def first_lagrange(self, t: int, grad_fx: Optional[np.ndarray] = None, diag_scale: Optional[np.ndarray] = None,
                       eps_rank: float = SQRT_EPS, prob: int = 0):
        """first_lagrange_mult_estimate!: returns (lambda, grad_res)."""
        lam = np.zeros(t)
        gres = C.c_double(0.0)
        g = None if grad_fx is None else np.ascontiguousarray(grad_fx, dtype=np.float64)
        ds = None if diag_scale is None else np.ascontiguousarray(diag_scale, dtype=np.float64)
        self._chk(self._lib.enlsip_gn_first_lagrange(self._h, prob, _fptr(g), _fptr(ds), eps_rank, _fptr(lam),
                                                     C.byref(gres)))
        return lam, float(gres.value)

    def second_lagrange(self, t: int, p_gn: np.ndarray, diag_scale: Optional[np.ndarray] = None,
                        eps_rank: float = SQRT_EPS, prob: int = 0) -> np.ndarray:
        """second_lagrange_mult_estimate!: lambda from the resident J1 = (J*F_A.Q)[:, 1:t]."""
        lam = np.zeros(t)
        p = np.ascontiguousarray(p_gn, dtype=np.float64)
        ds = None if diag_scale is None else np.ascontiguousarray(diag_scale, dtype=np.float64)
        self._chk(self._lib.enlsip_gn_second_lagrange(self._h, prob, _fptr(p), _fptr(ds), eps_rank, _fptr(lam)))
        return lam

    # ---- the same consumers over a range of the resident batch (one call, a fixed number of launches) ----------------------
    # Slot j of every array holds problem prob0 + j; lambda / Ap have t_max entries per problem (zero past a ragged problem's t).
    # The estimates return per-problem status (0, 1 singular triangular system, 2 pseudo-rank beyond the solve's rank).
    def _chk_batched(self, rc: int) -> int:
        if rc < 0 or rc > 1:
            self._chk(rc)
        return rc

    def gradient_batched(self, n: int, prob0: int = 0, count: int = 1) -> np.ndarray:
        """J' rx of problems prob0 .. prob0+count-1: (count, n)."""
        g = np.zeros((count, n))
        self._chk(self._lib.enlsip_gn_gradient_batched(self._h, prob0, count, _fptr(g)))
        return g

    def jacobian_times_batched(self, m: int, t_max: int, p: np.ndarray, prob0: int = 0, jp: bool = True, ap: bool = True):
        """(J p, A_active p) per problem; p: (count, n).  Returns (Jp (count, m) or None, Ap (count, t_max) or None)."""
        pv = np.ascontiguousarray(p, dtype=np.float64)
        count = pv.shape[0]
        Jp = np.zeros((count, m)) if jp else None
        Ap = np.zeros((count, t_max)) if ap else None
        self._chk(self._lib.enlsip_gn_jacobian_times_batched(self._h, prob0, count, _fptr(pv), _fptr(Jp), _fptr(Ap)))
        return Jp, Ap

    def first_lagrange_batched(self, t_max: int, prob0: int = 0, count: int = 1, grad_fx: Optional[np.ndarray] = None,
                               diag_scale: Optional[np.ndarray] = None, eps_rank: float = SQRT_EPS):
        """first_lagrange_mult_estimate! per problem: (lambda (count, t_max), grad_res (count,), status (count,), rc)."""
        g = None if grad_fx is None else np.ascontiguousarray(grad_fx, dtype=np.float64)
        ds = None if diag_scale is None else np.ascontiguousarray(diag_scale, dtype=np.float64)
        lam, gres, st = np.zeros((count, t_max)), np.zeros(count), np.zeros(count, dtype=np.int32)
        rc = self._chk_batched(self._lib.enlsip_gn_first_lagrange_batched(
            self._h, prob0, count, _fptr(g), _fptr(ds), eps_rank, _fptr(lam), _fptr(gres), st.ctypes.data_as(C.c_void_p)))
        return lam, gres, st, rc

    def second_lagrange_batched(self, t_max: int, p_gn: np.ndarray, prob0: int = 0, diag_scale: Optional[np.ndarray] = None,
                                eps_rank: float = SQRT_EPS):
        """second_lagrange_mult_estimate! per problem; p_gn: (count, n).  Returns (lambda (count, t_max), status, rc)."""
        p = np.ascontiguousarray(p_gn, dtype=np.float64)
        count = p.shape[0]
        ds = None if diag_scale is None else np.ascontiguousarray(diag_scale, dtype=np.float64)
        lam, st = np.zeros((count, t_max)), np.zeros(count, dtype=np.int32)
        rc = self._chk_batched(self._lib.enlsip_gn_second_lagrange_batched(
            self._h, prob0, count, _fptr(p), _fptr(ds), eps_rank, _fptr(lam), st.ctypes.data_as(C.c_void_p)))
        return lam, st, rc

    # device forms: raw device pointers (e.g. torch tensor .data_ptr(), 0 = NULL); return the call's rc (0 or 1)
    def gradient_batched_dev(self, prob0: int, count: int, dgrad: int) -> int:
        return self._chk_batched(self._lib.enlsip_gn_gradient_batched_dev(self._h, prob0, count, _dptr(dgrad)))

    def jacobian_times_batched_dev(self, prob0: int, count: int, dp: int, dJp: int = 0, dAp: int = 0) -> int:
        return self._chk_batched(self._lib.enlsip_gn_jacobian_times_batched_dev(
            self._h, prob0, count, _dptr(dp), _dptr(dJp), _dptr(dAp)))

    def first_lagrange_batched_dev(self, prob0: int, count: int, dlambda: int, dgrad_fx: int = 0, ddiag_scale: int = 0,
                                   eps_rank: float = SQRT_EPS, dgrad_res: int = 0, dstatus: int = 0) -> int:
        return self._chk_batched(self._lib.enlsip_gn_first_lagrange_batched_dev(
            self._h, prob0, count, _dptr(dgrad_fx), _dptr(ddiag_scale), eps_rank, _dptr(dlambda), _dptr(dgrad_res), _dptr(dstatus)))

    def second_lagrange_batched_dev(self, prob0: int, count: int, dp_gn: int, dlambda: int, ddiag_scale: int = 0,
                                    eps_rank: float = SQRT_EPS, dstatus: int = 0) -> int:
        return self._chk_batched(self._lib.enlsip_gn_second_lagrange_batched_dev(
            self._h, prob0, count, _dptr(dp_gn), _dptr(ddiag_scale), eps_rank, _dptr(dlambda), _dptr(dstatus)))

    def _form(self, getter_name: str) -> int:
        f = C.c_int(0)
        self._chk(getattr(self._lib, getter_name)(self._h, C.byref(f)))
        return int(f.value)

    def consumer_form(self) -> int:
        """Form of the last batched multiplier estimate: 0 general, 1 wave per problem, -1 none yet."""
        return self._form("enlsip_gn_get_consumer_form")

    # ---- the subspace re-solve over a range of the resident batch (src/enlsip_functions.jl:1249-1253, :1118-1176, :116-153) ------
    @staticmethod
    def pack_resolve(count: int, dimA, dimJ2, code=-1):
        """The three host request arrays of resolve_batched (int64, count entries each) from scalars or sequences.  code 0 leaves a
        problem alone; DIM_HOLD in dimJ2 stops after b and d, DIM_HOLD in dimA starts from the result such a call left."""
        def arr(x, name):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.int64), (count,))).copy()
            if a.shape != (count,):
                raise ValueError(f"pack_resolve: {name} must have {count} entries")
            return a
        dA, dJ, cd = arr(dimA, "dimA"), arr(dimJ2, "dimJ2"), arr(code, "code")
        if np.any((cd != 0) & (cd != 1) & (cd != -1)):
            raise ValueError("pack_resolve: code entries are 1, -1 or 0 (leave the problem alone)")
        return dA, dJ, cd

    @staticmethod
    def resolve_outputs(count: int, m: int, n: int, t_max: int, fill: float = np.nan, want=("p", "b", "d", "info", "status")):
        """Output arrays of resolve_batched in its slot layout: p (count, n), b (count, t_max), d (count, m), info (count, 6) int64
        (rankA, rankJ2, code, dimA, dimJ2, status), status (count,) int32.  Slots of problems the call leaves alone keep `fill`
        (info and status: -1).  An output not named in `want` is None (a NULL pointer: not computed into)."""
        return {
            "p": np.full((count, n), fill) if "p" in want else None,
            "b": np.full((count, t_max), fill) if "b" in want else None,
            "d": np.full((count, m), fill) if "d" in want else None,
            "info": np.full((count, 6), -1, dtype=np.int64) if "info" in want else None,
            "status": np.full(count, -1, dtype=np.int32) if "status" in want else None,
        }

    def resolve_batched(self, m: int, n: int, t_max: int, dimA, dimJ2, code=-1, prob0: int = 0, count: Optional[int] = None,
                        want=("p", "b", "d", "info", "status"), out: Optional[dict] = None):
        """sub_search_direction per problem of prob0 .. prob0+count-1 on the resident factors, one call.  Returns
        (out, rc): out as resolve_outputs, rc 0 or 1 (some status non-zero)."""
        if count is None:
            count = len(np.atleast_1d(np.asarray(code if np.ndim(code) else dimA)))
        dA, dJ, cd = self.pack_resolve(count, dimA, dimJ2, code)
        o = out if out is not None else self.resolve_outputs(count, m, n, t_max, want=want)
        rc = self._chk_batched(self._lib.enlsip_gn_resolve_batched(
            self._h, prob0, count, _fptr(dA), _fptr(dJ), _fptr(cd), _fptr(o["p"]), _fptr(o["b"]), _fptr(o["d"]),
            _fptr(o["info"]), _fptr(o["status"])))
        return o, rc

    def resolve_batched_dev(self, prob0: int, count: int, dimA, dimJ2, code=-1, dp: int = 0, db: int = 0, dd: int = 0,
                            dinfo: int = 0, dstatus: int = 0) -> int:
        """Device form: dimA / dimJ2 / code stay host arrays, the outputs are raw device pointers (0 = NULL)."""
        dA, dJ, cd = self.pack_resolve(count, dimA, dimJ2, code)
        return self._chk_batched(self._lib.enlsip_gn_resolve_batched_dev(
            self._h, prob0, count, _fptr(dA), _fptr(dJ), _fptr(cd), _dptr(dp), _dptr(db), _dptr(dd), _dptr(dinfo), _dptr(dstatus)))

    def diagR_batched(self, which: int, stride: int, prob0: int = 0, count: int = 1) -> np.ndarray:
        """diag(F.R) of problems prob0 .. prob0+count-1: (count, stride), zeros past each problem's own length."""
        out = np.zeros((count, max(stride, 1)))
        self._chk(self._lib.enlsip_gn_get_diagR_batched(self._h, which, prob0, count, _fptr(out), max(stride, 1)))
        return out

    def resolve_form(self) -> int:
        """Kernel form of the last resolve_batched: 0 general, 1 one wave per problem, -1 none yet."""
        return self._form("enlsip_gn_get_resolve_form")

    def resolve_q0_ms(self) -> float:
        """HIP-event time of the Q0' launches of the last resolve_batched (set_profiling(True) before it; 0 otherwise)."""
        ms = C.c_float(0.0)
        self._chk(self._lib.enlsip_gn_get_resolve_q0_ms(self._h, C.byref(ms)))
        return float(ms.value)

    # ---- subspace minimisation in one call: the dimension choice on the device (src/enlsip_functions.jl:1118-1176, :1249-1253) ----
    PREV_DTYPE = np.dtype([("previous_dimA", np.int64), ("previous_dimJ2", np.int64), ("restart", np.int64),
                           ("previous_alpha", np.float64), ("constraint_progress", np.float64), ("residual_progress", np.float64)])

    @classmethod
    def pack_subspace_prev(cls, count: int, previous_dimA, previous_dimJ2, restart, previous_alpha, constraint_progress,
                           residual_progress) -> np.ndarray:
        """The `prev` array of subspace_direction_batched (enlsip_gn_subspace_prev, 48 bytes per problem): scalars broadcast to
        `count` entries.  previous_dimA = abs(prev.dimA) + t - prev.t (:1144), previous_dimJ2 = abs(prev.dimJ2) + prev.t - t
        (:1165), constraint_progress = dot(prev.cx, prev.cx) - active_cx_sum (:1147), residual_progress = dot(prev.rx, prev.rx)
        - rx_sum (:1168)."""
        out = np.zeros(count, dtype=cls.PREV_DTYPE)
        for name, v in (("previous_dimA", previous_dimA), ("previous_dimJ2", previous_dimJ2), ("restart", restart),
                        ("previous_alpha", previous_alpha), ("constraint_progress", constraint_progress),
                        ("residual_progress", residual_progress)):
            a = np.asarray(v)
            if a.ndim > 1 or (a.ndim == 1 and a.shape != (count,)):
                raise ValueError(f"pack_subspace_prev: {name} must be a scalar or have {count} entries")
            out[name] = a
        return out

    def _prev_arg(self, count: int, prev):
        if prev is None:
            return None
        pv = np.ascontiguousarray(prev)
        if pv.dtype != self.PREV_DTYPE or pv.shape != (count,):
            raise ValueError(f"prev must come from pack_subspace_prev with {count} entries")
        return pv

    def subspace_direction_batched(self, m: int, n: int, t_max: int, prev, prob0: int = 0, count: Optional[int] = None, take=None,
                                   want=("p", "b", "d", "info", "status"), out: Optional[dict] = None):
        """The subspace branch of search_direction_analys (:1251-1253) for problems prob0 .. prob0+count-1 in one call: b, the
        chosen dimA, d, the chosen dimJ2 and p; info[:, 3:5] carry the chosen dimensions.  Returns (out, rc) as resolve_batched;
        status 1 / 2: the final dimA / dimJ2 is out of range (b, d written, p not), 5: the reference would index out of bounds
        (nothing written)."""
        if count is None:
            count = len(prev)
        pv = self._prev_arg(count, prev)
        tk = self._pack_take(count, take)
        o = out if out is not None else self.resolve_outputs(count, m, n, t_max, want=want)
        rc = self._chk_batched(self._lib.enlsip_gn_subspace_direction_batched(
            self._h, prob0, count, _fptr(tk), _fptr(pv), _fptr(o["p"]), _fptr(o["b"]), _fptr(o["d"]), _fptr(o["info"]),
            _fptr(o["status"])))
        return o, rc

    def subspace_direction_batched_dev(self, prob0: int, count: int, prev, take=None, dp: int = 0, db: int = 0, dd: int = 0,
                                       dinfo: int = 0, dstatus: int = 0) -> int:
        """Device form: prev and take stay host arrays, the outputs are raw device pointers (0 = NULL)."""
        pv = self._prev_arg(count, prev)
        tk = self._pack_take(count, take)
        return self._chk_batched(self._lib.enlsip_gn_subspace_direction_batched_dev(
            self._h, prob0, count, _fptr(tk), _fptr(pv), _dptr(dp), _dptr(db), _dptr(dd), _dptr(dinfo), _dptr(dstatus)))

    def subspace_form(self) -> int:
        """Kernel form of the last subspace_direction_batched: 0 general, 1 one wave per problem, -1 none yet."""
        return self._form("enlsip_gn_get_subspace_form")

    # ---- the deletion test and the working-set edit on device buffers (src/enlsip_functions.jl:574-603, :708-719, :731-739) --------
    @staticmethod
    def _host_i64(x, batch: int, name: str):
        a = np.ascontiguousarray(np.asarray(x).astype(np.int64))
        if a.shape != (batch,):
            raise ValueError(f"{name} must have {batch} entries")
        return a

    @staticmethod
    def _host_lists(batch: int, *lists):
        """(name, x, stride) per ragged index list -> the host int64 pointer to its batch x stride entries, NULL when empty (a
        pointer keeps its array alive)"""
        arrs = [np.ascontiguousarray(np.asarray(x).astype(np.int64)) for _, x, _ in lists]
        if any(a.size != batch * stride for a, (_, _, stride) in zip(arrs, lists)):
            (name, _, stride), rest = lists[0], lists[1:]
            raise ValueError(f"{name} must have {batch} x {stride} entries" + "".join(f", {n} {batch} x {st}" for n, _, st in rest))
        return [_fptr(a) if a.size else None for a in arrs]

    def delete_constraints_batched_dev(self, batch, n, t_max, t, q, scaling, dlambda, ddiag_scale, dAt, ldat, strideAt, dcx,
                                       dgrad_res=0, dsaved=0, take=None) -> np.ndarray:
        """check_constraint_deletion per taken problem on the device buffers and, where it names a row, its removal in place
        (A', cx, lambda, diag_scale in the padded ragged layout; the removed record into dsaved, n + 3 doubles per problem).  t, q,
        take (None: all) stay host arrays; dgrad_res = 0: grad_res = 0.0 (the second-order test).  Returns s (batch,) int64,
        1-based, 0 = nothing; t is the caller's to decrement."""
        t = self._host_i64(t, batch, "t")
        q = self._host_i64(q, batch, "q")
        tk = self._pack_take(batch, take)
        s = np.zeros(batch, dtype=np.int64)
        self._chk(self._lib.enlsip_gn_delete_constraints_batched_dev(
            self._h, batch, n, t_max, _fptr(t), _fptr(q), _fptr(tk), int(bool(scaling)), _dptr(dlambda), _dptr(ddiag_scale),
            _dptr(dgrad_res), _dptr(dAt), ldat, strideAt, _dptr(dcx), _dptr(dsaved), _fptr(s)))
        return s

    def restore_constraints_batched_dev(self, batch, n, t_max, t, s, dlambda, ddiag_scale, dAt, ldat, strideAt, dcx, dsaved):
        """The exact inverse of delete_constraints_batched_dev for the problems with s[k] != 0; t[k] is the count after the
        deletion.  The caller increments t."""
        t = self._host_i64(t, batch, "t")
        s = self._host_i64(s, batch, "s")
        self._chk(self._lib.enlsip_gn_restore_constraints_batched_dev(
            self._h, batch, n, t_max, _fptr(t), _fptr(s), _dptr(dlambda), _dptr(ddiag_scale), _dptr(dAt), ldat, strideAt, _dptr(dcx),
            _dptr(dsaved)))

    def deletion_form(self) -> int:
        """Kernel form of the last delete / restore call: 0 general, 1 one wave per problem, -1 none yet."""
        return self._form("enlsip_gn_get_deletion_form")

    # ---- the working-set additions and the rebuild of the active constraints on device buffers (:608-650, :2854-2855) --------------
    def add_constraints_batched_dev(self, batch, n, l, t_max, q, t, active, inactive, index_alpha_upp, scaling, dA, lda, strideA,
                                    dcx_all, dAt, ldat, strideAt, dcx, ddiag_scale, take=None):
        """evaluate_violated_constraints per walked problem on dcx_all (l per problem), then the padded slot of the ragged solve
        (dAt, dcx, ddiag_scale) gathered from dA / dcx_all by the active lists, scaled when `scaling`.  take (None: 1 everywhere):
        0 leave the problem alone, 1 walk and rebuild, 2 rebuild only.  q, t (batch,), active, inactive (batch, l; 1-based, 0
        padded) and index_alpha_upp (batch,; None: 0) are host arrays and are not modified.  Returns (t, active, inactive, added,
        status) as new arrays: int64 (batch,), (batch, l), (batch, l), (batch,), (batch,); status 1: the reference would repeat a
        swap pass for ever and the lists are in that unchanged state."""
        q = self._host_i64(q, batch, "q")
        t = self._host_i64(t, batch, "t").copy()
        act = np.ascontiguousarray(np.asarray(active).astype(np.int64)).copy()
        ina = np.ascontiguousarray(np.asarray(inactive).astype(np.int64)).copy()
        if act.size != batch * l or ina.size != batch * l:
            raise ValueError(f"active and inactive must have {batch} x {l} entries")
        iau = None if index_alpha_upp is None else self._host_i64(index_alpha_upp, batch, "index_alpha_upp")
        tk = None if take is None else self._host_i64(take, batch, "take")
        added = np.zeros(batch, dtype=np.int64)
        status = np.zeros(batch, dtype=np.int64)
        self._chk(self._lib.enlsip_gn_add_constraints_batched_dev(
            self._h, batch, n, l, t_max, _fptr(q), _fptr(t), _fptr(act) if act.size else None, _fptr(ina) if ina.size else None,
            _fptr(iau), _fptr(tk), int(bool(scaling)), _dptr(dA), lda, strideA, _dptr(dcx_all), _dptr(dAt), ldat, strideAt,
            _dptr(dcx), _dptr(ddiag_scale), _fptr(added), _fptr(status)))
        return t, act.reshape(batch, l), ina.reshape(batch, l), added, status

    def addition_form(self) -> int:
        """Kernel form of the last add_constraints_batched_dev: 0 general, 1 one wave per problem, -1 none yet."""
        return self._form("enlsip_gn_get_addition_form")

    # ---- the line-search set-up on device buffers (src/enlsip_functions.jl:2149-2178, :2226-2229, :1561-1584, :2269) ---------------
    def linesearch_setup_batched_dev(self, batch, m, n, l, dp, dA, lda, strideA, dcx, inactive, n_inactive, dAp, index_del=None,
                                     dJp=0, drx=0):
        """Ap = A * p with the full constraint Jacobian into dAp (l per problem), upper_bound_steplength on it, and with dJp and
        drx (m per problem; both or neither) the sums Jp.Jp, Jp.rx, rx.rx.  inactive (batch, l) and n_inactive, index_del (batch,;
        None: 0) stay host arrays.  Returns (alpha_upp (batch,), index_alpha_upp (batch,) int64, sums (batch, 3) or None)."""
        ni = self._host_i64(n_inactive, batch, "n_inactive")
        idel = None if index_del is None else self._host_i64(index_del, batch, "index_del")
        inact, = self._host_lists(batch, ("inactive", inactive, l))
        if bool(dJp) != bool(drx):
            raise ValueError("dJp and drx go together")
        alpha = np.zeros(batch)
        index = np.zeros(batch, dtype=np.int64)
        sums = np.zeros((batch, 3)) if dJp else None
        self._chk(self._lib.enlsip_gn_linesearch_setup_batched_dev(
            self._h, batch, m, n, l, _dptr(dp), _dptr(dA), lda, strideA, _dptr(dcx), inact, _fptr(ni),
            _fptr(idel), _dptr(dJp), _dptr(drx), _dptr(dAp), _fptr(alpha), _fptr(index), _fptr(sums)))
        return alpha, index, sums

    def linesearch_form(self) -> int:
        """Kernel form of the last linesearch_setup_batched_dev: 0 general, 1 one wave per problem, -1 none yet."""
        return self._form("enlsip_gn_get_linesearch_form")

    # ---- the penalty weights and the merit function on device buffers (src/enlsip_functions.jl:1545-1629, :2243, :2268, :1307-1340)
    def penalty_weights_batched_dev(self, batch, l, t_max, t, dimA, active, norm_code, scaling, dw_old, dactive_Ap, ddiag_scale, dcx,
                                    dK, sums, dw, take=None):
        """penalty_weight_update per taken problem on the device buffers: dw (l per problem) and dK (4 l per problem) are written
        there.  t, dimA (batch,), active (batch, t_max; 1-based, 0 padded), take (None: all) and sums (batch, 3: Jp.Jp, Jp.rx, rx.rx
        as linesearch_setup_batched_dev returns them) stay host arrays.  dw may be dw_old.  Returns (scalars (batch, 3): dpsi0, psi0,
        atwa; branch (batch,) int32); both 0 for a problem not taken."""
        t = self._host_i64(t, batch, "t")
        dimA = self._host_i64(dimA, batch, "dimA")
        act, = self._host_lists(batch, ("active", active, t_max))
        sm = np.ascontiguousarray(sums, dtype=np.float64)
        if sm.size != 3 * batch:
            raise ValueError(f"sums must have {batch} x 3 entries")
        tk = self._pack_take(batch, take)
        scalars = np.zeros((batch, 3))
        branch = np.zeros(batch, dtype=np.int32)
        self._chk(self._lib.enlsip_gn_penalty_weights_batched_dev(
            self._h, batch, l, t_max, _fptr(t), _fptr(dimA), act, _fptr(tk), int(norm_code),
            int(bool(scaling)), _dptr(dw_old), _dptr(dactive_Ap), _dptr(ddiag_scale), _dptr(dcx), _dptr(dK), _fptr(sm), _dptr(dw),
            _fptr(scalars), _fptr(branch)))
        return scalars, branch

    def penalty_form(self) -> int:
        """Kernel form of the last penalty_weights_batched_dev: 0 general, 1 one wave per problem, -1 none yet."""
        return self._form("enlsip_gn_get_penalty_form")

    def merit_batched_dev(self, batch, m, l, t_max, t, active, inactive, n_inactive, drx, dcx, dw, take=None) -> np.ndarray:
        """psi (:1307-1340) of a batch of evaluated trial points: drx (m per problem), dcx, dw (l per problem) on the device; t,
        n_inactive (batch,), active (batch, t_max), inactive (batch, l) (1-based, 0 padded) and take (None: all) stay host arrays.
        Returns psi (batch,), 0 for a problem not taken."""
        t = self._host_i64(t, batch, "t")
        ni = self._host_i64(n_inactive, batch, "n_inactive")
        act, inact = self._host_lists(batch, ("active", active, t_max), ("inactive", inactive, l))
        tk = self._pack_take(batch, take)
        psi = np.zeros(batch)
        self._chk(self._lib.enlsip_gn_merit_batched_dev(
            self._h, batch, m, l, t_max, _fptr(t), act, inact, _fptr(ni), _fptr(tk), _dptr(drx), _dptr(dcx), _dptr(dw), _fptr(psi)))
        return psi

    # ---- the polynomial fit of the line search on device buffers (src/enlsip_functions.jl:1665-1689, :1986-1998, :1841-1862) ----------
    def linesearch_fit_batched_dev(self, batch, m, l, t_max, t, active, inactive, n_inactive, alpha_k, x_min, alpha_min, alpha_max,
                                   drx, drx_new, dJp, dcx, dcx_new, dAp, dw, take=None, psi=False):
        """The six sums of coefficients_linesearch! per taken problem on the device buffers (drx, drx_new, dJp m per problem; dcx,
        dcx_new, dAp, dw l per problem; none is written) and linesearch_fit on them, on the host inside the call.  t, n_inactive,
        alpha_k, x_min, alpha_min, alpha_max (batch,), active (batch, t_max), inactive (batch, l) and take (None: all) stay host
        arrays.  Returns (sums (batch, 6), out (batch, 6): alpha_kp1, pk, alpha_hat, s_alpha, beta_hat, s_beta; arm (batch,) int32;
        psi_new (batch,) = psi of (drx_new, dcx_new, dw) as merit_batched_dev returns it, or None); zeros for a problem not taken."""
        t = self._host_i64(t, batch, "t")
        ni = self._host_i64(n_inactive, batch, "n_inactive")
        act, inact = self._host_lists(batch, ("active", active, t_max), ("inactive", inactive, l))
        sc = []
        for name, v in (("alpha_k", alpha_k), ("x_min", x_min), ("alpha_min", alpha_min), ("alpha_max", alpha_max)):
            v = np.ascontiguousarray(v, dtype=np.float64)
            if v.size != batch:
                raise ValueError(f"{name} must have {batch} entries")
            sc.append(v)
        tk = self._pack_take(batch, take)
        sums, out = np.zeros((batch, 6)), np.zeros((batch, 6))
        arm = np.zeros(batch, dtype=np.int32)
        psi_new = np.zeros(batch) if psi else None
        self._chk(self._lib.enlsip_gn_linesearch_fit_batched_dev(
            self._h, batch, m, l, t_max, _fptr(t), act, inact, _fptr(ni), _fptr(tk), _fptr(sc[0]), _fptr(sc[1]), _fptr(sc[2]),
            _fptr(sc[3]), _dptr(drx), _dptr(drx_new), _dptr(dJp), _dptr(dcx), _dptr(dcx_new), _dptr(dAp), _dptr(dw), _fptr(sums),
            _fptr(out), _fptr(arm), _fptr(psi_new)))
        return sums, out, arm, psi_new

    def newton_direction(self, Gamma: np.ndarray, prob: int = 0):
        """newton_search_direction (src/enlsip_functions.jl:348-423) after its Hessian sums: Gamma = r_mat - c_mat (n x n).
        Returns (p, error) as the reference does (error = True: W22 not positive definite, p = 0)."""
        G = np.asfortranarray(Gamma, dtype=np.float64)
        n = G.shape[0]
        p = np.zeros(n)
        bad = C.c_int64(0)
        self._chk(self._lib.enlsip_gn_newton_direction(self._h, prob, _fptr(G), n, _fptr(p), C.byref(bad)))
        return p, bool(bad.value)

    # ---- the Newton direction over a range of the resident batch (src/enlsip_functions.jl:371-421) ---------------------------------
    @staticmethod
    def _pack_take(count: int, take):
        return None if take is None else GNSolver._host_i64(take, count, "take")

    def newton_direction_batched(self, Gammas: np.ndarray, prob0: int = 0, count: Optional[int] = None, take=None,
                                 out_p: Optional[np.ndarray] = None, out_status: Optional[np.ndarray] = None):
        """newton_search_direction after its Hessian sums for problems prob0 .. prob0+count-1, one call.  Gammas: (count, n, n),
        Gammas[j] = r_mat - c_mat of problem prob0 + j.  take: per slot, 0 leaves the problem alone (its slots keep what out_p /
        out_status held: NaN / -1 by default).  Returns (p (count, n), status (count,) int32, rc): status 0, 1 not positive
        definite (p = 0), 2 rank-deficient working set with t < n; rc 0 or 1 (some status non-zero)."""
        G = np.asarray(Gammas, dtype=np.float64)
        if G.ndim != 3 or G.shape[1] != G.shape[2]:
            raise ValueError("Gammas must be (count, n, n)")
        if count is None:
            count = G.shape[0]
        n = G.shape[1]
        if count < 1 or count > G.shape[0]:
            raise ValueError(f"count must be in 1..{G.shape[0]} (the number of Gammas)")
        Gf = np.ascontiguousarray(np.transpose(G[:count], (0, 2, 1)))      # column-major n x n per slot
        p = out_p if out_p is not None else np.full((count, n), np.nan)
        st = out_status if out_status is not None else np.full(count, -1, dtype=np.int32)
        if p.dtype != np.float64 or p.shape != (count, n) or not p.flags.c_contiguous:
            raise ValueError(f"out_p must be a C-contiguous float64 array of shape ({count}, {n})")
        if st.dtype != np.int32 or st.shape != (count,) or not st.flags.c_contiguous:
            raise ValueError(f"out_status must be a contiguous int32 array of {count} entries")
        tk = self._pack_take(count, take)
        rc = self._chk_batched(self._lib.enlsip_gn_newton_direction_batched(
            self._h, prob0, count, _fptr(Gf), n, n * n, _fptr(tk), _fptr(p), st.ctypes.data_as(C.c_void_p)))
        return p, st, rc

    def newton_direction_batched_dev(self, prob0: int, count: int, dGamma: int, ldg: int, strideG: int, dp: int, dstatus: int = 0,
                                     take=None) -> int:
        """Device form: dGamma (column-major n x n per slot, ldg, strideG), dp (count x n) and dstatus are raw device pointers
        (0 = NULL); take stays a host array."""
        tk = self._pack_take(count, take)
        return self._chk_batched(self._lib.enlsip_gn_newton_direction_batched_dev(
            self._h, prob0, count, _dptr(dGamma), ldg, strideG, _fptr(tk), _dptr(dp), _dptr(dstatus)))

    def newton_form(self) -> int:
        """Kernel form of the last newton_direction_batched: 0 general, 1 one wave per problem, -1 none yet."""
        return self._form("enlsip_gn_get_newton_form")

    def newton_stage_ms(self):
        """HIP-event times of the four stages of the last newton_direction_batched (set_profiling(True) before it; zeros otherwise):
        default b / p1 / d, E, W22 and the right-hand side, factorisation + solves + p."""
        ms = (C.c_float * 4)()
        self._chk(self._lib.enlsip_gn_get_newton_stage_ms(self._h, ms))
        return [float(x) for x in ms]

    # ---- instrumentation ------------------------------------------------------------------------
    def set_profiling(self, on: bool, all_updates: bool = False):
        """HIP-event timing of the stages and the level-0 far updates; all_updates: every trailing-update launch (update_totals)."""
        self._chk(self._lib.enlsip_gn_set_profiling(self._h, (2 if all_updates else 1) if on else 0))

    def stage_ms(self) -> dict:
        arr = (C.c_float * len(L.STAGE_NAMES))()
        self._chk(self._lib.enlsip_gn_get_stage_ms(self._h, arr))
        return dict(zip(L.STAGE_NAMES, [float(x) for x in arr]))

    def update_stats(self):
        ms, cnt, by = C.c_float(), C.c_int64(), C.c_double()
        self._chk(self._lib.enlsip_gn_get_update_stats(self._h, C.byref(ms), C.byref(cnt), C.byref(by)))
        return float(ms.value), int(cnt.value), float(by.value)

    def update_table(self):
        """Per timed level-0 far-update launch of the last profiled solve: [(SURVEY 8d bytes, ms), ...] in sweep order."""
        cap = 256
        by = (C.c_double * cap)()
        ms = (C.c_float * cap)()
        cnt = C.c_int64(0)
        self._chk(self._lib.enlsip_gn_get_update_table(self._h, cap, by, ms, C.byref(cnt)))
        return [(float(by[i]), float(ms[i])) for i in range(min(int(cnt.value), cap))]

    def launch_plan(self):
        """(pipeline_split, panel_pairs, tile_rows) of the last solve: what the library chose on its own."""
        sp, pr, tr = C.c_int64(), C.c_int(), C.c_int64()
        self._chk(self._lib.enlsip_gn_get_launch_plan(self._h, C.byref(sp), C.byref(pr), C.byref(tr)))
        return int(sp.value), bool(pr.value), int(tr.value)

    def route(self) -> set:
        """Names of the kernel-selection branches the last solve took (enlsip_gn_get_route; include/enlsip_gn.h ENLSIP_GN_ROUTE_*)."""
        mask = C.c_uint64(0)
        self._chk(self._lib.enlsip_gn_get_route(self._h, C.byref(mask)))
        return {name for bit, name in enumerate(route_names(self._lib)) if (mask.value >> bit) & 1}

    def pipeline_split(self) -> int:
        return self.launch_plan()[0]

    def plan_uses_pairs(self) -> bool:
        return self.launch_plan()[1]

    def update_totals(self):
        """(far_ms, other_ms, other_launches, all_panels_bytes) of the last profiled solve: HIP-event time of the level-0 far
        passes and of every other trailing-update launch (tree levels, second-panel columns); SURVEY 8d bytes of all panels."""
        far, oth, cnt, by = C.c_float(), C.c_float(), C.c_int64(), C.c_double()
        self._chk(self._lib.enlsip_gn_get_update_totals(self._h, C.byref(far), C.byref(oth), C.byref(cnt), C.byref(by)))
        return float(far.value), float(oth.value), int(cnt.value), float(by.value)

    def measure_stream(self, nbytes: int = 1 << 30, reps: int = 5) -> float:
        """GB/s of an in-place non-temporal read-modify-write stream with the trailing update's access shape on this device."""
        out = C.c_double(0.0)
        self._chk(self._lib.enlsip_gn_measure_stream(self._h, nbytes, reps, C.byref(out)))
        return float(out.value)

    def synchronize(self):
        self._chk(self._lib.enlsip_gn_synchronize(self._h))
