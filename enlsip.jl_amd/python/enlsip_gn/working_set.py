"""Host mirror of the reference's ``update_working_set`` (src/enlsip_functions.jl:686-795) over the
HIP library: same arguments, same mutations of ``W`` / ``C`` / ``iter_k``, same return triple
``(F_A, F_L11, F_J2)`` — with every ``qr(·, ColumnNorm())`` + ``gn_search_direction`` group replaced
by ONE device solve and the factor objects replaced by device-backed views (``FactorView``).

The multiplier estimates run on the device, on the resident ``F_A``, ``J`` and
``J*F_A.Q`` (``GNSolver.first_lagrange`` / ``second_lagrange``); the host restatements over the accessors
(``.R``, ``.p``, ``Qt_mul``) are kept below as the form the Julia glue would use without those entry points.
The deletion test and the sequencing of 1-3 subproblem solves per call (including quirk Q1: a first-order
deletion is always undone, App. C) are reproduced on the host.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from ._lib import FACTOR_A, FACTOR_L11, FACTOR_J2
from .api import GNSolver

EPS = float(np.finfo(np.float64).eps)
SQRT_EPS = math.sqrt(EPS)


# ---- records mirrored from src/structures.jl -------------------------------------------------------
@dataclass
class WorkingSet:                      # src/structures.jl:209-225
    q: int
    t: int
    l: int
    active: np.ndarray
    inactive: np.ndarray

    @staticmethod
    def create(q: int, l: int) -> "WorkingSet":
        active = np.zeros(l, dtype=np.int64)
        inactive = np.zeros(l - q, dtype=np.int64)
        active[:q] = np.arange(1, q + 1)
        inactive[:] = np.arange(q + 1, l + 1)
        return WorkingSet(q, q, l, active, inactive)

    def remove_constraint(self, s: int) -> None:      # :230-245, s 1-based
        l, t = self.l, self.t
        self.inactive[l - t] = self.active[s - 1]
        self.inactive[: l - t + 1] = np.sort(self.inactive[: l - t + 1])
        for i in range(s, t):
            self.active[i - 1] = self.active[i]
        self.active[t - 1] = 0
        self.t -= 1

    def add_constraint(self, s: int) -> None:         # :250-263, s 1-based index into inactive
        l, t = self.l, self.t
        self.active[t] = self.inactive[s - 1]
        self.active[: t + 1] = np.sort(self.active[: t + 1])
        for i in range(s, l - t):
            self.inactive[i - 1] = self.inactive[i]
        self.inactive[l - t - 1] = 0
        self.t += 1


@dataclass
class Constraint:                      # src/structures.jl:145-150
    cx: np.ndarray
    A: np.ndarray
    scaling: bool
    diag_scale: np.ndarray


@dataclass
class IterationRecord:                 # hot-path fields of src/structures.jl:63-91
    rankA: int = 0
    rankJ2: int = 0
    dimA: int = 0
    dimJ2: int = 0
    b_gn: np.ndarray = field(default_factory=lambda: np.zeros(0))
    d_gn: np.ndarray = field(default_factory=lambda: np.zeros(0))
    grad_res: float = 0.0
    lam: np.ndarray = field(default_factory=lambda: np.zeros(0))
    delete: bool = False
    index_del: int = 0
    code: int = 0                      # method_code of the direction (2: undamped step, no line search; :2284-2290)


def pseudo_rank(diag_T, eps_rank: float) -> int:      # src/enlsip_functions.jl:17-31
    l = len(diag_T)
    if l == 0 or abs(diag_T[0]) < eps_rank:
        return 0
    tol = abs(diag_T[0]) * math.sqrt(float(l)) * eps_rank
    r = 1
    while r < l and abs(diag_T[r - 1]) > tol:
        r += 1
    return r - (0 if (r == l and abs(diag_T[r - 1]) > tol) else 1)


def _invperm(p1):
    p0 = np.asarray(p1, dtype=np.int64) - 1
    inv = np.empty_like(p0)
    inv[p0] = np.arange(p0.size)
    return inv


def _tri_solve(T, b, lower):
    """``Triangular(T) \\ b`` on the host for the t x t multiplier systems (t is small)."""
    b = np.asarray(b, dtype=np.float64)
    if b.size == 0:
        return b.copy()
    if np.any(np.diag(T) == 0.0):
        raise np.linalg.LinAlgError("singular triangular system")
    from scipy.linalg import solve_triangular
    return solve_triangular(T, b, lower=lower)


# ---- consumers of the resident factors (src/enlsip_functions.jl:461-537, 574-603) -------------------
def first_lagrange_mult_estimate(A, grad_fx, cx, scaling_done, diag_scale, F_A, it: IterationRecord, eps_rank):
    t, n = A.shape
    R = F_A.R
    p = F_A.p
    inv_p = _invperm(p)
    prankA = pseudo_rank(np.diag(R[: min(R.shape), : min(R.shape)]), eps_rank)
    b = F_A.Qt_mul(grad_fx)
    v = np.zeros(t)
    v[:prankA] = _tri_solve(R[:prankA, :prankA], b[:prankA], lower=False)
    lam_ls = v[inv_p]
    it.grad_res = float(np.linalg.norm(b[prankA:n])) if n > prankA else 0.0
    b2 = -np.asarray(cx, dtype=np.float64)[p - 1]
    y = np.zeros(t)
    y[:prankA] = _tri_solve(R.T[:prankA, :prankA], b2[:prankA], lower=True)
    u = np.zeros(t)
    u[:prankA] = _tri_solve(R[:prankA, :prankA], y[:prankA], lower=False)
    lam = lam_ls + u[inv_p]
    return lam * diag_scale if scaling_done else lam


def second_lagrange_mult_estimate(solver: GNSolver, J, F_A, rx, p_gn, t, scaling, diag_scale, eps_rank=SQRT_EPS):
    m, n = J.shape
    R = F_A.R
    prankA = pseudo_rank(np.diag(R[: min(R.shape), : min(R.shape)]), eps_rank)
    J1 = solver.JQ1(m, n)[:, :t]                       # J * F_A.Q served from the device (:526, quirk Q6)
    b = J1.T @ (rx + J @ p_gn)
    v = np.zeros(t)
    v[:prankA] = _tri_solve(R[:prankA, :prankA], b[:prankA], lower=False)
    lam = v[_invperm(F_A.p)]
    return lam * diag_scale if scaling else lam


def check_constraint_deletion(q, A, lam, scaling, diag_scale, grad_res) -> int:
    t = A.shape[0]
    delta = 10.0
    lam_max = 1.0 if len(lam) == 0 else float(np.max(np.abs(lam)))
    sq_rel = SQRT_EPS * lam_max
    s = 0
    if t > q:
        e = sq_rel
        for i in range(q + 1, t + 1):
            row_i = (1.0 / diag_scale[i - 1]) if scaling else diag_scale[i - 1]
            if row_i * lam[i - 1] <= sq_rel and row_i * lam[i - 1] <= e:
                e = row_i * lam[i - 1]
                s = i
        if grad_res > -e * delta:
            s = 0
    return s


# ---- update_working_set (src/enlsip_functions.jl:686-795) -------------------------------------------
def update_working_set(solver: GNSolver, W: WorkingSet, rx, A, C: Constraint, grad_fx, J, p_gn, it: IterationRecord,
                       eps_rank: float, on_solve=None):
    """Returns (F_A, F_L11, F_J2) as device-backed views, valid until the next solve on ``solver``."""
    m, n = J.shape

    def _direction(factored=False):
        # F_A = qr(C.A'); rankA; F_L11 = qr(F_A.R'); p_gn, F_J2 = gn_search_direction(...)  -> one device solve;
        # factored: the working set is the one just factored at :700, the solve goes on with that factorisation (:768-771)
        out = solver.solve_factored(J, rx, C.A.shape[0], eps_rank) if factored else solver.solve(J, rx, C.A, C.cx, eps_rank)
        p_gn[:] = out.p
        it.rankA, it.rankJ2 = out.rankA, out.rankJ2
        it.dimA, it.dimJ2 = out.rankA, out.rankJ2
        it.b_gn, it.d_gn = out.b, out.d
        if on_solve is not None:
            on_solve()
        return out.rankA

    def _views():
        return solver.factor(FACTOR_A), solver.factor(FACTOR_L11), solver.factor(FACTOR_J2)

    def _second_order(rankA, lam):
        if not (W.t != rankA or it.rankJ2 != min(m, n - rankA)):       # :745 / :773
            # second_lagrange_mult_estimate! on the device: J1 = (J*F_A.Q)[:, 1:t] is resident (:526, quirk Q6)
            lam[:] = solver.second_lagrange(W.t, p_gn, C.diag_scale if C.scaling else None)
            s2 = check_constraint_deletion(W.q, C.A, lam, C.scaling, C.diag_scale, 0.0)
            if s2 != 0:
                index_s2 = int(W.active[s2 - 1])
                lam = np.delete(lam, s2 - 1)
                C.diag_scale = np.delete(C.diag_scale, s2 - 1)
                C.cx = np.delete(C.cx, s2 - 1)
                W.remove_constraint(s2)
                it.delete = True
                it.index_del = index_s2
                C.A = np.delete(C.A, s2 - 1, axis=0)
                rankA = _direction()
        return rankA, lam

    # F_A = qr(C.A', ColumnNorm()) (:700) and first_lagrange_mult_estimate! (:704) on the device, before any solve:
    # the constraint stage alone leaves F_A resident for the estimate
    solver.factor_constraints(J.shape[0], C.A, C.cx, eps_rank)
    lam, it.grad_res = solver.first_lagrange(W.t, grad_fx, C.diag_scale if C.scaling else None, eps_rank)
    s = check_constraint_deletion(W.q, C.A, lam, C.scaling, C.diag_scale, it.grad_res)
    if s != 0:                                                         # :706-765
        cx_s = C.cx[s - 1]
        A_s = C.A[s - 1, :].copy()
        lam_s = lam[s - 1]
        diag_scale_s = C.diag_scale[s - 1]
        index_s = int(W.active[s - 1])
        lam = np.delete(lam, s - 1)
        C.cx = np.delete(C.cx, s - 1)
        C.diag_scale = np.delete(C.diag_scale, s - 1)
        W.remove_constraint(s)
        it.delete = True
        it.index_del = index_s
        C.A = np.delete(C.A, s - 1, axis=0)
        rankA = _direction()
        As_p = 0.0 if rankA <= W.t else float(A_s @ p_gn)              # :728 (quirk Q1)
        feasible = (As_p >= -cx_s) and (As_p > 0)
        if not feasible:
            C.cx = np.insert(C.cx, s - 1, cx_s)
            lam = np.insert(lam, s - 1, lam_s)
            C.diag_scale = np.insert(C.diag_scale, s - 1, diag_scale_s)
            s_inact = int(np.where(W.inactive == index_s)[0][0]) + 1
            W.add_constraint(s_inact)
            it.index_del = 0
            it.delete = False
            rows = A[W.active[: W.t] - 1, :]
            C.A = rows * C.diag_scale[:, None] if C.scaling else rows.copy()
            rankA = _direction()
            rankA, lam = _second_order(rankA, lam)
    else:                                                              # :767-791
        rankA = _direction(factored=True)
        rankA, lam = _second_order(rankA, lam)
    it.lam = lam
    return _views()


# ---- update_working_set for a batch (src/enlsip_functions.jl:686-795 per problem) -----------------------
def update_working_set_batched(solver: GNSolver, Ws, rxs, A, Cs, grad_fxs, Js, p_gns, its, eps_rank: float):
    """``update_working_set`` for B problems of one shape (m, n) with the batched calls: the constraint stage of the whole batch
    (:700), the first estimate (:704), the host deletion test, then the Jacobian side on the working sets that survived (:725 /
    :771), with the constraint stage run again only for the problems whose set changed.  ``A`` is the full (l x n) constraint
    Jacobian of every problem (a list, or one matrix shared by all).  Leaves in ``Ws[k]``, ``Cs[k]``, ``its[k]``, ``p_gns[k]``
    what ``update_working_set`` leaves for problem k and returns the (F_A, F_L11, F_J2) views per problem; the whole batch is
    resident afterwards.  A later change of some working set (the undo of :728-743, a second-order deletion :745 / :773) is one
    ``solve_changed_batched`` call: the constraint stage and the Jacobian side again for exactly the problems whose set changed, in
    place, in the padded layout (t_max) of the resident batch.  After the first pair there is no further whole-batch call."""
    B = len(Ws)
    m, n = Js[0].shape
    As_full = A if isinstance(A, (list, tuple)) else [A] * B
    J = np.stack([np.asfortranarray(Jk, dtype=np.float64).T for Jk in Js])        # (B, n, m): problem k column-major
    rx = np.stack([np.asarray(r, dtype=np.float64) for r in rxs])
    G = np.stack([np.asarray(g, dtype=np.float64) for g in grad_fxs])

    def packed():
        Ak = [np.asarray(C.A, dtype=np.float64).reshape(-1, n) for C in Cs]
        return GNSolver.pack_ragged(Ak, [C.cx for C in Cs], n=n)

    def scales(t_max):
        if not any(C.scaling for C in Cs):
            return None
        ds = np.ones((B, max(t_max, 1)))
        for k, C in enumerate(Cs):
            if C.scaling:
                ds[k, :Ws[k].t] = C.diag_scale
        return ds[:, :t_max] if t_max else None

    def take(out, ks):
        p, b, d, infos = out[:4]
        for k in ks:
            p_gns[k][:] = p[k]
            its[k].rankA, its[k].rankJ2 = infos[k][0], infos[k][1]
            its[k].dimA, its[k].dimJ2 = infos[k][0], infos[k][1]
            its[k].b_gn, its[k].d_gn = b[k, :Ws[k].t].copy(), d[k].copy()

    def padded():
        """the current working sets in the padded layout of the resident batch (no set outgrows the t_max it started with)"""
        At, cx, t = packed()
        pad = t_max - At.shape[1]
        if pad:
            At = np.concatenate([At, np.zeros((B, pad, n))], axis=1)
            cx = np.concatenate([cx, np.zeros((B, pad))], axis=1)
        return At, cx, t

    def solve_again(ks):
        """the problems ks, whose working set changed, again on the resident batch; nothing else of it is touched"""
        At, cx, t = padded()
        flags = np.zeros(B, dtype=np.int64)
        flags[list(ks)] = 1
        take(solver.solve_changed_batched(At, cx, t, flags, eps_rank, m=m), ks)

    At, cx, t = packed()
    t_max = At.shape[1]
    solver.factor_constraints_batched(m, At, cx, t, eps_rank)                               # :700
    lam_b, gres, _, _ = solver.first_lagrange_batched(t_max, 0, B, G, scales(t_max), eps_rank)   # :704
    lams, removed = [], {}
    for k in range(B):
        W, C, it = Ws[k], Cs[k], its[k]
        lam = lam_b[k, :W.t].copy()
        it.grad_res = float(gres[k])
        s = check_constraint_deletion(W.q, C.A, lam, C.scaling, C.diag_scale, it.grad_res)
        if s != 0:                                                                          # :706-723
            removed[k] = (s, C.cx[s - 1], C.A[s - 1, :].copy(), lam[s - 1], C.diag_scale[s - 1], int(W.active[s - 1]))
            lam = np.delete(lam, s - 1)
            C.cx = np.delete(C.cx, s - 1)
            C.diag_scale = np.delete(C.diag_scale, s - 1)
            W.remove_constraint(s)
            it.delete = True
            it.index_del = removed[k][5]
            C.A = np.delete(C.A, s - 1, axis=0)
        lams.append(lam)
    flags = np.array([1 if k in removed else 0 for k in range(B)], dtype=np.int64)
    At, cx, t = padded()            # (every longest working set may have lost a row: the layout of the factor call stays)
    take(solver.solve_factored_batched(J, rx, At, cx, t, flags, eps_rank), range(B))        # :725 / :771
    undone = []
    for k, (s, cx_s, A_s, lam_s, ds_s, index_s) in removed.items():                         # :728-743
        W, C, it = Ws[k], Cs[k], its[k]
        As_p = 0.0 if it.rankA <= W.t else float(A_s @ p_gns[k])                            # quirk Q1
        if (As_p >= -cx_s) and (As_p > 0):
            continue
        C.cx = np.insert(C.cx, s - 1, cx_s)
        lams[k] = np.insert(lams[k], s - 1, lam_s)
        C.diag_scale = np.insert(C.diag_scale, s - 1, ds_s)
        W.add_constraint(int(np.where(W.inactive == index_s)[0][0]) + 1)
        it.index_del = 0
        it.delete = False
        rows = As_full[k][W.active[: W.t] - 1, :]
        C.A = rows * C.diag_scale[:, None] if C.scaling else rows.copy()
        undone.append(k)
    if undone:
        solve_again(undone)
    # second-order estimate where :745 / :773 ask for it: the problems that kept their set or got it back
    cand = [k for k in range(B) if (k not in removed or k in undone)
            and not (Ws[k].t != its[k].rankA or its[k].rankJ2 != min(m, n - its[k].rankA))]
    if cand:
        lam2, _, _ = solver.second_lagrange_batched(t_max, np.stack(p_gns), 0, scales(t_max))
        dropped = []
        for k in cand:
            W, C, it = Ws[k], Cs[k], its[k]
            lam = lam2[k, :W.t].copy()
            s2 = check_constraint_deletion(W.q, C.A, lam, C.scaling, C.diag_scale, 0.0)
            if s2 != 0:
                it.index_del = int(W.active[s2 - 1])
                lam = np.delete(lam, s2 - 1)
                C.diag_scale = np.delete(C.diag_scale, s2 - 1)
                C.cx = np.delete(C.cx, s2 - 1)
                W.remove_constraint(s2)
                it.delete = True
                C.A = np.delete(C.A, s2 - 1, axis=0)
                dropped.append(k)
            lams[k] = lam
        if dropped:
            solve_again(dropped)
    for k in range(B):
        its[k].lam = lams[k]
    return [(solver.factor(FACTOR_A, k), solver.factor(FACTOR_L11, k), solver.factor(FACTOR_J2, k)) for k in range(B)]


# ---- the same with the batch resident in device buffers: nothing but s and info crosses PCIe between the stages -------------------
def update_working_set_batched_dev(solver: GNSolver, Ws, rxs, A, Cs, grad_fxs, Js, p_gns, its, eps_rank: float, built=None):
    """``update_working_set_batched`` with J, rx, A', cx, diag_scale, lambda, grad_res and p in device buffers (torch tensors) and
    only ``_dev`` entry points: the deletion test and the removal of a row (:574-603, :708-719, :748-756, :776-785) and the undo
    (:731-739) are ``delete_constraints_batched_dev`` / ``restore_constraints_batched_dev`` on those buffers.  Per stage only s and
    the info records come down; p, b, d, lambda and grad_res come down once at the end for the records.  t, the flags, ``active`` /
    ``inactive`` and ``index_del`` are derived on the host from s, and the rows of ``C.A`` / ``C.cx`` / ``C.diag_scale`` (host inputs)
    follow by the same index.  Same arguments, mutations and return value as ``update_working_set_batched``; the undo puts back the
    row that was removed (the reference recomputes it from ``A`` and ``diag_scale``, :739: the same row), so ``A`` is not read.
    A batch may mix problems with and without row scaling: the test and the edit then run once per kind, each over its own
    problems (``take``), on a diag_scale buffer of that kind.
    ``built``: None, or ``(t_max, dAt, dcx, dds, ddsn)``, the slot ``add_constraints_batched_dev`` (below) left on the device: torch
    float64 tensors (B, n * t_max), (B, t_max), (B, t_max), (B, t_max) with ldat = n (dds: the scaled problems' diag_scale, ones
    elsewhere; ddsn: the row norms of the problems without row scaling).  The call then starts from these buffers, edits them in
    place, and skips ``pack_ragged`` and the upload of A', cx and diag_scale; ``Cs`` must still hold the same rows on the host."""
    import torch
    B = len(Ws)
    m, n = Js[0].shape
    scal = np.array([1 if C.scaling else 0 for C in Cs], dtype=np.int64)
    if built is None:
        Ak = [np.asarray(C.A, dtype=np.float64).reshape(-1, n) for C in Cs]
        At_h, cx_h, t = GNSolver.pack_ragged(Ak, [C.cx for C in Cs], n=n)
        t = np.ascontiguousarray(t, dtype=np.int64)
        t_max = At_h.shape[1]
    else:
        t = np.array([W.t for W in Ws], dtype=np.int64)
        t_max = int(built[0])
        if t_max < 1 or t.max() > t_max:
            raise ValueError("built: t_max must be at least 1 and no working set may exceed it")
    tm1 = max(t_max, 1)
    # diag_scale per kind: the scaled problems' (ones elsewhere: what the estimates' back-transform takes, as scales() of the host
    # flow), and that of the problems without row scaling, which only the deletion test reads (:592)
    ds_h, dsn_h = np.ones((B, tm1)), np.ones((B, tm1))
    for k, C in enumerate(Cs):
        (ds_h if C.scaling else dsn_h)[k, :Ws[k].t] = C.diag_scale
    q = np.array([W.q for W in Ws], dtype=np.int64)
    dev = torch.device("cuda", solver._device if solver._device >= 0 else torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    new = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    dJ = up(np.stack([np.asfortranarray(Jk, dtype=np.float64).T for Jk in Js]))       # (B, n, m): problem k column-major
    drx = up(np.stack([np.asarray(r, dtype=np.float64) for r in rxs]))
    dG = up(np.stack([np.asarray(g, dtype=np.float64) for g in grad_fxs]))
    if built is None:
        dAt, dcx, dds = up(At_h.reshape(B, -1) if t_max else np.zeros((B, 1))), up(cx_h if t_max else np.zeros((B, 1))), up(ds_h)
        ddsn = up(dsn_h)
    else:
        dAt, dcx, dds, ddsn = built[1:]
    dlam, dlam2, dgres, dsaved = new(B, tm1), new(B, tm1), new(B), new(B, n + 3)
    dp, db, dd, dinfo = new(B, n), new(B, tm1), new(B, m), new(B, 6, dtype=torch.int64)
    torch.cuda.synchronize(dev)
    ptr = lambda x: x.data_ptr()
    A_args = (ptr(dAt), max(n, 1), n * t_max, ptr(dcx))
    pds = ptr(dds) if (scal.any() and t_max) else 0
    kinds = [(mask, flag, buf) for mask, flag, buf in ((scal, True, dds), (1 - scal, False, ddsn)) if mask.any()]

    def delete(dl, take=None, **kw):
        """the deletion test and the edit, once per kind of row scaling over that kind's problems"""
        s = np.zeros(B, dtype=np.int64)
        for mask, flag, buf in kinds:
            tk = mask if take is None else mask * take
            if tk.any():
                s += solver.delete_constraints_batched_dev(B, n, t_max, t, q, flag, ptr(dl), ptr(buf), *A_args, take=tk, **kw)
        return s

    def infos():
        solver.synchronize()
        return dinfo.cpu().numpy()

    def drop_row(k, s):
        """the host records of problem k after the deletion of row s (1-based); returns what the undo puts back"""
        W, C, it = Ws[k], Cs[k], its[k]
        rec = (C.cx[s - 1], C.A[s - 1, :].copy(), C.diag_scale[s - 1], int(W.active[s - 1]))
        C.cx = np.delete(C.cx, s - 1)
        C.diag_scale = np.delete(C.diag_scale, s - 1)
        W.remove_constraint(s)
        it.delete = True
        it.index_del = rec[3]
        C.A = np.delete(C.A, s - 1, axis=0)
        return rec

    solver.factor_constraints_batched_dev(B, m, n, t_max, t, *A_args, eps_rank)                                  # :700
    solver.first_lagrange_batched_dev(0, B, ptr(dlam), dgrad_fx=ptr(dG), ddiag_scale=pds, eps_rank=eps_rank,
                                      dgrad_res=ptr(dgres))                                                       # :704
    s1 = delete(dlam, dgrad_res=ptr(dgres), dsaved=ptr(dsaved))                                                   # :705-723
    removed = {int(k): (int(s1[k]),) + drop_row(int(k), int(s1[k])) for k in np.flatnonzero(s1)}
    t = t - (s1 != 0)
    out = dict(dp=ptr(dp), db=ptr(db), dd=ptr(dd), dinfo=ptr(dinfo))
    solver.solve_factored_batched_dev(B, m, n, t_max, t, (s1 != 0).astype(np.int64), ptr(dJ), m, m * n, ptr(drx), *A_args,
                                      eps_rank, **out)                                                            # :725 / :771
    info = infos()
    s_back = np.zeros(B, dtype=np.int64)
    for k, (s, cx_s, A_s, ds_s, index_s) in removed.items():                                                      # :728-743
        W, C, it = Ws[k], Cs[k], its[k]
        # quirk Q1: rankA <= min(n, t), so the dot(A_s, p_gn) arm of :728 is never taken and As_p = 0.0
        assert int(info[k, 0]) <= W.t
        As_p = 0.0
        if (As_p >= -cx_s) and (As_p > 0):
            continue
        s_back[k] = s
        C.cx = np.insert(C.cx, s - 1, cx_s)
        C.diag_scale = np.insert(C.diag_scale, s - 1, ds_s)
        W.add_constraint(int(np.where(W.inactive == index_s)[0][0]) + 1)
        it.index_del = 0
        it.delete = False
        C.A = np.insert(C.A, s - 1, A_s, axis=0)
    if s_back.any():
        for mask, _, buf in kinds:
            if (mask * s_back).any():
                solver.restore_constraints_batched_dev(B, n, t_max, t, mask * s_back, ptr(dlam), ptr(buf), *A_args, ptr(dsaved))
        t = t + (s_back != 0)
        solver.solve_changed_batched_dev(B, m, n, t_max, t, (s_back != 0).astype(np.int64), *A_args, eps_rank, **out)
        info = infos()
    # second-order estimate where :745 / :773 ask for it: the problems that kept their set or got it back
    cand = np.array([1 if (k not in removed or s_back[k]) and not (Ws[k].t != info[k, 0] or info[k, 1] != min(m, n - info[k, 0]))
                     else 0 for k in range(B)], dtype=np.int64)
    if cand.any():
        solver.second_lagrange_batched_dev(0, B, ptr(dp), ptr(dlam2), ddiag_scale=pds)
        s2 = delete(dlam2, take=cand)
        for k in np.flatnonzero(s2):
            drop_row(int(k), int(s2[k]))
        if s2.any():
            t = t - (s2 != 0)
            solver.solve_changed_batched_dev(B, m, n, t_max, t, (s2 != 0).astype(np.int64), *A_args, eps_rank, **out)
    info = infos()
    p, b, d, lam, lam2, gres = (x.cpu().numpy() for x in (dp, db, dd, dlam, dlam2, dgres))
    for k in range(B):
        W, it = Ws[k], its[k]
        p_gns[k][:] = p[k]
        it.rankA, it.rankJ2 = int(info[k, 0]), int(info[k, 1])
        it.dimA, it.dimJ2 = int(info[k, 0]), int(info[k, 1])
        it.b_gn, it.d_gn = b[k, :W.t].copy(), d[k].copy()
        it.grad_res = float(gres[k])
        it.lam = (lam2 if cand[k] else lam)[k, :W.t].copy()
    return [(solver.factor(FACTOR_A, k), solver.factor(FACTOR_L11, k), solver.factor(FACTOR_J2, k)) for k in range(B)]


# ---- the additions after a step and the rebuild of the active constraints, on device buffers ------------------------------------------
def add_constraints_batched_dev(solver: GNSolver, Ws, its_or_index_alpha_upp, dA, dcx_all, dAt, dcx, dds, *, n: int, t_max: int,
                                scaling, lda=None, strideA=None, ldat=None, strideAt=None, take=None, ddsn=None):
    """``evaluate_violated_constraints`` (src/enlsip_functions.jl:608-650) and the rebuild of ``active_C`` (:2854-2855 with
    ``evaluate_scaling!``) for B problems of one shape through ``GNSolver.add_constraints_batched_dev``: the full ``A`` (l x n per
    problem, column-major) and ``cx`` are the device buffers ``dA`` / ``dcx_all`` (raw pointers), and the padded slot of the ragged
    solve is written to ``dAt`` / ``dcx`` / ``dds``.  ``its_or_index_alpha_upp``: the iteration records (their ``index_alpha_upp``
    is read) or the indices themselves.  ``scaling``: one flag or one per problem; like the deletion driver a mixed batch runs once
    per kind of row scaling, each over its own problems, the kind without scaling writing its row norms to ``ddsn`` (default
    ``dds``).  ``take`` as in the entry point (None: walk and rebuild everywhere).  Updates ``W.t``, ``W.active`` and
    ``W.inactive`` of every walked problem and returns ``(added, status)`` (int64, 0 where no walk ran); status 1 means the
    reference would repeat a swap pass for ever there (the lists are in that unchanged state and the slot is built from them)."""
    B = len(Ws)
    l = Ws[0].l
    if any(W.l != l for W in Ws):
        raise ValueError("one shape per batch: every problem needs the same l")
    iau = np.array([int(getattr(x, "index_alpha_upp", x)) for x in its_or_index_alpha_upp], dtype=np.int64)
    scal = np.broadcast_to(np.asarray(scaling, dtype=bool), (B,)).astype(np.int64)
    tk = np.ones(B, dtype=np.int64) if take is None else np.asarray(take).astype(np.int64)
    q = np.array([W.q for W in Ws], dtype=np.int64)
    t = np.array([W.t for W in Ws], dtype=np.int64)
    act, ina = np.zeros((B, l), dtype=np.int64), np.zeros((B, l), dtype=np.int64)
    for k, W in enumerate(Ws):      # the reference's inactive has l - q entries: zero-padded to l for the call
        act[k, :] = W.active
        ina[k, :l - W.q] = W.inactive
    lda = max(l, 1) if lda is None else lda
    ldat = max(n, 1) if ldat is None else ldat
    strideA = lda * n if strideA is None else strideA
    strideAt = ldat * t_max if strideAt is None else strideAt
    added, status = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for mask, flag, buf in ((scal, True, dds), (1 - scal, False, dds if ddsn is None else ddsn)):
        kind = mask * tk
        if not kind.any():
            continue
        t1, a1, i1, ad, st = solver.add_constraints_batched_dev(B, n, l, t_max, q, t, act, ina, iau, flag, dA, lda, strideA, dcx_all,
                                                                dAt, ldat, strideAt, dcx, buf, take=kind)
        for k in np.flatnonzero(kind == 1):
            W = Ws[k]
            W.t = int(t1[k])
            W.active[:] = a1[k]
            W.inactive[:] = i1[k, :l - W.q]
            added[k], status[k] = ad[k], st[k]
    return added, status
