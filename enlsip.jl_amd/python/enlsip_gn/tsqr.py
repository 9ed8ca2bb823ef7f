"""Row-sharded TSQR of one tall residual Jacobian across the GPUs of a node (config C4).

One process per GPU under ``torch.distributed`` (backend ``nccl`` = RCCL over xGMI).  Rank g holds
rows ``[g*m/G, (g+1)*m/G)`` of ``J`` and ``rx``; the small constraint data are replicated.  There is
exactly ONE exchange step on the path: an all-gather of the ``n2 x n2`` triangles (8*n2^2 bytes per
rank, 8.4 MB at n2 = 1024) and of the ``n2``-vectors, plus a scalar all-reduce for ``||d||``.  xGMI
is point-to-point (7 links per GPU), so the all-gather of G-1 messages uses all links at once
and costs tens of microseconds against ~1 ms of local factorisation.

The local and combine stages are the HIP library's ``enlsip_gn_tsqr_local_dev`` /
``enlsip_gn_tsqr_combine_dev``; they are injectable only so that the exchange / stacking logic can be
exercised with the ``gloo`` backend on machines without a GPU (tests/test_tsqr_host.py).

Magnitudes: with ``scaled=True`` the stages are ``enlsip_gn_tsqr_local_scaled_dev`` / ``enlsip_gn_tsqr_combine_scaled_dev``: a
shard outside the band 2^-400 .. 2^400 is factored at a power-of-two scale of its own, and its exponent and tail^2 are gathered
next to the triangles (still one exchange step).  ``tsqr_solve_lib`` does the same inside the library.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from . import _lib as L
from .api import GNSolver, SQRT_EPS


@dataclass
class TSQRResult:
    p: np.ndarray          # search direction (n)
    dlead: np.ndarray      # leading n2 entries of F_J2.Q' d
    d_norm: float          # ||d||_2 over all ranks
    rankA: int
    rankJ2: int
    code: int
    jpvtJ2: np.ndarray
    n2: int


def row_range(m: int, G: int, g: int):
    """Rows of rank g: contiguous blocks, the first m % G ranks get one extra row."""
    base, extra = divmod(m, G)
    lo = g * base + min(g, extra)
    return lo, lo + base + (1 if g < extra else 0)


def hip_local_stage(solver: GNSolver, m_loc, n, t, dJ, ldj, drx, dAt, dcx, dR, dz, eps_rank):
    """enlsip_gn_tsqr_local_dev on raw device pointers; returns (n2, tail_sq)."""
    tail = C.c_double(0.0)
    n2 = C.c_int64(0)
    v = lambda x: C.c_void_p(x) if x else None
    solver._chk(solver._lib.enlsip_gn_tsqr_local_dev(solver._h, m_loc, n, t, v(dJ), ldj, v(drx), v(dAt), max(n, 1),
                                                     v(dcx), eps_rank, v(dR), v(dz), C.byref(tail), C.byref(n2)))
    return int(n2.value), float(tail.value)


def hip_combine_stage(solver: GNSolver, G, n, n2, dRstack, dzstack, eps_rank):
    p = np.zeros(n)
    dlead = np.zeros(n2)
    jp = np.zeros(n2, dtype=np.int64)
    ct = C.c_double(0.0)
    info = L.Info()
    v = lambda x: C.c_void_p(x) if x else None
    solver._chk(solver._lib.enlsip_gn_tsqr_combine_dev(solver._h, G, n2, v(dRstack), v(dzstack), eps_rank,
                                                       p.ctypes.data_as(C.c_void_p), dlead.ctypes.data_as(C.c_void_p),
                                                       C.byref(ct), C.byref(info), jp.ctypes.data_as(C.c_void_p)))
    return p, dlead, float(ct.value), info, jp


def hip_local_stage_scaled(solver: GNSolver, m_loc, n, t, dJ, ldj, drx, dAt, dcx, dR, dz, eps_rank):
    """enlsip_gn_tsqr_local_scaled_dev on raw device pointers; returns (n2, tail_sq, e): R, z and tail_sq are those of the shard
    times 2^-e (tail_sq: 2^-2e)."""
    tail = C.c_double(0.0)
    n2 = C.c_int64(0)
    e = C.c_int64(0)
    v = lambda x: C.c_void_p(x) if x else None
    solver._chk(solver._lib.enlsip_gn_tsqr_local_scaled_dev(solver._h, m_loc, n, t, v(dJ), ldj, v(drx), v(dAt), max(n, 1),
                                                            v(dcx), eps_rank, v(dR), v(dz), C.byref(tail), C.byref(n2),
                                                            C.byref(e)))
    return int(n2.value), float(tail.value), int(e.value)


def hip_combine_stage_scaled(solver: GNSolver, G, n, n2, dRstack, dzstack, e, tail_sq, eps_rank):
    """enlsip_gn_tsqr_combine_scaled_dev: ``e`` / ``tail_sq`` are the G ranks' exponents and tail^2 (each at its rank's scale);
    returns (p, dlead, d_norm, info, jpvtJ2) of the unscaled problem."""
    p = np.zeros(n)
    dlead = np.zeros(n2)
    jp = np.zeros(n2, dtype=np.int64)
    dn = C.c_double(0.0)
    info = L.Info()
    ee = np.ascontiguousarray(e, dtype=np.int64)
    tt = np.ascontiguousarray(tail_sq, dtype=np.float64)
    assert ee.shape == (G,) and tt.shape == (G,)
    v = lambda x: C.c_void_p(x) if x else None
    solver._chk(solver._lib.enlsip_gn_tsqr_combine_scaled_dev(solver._h, G, n2, v(dRstack), v(dzstack),
                                                              ee.ctypes.data_as(C.c_void_p), tt.ctypes.data_as(C.c_void_p),
                                                              eps_rank, p.ctypes.data_as(C.c_void_p),
                                                              dlead.ctypes.data_as(C.c_void_p), C.byref(dn), C.byref(info),
                                                              jp.ctypes.data_as(C.c_void_p)))
    return p, dlead, float(dn.value), info, jp


def tsqr_scale(solver: GNSolver):
    """(e_local, e_common) of the handle's last TSQR call (enlsip_gn_tsqr_get_scale); (0, 0) for inputs inside the band."""
    a, b = C.c_int64(0), C.c_int64(0)
    solver._chk(solver._lib.enlsip_gn_tsqr_get_scale(solver._h, C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def tsqr_solve(solver: Optional[GNSolver], J_loc, rx_loc, At, cx, eps_rank: float = SQRT_EPS, group=None,
               local_stage: Callable = None, combine_stage: Callable = None, scaled: bool = False) -> TSQRResult:
    """Collective over ``group``.  ``J_loc``: torch tensor (n, m_loc) C-order == column-major
    m_loc x n on this rank's device; ``rx_loc`` (m_loc); ``At`` (t, n) C-order == column-major n x t
    (replicated); ``cx`` (t).  Every rank returns the same result.

    ``scaled``: the stages that carry a per-rank exponent.  An injected ``local_stage`` then returns ``(n2, tail_sq, e)`` and an
    injected ``combine_stage`` is called as ``combine_stage(G, n, n2, Rstack, zstack, e, tail_sq, eps_rank)`` with the gathered
    exponents (int64, G) and tail^2 (G, each at its rank's scale) and returns ``d_norm`` where the unscaled one returns its part
    of the sum of squares."""
    import torch
    import torch.distributed as dist
    if scaled:
        return _tsqr_solve_scaled(solver, J_loc, rx_loc, At, cx, eps_rank, group, local_stage, combine_stage)

    G = dist.get_world_size(group) if dist.is_initialized() else 1
    n, m_loc = J_loc.shape
    t = 0 if At is None else At.shape[0]
    dev = J_loc.device
    # no fill: k_tsqr_extract writes every entry it hands back, and a fill on torch's stream would not be ordered against the
    # library's own stream
    R = torch.empty((n * n,), dtype=torch.float64, device=dev)
    z = torch.empty((n,), dtype=torch.float64, device=dev)
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()      # inputs produced on torch's stream are complete before the library reads them
    if local_stage is None:
        n2, tail = hip_local_stage(solver, m_loc, n, t, J_loc.data_ptr(), m_loc, rx_loc.data_ptr(),
                                   At.data_ptr() if t else 0, cx.data_ptr() if t else 0, R.data_ptr(), z.data_ptr(),
                                   eps_rank)
    else:
        n2, tail = local_stage(J_loc, rx_loc, At, cx, R, z, eps_rank)
    # ---- the one exchange step --------------------------------------------------------------------
    Rstack = torch.empty((G * n2 * n2,), dtype=torch.float64, device=dev)
    zstack = torch.empty((G * n2,), dtype=torch.float64, device=dev)
    tails = torch.tensor([tail], dtype=torch.float64, device=dev)
    if G > 1:
        if dev.type == "cuda" and dist.get_backend(group) != "nccl":
            # rehearsal only (several ranks on one GPU under gloo, tests/tsqr_rank_worker.py): RCCL refuses two ranks on one
            # device, gloo moves host tensors
            Rc, zc, tc = torch.empty(Rstack.shape, dtype=torch.float64), torch.empty(zstack.shape, dtype=torch.float64), tails.cpu()
            dist.all_gather_into_tensor(Rc, R[: n2 * n2].cpu().contiguous(), group=group)
            dist.all_gather_into_tensor(zc, z[:n2].cpu().contiguous(), group=group)
            dist.all_reduce(tc, op=dist.ReduceOp.SUM, group=group)
            Rstack.copy_(Rc); zstack.copy_(zc); tails.copy_(tc)
        else:
            dist.all_gather_into_tensor(Rstack, R[: n2 * n2].contiguous(), group=group)
            dist.all_gather_into_tensor(zstack, z[:n2].contiguous(), group=group)
            dist.all_reduce(tails, op=dist.ReduceOp.SUM, group=group)
    else:
        Rstack.copy_(R[: n2 * n2])
        zstack.copy_(z[:n2])
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()      # the library runs on its own stream
    if combine_stage is None:
        p, dlead, ctail, info, jp = hip_combine_stage(solver, G, n, n2, Rstack.data_ptr(), zstack.data_ptr(), eps_rank)
        rankA, rankJ2, code = int(info.rankA), int(info.rankJ2), int(info.code)
    else:
        p, dlead, ctail, rankA, rankJ2, code, jp = combine_stage(G, n, n2, Rstack, zstack, eps_rank)
    d_norm = float(np.sqrt(float(tails.item()) + ctail + float(np.dot(dlead, dlead))))
    return TSQRResult(p=p, dlead=dlead, d_norm=d_norm, rankA=rankA, rankJ2=rankJ2, code=code, jpvtJ2=jp, n2=n2)


def _tsqr_solve_scaled(solver, J_loc, rx_loc, At, cx, eps_rank, group, local_stage, combine_stage) -> TSQRResult:
    """tsqr_solve(scaled=True): the same exchange step, with (e_g, tail_g^2) gathered instead of the tails summed — a sum of
    squares taken at different scales means nothing, and one taken at the largest scale may overflow."""
    import torch
    import torch.distributed as dist

    G = dist.get_world_size(group) if dist.is_initialized() else 1
    n, m_loc = J_loc.shape
    t = 0 if At is None else At.shape[0]
    dev = J_loc.device
    R = torch.empty((n * n,), dtype=torch.float64, device=dev)
    z = torch.empty((n,), dtype=torch.float64, device=dev)
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()
    if local_stage is None:
        n2, tail, e = hip_local_stage_scaled(solver, m_loc, n, t, J_loc.data_ptr(), m_loc, rx_loc.data_ptr(),
                                             At.data_ptr() if t else 0, cx.data_ptr() if t else 0, R.data_ptr(), z.data_ptr(),
                                             eps_rank)
    else:
        n2, tail, e = local_stage(J_loc, rx_loc, At, cx, R, z, eps_rank)
    # ---- the one exchange step: triangles, vectors and (e_g, tail_g^2), the exponent as an exact small double --------------
    Rstack = torch.empty((G * n2 * n2,), dtype=torch.float64, device=dev)
    zstack = torch.empty((G * n2,), dtype=torch.float64, device=dev)
    mine = torch.tensor([float(e), tail], dtype=torch.float64)
    every = torch.empty((2 * G,), dtype=torch.float64)
    if G > 1:
        host_path = dev.type == "cuda" and dist.get_backend(group) != "nccl"      # rehearsal: several ranks on one GPU under gloo
        if host_path:
            Rc, zc = torch.empty(Rstack.shape, dtype=torch.float64), torch.empty(zstack.shape, dtype=torch.float64)
            dist.all_gather_into_tensor(Rc, R[: n2 * n2].cpu().contiguous(), group=group)
            dist.all_gather_into_tensor(zc, z[:n2].cpu().contiguous(), group=group)
            dist.all_gather_into_tensor(every, mine, group=group)
            Rstack.copy_(Rc); zstack.copy_(zc)
        else:
            dist.all_gather_into_tensor(Rstack, R[: n2 * n2].contiguous(), group=group)
            dist.all_gather_into_tensor(zstack, z[:n2].contiguous(), group=group)
            if dev.type == "cuda":
                ev = every.to(dev)
                dist.all_gather_into_tensor(ev, mine.to(dev), group=group)
                every = ev.cpu()
            else:
                dist.all_gather_into_tensor(every, mine, group=group)
    else:
        Rstack.copy_(R[: n2 * n2])
        zstack.copy_(z[:n2])
        every.copy_(mine)
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()
    pairs = every.numpy().reshape(G, 2)
    es, tails = pairs[:, 0].astype(np.int64), pairs[:, 1].copy()
    if combine_stage is None:
        p, dlead, d_norm, info, jp = hip_combine_stage_scaled(solver, G, n, n2, Rstack.data_ptr(), zstack.data_ptr(), es, tails,
                                                              eps_rank)
        rankA, rankJ2, code = int(info.rankA), int(info.rankJ2), int(info.code)
    else:
        p, dlead, d_norm, rankA, rankJ2, code, jp = combine_stage(G, n, n2, Rstack, zstack, es, tails, eps_rank)
    return TSQRResult(p=p, dlead=dlead, d_norm=float(d_norm), rankA=rankA, rankJ2=rankJ2, code=code, jpvtJ2=jp, n2=n2)


# ---- the collective inside the library (enlsip_gn_solve_tsqr) --------------------------------------------------------------
def tsqr_attach(solver: GNSolver, group=None, transport: str = "rccl"):
    """Give the handle its communicator for ``tsqr_solve_lib`` (collective over ``group``).

    ``rccl``: rank 0 asks the library for an RCCL unique id, ``torch.distributed`` only carries those 128 bytes to the other
    ranks, and every rank lets the library create its own RCCL communicator (ncclCommInitRank) — the data path never touches
    torch.  ``host``: an all-gather callback that stages through host memory and the group's (gloo) backend — the rehearsal
    transport for several ranks on ONE GPU, which RCCL refuses."""
    import torch
    import torch.distributed as dist
    G = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    lib, h = solver._lib, solver._h
    if G == 1 and transport != "rccl":
        solver._chk(lib.enlsip_gn_tsqr_set_exchange(h, None, None, 1, 0))
        return
    if transport == "rccl":
        # also with ONE rank: the library then runs its exchange as a self-gather through RCCL (transport "rccl" in
        # tsqr_transport), so the RCCL leg is exercised on a one-GPU box
        ident = C.create_string_buffer(128)
        if rank == 0:
            rc = lib.enlsip_gn_tsqr_unique_id(ident)
            if rc != 0:
                raise RuntimeError(f"enlsip_gn_tsqr_unique_id failed with code {rc} (RCCL not loadable?)")
        if G > 1:
            box = [ident.raw if rank == 0 else None]
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            ident = C.create_string_buffer(box[0], 128)
        solver._chk(lib.enlsip_gn_tsqr_init_rccl(h, ident, G, rank))
        return
    if transport != "host":
        raise ValueError(transport)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int

    def _gather(ctx, dsend, drecv, nbytes, stream):
        try:
            mine = torch.empty(nbytes, dtype=torch.uint8)
            if hip.hipMemcpy(mine.data_ptr(), dsend, nbytes, 2) != 0:          # hipMemcpyDeviceToHost
                return 1
            every = torch.empty(G * nbytes, dtype=torch.uint8)
            dist.all_gather_into_tensor(every, mine, group=group)
            return 2 if hip.hipMemcpy(drecv, every.data_ptr(), G * nbytes, 1) != 0 else 0      # hipMemcpyHostToDevice
        except Exception:                                                           # never unwind through the C frames
            return 3

    cb = L.ALLGATHER_FN(_gather)
    solver._tsqr_cb = cb                                                            # keep the thunk alive with the handle
    solver._chk(lib.enlsip_gn_tsqr_set_exchange(h, C.cast(cb, C.c_void_p), None, G, rank))


def tsqr_solve_lib(solver: GNSolver, J_loc, rx_loc, At, cx, eps_rank: float = SQRT_EPS) -> TSQRResult:
    """``enlsip_gn_solve_tsqr``: collective over the communicator attached with ``tsqr_attach``.  Arguments as ``tsqr_solve``;
    the inputs must be complete (synchronise the producing stream first: the library runs on its own)."""
    n, m_loc = J_loc.shape
    t = 0 if At is None else At.shape[0]
    p, dlead, jp = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    dn = C.c_double(0.0)
    info = L.Info()
    v = lambda x: C.c_void_p(x) if x else None
    solver._chk(solver._lib.enlsip_gn_solve_tsqr(
        solver._h, m_loc, n, t, v(J_loc.data_ptr()), m_loc, v(rx_loc.data_ptr()), v(At.data_ptr()) if t else None, max(n, 1),
        v(cx.data_ptr()) if t else None, eps_rank, p.ctypes.data_as(C.c_void_p), dlead.ctypes.data_as(C.c_void_p),
        C.byref(dn), C.byref(info), jp.ctypes.data_as(C.c_void_p)))
    n2 = n - int(info.rankA)
    return TSQRResult(p=p, dlead=dlead[:n2].copy(), d_norm=float(dn.value), rankA=int(info.rankA), rankJ2=int(info.rankJ2),
                      code=int(info.code), jpvtJ2=jp[:n2].copy(), n2=n2)


TRANSPORT_NAMES = {0: "none", 1: "rccl", 2: "callback"}


def tsqr_transport(solver: GNSolver) -> str:
    """What moved the messages in the handle's last ``enlsip_gn_solve_tsqr``: "none" (one rank, device copy), "rccl", "callback"."""
    code = C.c_int(-1)
    solver._chk(solver._lib.enlsip_gn_tsqr_get_transport(solver._h, C.byref(code)))
    return TRANSPORT_NAMES.get(int(code.value), str(code.value))


def tsqr_exchange(solver: GNSolver) -> dict:
    """Transport, rank count and rank tags seen in the handle's last ``enlsip_gn_solve_tsqr`` (enlsip_gn_tsqr_get_exchange):
    ``rank_tags_seen == ranks`` means one message from each distinct rank arrived in its slot."""
    tr, rk, seen = C.c_int(-1), C.c_int(0), C.c_int(-1)
    solver._chk(solver._lib.enlsip_gn_tsqr_get_exchange(solver._h, C.byref(tr), C.byref(rk), C.byref(seen)))
    return {"transport": TRANSPORT_NAMES.get(int(tr.value), str(tr.value)), "ranks": int(rk.value), "rank_tags_seen": int(seen.value)}


def tsqr_stage_ms(solver: GNSolver):
    arr = (C.c_float * 3)()
    solver._chk(solver._lib.enlsip_gn_tsqr_get_stage_ms(solver._h, arr))
    return {"local": float(arr[0]), "exchange": float(arr[1]), "combine": float(arr[2])}


def tsqr_solve_shards_dev(solver: GNSolver, Jd, rxd, Atd, cxd, G: int, eps_rank: float = SQRT_EPS, scaled: bool = False,
                          row_blocks=None, in_place: bool = False) -> TSQRResult:
    """Single-process rehearsal on ONE GPU with the data already in HBM: ``Jd`` (n, m) C-order == column-major m x n,
    ``rxd`` (m), ``Atd`` (t, n) C-order == column-major n x t or None, ``cxd`` (t) or None.  The G row blocks are factored one after
    the other on the same handle and stacked exactly as the all-gather would (the handle's resident F_A / p1 come from the
    last local stage, identical on every 'rank').  ``row_blocks``: the G block heights (default: ``row_range``).  ``scaled``: the
    stages that carry each block's exponent (magnitudes outside 2^-400 .. 2^400).  ``in_place``: the local stage reads block g
    where it lies, ``J + lo`` with ``ldj = m`` and ``rx + lo``, as a caller with one resident matrix would shard it (an odd ``lo``
    gives a base that is 8-byte but not 16-byte aligned); default: a contiguous copy of the block with ``ldj = m_loc``."""
    import torch
    n, m = Jd.shape
    if in_place and not (Jd.is_contiguous() and rxd.is_contiguous() and Jd.dtype == rxd.dtype == torch.float64):
        raise ValueError("in_place needs contiguous float64 Jd and rxd")
    t = 0 if Atd is None else Atd.shape[0]
    dev = Jd.device
    if row_blocks is None:
        edges = [row_range(m, G, g) for g in range(G)]
    else:
        if len(row_blocks) != G or sum(row_blocks) != m or min(row_blocks) < 1:
            raise ValueError("row_blocks must be G positive heights that add up to m")
        ends = np.cumsum(row_blocks)
        edges = [(int(b - a), int(b)) for a, b in zip(row_blocks, ends)]
    Rs, zs, tail_total, n2 = [], [], 0.0, None
    es, tails = [], []
    for g in range(G):
        lo, hi = edges[g]
        if in_place:
            Jl, rl = None, None
            pJ, ldj, prx = Jd.data_ptr() + 8 * lo, m, rxd.data_ptr() + 8 * lo
        else:
            Jl = Jd[:, lo:hi].contiguous()             # column-major (hi - lo) x n
            rl = rxd[lo:hi].contiguous()
            pJ, ldj, prx = Jl.data_ptr(), hi - lo, rl.data_ptr()
        R = torch.empty((n * n,), dtype=torch.float64, device=dev)      # k_tsqr_extract writes all n2 * n2 / n2 entries it hands back
        z = torch.empty((n,), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)                    # the library runs on its own stream
        if scaled:
            n2, tail, e = hip_local_stage_scaled(solver, hi - lo, n, t, pJ, ldj, prx,
                                                 Atd.data_ptr() if t else 0, cxd.data_ptr() if t else 0, R.data_ptr(),
                                                 z.data_ptr(), eps_rank)
            es.append(e)
            tails.append(tail)
        else:
            n2, tail = hip_local_stage(solver, hi - lo, n, t, pJ, ldj, prx,
                                       Atd.data_ptr() if t else 0, cxd.data_ptr() if t else 0, R.data_ptr(), z.data_ptr(),
                                       eps_rank)
            tail_total += tail
        Rs.append(R[: n2 * n2].clone())
        zs.append(z[:n2].clone())
        del Jl, rl
    Rstack = torch.cat(Rs).contiguous()
    zstack = torch.cat(zs).contiguous()
    torch.cuda.synchronize(dev)
    if scaled:
        p, dlead, d_norm, info, jp = hip_combine_stage_scaled(solver, G, n, n2, Rstack.data_ptr(), zstack.data_ptr(), es, tails,
                                                              eps_rank)
        return TSQRResult(p=p, dlead=dlead, d_norm=d_norm, rankA=int(info.rankA), rankJ2=int(info.rankJ2),
                          code=int(info.code), jpvtJ2=jp, n2=n2)
    p, dlead, ctail, info, jp = hip_combine_stage(solver, G, n, n2, Rstack.data_ptr(), zstack.data_ptr(), eps_rank)
    d_norm = float(np.sqrt(tail_total + ctail + float(np.dot(dlead, dlead))))
    return TSQRResult(p=p, dlead=dlead, d_norm=d_norm, rankA=int(info.rankA), rankJ2=int(info.rankJ2),
                      code=int(info.code), jpvtJ2=jp, n2=n2)


def tsqr_solve_shards(solver: GNSolver, J, rx, A_active, cx, G: int, eps_rank: float = SQRT_EPS, scaled: bool = False,
                      row_blocks=None, in_place: bool = False) -> TSQRResult:
    """Same, host arrays in: ``J`` (m, n), ``rx`` (m), ``A_active`` (t, n), ``cx`` (t)."""
    import torch
    t = A_active.shape[0]
    dev = torch.device("cuda", 0)
    Jd = torch.tensor(np.ascontiguousarray(np.asarray(J).T), dtype=torch.float64, device=dev)
    rxd = torch.tensor(np.asarray(rx), dtype=torch.float64, device=dev)
    Atd = torch.tensor(np.ascontiguousarray(A_active), dtype=torch.float64, device=dev) if t else None
    cxd = torch.tensor(np.asarray(cx), dtype=torch.float64, device=dev) if t else None
    return tsqr_solve_shards_dev(solver, Jd, rxd, Atd, cxd, G, eps_rank, scaled=scaled, row_blocks=row_blocks, in_place=in_place)


# ---- the consumers around the subproblem on a row-sharded J (enlsip_gn_tsqr_products*) ----------------------------------------
PRODUCTS_HDR = 4          # [rank + 1 | rank count | n | 0], then g (n), then dot(rx,rx), dot(Jp,Jp), dot(Jp,rx)


def tsqr_products_msg_len(n: int) -> int:
    """Doubles per message (enlsip_gn_tsqr_products_msg_len): header, n, three sums, rounded up to 16-byte granules."""
    return (PRODUCTS_HDR + n + 3 + 1) & ~1


@dataclass
class TSQRProducts:
    grad: np.ndarray                 # J' (rx + J p) over all ranks (p None: J' rx)
    sums: np.ndarray                 # dot(rx,rx), dot(Jp,Jp), dot(Jp,rx) over all ranks
    Ap: Optional[np.ndarray] = None  # C.A p on the active rows (library collective with p and t > 0)
    Jp: object = None                # this rank's J_g p (device tensor), or the whole J p in the rehearsal


def _host(x, count=None):
    if x is None:
        return None, None
    a = np.ascontiguousarray(x, dtype=np.float64)
    assert count is None or a.shape == (count,), (a.shape, count)
    return a, a.ctypes.data_as(C.c_void_p)


def tsqr_products_lib(solver: GNSolver, n: int, t: int, p=None, Jp_out=None) -> TSQRProducts:
    """``enlsip_gn_tsqr_products``: collective on the shard and communicator of the handle's last ``tsqr_solve_lib``.  ``p`` (n) or
    None; ``Jp_out``: a device tensor of m_loc doubles that receives this rank's J_g p, or None."""
    pa, pp = _host(p, n)
    grad, sums = np.zeros(n), np.zeros(3)
    Ap = np.zeros(t) if (pa is not None and t > 0) else None
    solver._chk(solver._lib.enlsip_gn_tsqr_products(
        solver._h, pp, C.c_void_p(Jp_out.data_ptr()) if Jp_out is not None else None, grad.ctypes.data_as(C.c_void_p),
        sums.ctypes.data_as(C.c_void_p), Ap.ctypes.data_as(C.c_void_p) if Ap is not None else None))
    return TSQRProducts(grad=grad, sums=sums, Ap=Ap, Jp=Jp_out)


def tsqr_first_lagrange_lib(solver: GNSolver, n: int, t: int, grad_fx=None, diag_scale=None, eps_rank: float = SQRT_EPS):
    """``enlsip_gn_tsqr_first_lagrange`` -> (lambda (t), grad_res).  ``grad_fx`` None: J' rx over the ranks (collective)."""
    ga, gp = _host(grad_fx, n)
    da, dp = _host(diag_scale, t)
    lam = np.zeros(t)
    gres = C.c_double(0.0)
    solver._chk(solver._lib.enlsip_gn_tsqr_first_lagrange(solver._h, gp, dp, eps_rank, lam.ctypes.data_as(C.c_void_p),
                                                          C.byref(gres)))
    return lam, float(gres.value)


def tsqr_second_lagrange_lib(solver: GNSolver, n: int, t: int, p_gn, diag_scale=None, eps_rank: float = SQRT_EPS):
    """``enlsip_gn_tsqr_second_lagrange`` -> lambda (t).  Collective."""
    pa, pp = _host(p_gn, n)
    da, dp = _host(diag_scale, t)
    lam = np.zeros(t)
    solver._chk(solver._lib.enlsip_gn_tsqr_second_lagrange(solver._h, pp, dp, eps_rank, lam.ctypes.data_as(C.c_void_p)))
    return lam


def tsqr_newton_direction_lib(solver: GNSolver, n: int, Gamma):
    """``enlsip_gn_tsqr_newton_direction`` -> (p (n), not_posdef): newton_search_direction after its Hessian sums on the resident
    result of the handle's last sharded solve.  ``Gamma`` = r_mat - c_mat, (n, n); NumPy's C order is transposed into the column-major
    layout of the C ABI.  Not collective: nothing is exchanged, and ranks that pass the same Gamma get the same bits."""
    G = np.ascontiguousarray(np.asarray(Gamma, dtype=np.float64).T)
    assert G.shape == (n, n), (G.shape, n)
    p = np.zeros(n)
    bad = C.c_int64(0)
    solver._chk(solver._lib.enlsip_gn_tsqr_newton_direction(solver._h, G.ctypes.data_as(C.c_void_p), n, p.ctypes.data_as(C.c_void_p),
                                                            C.byref(bad)))
    return p, bool(bad.value)


def tsqr_newton_direction_dev(solver: GNSolver, n: int, Gamma_d, p_d=None, status_d=None, ldg: Optional[int] = None):
    """``enlsip_gn_tsqr_newton_direction_dev`` on torch device tensors -> (p_d, status_d).  ``Gamma_d``: float64, column-major n x n
    with leading dimension ``ldg`` (default n), i.e. a C-order (n, ldg) tensor holding Gamma'.  ``p_d`` (n, float64) and
    ``status_d`` (1, int32) are allocated when not given; status 1 = the symmetrised W22 is not positive definite, p = 0.  The inputs
    must be complete (the library runs on its own stream); the call returns after one synchronisation of that stream."""
    import torch
    dev = Gamma_d.device
    if p_d is None:
        p_d = torch.zeros(n, dtype=torch.float64, device=dev)
    if status_d is None:
        status_d = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    solver._chk(solver._lib.enlsip_gn_tsqr_newton_direction_dev(solver._h, C.c_void_p(Gamma_d.data_ptr()), n if ldg is None else ldg,
                                                                C.c_void_p(p_d.data_ptr()), C.c_void_p(status_d.data_ptr())))
    return p_d, status_d


def hip_products_local(solver: GNSolver, m_loc, n, dJ, ldj, drx, dp, dJp, dmsg):
    """enlsip_gn_tsqr_products_local_dev on raw device pointers (0: NULL)."""
    v = lambda x: C.c_void_p(x) if x else None
    solver._chk(solver._lib.enlsip_gn_tsqr_products_local_dev(solver._h, m_loc, n, v(dJ), ldj, v(drx), v(dp), v(dJp), v(dmsg)))


def hip_products_combine(solver: GNSolver, G, n, dmsgs):
    grad, sums = np.zeros(n), np.zeros(3)
    solver._chk(solver._lib.enlsip_gn_tsqr_products_combine_dev(solver._h, G, n, C.c_void_p(dmsgs) if dmsgs else None,
                                                                grad.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p)))
    return grad, sums


def products_combine_host(msgs: np.ndarray, G: int, n: int):
    """The combine on the host: the G messages added in rank order, rank 0's value first, with plain additions — the same IEEE
    operations in the same order as the device combine, hence the same bits.  Raises on a header that does not fit."""
    L = tsqr_products_msg_len(n)
    M = np.asarray(msgs, dtype=np.float64).reshape(G, L)
    for g in range(G):
        rk, cnt, nn = M[g, 0], M[g, 1], M[g, 2]
        if nn != n or cnt not in (0.0, float(G)) or rk not in (0.0, float(g + 1)):
            raise ValueError(f"message {g}: header (rank+1, ranks, n) = ({rk}, {cnt}, {nn}) does not fit slot {g} of {G}, n = {n}")
    acc = M[0, PRODUCTS_HDR:PRODUCTS_HDR + n + 3].copy()
    for g in range(1, G):
        acc = acc + M[g, PRODUCTS_HDR:PRODUCTS_HDR + n + 3]
    return acc[:n].copy(), acc[n:n + 3].copy()


def tsqr_products(solver: Optional[GNSolver], J_loc, rx_loc, p, group=None, local_stage: Callable = None) -> TSQRProducts:
    """The stage form, collective over ``group``: local products, ONE all-gather of the messages, the combine on every rank.
    ``J_loc`` (n, m_loc) C-order == column-major m_loc x n, ``rx_loc`` (m_loc): torch tensors on this rank's device; ``p``: (n)
    array-like or None.  ``local_stage(J_loc, rx_loc, p, msg)`` fills the message tensor (body; the header's n) and returns this
    rank's J p or None — a NumPy stage can stand in without a GPU; the combine then runs on the host.  Every rank returns the same
    bits."""
    import torch
    import torch.distributed as dist
    G = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    n, m_loc = J_loc.shape
    dev = J_loc.device
    L = tsqr_products_msg_len(n)
    msg = torch.zeros((L,), dtype=torch.float64, device=dev)
    Jp = None
    if local_stage is None:
        pd = torch.as_tensor(np.asarray(p, dtype=np.float64), device=dev) if p is not None else None
        Jp = torch.empty((max(m_loc, 1),), dtype=torch.float64, device=dev)[:m_loc] if p is not None else None
        if dev.type == "cuda":
            torch.cuda.current_stream(dev).synchronize()      # the library runs on its own stream
        hip_products_local(solver, m_loc, n, J_loc.data_ptr() if m_loc else 0, max(m_loc, 0), rx_loc.data_ptr() if m_loc else 0,
                           pd.data_ptr() if pd is not None else 0, Jp.data_ptr() if (Jp is not None and m_loc) else 0,
                           msg.data_ptr())
    else:
        Jp = local_stage(J_loc, rx_loc, p, msg)
    msg[0], msg[1], msg[2] = float(rank + 1), float(G), float(n)      # the sender states its slot and the count it believes in
    every = torch.empty((G * L,), dtype=torch.float64, device=dev)
    if G > 1:
        if dev.type == "cuda" and dist.get_backend(group) != "nccl":   # rehearsal: several ranks on one GPU under gloo
            ec = torch.empty((G * L,), dtype=torch.float64)
            dist.all_gather_into_tensor(ec, msg.cpu().contiguous(), group=group)
            every.copy_(ec)
        else:
            dist.all_gather_into_tensor(every, msg.contiguous(), group=group)
    else:
        every.copy_(msg)
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()
    if local_stage is None:
        grad, sums = hip_products_combine(solver, G, n, every.data_ptr())
    else:
        grad, sums = products_combine_host(every.cpu().numpy(), G, n)
    return TSQRProducts(grad=grad, sums=sums, Jp=Jp)


def tsqr_products_shards_dev(solver: GNSolver, Jd, rxd, p, G: int, row_blocks=None, in_place: bool = False) -> TSQRProducts:
    """Single-process rehearsal on ONE GPU: ``Jd`` (n, m) C-order == column-major m x n, ``rxd`` (m) in HBM.  The G row blocks go
    through ``enlsip_gn_tsqr_products_local_dev`` one after the other on the same handle, each message stated as rank g of G, and
    ``enlsip_gn_tsqr_products_combine_dev`` adds them as the all-gather would have stacked them.  ``row_blocks``: the G block
    heights (zero allowed; default ``row_range``).  ``in_place``: block g is read where it lies, ``J + lo`` with ``ldj = m``."""
    import torch
    n, m = Jd.shape
    if in_place and not (Jd.is_contiguous() and rxd.is_contiguous() and Jd.dtype == rxd.dtype == torch.float64):
        raise ValueError("in_place needs contiguous float64 Jd and rxd")
    dev = Jd.device
    if row_blocks is None:
        edges = [row_range(m, G, g) for g in range(G)]
    else:
        if len(row_blocks) != G or sum(row_blocks) != m or min(row_blocks) < 0:
            raise ValueError("row_blocks must be G non-negative heights that add up to m")
        ends = np.cumsum(row_blocks)
        edges = [(int(b - a), int(b)) for a, b in zip(row_blocks, ends)]
    L = tsqr_products_msg_len(n)
    msgs = torch.zeros((G, L), dtype=torch.float64, device=dev)
    pd = torch.as_tensor(np.asarray(p, dtype=np.float64), device=dev) if p is not None else None
    Jp = torch.zeros((m,), dtype=torch.float64, device=dev) if p is not None else None
    for g in range(G):
        lo, hi = edges[g]
        ml = hi - lo
        if in_place:
            Jl, rl = None, None
            pJ, ldj, prx = Jd.data_ptr() + 8 * lo, m, rxd.data_ptr() + 8 * lo
        else:
            Jl = Jd[:, lo:hi].contiguous()
            rl = rxd[lo:hi].contiguous()
            pJ, ldj, prx = Jl.data_ptr(), ml, rl.data_ptr()
        torch.cuda.synchronize(dev)                    # the library runs on its own stream
        hip_products_local(solver, ml, n, pJ if ml else 0, ldj if ml else 0, prx if ml else 0, pd.data_ptr() if pd is not None else 0,
                           (Jp.data_ptr() + 8 * lo) if (Jp is not None and ml) else 0, msgs[g].data_ptr())
        del Jl, rl
    msgs[:, 0] = torch.arange(1, G + 1, dtype=torch.float64, device=dev)
    msgs[:, 1] = float(G)
    torch.cuda.synchronize(dev)
    grad, sums = hip_products_combine(solver, G, n, msgs.data_ptr())
    return TSQRProducts(grad=grad, sums=sums, Jp=Jp)
