"""The deletion test and the working-set edit of a batch on device buffers (enlsip_gn_delete_constraints_batched_dev,
enlsip_gn_restore_constraints_batched_dev) and the driver built on them (working_set.update_working_set_batched_dev).  Every
comparison is exact: the outputs are indices or copies of input bytes."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import synth

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

BATCH = 67      # not a multiple of four: the last workgroup of the wave form is partly empty
SHAPES = [(1, 1), (3, 2), (32, 4), (64, 64), (65, 64), (64, 65), (7, 130)]      # (n, t_max)


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ref_solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def rc_of(call):
    try:
        call()
    except Exception as e:      # GNError: "libenlsip_gn error <rc>: ..."
        return int(re.search(r"error (-?\d+)", str(e)).group(1))
    return 0


class Buffers:
    """Host images of the device buffers of one call, NaN outside the live entries, and their upload."""

    def __init__(self, n, t_max, t, padded, seed):
        rng = np.random.default_rng(seed)
        B = len(t)
        self.n, self.t_max, self.t, self.B = n, t_max, np.asarray(t, dtype=np.int64), B
        self.ldat = n + 3 if padded else n
        self.strideAt = self.ldat * t_max + (5 if padded else 0)
        self.At = np.full((B, self.strideAt), np.nan)
        self.cx, self.lam, self.ds = (np.full((B, t_max), np.nan) for _ in range(3))
        self.gres = np.where(np.arange(B) % 3 == 0, 0.0, np.where(np.arange(B) % 3 == 1, 10.0 * np.abs(rng.standard_normal(B)), 1e-3))
        self.saved = np.full((B, n + 3), np.nan)
        for k in range(B):
            tk = int(self.t[k])
            self.block(k)[:tk, :n] = rng.standard_normal((tk, n))
            self.cx[k, :tk] = rng.standard_normal(tk)
            self.lam[k, :tk] = rng.standard_normal(tk)
            self.ds[k, :tk] = rng.uniform(0.5, 2.0, tk) if k % 2 else 1.0
            if k % 5 == 0 and tk >= 2:      # a tie
                self.lam[k, tk - 2], self.ds[k, tk - 2] = self.lam[k, tk - 1], self.ds[k, tk - 1]
        self.names = ("At", "cx", "lam", "ds", "saved", "gres")

    def block(self, k, At=None):
        """problem k's A' block as (t_max, ldat): row c is column c of the column-major block"""
        At = self.At if At is None else At
        return At[k, :self.ldat * self.t_max].reshape(self.t_max, self.ldat)

    def images(self):
        return {nm: getattr(self, nm).copy() for nm in self.names}

    def upload(self):
        import torch
        self.dev = {nm: torch.from_numpy(getattr(self, nm).copy()).to("cuda:0") for nm in self.names}
        torch.cuda.synchronize()
        return self.dev

    def download(self):
        import torch
        torch.cuda.synchronize()
        return {nm: self.dev[nm].cpu().numpy() for nm in self.names}

    def ptr(self, nm):
        return self.dev[nm].data_ptr()

    def a_args(self):
        return self.ptr("At"), self.ldat, self.strideAt, self.ptr("cx")


def host_s(q, lam, scaling, ds, grad_res):
    from enlsip_gn import check_constraint_deletion
    return check_constraint_deletion(q, lam, scaling, ds, grad_res)


def model_delete(buf, img, s, t, with_saved=True):
    """delete-and-pad in NumPy on the images, in place"""
    n = buf.n
    for k in np.flatnonzero(s):
        sk, tk = int(s[k]), int(t[k])
        blk = buf.block(k, img["At"])
        if with_saved:
            img["saved"][k, :n] = blk[sk - 1, :n]
            img["saved"][k, n:] = img["cx"][k, sk - 1], img["lam"][k, sk - 1], img["ds"][k, sk - 1]
        blk[sk - 1:tk - 1, :n] = blk[sk:tk, :n].copy()
        blk[tk - 1, :n] = 0.0
        for nm, pad in (("cx", 0.0), ("lam", 0.0), ("ds", 1.0)):
            img[nm][k, sk - 1:tk - 1] = img[nm][k, sk:tk].copy()
            img[nm][k, tk - 1] = pad


def same_images(got, want):
    for nm in want:
        assert got[nm].tobytes() == want[nm].tobytes(), nm


def batch_t_q(t_max, seed, batch=BATCH):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, t_max + 1, batch)
    t[1], t[2] = 0, t_max
    t[batch - 1] = t_max
    q = np.array([rng.integers(0, tk + 1) for tk in t], dtype=np.int64)
    q[2] = 0
    return t.astype(np.int64), q


# ---- 1. decision and edit, 3. restore ----------------------------------------------------------------------------------------------
def edit_cases(n, t_max, padded, batch=BATCH):
    """The inputs of test 1 / 3 with what the host routine and the NumPy model say about them (no GPU involved): per case the
    buffers, scaling, take, the expected s, the expected images after the delete and the rows to put back."""
    t, q = batch_t_q(t_max, seed=n * 1000 + t_max, batch=batch)
    rng = np.random.default_rng(5)
    cases = []
    for scaling, take, gres, record in ((True, None, True, True), (False, (rng.random(batch) < 0.6).astype(np.int64), True, True),
                                        (True, None, False, False)):      # the last: the second-order form, no record
        buf = Buffers(n, t_max, t, padded, seed=n + 7 * t_max + int(scaling) + 2 * int(gres))
        want = buf.images()
        s_want = np.array([host_s(int(q[k]), buf.lam[k, :t[k]], scaling, buf.ds[k, :t[k]], buf.gres[k] if gres else 0.0)
                           if (take is None or take[k]) else 0 for k in range(batch)], dtype=np.int64)
        assert s_want.any() and not s_want.all()
        model_delete(buf, want, s_want, t, with_saved=record)
        back = None
        if take is None and record:      # the rows to put back: a random half of the deleted ones, at least one, not all
            hit = np.flatnonzero(s_want)
            assert hit.size >= 2
            pick = rng.permutation(hit)[:max(1, hit.size // 2)]
            back = np.zeros(batch, dtype=np.int64)
            back[pick] = s_want[pick]
        cases.append(dict(buf=buf, t=t, q=q, scaling=scaling, take=take, gres=gres, record=record, s=s_want, want=want, back=back))
    return cases


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("n,t_max", SHAPES)
def test_decision_edit_and_restore(solver, n, t_max, padded):
    form = 1 if (n <= 64 and t_max <= 64) else 0
    for c in edit_cases(n, t_max, padded):
        buf, t, q = c["buf"], c["t"], c["q"]
        buf.upload()
        s = solver.delete_constraints_batched_dev(BATCH, n, t_max, t, q, c["scaling"], buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(),
                                                  dgrad_res=buf.ptr("gres") if c["gres"] else 0,
                                                  dsaved=buf.ptr("saved") if c["record"] else 0, take=c["take"])
        assert solver.deletion_form() == form
        assert np.array_equal(s, c["s"])
        after = buf.download()
        same_images(after, c["want"])
        if c["back"] is None:
            continue
        # restore a random subset of the deleted rows: those slots are the original bytes, the others stay
        orig, back = buf.images(), c["back"]
        t1 = t - (s != 0)
        solver.restore_constraints_batched_dev(BATCH, n, t_max, t1, back, buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(), buf.ptr("saved"))
        assert solver.deletion_form() == form
        got = buf.download()
        for nm in ("At", "cx", "lam", "ds"):
            for k in range(BATCH):
                src = orig if back[k] else after
                assert got[nm][k].tobytes() == src[nm][k].tobytes(), (nm, k)
        assert got["saved"].tobytes() == after["saved"].tobytes() and got["gres"].tobytes() == after["gres"].tobytes()
        # nothing to restore: nothing is written (and no buffer is needed for the record)
        solver.restore_constraints_batched_dev(BATCH, n, t_max, t1, np.zeros(BATCH, dtype=np.int64), buf.ptr("lam"), buf.ptr("ds"),
                                               *buf.a_args(), 0)
        same_images(buf.download(), got)


@pytest.mark.parametrize("n,t_max", [(8, 4), (80, 70)], ids=["wave", "general"])
def test_scratch_growth_changes_no_result(n, t_max):
    """the records of a call (device and pinned) grow between batch 3 and batch 40 on the SAME solver: the delete and the restore
    at batch 40 answer bit for bit as on a solver that never made the smaller calls"""
    from enlsip_gn import GNSolver

    def delete_and_restore(s, batch):
        t, q = batch_t_q(t_max, seed=40 * n + batch, batch=batch)
        buf = Buffers(n, t_max, t, True, seed=batch)
        buf.upload()
        sd = s.delete_constraints_batched_dev(batch, n, t_max, t, q, True, buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(),
                                              dgrad_res=buf.ptr("gres"), dsaved=buf.ptr("saved"))
        after = buf.download()
        s.restore_constraints_batched_dev(batch, n, t_max, t - (sd != 0), sd, buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(),
                                          buf.ptr("saved"))
        return sd, after, buf.download(), s.deletion_form()

    grown, fresh = GNSolver(device=0), GNSolver(device=0)
    try:
        small = delete_and_restore(grown, 3)
        got = delete_and_restore(grown, 40)
        want = delete_and_restore(fresh, 40)
        assert small[0].any() and want[0].any() and not want[0].all()      # rows were deleted and put back at both sizes
        assert got[3] == want[3] == (1 if n <= 64 else 0)
        assert got[0].tobytes() == want[0].tobytes()
        same_images(got[1], want[1])
        same_images(got[2], want[2])
    finally:
        grown.close()
        fresh.close()


# ---- 2. the edge inputs of the CPU file, through both forms ------------------------------------------------------------------------
@pytest.mark.parametrize("t_max", [8, 65])
def test_edges_through_both_forms(solver, t_max):
    import torch
    from test_deletion_test_host import edge_cases, oracle_s
    n = 3
    for scaling in (False, True):
        cases = [c for c in edge_cases() if c[3] == scaling]
        B = len(cases)
        t = np.array([len(c[2]) for c in cases], dtype=np.int64)
        q = np.array([c[1] for c in cases], dtype=np.int64)
        lam, ds = np.full((B, t_max), np.nan), np.full((B, t_max), np.nan)
        for k, c in enumerate(cases):
            lam[k, :t[k]], ds[k, :t[k]] = c[2], c[4]
        gres = np.array([c[5] for c in cases])
        want = np.array([oracle_s(c[1], c[2], c[3], c[4], c[5]) for c in cases], dtype=np.int64)
        d = {nm: torch.from_numpy(a).to("cuda:0") for nm, a in
             (("lam", lam), ("ds", ds), ("gres", gres), ("At", np.ones((B, n * t_max))), ("cx", np.ones((B, t_max))))}
        torch.cuda.synchronize()
        s = solver.delete_constraints_batched_dev(B, n, t_max, t, q, scaling, d["lam"].data_ptr(), d["ds"].data_ptr(),
                                                  d["At"].data_ptr(), n, n * t_max, d["cx"].data_ptr(), dgrad_res=d["gres"].data_ptr())
        assert solver.deletion_form() == (1 if t_max <= 64 else 0)
        assert np.array_equal(s, want), [(c[0], int(a), int(b)) for c, a, b in zip(cases, s, want) if a != b]


# ---- 4. errors, and the state of the handle ----------------------------------------------------------------------------------------
def test_argument_errors_leave_the_buffers(solver):
    n, t_max, B = 5, 4, 6
    t = np.array([4, 3, 0, 2, 4, 1], dtype=np.int64)
    q = np.array([1, 0, 0, 2, 0, 1], dtype=np.int64)
    buf = Buffers(n, t_max, t, True, seed=1)
    before = buf.images()
    buf.upload()
    L, h = solver._lib, solver._h
    v = lambda x: C.c_void_p(x) if x else None
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    s = np.full(B, -9, dtype=np.int64)

    def delete(batch=B, n=n, t_max=t_max, t=t, q=q, lam=buf.ptr("lam"), ds=buf.ptr("ds"), At=buf.ptr("At"), ldat=buf.ldat,
               stride=buf.strideAt, cx=buf.ptr("cx"), s=s):
        return L.enlsip_gn_delete_constraints_batched_dev(h, batch, n, t_max, hp(t), hp(q), None, 0, v(lam), v(ds), v(buf.ptr("gres")),
                                                          v(At), ldat, stride, v(cx), v(buf.ptr("saved")), hp(s))

    def restore(batch=B, t_max=t_max, t=t - 1 * (t > 0), sb=np.where(t > 0, 1, 0).astype(np.int64), lam=buf.ptr("lam"),
                ldat=buf.ldat, stride=buf.strideAt, saved=buf.ptr("saved")):
        return L.enlsip_gn_restore_constraints_batched_dev(h, batch, n, t_max, hp(t), hp(sb), v(lam), v(buf.ptr("ds")),
                                                           v(buf.ptr("At")), ldat, stride, v(buf.ptr("cx")), v(saved))

    def bad(vec, k, val):
        out = vec.copy()
        out[k] = val
        return out

    assert L.enlsip_gn_delete_constraints_batched_dev(None, B, n, t_max, hp(t), hp(q), None, 0, None, None, None, None, n, n * t_max,
                                                      None, None, hp(s)) == -1
    checks = [
        (lambda: delete(batch=0), -2), (lambda: restore(batch=0), -2),
        (lambda: delete(n=0), -3), (lambda: delete(t_max=1025), -3), (lambda: restore(t_max=1025), -3),
        (lambda: delete(t=None), -4), (lambda: delete(q=None), -4), (lambda: delete(s=None), -4),
        (lambda: delete(lam=0), -4), (lambda: delete(ds=0), -4),
        (lambda: delete(At=0), -4), (lambda: delete(cx=0), -4), (lambda: restore(t=None), -4),
        (lambda: restore(sb=None), -4), (lambda: restore(lam=0), -4),
        (lambda: delete(t=bad(t, 1, 5)), -5), (lambda: delete(t=bad(t, 1, -1)), -5),
        (lambda: restore(t=bad(t - 1 * (t > 0), 0, 4)), -5),                  # a row comes back into a full slot
        (lambda: delete(q=bad(q, 3, 3)), -6), (lambda: delete(q=bad(q, 3, -1)), -6),
        (lambda: restore(sb=bad(np.where(t > 0, 1, 0).astype(np.int64), 1, 4)), -7),      # t[1] is 2 after the deletion: s in 0..3
        (lambda: restore(sb=bad(np.where(t > 0, 1, 0).astype(np.int64), 1, -1)), -7),
        (lambda: delete(ldat=n - 1), -9), (lambda: restore(ldat=n - 1), -9),
        (lambda: delete(stride=buf.ldat * t_max - 1), -10), (lambda: restore(stride=buf.ldat * t_max - 1), -10),
        (lambda: restore(saved=0), -12),
    ]
    seen = set()
    for i, (call, want) in enumerate(checks):      # one at a time: the code, then the message this very call left
        got = call()
        msg = L.enlsip_gn_last_error(h)
        assert got == want and msg, (i, got, want, msg)
        seen.add(msg)
    assert len(seen) >= 10                         # the messages differ by condition
    # two faults at once: the checks run per problem, so the lower k wins
    assert delete(t=bad(t, 1, 5), q=bad(q, 0, 5)) == -6 and b"q[0]" in L.enlsip_gn_last_error(h)
    assert np.all(s == -9)
    same_images(buf.download(), before)
    assert restore(sb=np.zeros(B, dtype=np.int64), saved=0) == 0      # nothing comes back: no record is needed
    same_images(buf.download(), before)
    assert delete() == 0 and s[2] == 0


def test_fresh_handle_and_between_factor_and_solve(ref_solver):
    import torch
    from enlsip_gn import GNSolver
    from test_gpu_factored_batched import pack, same
    from test_gpu_ragged_batch import make_batch
    m, n, t_max, B = 48, 12, 4, 5
    ts = [4, 2, 0, 3, 4]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=19)
    As = [A if tk else np.zeros((0, n)) for A, tk in zip(As, ts)]
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    q = np.zeros(B, dtype=np.int64)
    buf = Buffers(n, t_max, t, False, seed=2)
    want = buf.images()
    s_want = np.array([host_s(0, buf.lam[k, :t[k]], False, buf.ds[k, :t[k]], 0.0) for k in range(B)], dtype=np.int64)
    assert s_want.any()
    model_delete(buf, want, s_want, t)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(a).to(dev)
    dJ, drx, dAt, dcx = up(J), up(rx), up(At), up(cx)
    dp, dp_ref = (torch.zeros((B, n), dtype=torch.float64, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    s = GNSolver(device=0)
    try:
        def edit():
            buf.upload()
            got = s.delete_constraints_batched_dev(B, n, t_max, t, q, False, buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(),
                                                   dsaved=buf.ptr("saved"))
            assert np.array_equal(got, s_want)
            same_images(buf.download(), want)
            s.restore_constraints_batched_dev(B, n, t_max, t - (got != 0), got, buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(),
                                              buf.ptr("saved"))
            back = buf.download()
            for nm in ("At", "cx", "lam", "ds"):
                assert back[nm].tobytes() == getattr(buf, nm).tobytes(), nm
        assert s.deletion_form() == -1
        edit()                                       # nothing resident at all
        A_args = (dAt.data_ptr(), n, n * t_max, dcx.data_ptr())
        s.factor_constraints_batched_dev(B, m, n, t_max, t, *A_args)
        edit()                                       # between the factor call and its solve, on other buffers
        s.solve_factored_batched_dev(B, m, n, t_max, t, None, dJ.data_ptr(), m, m * n, drx.data_ptr(), *A_args, dp=dp.data_ptr())
        ref_solver.factor_constraints_batched_dev(B, m, n, t_max, t, *A_args)
        ref_solver.solve_factored_batched_dev(B, m, n, t_max, t, None, dJ.data_ptr(), m, m * n, drx.data_ptr(), *A_args,
                                              dp=dp_ref.data_ptr())
        torch.cuda.synchronize()
        assert same(dp.cpu().numpy(), dp_ref.cpu().numpy()) and np.isfinite(dp.cpu().numpy()).all()
    finally:
        s.close()


# ---- 5. the driver: update_working_set_batched_dev against update_working_set_batched ----------------------------------------------
def build_flow(m, n, t_max, scaling, B=9):
    """The construction of tests/test_gpu_factored_batched.py's working-set mirror test, ragged: problem k holds its q equalities
    and t_k - q inequalities, and a gradient A' lambda* whose multiplier at one inequality is clearly negative where `fires`.
    scaling: False, True, or "mixed": every other problem scales its rows, the others keep diag_scale = the row norms
    (evaluate_scaling, src/structures.jl:160-178)."""
    from enlsip_gn import working_set as ws
    q, l = t_max // 3, t_max + 3
    Ws, Cs, its, Js, rxs, As, Gs, ps, fires = [], [], [], [], [], [], [], [], []
    for k in range(B):
        tk = q if k % 4 == 3 else (t_max if k % 2 == 0 else t_max - 1)
        A = synth.normal_stream(300 + k, 1, l * n).reshape(l, n)
        J = synth.normal_stream(300 + k, 2, m * n).reshape(m, n)
        rx = synth.normal_stream(300 + k, 3, m)
        W = ws.WorkingSet.create(q, l)
        for _ in range(tk - q):
            W.add_constraint(1)
        assert W.t == tk and list(W.active[:tk]) == list(range(1, tk + 1))
        rows = A[W.active[:tk] - 1, :].copy()
        scaled = (k % 2 == 0) if scaling == "mixed" else bool(scaling)
        norms = np.linalg.norm(rows, axis=1)
        ds = 1.0 / norms if scaled else (norms if scaling == "mixed" else np.ones(tk))
        Aact = rows * ds[:, None] if scaled else rows
        lam_star = np.ones(tk)
        fire = tk > q and k % 3 != 2
        if fire:
            lam_star[q + k % (tk - q)] = -1.0
        fires.append(fire)
        Ws.append(W); As.append(A); Js.append(J); rxs.append(rx)
        Cs.append(ws.Constraint(1e-3 * synth.normal_stream(300 + k, 4, tk), Aact, scaled, ds))
        Gs.append(Aact.T @ lam_star)
        its.append(ws.IterationRecord()); ps.append(np.zeros(n))
    return Ws, Cs, its, Js, rxs, As, Gs, ps, fires


class Recording:
    def __init__(self, inner, calls):
        self._inner, self._calls = inner, calls

    def __getattr__(self, name):
        f = getattr(self._inner, name)
        if not callable(f) or name in ("factor", "synchronize"):
            return f

        def wrapped(*a, **kw):
            out = f(*a, **kw)
            flags = None
            if name in ("solve_changed_batched", "solve_changed_batched_dev"):
                flags = np.flatnonzero(a[3] if name == "solve_changed_batched" else a[5]).tolist()
            if name in ("solve_factored_batched", "solve_factored_batched_dev"):
                flags = np.flatnonzero(a[5]).tolist()
            self._calls.append((name, flags, self._inner.jacobian_resolved() if flags is not None else None))
            return out
        return wrapped


@pytest.mark.parametrize("scaling", [False, True, "mixed"], ids=["plain", "scaled", "mixed"])
@pytest.mark.parametrize("m,n,t_max", [(40, 6, 3), (96, 65, 9)])
def test_flow_parity(solver, ref_solver, m, n, t_max, scaling):
    from enlsip_gn import working_set as ws
    eps, B = ws.SQRT_EPS, 9
    Ws, Cs, its, Js, rxs, As, Gs, ps, fires = build_flow(m, n, t_max, scaling)
    calls = []
    ws.update_working_set_batched(Recording(ref_solver, calls), Ws, rxs, As, Cs, Gs, Js, ps, its, eps)
    # the host flow's records first: first-order deletions (always undone, quirk Q1), second-order deletions, untouched problems
    names = [c[0] for c in calls]
    assert names[:3] == ["factor_constraints_batched", "first_lagrange_batched", "solve_factored_batched"]
    first = calls[2][1]
    assert first == [k for k in range(B) if fires[k]] and 0 < len(first) < B
    changed = [c for c in calls if c[0] == "solve_changed_batched"]
    assert len(changed) == 2 and changed[0][1] == first                           # every first-order deletion is undone
    second = changed[1][1]
    assert second and all(its[k].delete and its[k].index_del for k in second)
    untouched = [k for k in range(B) if k not in first and k not in second]
    assert untouched and all(not its[k].delete and its[k].index_del == 0 for k in untouched)
    assert set(first) & set(second) and set(second) - set(first)                  # a deletion after an undo, and one without

    Ws1, Cs1, its1, Js1, rxs1, As1, Gs1, ps1, _ = build_flow(m, n, t_max, scaling)
    calls1 = []
    ws.update_working_set_batched_dev(Recording(solver, calls1), Ws1, rxs1, As1, Cs1, Gs1, Js1, ps1, its1, eps)
    assert calls1 and all(nm.endswith("_dev") for nm, _, _ in calls1), calls1      # no host-form entry point
    ch1 = [c for c in calls1 if c[0] == "solve_changed_batched_dev"]
    assert [c[1] for c in ch1] == [first, second]
    assert all(resolved == len(flags) for _, flags, resolved in ch1)              # exactly the changed problems
    assert solver.deletion_form() == (1 if n <= 64 else 0)
    for k in range(B):
        W, W1, C, C1, it, it1 = Ws[k], Ws1[k], Cs[k], Cs1[k], its[k], its1[k]
        assert (W.q, W.t, W.l) == (W1.q, W1.t, W1.l), k
        assert np.array_equal(W.active, W1.active) and np.array_equal(W.inactive, W1.inactive), k
        assert C.scaling == C1.scaling, k
        for a, b in ((C.cx, C1.cx), (C.A, C1.A), (C.diag_scale, C1.diag_scale), (ps[k], ps1[k]), (it.b_gn, it1.b_gn),
                     (it.d_gn, it1.d_gn), (it.lam, it1.lam)):
            assert np.asarray(a).shape == np.asarray(b).shape and np.array_equal(a, b), k
        assert (it.rankA, it.rankJ2, it.dimA, it.dimJ2, it.grad_res, it.delete, it.index_del) == \
               (it1.rankA, it1.rankJ2, it1.dimA, it1.dimJ2, it1.grad_res, it1.delete, it1.index_del), k
