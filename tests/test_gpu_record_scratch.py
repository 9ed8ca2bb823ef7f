"""The one record scratch of the calls on the caller's device buffers: delete, restore, line-search set-up,
penalty weights, merit, fit (with and without psi_new), additions, termination test, direction check and Hessian sums place
their layouts in the same device buffer and the same pinned buffer of the handle.  What could go wrong is a call reading what
another family left there: list tails, `out` records of problems that are not taken, partial sums.

One handle makes all the calls on a wave shape, then on a general shape (the scratch grows under every layout), then on the wave
shape again (the small layouts now lie in a large buffer full of the general shape's bytes).  Every call is checked against the
reference its own test file uses (the case builders and comparisons are imported from those files), and every output, host and
device, equals bit for bit that of the same call on a fresh handle that has made no other call.  Host outputs lie between guard
rows.  In every batch one problem is not taken (slot < 0 for the Hessian sums) and a taken one has t = 0 (the set-up, which has
neither, has a problem whose list holds all l constraints).

Shapes (batch not a multiple of the four problems per workgroup of the wave forms; the general ones leave every wave form, have
sum_blocks(m) = 2 partial sums and l one past a 64-tile):
  wave     n = 5, l = 6, t_max = 4, m = 7, batch = 5    general  n = 65, l = 65, t_max = 65, m = 1025, batch = 3
but for what the imported builders fix: the penalty weights run on the problems of their own file (l = 12, t_max = 8, batch 9 and
l = 80, t_max = 70, batch 5, t as the cases have it, a taken one with t = 0 among them); the additions need t_max >= min(l, n)
where a problem is walked, so their wave shape has t_max = 5; the termination cases choose their own t (t_max = the largest, a
taken one with t = 0 among them)."""
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

import linesearch_cases as lc  # noqa: E402
import test_gpu_add_constraints_batched as ad  # noqa: E402
import test_gpu_delete_constraints_batched as dl  # noqa: E402
import test_gpu_direction_check_batched as dr  # noqa: E402
import test_gpu_hessian_sums_batched as hs  # noqa: E402
import test_gpu_linesearch_fit_batched as lf  # noqa: E402
import test_gpu_linesearch_setup_batched as ls  # noqa: E402
import test_gpu_penalty_weights_batched as pw  # noqa: E402
import test_gpu_termination_batched as tm  # noqa: E402

GUARD = -77      # what the guard rows of the host outputs hold, in every dtype
SHAPES = dict(wave=dict(n=5, l=6, t_max=4, m=7, B=5, ts=[4, 0, 2, 1, 4], form=1),
              general=dict(n=65, l=65, t_max=65, m=1025, B=3, ts=[65, 0, 32], form=0))
U = 2.0 ** -53


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def take_of(B):
    """problem 2 is not taken; problem 1 is the one with t = 0"""
    take = np.ones(B, dtype=np.int64)
    take[2] = 0
    return take


def guarded(a):
    """a copy of `a` between two guard rows: (the whole array, its inside as the call sees it)"""
    a = np.asarray(a)
    big = np.full((a.shape[0] + 2,) + a.shape[1:], GUARD, dtype=a.dtype)
    big[1:-1] = a
    return big, big[1:-1]


def guards_intact(big):
    fill = np.full(big[:1].shape, GUARD, dtype=big.dtype)
    return raw(big[:1]) == raw(fill) and raw(big[-1:]) == raw(fill)


class GuardedZeros:
    """Stands in for numpy inside enlsip_gn.api while one of its wrappers runs: the host outputs a wrapper allocates with np.zeros
    and hands to the library become the inside of an array with a guard row before and behind."""

    def __init__(self):
        self.bigs = []

    def __getattr__(self, name):
        return getattr(np, name)

    def zeros(self, shape, dtype=np.float64):
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        big, inside = guarded(np.zeros(shape, dtype=dtype))
        self.bigs.append(big)
        return inside


@contextmanager
def guarded_outputs(solver, method, count):
    """While the block runs, solver.<method> allocates its host outputs between guard rows (nothing else that the block calls
    does).  `count`: the host outputs of that call as include/enlsip_gn.h declares them; an output that the wrapper allocated in
    another way than np.zeros would go unguarded, and fails here."""
    import enlsip_gn.api as api
    g, inner = GuardedZeros(), getattr(solver, method)

    def call(*args, **kw):
        real, api.np = api.np, g
        try:
            return inner(*args, **kw)
        finally:
            api.np = real
    setattr(solver, method, call)
    try:
        yield g
    finally:
        delattr(solver, method)
    assert len(g.bigs) == count, (method, len(g.bigs), count)
    assert all(guards_intact(b) for b in g.bigs), "a guard row of a host output was written"


CASES = {}


def case(name, kind, build):
    """the host side of a family's batch and its references: built once, never changed"""
    if (name, kind) not in CASES:
        CASES[name, kind] = build(SHAPES[kind])
    return CASES[name, kind]


# ---- delete, then restore ----------------------------------------------------------------------------------------------------------
def build_delete(sh):
    n, t_max, B = sh["n"], sh["t_max"], sh["B"]
    take = take_of(B)
    for seed in range(40):      # a batch in which the test deletes somewhere: the restore has something to put back
        t, q = dl.batch_t_q(t_max, seed=seed, batch=B)      # t[1] = 0, t[2] = t[B - 1] = t_max
        buf = dl.Buffers(n, t_max, t, True, seed=seed + 1)
        s = np.array([dl.host_s(int(q[k]), buf.lam[k, :t[k]], True, buf.ds[k, :t[k]], buf.gres[k]) if take[k] else 0 for k in range(B)],
                     dtype=np.int64)
        if s.any():
            break
    assert s.any() and t[1] == 0 and s[2] == 0
    want = buf.images()
    dl.model_delete(buf, want, s, t)
    return dict(n=n, t_max=t_max, B=B, t=t, q=q, take=take, buf=buf, s=s, want=want, orig=buf.images())


def run_delete(s, kind, ctx):
    c = case("delete", kind, build_delete)
    buf = c["buf"]
    buf.upload()
    with guarded_outputs(s, "delete_constraints_batched_dev", 1):      # s
        got = s.delete_constraints_batched_dev(c["B"], c["n"], c["t_max"], c["t"], c["q"], True, buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(),
                                               dgrad_res=buf.ptr("gres"), dsaved=buf.ptr("saved"), take=c["take"])
    assert s.deletion_form() == SHAPES[kind]["form"]
    assert np.array_equal(got, c["s"])      # 0 where the problem is not taken
    after = buf.download()
    dl.same_images(after, c["want"])
    ctx["deleted"] = dict(buf.dev)      # the restore goes on from these device buffers
    return dict(s=raw(got), **{nm: raw(v) for nm, v in after.items()})


def run_restore(s, kind, ctx):
    c = case("delete", kind, build_delete)
    buf = c["buf"]
    buf.dev = ctx.pop("deleted")
    s.restore_constraints_batched_dev(c["B"], c["n"], c["t_max"], c["t"] - (c["s"] != 0), c["s"], buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(),
                                      buf.ptr("saved"))
    assert s.deletion_form() == SHAPES[kind]["form"]
    got = buf.download()
    for nm in ("At", "cx", "lam", "ds"):      # every slot is the original again, byte for byte
        assert raw(got[nm]) == raw(c["orig"][nm]), nm
    assert raw(got["saved"]) == raw(c["want"]["saved"]) and raw(got["gres"]) == raw(c["orig"]["gres"])
    return {nm: raw(v) for nm, v in got.items()}


# ---- line-search set-up ------------------------------------------------------------------------------------------------------------
def build_setup(sh):
    B, n, l, m = sh["B"], sh["n"], sh["l"], sh["m"]
    b = lc.random_batch(7 + n, B, n, l, m)
    b["inactive"][1], b["n_inactive"][1], b["index_del"][1] = np.arange(1, l + 1), l, 0      # t = 0: every constraint in the list
    exact_Ap = np.array([[ls.exact_dot(b["A"][k][j], b["p"][k]) for j in range(l)] for k in range(B)])
    exact_sums = np.array([[ls.exact_dot(u, v) for u, v in ((x, x), (x, y), (y, y))] for x, y in zip(b["Jp"], b["rx"])])
    return dict(b=b, exact_Ap=exact_Ap, exact_sums=exact_sums)


def run_setup(s, kind, ctx):
    c = case("setup", kind, build_setup)
    b, sh = c["b"], SHAPES[kind]
    call = ls.Call(b)
    with guarded_outputs(s, "linesearch_setup_batched_dev", 3):      # alpha_upp, index_alpha_upp, sums
        Ap, alpha, index, sums = call.run(s)      # inputs unwritten, the guard slots of dAp kept
    assert call.form == sh["form"]
    for k in range(sh["B"]):
        A, p, x, y = b["A"][k], b["p"][k], b["Jp"][k], b["rx"][k]
        assert np.all(np.abs(Ap[k] - c["exact_Ap"][k]) <= 2 * sh["n"] * U * (np.abs(A) @ np.abs(p))), k
        want = ls.host_bound(Ap[k], b["cx"][k], b["inactive"][k], b["n_inactive"][k], b["index_del"][k])
        assert ls.same(alpha[k], want[0]) and index[k] == want[1], (k, alpha[k], index[k], want)
        for q, (u, v) in enumerate(((x, x), (x, y), (y, y))):
            assert abs(sums[k, q] - c["exact_sums"][k, q]) <= 2 * sh["m"] * U * float(np.abs(u) @ np.abs(v)), (k, q)
    return dict(Ap=raw(Ap), alpha=raw(alpha), index=raw(index), sums=raw(sums))


# ---- penalty weights (the problems of their own file) ---------------------------------------------------------------------------------
def build_penalty(sh):
    l, t_max, B, seed = (12, 8, 9, 42) if sh["form"] else (80, 70, 5, 62)
    probs, take = pw.small_by_branch(2, l, t_max, B, seed), take_of(B)
    assert any(c["t"] == 0 and take[k] for k, c in enumerate(probs)), "no taken problem with t = 0"
    return dict(probs=probs, l=l, t_max=t_max, take=take)


def run_penalty(s, kind, ctx):
    c = case("penalty", kind, build_penalty)
    call = pw.Call(c["probs"], c["l"], c["t_max"], 2, True, take=c["take"])
    with guarded_outputs(s, "penalty_weights_batched_dev", 2):      # scalars, branch
        w, K, scalars, branch = call.check(s)      # against the host routine; not taken: w and K untouched, zeros in scalars and branch
    assert call.form == SHAPES[kind]["form"]
    return dict(w=raw(w), K=raw(K), scalars=raw(scalars), branch=raw(branch))


# ---- merit function ----------------------------------------------------------------------------------------------------------------
def build_merit(sh):
    B, m, l, t_max = sh["B"], sh["m"], sh["l"], sh["t_max"]
    b = pw.merit_batch(300 + m, B, m, l, t_max)
    b["t"][1], b["n_inactive"][1], b["active"][1], b["inactive"][1] = 0, l, 0, np.arange(1, l + 1)
    return dict(b=b, exact=[pw.exact_psi(b, k) for k in range(B)], take=take_of(B))


def run_merit(s, kind, ctx):
    c = case("merit", kind, build_merit)
    sh = SHAPES[kind]
    with guarded_outputs(s, "merit_batched_dev", 1):      # psi
        psi = pw.run_merit(s, c["b"], take=c["take"])
    for k, (ref, mag) in enumerate(c["exact"]):
        if not c["take"][k]:
            assert psi[k] == 0.0
        else:
            assert abs(psi[k] - ref) <= (sh["m"] + sh["l"] + 4) * U * mag, (k, psi[k], ref)
    return dict(psi=raw(psi))


# ---- polynomial fit, with and without psi_new ----------------------------------------------------------------------------------------
def build_fit(sh):
    return dict(b=lf.make_batch(100 * sh["m"] + sh["l"], sh["B"], sh["m"], sh["l"], sh["ts"]), take=take_of(sh["B"]))


def run_fit(psi):
    def run(s, kind, ctx):
        c = case("fit", kind, build_fit)
        with guarded_outputs(s, "linesearch_fit_batched_dev", 4 if psi else 3):      # sums, out, arm and psi_new
            got = lf.run(s, c["b"], take=c["take"], psi=psi)      # every device buffer comes back byte for byte
        assert (got[3] is None) == (not psi)
        if ctx.get("check"):      # the sums against exact dots, the fit against the host routine, psi_new against the merit call
            lf.check_values(s, c["b"], got, take=c["take"])
        return {nm: raw(v) for nm, v in zip(("sums", "out", "arm", "psi_new"), got) if v is not None}
    return run


# ---- working-set additions ---------------------------------------------------------------------------------------------------------
def build_add(sh):
    n, l, B = sh["n"], sh["l"], sh["B"]
    t_max = max(sh["t_max"], min(l, n))
    q, t, act, ina, iau, cx = ad.problems(n, l, B, 5 + n)
    q[1], t[1], act[1], ina[1] = 0, 0, 0, np.arange(1, l + 1)      # t = 0
    take = take_of(B)
    take[0] = 2      # a rebuild without a walk
    buf = ad.Buffers(n, l, t_max, cx, True, 6 + n)
    want = buf.images()
    model = ad.host_model(buf, want, q, t, act, ina, iau, take, True)
    return dict(n=n, l=l, B=B, t_max=t_max, q=q, t=t, act=act, ina=ina, iau=iau, take=take, buf=buf, want=want, model=model)


def run_add(s, kind, ctx):
    from enlsip_gn.api import _dptr, _fptr
    c = case("add", kind, build_add)
    buf, B = c["buf"].upload(), c["B"]
    A, lda, strideA, cx_all, At, ldat, strideAt, cx, ds = buf.args()
    bigs, host = zip(*(guarded(a) for a in (c["t"], c["act"], c["ina"], np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64))))
    t, act, ina, added, status = host
    s._chk(s._lib.enlsip_gn_add_constraints_batched_dev(
        s._h, B, c["n"], c["l"], c["t_max"], _fptr(c["q"]), _fptr(t), _fptr(act), _fptr(ina), _fptr(c["iau"]), _fptr(c["take"]), 1,
        _dptr(A), lda, strideA, _dptr(cx_all), _dptr(At), ldat, strideAt, _dptr(cx), _dptr(ds), _fptr(added), _fptr(status)))
    assert s.addition_form() == SHAPES[kind]["form"]
    assert all(guards_intact(b) for b in bigs), "a guard row of a host output was written"
    for got, want in zip(host, c["model"]):      # not taken: t and the lists as given, added and status 0
        assert np.array_equal(got, want)
    after = buf.download()
    ad.same_images(after, c["want"], kind)
    return dict({nm: raw(v) for nm, v in zip(("t", "act", "ina", "added", "status"), host)}, **{nm: raw(v) for nm, v in after.items()})


# ---- termination test --------------------------------------------------------------------------------------------------------------
def build_term(sh):
    cases = tm.make_batch(sh["n"], sh["l"], sh["m"], sh["B"], seed=sh["n"] + sh["l"] + sh["m"], scaling=True)
    take = take_of(sh["B"])
    assert any(c["t"] == 0 and take[k] for k, c in enumerate(cases)), "no taken problem with t = 0"
    return dict(cases=cases, take=take)


def run_term(s, kind, ctx):
    from enlsip_gn import termination as T
    c = case("term", kind, build_term)
    B = SHAPES[kind]["B"]
    b = tm.Batch(c["cases"]).upload()
    before = b.download()
    s0 = np.zeros(B + 2, dtype=T.SUMS_DTYPE)
    s0["rx_sum"] = -77.0      # what check_call expects where a problem is not taken
    e0 = np.full(B + 2, -77, dtype=np.int64)
    sums, codes = b.run(s, take=c["take"], sums=s0[1:-1], exit_code=e0[1:-1])
    assert T.termination_form(s) == SHAPES[kind]["form"]
    fresh = np.zeros(1, dtype=T.SUMS_DTYPE)
    fresh["rx_sum"] = -77.0
    assert all(raw(s0[i:][:1]) == raw(fresh) and e0[i] == -77 for i in (0, -1)), "a guard row of a host output was written"
    tm.check_call(s, b, sums, codes, c["take"], before)      # host sums, decision, oracle exit, untouched slots and inputs
    return dict(sums=raw(sums), codes=raw(codes), grad=raw(b.download()["grad"]))


# ---- direction check ---------------------------------------------------------------------------------------------------------------
def build_dir(sh):
    return dict(b=dr.Batch(sh["m"], sh["n"], sh["l"], sh["t_max"], sh["ts"], seed=100 * sh["m"] + sh["l"], scaling=True), take=take_of(sh["B"]))


def run_dir(s, kind, ctx):
    from enlsip_gn import direction as D
    c = case("dir", kind, build_dir)
    b, B = c["b"], SHAPES[kind]["B"]
    big = dr.sentinel_out(B + 2)
    fill = [raw(a[:1]) for a in (big.method_code, big.beta, big.status, big.sums)]
    out = b.run(s, take=c["take"], out=D.DirectionCheck(big.method_code[1:-1], big.beta[1:-1], big.status[1:-1], big.sums[1:-1]))
    assert s.direction_form() == SHAPES[kind]["form"]
    for a, f in zip((big.method_code, big.beta, big.status, big.sums), fill):
        assert raw(a[:1]) == f and raw(a[-1:]) == f, "a guard row of a host output was written"
    dr.check_against_host(b, out, taken=c["take"])      # the host routines' bytes; not taken: every output keeps its fill
    assert b.inputs_unchanged()
    return dict(code=raw(out.method_code), beta=raw(out.beta), status=raw(out.status), sums=raw(out.sums))


# ---- Hessian sums ------------------------------------------------------------------------------------------------------------------
def build_hess(sh):
    n, B = sh["n"], sh["B"]
    npairs = 4
    b = hs.Batch(sh["m"], n, sh["l"], sh["ts"], pair0=n * (n + 1) // 2 - 6, npairs=npairs, seed=1000 * sh["m"] + n)
    ldg, slot = n + 3, [B + 1 - k for k in range(B)]
    slot[2] = -1      # left alone
    strideG = ldg * n + 5
    flat = hs.pattern((B + 2) * strideG)
    return dict(b=b, ldg=ldg, strideG=strideG, slot=slot, flat=flat, want=b.expected(flat, ldg, strideG, slot))


def run_hess(s, kind, ctx):
    import torch
    c = case("hess", kind, build_hess)
    dGam = hs.dev(c["flat"])
    torch.cuda.synchronize()
    c["b"].run(s, dGam, c["ldg"], c["strideG"], slot=c["slot"])
    got = dGam.cpu().numpy()
    assert hs.same_bytes(got, c["want"])      # the host routine's entries; every other byte of Gamma keeps the pattern
    return dict(Gamma=raw(got))


FAMILIES = [("delete", run_delete), ("restore", run_restore), ("setup", run_setup), ("penalty", run_penalty), ("merit", run_merit),
            ("fit", run_fit(False)), ("fit_psi_new", run_fit(True)), ("add", run_add), ("termination", run_term), ("direction", run_dir),
            ("hessian_sums", run_hess)]


def test_calls_on_one_handle_read_nothing_another_family_left_in_the_scratch():
    from enlsip_gn import GNSolver
    want = {}
    for kind in SHAPES:      # each call on a handle of its own that makes no other call (the restore: on the delete's device buffers)
        ctx = {}
        for name, run in FAMILIES:
            fresh = GNSolver(device=0)
            try:
                want[kind, name] = run(fresh, kind, ctx)
            finally:
                fresh.close()
    one = GNSolver(device=0)
    try:
        for rnd, kind in enumerate(("wave", "general", "wave")):      # grow under every layout, then small layouts in the large buffer
            ctx = dict(check=True)
            for name, run in FAMILIES:
                got = run(one, kind, ctx)
                assert got.keys() == want[kind, name].keys()
                for nm in got:
                    assert got[nm] == want[kind, name][nm], (rnd, kind, name, nm)
    finally:
        one.close()
