"""The Gauss-Newton direction check of a batch on device buffers (enlsip_gn_direction_check_batched_dev).  The sums are compared
bit for bit with enlsip_gn_direction_sums on the same data (tests/test_direction_check_host.py checks that routine against exact
arithmetic), method_code and beta with enlsip_gn_check_gn_direction on the returned sums (checked there against the oracle on a
table that walks every condition), in both kernel forms, at the wave form's bound on m, with ragged t, batches that are no
multiple of four, take masks and every argument error."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

import direction_cases as dc  # noqa: E402

SENT = -7.25e33      # behind every live entry of every device buffer
WAVE_MAX_M = 1024    # DIR_WAVE_MAX_M of gn_kernels_direction_batched.hpp


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


class Batch:
    """B random problems of one shape in the padded ragged layout, sentinels behind the live entries, on the device"""

    def __init__(self, m, n, l, t_max, ts, seed, scaling=False, status1=()):
        rng = np.random.default_rng(seed)
        self.m, self.n, self.l, self.t_max, self.B, self.scaling = m, n, l, t_max, len(ts), scaling
        self.problems = []
        for k, t in enumerate(ts):
            st, a = dc.random_problem(rng, m, n, l, t, int(rng.integers(0, t + 1)), scaling=scaling,
                                      k_prev=m + 1 if k in status1 else None)
            st.update(prev_code=(1, -1, 2)[k % 3], iter_number=k % 2 * 3, restart=k % 5 == 4, prev_beta=float(rng.random()) * 40.0,
                      prev_alpha=(0.01, 1.0)[k % 2], add=k % 7 == 3)
            self.problems.append((st, a))
        self.fill()

    @classmethod
    def of(cls, problems, m, n, l, t_max, scaling=False):
        b = cls.__new__(cls)
        b.m, b.n, b.l, b.t_max, b.B, b.scaling, b.problems = m, n, l, t_max, len(problems), scaling, list(problems)
        b.fill()
        return b

    def fill(self):
        import torch
        B, full = self.B, lambda cols: np.full((self.B, max(cols, 1)), SENT)
        h = dict(b=full(self.t_max), d=full(self.m), lam=full(self.t_max), diag_scale=full(self.t_max), cx_all=full(self.l))
        self.active, self.inactive = np.zeros((B, self.l), dtype=np.int64), np.zeros((B, self.l), dtype=np.int64)
        for k, (st, a) in enumerate(self.problems):
            for nm in h:
                h[nm][k, :a[nm].size] = a[nm]
            self.active[k], self.inactive[k] = a["active"], a["inactive"]
        self.host = h
        self.dev = {nm: torch.from_numpy(a.copy()).to("cuda:0") for nm, a in h.items()}
        torch.cuda.synchronize()

    def run(self, solver, take=None, out=None, **over):
        from enlsip_gn import direction as D
        p = lambda nm: self.dev[nm].data_ptr()
        a = dict(batch=self.B, m=self.m, n=self.n, l=self.l, t_max=self.t_max, states=[D.make_state(**st) for st, _ in self.problems],
                 active=self.active, inactive=self.inactive, scaling=self.scaling, db=p("b") if self.t_max else 0,
                 dd=p("d") if self.m else 0, dlambda=p("lam") if self.t_max else 0, ddiag_scale=p("diag_scale") if self.t_max else 0,
                 dcx_all=p("cx_all") if self.l else 0)
        a.update(over)
        return solver.direction_check_batched_dev(a.pop("batch"), a.pop("m"), a.pop("n"), a.pop("l"), a.pop("t_max"), take=take, out=out, **a)

    def inputs_unchanged(self):
        import torch
        torch.cuda.synchronize()
        return all(same_bytes(self.dev[nm].cpu().numpy(), self.host[nm]) for nm in self.host)

    def expected(self, k):
        """(sums, status, code, beta) of problem k by the host routines"""
        from enlsip_gn import direction as D
        st, a = self.problems[k]
        state = D.make_state(**st)
        sums, status = D.direction_sums(state, m=self.m, n=self.n, **a)
        code, beta = D.check_gn_direction(state, sums, self.m, self.n) if status != 1 else (None, None)
        return sums, status, code, beta


def sentinel_out(B):
    from enlsip_gn import direction as D
    sums = np.frombuffer(np.full(B * 8, SENT).tobytes(), dtype=D.SUMS_DTYPE).copy()
    return D.DirectionCheck(np.full(B, -77, dtype=np.int64), np.full(B, SENT), np.full(B, -55, dtype=np.int64), sums)


def check_against_host(b, out, taken=None):
    sent = sentinel_out(b.B)
    codes = set()
    for k in range(b.B):
        if taken is not None and not taken[k]:
            assert same_bytes(out.sums[k], sent.sums[k]) and out.method_code[k] == -77 and same_bytes(out.beta[k], SENT) \
                and out.status[k] == -55, k
            continue
        sums, status, code, beta = b.expected(k)
        assert out.status[k] == status, (k, out.status[k], status)
        if status == 1:      # nothing but the status is written
            assert same_bytes(out.sums[k], sent.sums[k]) and out.method_code[k] == -77 and same_bytes(out.beta[k], SENT), k
            continue
        assert same_bytes(out.sums[k], sums), (k, out.sums[k], sums)
        assert out.method_code[k] == code and same_bytes(out.beta[k], np.float64(beta)), (k, out.method_code[k], code)
        codes.add(code)
    return codes


SHAPES = [  # (m, n, l, t_max), form
    ((5, 3, 2, 2), 1), ((64, 8, 64, 64), 1), ((WAVE_MAX_M, 8, 64, 64), 1), ((WAVE_MAX_M + 1, 8, 64, 64), 0),
    ((1000, 16, 65, 65), 0), ((130, 12, 1024, 1024), 0), ((20, 4, 0, 0), 1), ((20, 4, 5, 0), 1), ((0, 4, 5, 3), 1), ((40, 6, 65, 3), 0)]


@pytest.mark.parametrize("B", (1, 5))
@pytest.mark.parametrize("shape,form", SHAPES, ids=lambda s: "m%d_n%d_l%d_tmax%d" % s if isinstance(s, tuple) else "form%d" % s)
def test_bytes_are_the_host_routines(solver, shape, form, B):
    m, n, l, t_max = shape
    ts = [t_max, 0, t_max // 2, min(1, t_max), t_max][:B]      # ragged, 0 and t_max included
    for scaling in (False, True):
        b = Batch(m, n, l, t_max, ts, seed=100 * m + l + B, scaling=scaling, status1=(3,) if B == 5 else ())
        out = b.run(solver, out=sentinel_out(B))
        assert solver.direction_form() == form
        check_against_host(b, out)
        assert b.inputs_unchanged()


def test_every_code_comes_out_of_the_device_call(solver):
    """a larger ragged batch: all three method codes and all three statuses are among the answers"""
    ts = [int(t) for t in np.random.default_rng(3).integers(0, 10, size=41)]
    b = Batch(30, 12, 14, 9, ts, seed=77, status1=(5, 17))
    out = b.run(solver, out=sentinel_out(b.B))
    assert check_against_host(b, out) == {1, -1, 2}
    assert set(out.status.tolist()) == {0, 1, 2}


def test_take_masks_leave_every_slot_alone_and_slots_do_not_matter(solver):
    from enlsip_gn import direction as D
    m, n, l, t_max = 70, 9, 66, 40      # general form
    ts = [40, 3, 0, 17, 25]
    b = Batch(m, n, l, t_max, ts, seed=9)
    everything = b.run(solver, out=sentinel_out(5))
    for take in ([1, 0, 1, 0, 1], [0, 0, 0, 1, 0], [0, 0, 0, 0, 0]):
        out = b.run(solver, take=take, out=sentinel_out(5))
        check_against_host(b, out, taken=take)
        for k in range(5):
            if take[k]:
                assert same_bytes(out.sums[k], everything.sums[k]) and same_bytes(out.beta[k], everything.beta[k])
    # a problem that is not taken is not even checked
    bad = list(b.problems)
    bad[1] = (dict(bad[1][0], t=t_max + 5, dimJ2=m + 9), bad[1][1])
    b2 = Batch.of(bad, m, n, l, t_max)
    out = b2.run(solver, take=[1, 0, 1, 1, 1], out=sentinel_out(5))
    assert same_bytes(out.sums[[0, 2, 3, 4]], everything.sums[[0, 2, 3, 4]])
    # the same problem in two positions of two batches, other neighbours, other takes: the same bytes
    other = Batch(m, n, l, t_max, [1, 40, 9], seed=10)
    first = Batch.of([b.problems[3], other.problems[0], other.problems[1]], m, n, l, t_max)
    second = Batch.of([other.problems[2], other.problems[1], b.problems[0], b.problems[3], b.problems[4], other.problems[0]], m, n, l, t_max)
    o1 = first.run(solver, take=[1, 0, 1], out=sentinel_out(3))
    o2 = second.run(solver, out=sentinel_out(6))
    assert same_bytes(o1.sums[0], o2.sums[3]) and same_bytes(o1.sums[0], everything.sums[3])
    assert same_bytes(o1.beta[0], o2.beta[3]) and o1.method_code[0] == o2.method_code[3] == everything.method_code[3]
    # and in the wave form
    w = Batch(50, 9, 20, 12, [12, 3, 0, 7, 5], seed=11)
    all_w = w.run(solver, out=sentinel_out(5))
    assert solver.direction_form() == 1
    out = w.run(solver, take=[0, 1, 0, 0, 1], out=sentinel_out(5))
    check_against_host(w, out, taken=[0, 1, 0, 0, 1])
    moved = Batch.of([w.problems[4], w.problems[1]], 50, 9, 20, 12)
    o3 = moved.run(solver, out=sentinel_out(2))
    assert same_bytes(o3.sums[0], all_w.sums[4]) and same_bytes(o3.sums[1], all_w.sums[1]) and same_bytes(o3.beta[0], all_w.beta[4])
    assert D.direction_form(solver) == 1


def test_argument_errors_come_before_any_launch_and_leave_the_outputs(solver):
    import ctypes as C
    from enlsip_gn import GNError
    from enlsip_gn import direction as D
    m, n, l, t_max = 20, 5, 7, 4
    b = Batch(m, n, l, t_max, [4, 2, 0], seed=31)

    def raw(code, states=None, **over):
        out = sentinel_out(3)
        sts = [dict(st) for st, _ in b.problems]
        if states:
            states(sts)
        with pytest.raises(GNError) as e:
            b.run(solver, out=out, states=[D.make_state(**st) for st in sts], **over)
        assert f"error {code}:" in str(e.value), (code, str(e.value))
        sent = sentinel_out(3)
        assert same_bytes(out.sums, sent.sums) and same_bytes(out.beta, sent.beta) and same_bytes(out.method_code, sent.method_code) \
            and same_bytes(out.status, sent.status), code
        assert b.inputs_unchanged()

    def edit(k, **f):
        return lambda sts: sts[k].update(f)
    raw(-3, m=-1)
    raw(-3, n=0)
    raw(-3, t_max=l + 1)
    raw(-4, dd=0)
    raw(-4, dcx_all=0)
    raw(-4, db=0)
    raw(-4, dlambda=0)
    raw(-4, ddiag_scale=0)
    raw(-5, states=edit(1, t=t_max + 1))
    raw(-5, states=edit(2, l=l - 1))
    raw(-6, states=edit(0, q=5))
    raw(-8, states=edit(1, dimA=3))
    raw(-8, states=edit(1, dimA=-1))
    raw(-8, states=edit(2, dimJ2=m + 1))
    act = b.active.copy()
    act[0, 1] = l + 1
    raw(-7, active=act)
    ina = b.inactive.copy()
    ina[1, 0] = -1
    raw(-7, inactive=ina)
    # the NULL host arrays and batch < 1, through the raw entry point
    lib, h = solver._lib, solver._h
    out = sentinel_out(3)
    states = (D.DirState * 3)(*[D.make_state(**st) for st, _ in b.problems])
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    dev = [C.c_void_p(b.dev[nm].data_ptr()) for nm in ("b", "d", "lam", "diag_scale", "cx_all")]
    host = dict(state=C.cast(states, C.c_void_p), active=ptr(b.active), inactive=ptr(b.inactive), sums=ptr(out.sums),
                method_code=ptr(out.method_code), beta=ptr(out.beta), status=ptr(out.status))

    def call(batch=3, handle=h, l_=l, **null):
        a = dict(host, **{k: None for k in null})
        return lib.enlsip_gn_direction_check_batched_dev(handle, batch, m, n, l_, t_max, a["state"], a["active"], a["inactive"], None, 0,
                                                         *dev, a["sums"], a["method_code"], a["beta"], a["status"])
    assert call(handle=None) == -1
    assert call(batch=0) == -2
    assert call(l_=1025) == -3
    for name in host:
        assert call(**{name: True}) == -4, name
    sent = sentinel_out(3)
    assert same_bytes(out.sums, sent.sums) and same_bytes(out.beta, sent.beta) and same_bytes(out.status, sent.status)
    assert call() == 0 and not same_bytes(out.sums, sent.sums)
    f = C.c_int(9)
    assert lib.enlsip_gn_get_direction_form(None, C.byref(f)) == -1 and lib.enlsip_gn_get_direction_form(h, None) == -2


def test_the_call_needs_nothing_resident():
    """legal on a fresh handle, and the form getter says -1 before the first call"""
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    try:
        assert s.direction_form() == -1
        b = Batch(9, 4, 3, 2, [2, 1], seed=1)
        check_against_host(b, b.run(s, out=sentinel_out(2)))
        assert s.direction_form() == 1
    finally:
        s.close()


def test_search_direction_analys_over_a_solved_batch_against_the_oracle(solver):
    """End to end: seven problems with m = 12, n = 6, l = 4 and ragged t (tests/direction_cases.py::e2e_problems), solved with
    solve_batched_ragged_dev, multipliers by first_lagrange_batched_dev, then search_direction_analys_batched_dev on the buffers
    those calls left, compared per problem with oracle.enlsip_outer.search_direction_analys on the oracle backend.  code, dimA,
    dimJ2 and error_code are exact.  Tolerances, those of tests/test_gpu_parity.py for the same quantities: p to TOL_P = 1e-11
    relative; beta is the norm of [d1; b1] and speed a multiple of it, held to the 1e-12 relative that file holds norm(d) to; the
    multipliers to rtol 1e-8, atol 1e-10 max(1, |lam|).  No comparison of check_gn_direction is decided within a relative 1e-6 of
    its threshold: asserted here on the oracle's own values, and on the CPU in tests/test_direction_check_host.py."""
    import torch
    from enlsip_gn import direction as D
    from test_gpu_parity import TOL_P
    m, n, l = dc.E2E_SHAPE
    Ps = dc.e2e_problems()
    B = len(Ps)
    assert B >= 7 and all(dc.e2e_margin(P) >= 1e-6 for P in Ps)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda:0")
    At, cxa, t = solver.pack_ragged([P["aC"].A for P in Ps], [P["aC"].cx for P in Ps], n=n)
    t_max = At.shape[1]
    dJ, drx = dev(np.stack([P["J"].T for P in Ps])), dev(np.stack([P["rx"] for P in Ps]))
    dAt, dcx = dev(At), dev(cxa)
    bufs = dict(p=zeros(B, n), b=zeros(B, t_max), d=zeros(B, m), lam=zeros(B, t_max), diag_scale=zeros(B, t_max),
                cx_all=dev(np.stack([P["cx"] for P in Ps])))
    ds = np.zeros((B, t_max))
    for k, P in enumerate(Ps):
        ds[k, :P["t"]] = P["aC"].diag_scale
    bufs["diag_scale"] = dev(ds)
    dinfo, dgrad = zeros(B, 6, dtype=torch.int64), zeros(B, n)
    solver.solve_batched_ragged_dev(B, m, n, t_max, t, dJ.data_ptr(), m, m * n, drx.data_ptr(), dAt.data_ptr(), n, n * t_max,
                                    dcx.data_ptr(), dp=bufs["p"].data_ptr(), db=bufs["b"].data_ptr(), dd=bufs["d"].data_ptr(),
                                    dinfo=dinfo.data_ptr())
    solver.gradient_batched_dev(0, B, dgrad.data_ptr())
    assert solver.first_lagrange_batched_dev(0, B, bufs["lam"].data_ptr(), dgrad_fx=dgrad.data_ptr()) == 0
    torch.cuda.synchronize()
    info, lam, p_gn = dinfo.cpu().numpy(), bufs["lam"].cpu().numpy(), bufs["p"].cpu().numpy()
    for k, P in enumerate(Ps):      # the solve and the multipliers are the oracle's: what the check reads is where it expects it
        assert (info[k, 0], info[k, 1]) == (P["ref"].rankA, P["ref"].rankJ2), k
        np.testing.assert_allclose(lam[k, :P["t"]], P["lam"], rtol=1e-8, atol=1e-10 * max(1.0, np.abs(P["lam"]).max()))
    hessians = lambda k: dc.e2e_hessians(Ps[k]) if Ps[k]["second"] else None
    take = [P["take"] for P in Ps]
    out = D.search_direction_analys_batched_dev(solver, [P["W"] for P in Ps], [P["cur"] for P in Ps], [P["prev"] for P in Ps], bufs,
                                                m=m, n=n, t_max=t_max, iter_number=[P["iter_number"] for P in Ps], scaling=False,
                                                rx_sum=[float(P["rx"] @ P["rx"]) for P in Ps], hessians=hessians, take=take)
    torch.cuda.synchronize()
    p = bufs["p"].cpu().numpy()
    seen = set()
    for k, (P, r) in enumerate(zip(Ps, out)):
        if P["kind"] == "not taken":
            assert not r.taken and r.status == -1 and r.code == 0 and same_bytes(p[k], p_gn[k])
            continue
        if P["kind"] == "status 1":     # the reference throws a BoundsError at :1231; nothing of the problem is touched
            assert P["prev"].dimJ2 + P["prev"].t - P["t"] - 1 > m and r.status == 1 and r.code == 0 and same_bytes(p[k], p_gn[k])
            continue
        err, cur = dc.e2e_oracle(P)
        print(f"{P['kind']}: code {r.code} dims ({r.dimA}, {r.dimJ2}) error {r.error_code}; beta rel "
              f"{abs(r.beta - cur.beta) / cur.beta:.2e}, speed rel {abs(r.speed - cur.speed) / cur.speed:.2e}, "
              f"p rel {np.linalg.norm(p[k] - cur.p) / np.linalg.norm(cur.p):.2e}")
        assert (r.code, r.dimA, r.dimJ2, r.error_code) == (cur.code, cur.dimA, cur.dimJ2, err), (P["kind"], r, cur.code, cur.dimA, cur.dimJ2, err)
        assert r.status == 0 and r.subspace_status == 0 and r.newton_status == 0 and r.nb_newton_steps == cur.nb_newton_steps
        assert abs(r.beta - cur.beta) <= 1e-12 * cur.beta and abs(r.speed - cur.speed) <= 1e-12 * cur.speed
        assert np.linalg.norm(p[k] - cur.p) <= TOL_P * np.linalg.norm(cur.p), P["kind"]
        seen.add((r.code, r.error_code, (r.dimA, r.dimJ2) == (cur.rankA, cur.rankJ2)))
    assert seen == {(1, 0, True), (-1, 0, False), (2, 0, False), (2, -4, True)}
    assert [P["kind"] for P in Ps if "back to 1" in P["kind"]] and out[2].code == 1 and out[2].taken
