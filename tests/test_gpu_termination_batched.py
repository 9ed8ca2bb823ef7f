"""The termination test of a batch on device buffers (enlsip_gn_termination_batched_dev).  The sums are compared bit for bit with
enlsip_gn_termination_sums on the downloaded inputs (tests/test_termination_host.py checks that routine against mpmath and the
decision against the oracle), dgrad with enlsip_gn_gradient_batched_dev after a ragged solve made the same J, rx resident, rx_sum
with the dot(rx, rx) of enlsip_gn_linesearch_setup_batched_dev, the exit codes with the host decision on the returned sums and,
away from the thresholds, with oracle/enlsip_outer.py on the same data."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

import termination_cases as tc  # noqa: E402

SENT = -7.25e33      # behind every live entry of every buffer


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


class Batch:
    """B cases of one shape in the padded ragged layout with slack everywhere, sentinels behind the live entries, on the device."""
    inputs = ("J", "rx", "cx_all", "x", "x_prev", "p", "d_gn", "lam", "cx_active", "diag_scale", "At", "w")

    def __init__(self, cases, t_max=None, padded=True):
        c0 = cases[0]
        self.cases, self.B = cases, len(cases)
        self.m, self.n, self.l = m, n, l = c0["m"], c0["n"], c0["l"]
        self.t_max = tm = max(c["t"] for c in cases) if t_max is None else t_max
        pad = 3 if padded else 0
        self.ldj, self.ldat = max(m, 1) + pad, n + pad
        self.strideJ, self.strideAt = self.ldj * n + 2 * pad, self.ldat * tm + 2 * pad
        B = self.B
        full = lambda cols: np.full((B, max(cols, 1)), SENT)
        h = dict(J=full(self.strideJ), rx=full(m), cx_all=full(l), x=full(n), x_prev=full(n), p=full(n), d_gn=full(n), lam=full(tm),
                 cx_active=full(tm), diag_scale=full(tm), At=full(self.strideAt), w=full(l), grad=np.full(B * n + 4, SENT))      # dgrad: n per problem, sentinels behind the batch
        for k, c in enumerate(cases):
            h["J"][k, :self.ldj * n].reshape(n, self.ldj)[:, :m] = c["J"].T
            for nm in ("rx", "cx_all", "x", "x_prev", "p", "d_gn", "w"):
                h[nm][k, :c[nm].size] = c[nm]
            t = c["t"]
            h["lam"][k, :t], h["cx_active"][k, :t], h["diag_scale"][k, :t] = c["lam"], c["cx_active"], c["diag_scale"]
            if tm:
                h["At"][k, :self.ldat * tm].reshape(tm, self.ldat)[:t, :n] = c["At"].T
        self.host = h
        self.active = np.array([c["active"] for c in cases], dtype=np.int64).reshape(B, l)
        self.inactive = np.array([c["inactive"] for c in cases], dtype=np.int64).reshape(B, l)

    def upload(self):
        import torch
        self.dev = {nm: torch.from_numpy(a.copy()).to("cuda:0") for nm, a in self.host.items()}
        torch.cuda.synchronize()
        return self

    def download(self):
        import torch
        torch.cuda.synchronize()
        return {nm: a.cpu().numpy() for nm, a in self.dev.items()}

    def bufs(self):
        from enlsip_gn.termination import TerminationBuffers
        p = lambda nm: self.dev[nm].data_ptr()
        return TerminationBuffers(dJ=p("J"), drx=p("rx"), dcx_all=p("cx_all"), dx=p("x"), dx_prev=p("x_prev"), dp=p("p"), dd_gn=p("d_gn"),
                                  dlambda=p("lam"), dcx_active=p("cx_active"), ddiag_scale=p("diag_scale"), dAt=p("At"), dw=p("w"),
                                  dgrad=p("grad"))

    def states(self):
        from enlsip_gn import termination as T
        out = []
        for c in self.cases:
            st = c["state"]
            out.append(T.make_state(restart=st["restart"], code=st["code"], delete=st["delete"], grad_res=st["grad_res"],
                                    nb_iter=st["nb_iter"], nb_newton_steps=st["nb_newton_steps"], error_code=st["error_code"],
                                    psi_error=st["psi_error"], delta_time=st["delta_time"], q=c["q"], t=c["t"], l=c["l"],
                                    dimJ2=c["dimJ2"], psi0=st["psi0"]))
        return out

    def run(self, solver, take=None, scaling=None, sums=None, exit_code=None, **over):
        from enlsip_gn import termination as T
        kw = dict(ldj=self.ldj, strideJ=self.strideJ, ldat=self.ldat, strideAt=self.strideAt)
        kw.update(over)
        scaling = self.cases[0]["scaling"] if scaling is None else scaling
        return T.termination_raw(solver, self.B, self.m, self.n, self.l, self.t_max, self.states(), T.make_tol(**tc.TOL), self.active,
                                 self.inactive, self.bufs(), scaling, take=take, sums=sums, exit_code=exit_code, **kw)


def make_batch(n, l, m, B, seed, scaling, arms=None):
    rng = np.random.default_rng(seed)
    arms = list(tc.ARMS) if arms is None else arms
    usable = [a for a in arms if not ((a in ("inactive_nonpos",) and l < 1) or (a == "sigma_small_t2" and l < 2) or
                                      (a in ("sigma_small_t1", "cx_active_large", "infeasible", "infeasible_beats_time",
                                             "psi_beats_infeasible") and l < 1))]
    cases = []
    for k in range(B):
        arm = usable[(seed * 7 + k) % len(usable)]
        # mixed t, q, dimJ2: t = 0, t == q, t == 1 > q, t == l among them
        t = [0, None, 1, min(l, n, 64) if l else 0, None][k % 5]
        q = {2: 0}.get(k % 5)
        c = tc.make_case(rng, arm, m, n, l, t=t, q=q, scaling=scaling)
        if k % 4 == 0 and arm not in tc.CONVERGED:
            c["dimJ2"] = 0 if k % 8 == 0 else n
        cases.append(c)
    return cases


def host_sums(T, c, grad, rx_sum):
    s, _ = T.termination_sums(J=c["J"], rx=c["rx"], cx_all=c["cx_all"], x=c["x"], x_prev=c["x_prev"], p=c["p"], d_gn=c["d_gn"],
                              dimJ2=c["dimJ2"], lam=c["lam"], cx_active=c["cx_active"], diag_scale=c["diag_scale"], At=c["At"],
                              w=c["w"], active=c["active"], inactive=c["inactive"], q=c["q"], t=c["t"], scaling=c["scaling"],
                              psi0=c["state"]["psi0"], grad_in=grad, rx_sum_in=rx_sum)
    return s


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def grad_of(b, image, k):
    return image["grad"][k * b.n:(k + 1) * b.n]


def grads(b, ks):
    g = b.download()["grad"][:b.B * b.n].reshape(b.B, b.n)
    return g[ks]


def check_call(solver, b, sums, codes, take, before):
    """every assertion on one finished call: the record against the host routine, the decision, the sentinels and the inputs"""
    from enlsip_gn import termination as T
    after = b.download()
    skipped = 0
    for k, c in enumerate(b.cases):
        if take is not None and not take[k]:
            assert same_bytes(grad_of(b, after, k), grad_of(b, before, k)) and codes[k] == -77 and sums[k]["rx_sum"] == -77.0, k
            continue
        grad = grad_of(b, after, k)
        want = host_sums(T, c, grad, float(sums[k]["rx_sum"]))
        for name in T.SUMS_DTYPE.names:
            assert same_bytes(sums[k][name], want[name]), (k, c["arm"], name, sums[k][name], want[name])
        # rx_sum and the gradient are pinned elsewhere; here: inside their rounding bounds of the host's strided sums
        ref, _ = T.termination_sums(J=c["J"], rx=c["rx"], cx_all=c["cx_all"], x=c["x"], x_prev=c["x_prev"], p=c["p"], d_gn=c["d_gn"],
                                    dimJ2=c["dimJ2"], lam=c["lam"], cx_active=c["cx_active"], diag_scale=c["diag_scale"], At=c["At"],
                                    w=c["w"], active=c["active"], inactive=c["inactive"], q=c["q"], t=c["t"], scaling=c["scaling"])
        bound = tc.rounding_bounds(c)
        assert abs(sums[k]["rx_sum"] - ref["rx_sum"]) <= 2 * bound["rx_sum"], k      # each within the bound of the exact value
        assert abs(sums[k]["grad_nrm"] - ref["grad_nrm"]) <= 2 * bound["grad_nrm"], k
        rec = sums[k]
        state = b.states()[k]
        assert codes[k] == T.check_termination_criteria(state, rec, T.make_tol(**tc.TOL)), (k, c["arm"])
        if tc.on_a_threshold(c):
            skipped += 1
        else:
            assert codes[k] == tc.oracle_exit(c), (k, c["arm"], codes[k])
    assert same_bytes(after["grad"][b.B * b.n:], before["grad"][b.B * b.n:]), "behind the last problem in dgrad"
    for nm in b.inputs:
        assert same_bytes(after[nm], before[nm]), nm
    return skipped


SHAPES = [  # (n, l, m): both sides of the wave / general boundary, the small shapes, two partial blocks, the lone column
    (64, 64, 63), (65, 64, 64), (64, 65, 65), (1, 0, 1), (5, 7, 1024), (130, 200, 1025), (5, 7, 1)]


@pytest.mark.parametrize("scaling", (False, True), ids=("plain", "scaled"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_l%d_m%d" % s)
def test_sums_codes_and_untouched_bytes(solver, shape, scaling):
    from enlsip_gn import termination as T
    n, l, m = shape
    B = 9
    cases = make_batch(n, l, m, B, seed=n + l + m, scaling=scaling)
    b = Batch(cases).upload()
    before = b.download()
    sums, codes = b.run(solver)
    assert T.termination_form(solver) == (1 if n <= 64 and l <= 64 else 0)
    skipped = check_call(solver, b, sums, codes, None, before)
    assert skipped <= 0.05 * B
    # the same problems with some neighbours not taken: their slots keep every byte, the others give the same bytes
    take = np.array([k % 3 != 1 for k in range(B)], dtype=np.int64)
    b2 = Batch(cases).upload()
    before2 = b2.download()
    s0 = np.zeros(B, dtype=T.SUMS_DTYPE)
    s0["rx_sum"] = -77.0
    sums2, codes2 = b2.run(solver, take=take, sums=s0, exit_code=np.full(B, -77, dtype=np.int64))
    check_call(solver, b2, sums2, codes2, take, before2)
    on = np.flatnonzero(take)
    assert same_bytes(sums2[on], sums[on]) and same_bytes(codes2[on], codes[on])
    assert same_bytes(grads(b2, on), grads(b, on))
    # another slot, another batch size, no slack in the layout
    order = [5, 2, 7]
    b3 = Batch([cases[k] for k in order], padded=False).upload()
    sums3, codes3 = b3.run(solver)
    assert same_bytes(sums3, sums[order]) and same_bytes(codes3, codes[order])
    assert same_bytes(grads(b3, slice(None)), grads(b, order))


@pytest.mark.parametrize("shape", [(70, 400, 5, 300), (1025, 65, 3, 40)], ids=lambda s: "n%d_l%d_m%d_t%d" % s)
def test_long_lists_and_more_rows_than_one_chunk(solver, shape):
    """k_term_short beyond one stride: t = 300 (t-length sums over several strides of a lane, cx_active filled past the first 256
    entries of its LDS copy) and n = 1025 (the second chunk of rows of At * cx_active, its partials carried across the chunks)"""
    n, l, m, t = shape
    rng = np.random.default_rng(n + t)
    cases = [tc.make_case(rng, arm, m, n, l, t=tk, q=qk, scaling=False)
             for k, (arm, tk, qk) in enumerate((("none", t, 7), ("c46", t - 1, 0), ("infeasible", t, t // 2), ("sigma_small_t2", t, 0),
                                                ("time", 0, 0)))]
    for scaling in (False, True):
        for c in cases:
            c["scaling"] = scaling
        b = Batch(cases).upload()
        before = b.download()
        sums, codes = b.run(solver)
        assert check_call(solver, b, sums, codes, None, before) == 0


def test_cap_of_the_partial_sum_workgroups(solver):
    """m = 64 * 1024 + 1, n = 2: nblk at its cap of 64 (general form by l = 65), every workgroup walks two strides"""
    cases = make_batch(2, 65, 64 * 1024 + 1, 3, seed=4, scaling=False, arms=["c45", "none", "time"])
    b = Batch(cases).upload()
    before = b.download()
    sums, codes = b.run(solver)
    assert check_call(solver, b, sums, codes, None, before) == 0


@pytest.mark.parametrize("shape", [(64, 8, 130), (65, 8, 1025)], ids=lambda s: "n%d_l%d_m%d" % s)
def test_gradient_and_rx_sum_are_the_existing_calls_bits(solver, shape):
    """dgrad against enlsip_gn_gradient_batched_dev after a ragged solve of the same J, rx; rx_sum against the line-search set-up"""
    import torch
    n, l, m = shape
    B = 5
    cases = make_batch(n, l, m, B, seed=11, scaling=False, arms=["none", "c4", "time"])
    b = Batch(cases, t_max=l).upload()
    sums, codes = b.run(solver)
    grad = grads(b, slice(None)).copy()
    # the line-search set-up on the same rx (Jp = rx: only the third sum is read); the form follows the same rule
    ni = np.array([l - c["t"] for c in cases], dtype=np.int64)
    dA = torch.zeros(B * l * n, dtype=torch.float64, device="cuda:0")
    dAp = torch.zeros(B * l, dtype=torch.float64, device="cuda:0")
    rx = torch.from_numpy(np.ascontiguousarray(b.host["rx"][:, :m])).to("cuda:0")
    cx = torch.from_numpy(np.ascontiguousarray(b.host["cx_all"][:, :l])).to("cuda:0")
    p = torch.from_numpy(np.ascontiguousarray(b.host["p"][:, :n])).to("cuda:0")
    _, _, ls = solver.linesearch_setup_batched_dev(B, m, n, l, p.data_ptr(), dA.data_ptr(), l, l * n, cx.data_ptr(), b.inactive, ni,
                                                   dAp.data_ptr(), dJp=rx.data_ptr(), drx=rx.data_ptr())
    assert same_bytes(ls[:, 2], sums["rx_sum"])
    # a ragged solve makes J, rx resident; the slot of the solve is a well-conditioned one of its own
    rng = np.random.default_rng(5)
    tm = 4
    t = np.array([0, 4, 1, 2, 3], dtype=np.int64)
    At = torch.from_numpy(rng.standard_normal((B, tm, n))).to("cuda:0")
    cxa = torch.from_numpy(rng.standard_normal((B, tm))).to("cuda:0")
    pp = torch.zeros(B * n, dtype=torch.float64, device="cuda:0")
    solver.solve_batched_ragged_dev(B, m, n, tm, t, b.dev["J"].data_ptr(), b.ldj, b.strideJ, rx.data_ptr(), At.data_ptr(), n, n * tm,
                                    cxa.data_ptr(), dp=pp.data_ptr())
    g = torch.zeros(B * n, dtype=torch.float64, device="cuda:0")
    solver.gradient_batched_dev(0, B, g.data_ptr())
    torch.cuda.synchronize()
    assert same_bytes(g.cpu().numpy().reshape(B, n), grad)


def test_fresh_handle_and_between_factor_and_solve():
    """The call needs nothing resident and touches nothing resident: on a fresh handle, and between the batched constraint stage
    and the solve that goes on with it, whose results stay bitwise those of the undisturbed flow."""
    import torch
    from enlsip_gn import GNSolver
    from enlsip_gn import termination as T
    n, l, m, B, tm = 12, 9, 40, 4, 3
    cases = make_batch(n, l, m, B, seed=21, scaling=False, arms=["none", "c46", "max_iter"])
    rng = np.random.default_rng(6)
    t = np.array([3, 0, 2, 1], dtype=np.int64)
    J = rng.standard_normal((B, n, m))
    rx = rng.standard_normal((B, m))
    At = rng.standard_normal((B, tm, n))
    cxa = rng.standard_normal((B, tm))

    def flow(disturb):
        s = GNSolver(device=0)
        try:
            d = {k: torch.from_numpy(v.copy()).to("cuda:0") for k, v in dict(J=J, rx=rx, At=At, cx=cxa).items()}
            out = {k: torch.zeros(B * sz, dtype=torch.float64, device="cuda:0") for k, sz in dict(p=n, b=tm, d=m).items()}
            res = None
            if disturb:
                assert T.termination_form(s) == -1
                b = Batch(cases).upload()
                res = b.run(s)                                        # fresh handle
            s.factor_constraints_batched_dev(B, m, n, tm, t, d["At"].data_ptr(), n, n * tm, d["cx"].data_ptr())
            if disturb:
                res2 = b.run(s)
                assert same_bytes(res2[0], res[0]) and same_bytes(res2[1], res[1])
            s.solve_factored_batched_dev(B, m, n, tm, t, None, d["J"].data_ptr(), m, m * n, d["rx"].data_ptr(), d["At"].data_ptr(), n,
                                         n * tm, d["cx"].data_ptr(), dp=out["p"].data_ptr(), db=out["b"].data_ptr(),
                                         dd=out["d"].data_ptr())
            torch.cuda.synchronize()
            return {k: v.cpu().numpy() for k, v in out.items()}, res
        finally:
            s.close()

    plain, _ = flow(False)
    mixed, res = flow(True)
    for k in plain:
        assert same_bytes(plain[k], mixed[k]), k
    assert [int(c) for c in res[1]] == [tc.oracle_exit(c) for c in cases]


def test_argument_errors_leave_every_buffer_untouched(solver):
    from enlsip_gn import GNError
    from enlsip_gn import termination as T
    n, l, m, B = 5, 7, 20, 3
    cases = make_batch(n, l, m, B, seed=31, scaling=False, arms=["none"])
    b = Batch(cases).upload()
    before = b.download()
    tol = T.make_tol(**tc.TOL)

    def raw(code, needle=None, **ch):
        a = dict(batch=B, m=m, n=n, l=l, t_max=b.t_max, states=b.states(), active=b.active.copy(), inactive=b.inactive.copy(),
                 bufs=b.bufs(), ldj=b.ldj, strideJ=b.strideJ, ldat=b.ldat, strideAt=b.strideAt)
        edit = ch.pop("edit", None)
        a.update(ch)
        if edit:
            edit(a)
        with pytest.raises(GNError) as e:
            T.termination_raw(solver, a["batch"], a["m"], a["n"], a["l"], a["t_max"], a["states"], tol, a["active"], a["inactive"],
                              a["bufs"], False, ldj=a["ldj"], strideJ=a["strideJ"], ldat=a["ldat"], strideAt=a["strideAt"])
        assert f"error {code}:" in str(e.value), (code, str(e.value))
        if needle:
            assert needle in str(e.value), str(e.value)

    def set_state(k, **f):
        def edit(a):
            for name, v in f.items():
                setattr(a["states"][k], name, v)
        return edit

    def set_list(name, k, i, v):
        def edit(a):
            a[name][k, i] = v
        return edit

    def drop(name):
        def edit(a):
            setattr(a["bufs"], name, 0)
        return edit

    def null_host(name):
        """the raw entry point with one HOST pointer NULL"""
        import ctypes as C
        from enlsip_gn.api import _dptr, _fptr
        st = (T.TermState * B)(*b.states())
        sums, codes = np.zeros(B, dtype=T.SUMS_DTYPE), np.zeros(B, dtype=np.int64)
        host = dict(state=C.cast(st, C.c_void_p), tol=C.byref(tol), active=_fptr(b.active), inactive=_fptr(b.inactive), sums=_fptr(sums),
                    exit_code=_fptr(codes), h=solver._h)
        host[name] = None
        u = b.bufs()
        rc = solver._lib.enlsip_gn_termination_batched_dev(
            host["h"], B, m, n, l, b.t_max, host["state"], host["tol"], host["active"], host["inactive"], None, 0, _dptr(u.dJ), b.ldj,
            b.strideJ, _dptr(u.drx), _dptr(u.dcx_all), _dptr(u.dx), _dptr(u.dx_prev), _dptr(u.dp), _dptr(u.dd_gn), _dptr(u.dlambda),
            _dptr(u.dcx_active), _dptr(u.ddiag_scale), _dptr(u.dAt), b.ldat, b.strideAt, _dptr(u.dw), _dptr(u.dgrad), host["sums"],
            host["exit_code"])
        return rc, sums, codes

    assert null_host("h")[0] == -1
    for name in ("state", "tol", "active", "inactive", "sums", "exit_code"):
        rc, sums, codes = null_host(name)
        assert rc == -4 and not codes.any() and not sums["rx_sum"].any(), name
    raw(-3, n=0)
    raw(-4, edit=drop("dcx_active"))
    raw(-4, edit=drop("ddiag_scale"))
    raw(-5, "[1]", edit=set_state(1, l=l + 1))
    raw(-3, m=-1)
    raw(-3, t_max=l + 1)
    for name in ("dJ", "drx", "dcx_all", "dw", "dlambda", "dAt", "dx", "dx_prev", "dp", "dd_gn", "dgrad"):
        raw(-4, edit=drop(name))
    raw(-5, "[1]", edit=set_state(1, t=b.t_max + 1))
    raw(-5, "[2]", edit=set_state(2, t=-1))
    raw(-6, "[1]", edit=set_state(1, q=cases[1]["t"] + 1))
    raw(-6, "[0]", edit=set_state(0, q=-1))
    k_act = next(k for k, c in enumerate(cases) if c["t"] > 0)
    raw(-7, f"[{k_act}]", edit=set_list("active", k_act, 0, l + 1))
    raw(-7, "[2]", edit=set_list("inactive", 2, 0, -1))
    raw(-8, "[1]", edit=set_state(1, dimJ2=n + 1))
    raw(-8, "[0]", edit=set_state(0, dimJ2=-1))
    raw(-9, ldj=m - 1)
    raw(-9, ldat=n - 1)
    raw(-10, strideJ=b.ldj * n - 1)
    raw(-10, strideAt=b.ldat * b.t_max - 1)
    with pytest.raises(GNError) as e:      # batch < 1: no array is read
        solver._chk(solver._lib.enlsip_gn_termination_batched_dev(solver._h, 0, m, n, l, 0, *([None] * 5), 0, None, 1, 1,
                                                                  *([None] * 10), 1, 1, None, None, None, None))
    assert "error -2:" in str(e.value)
    after = b.download()
    for nm in after:
        assert same_bytes(after[nm], before[nm]), nm


def test_driver_builds_the_records_from_working_sets(solver):
    """termination.termination_batched_dev from WorkingSet / IterationRecord objects gives what the raw call gives from the records"""
    import types
    from enlsip_gn import termination as T
    from enlsip_gn.working_set import IterationRecord, WorkingSet
    n, l, m, B = 6, 9, 30, 5
    cases = make_batch(n, l, m, B, seed=41, scaling=False, arms=["none", "c4567", "newton", "restart", "del"])
    b = Batch(cases, padded=False).upload()
    sums, codes = b.run(solver)
    Ws, its = [], []
    for c in cases:
        Ws.append(WorkingSet(c["q"], c["t"], l, c["active"].copy(), c["inactive"][:l - c["q"]].copy()))
        it = IterationRecord(dimJ2=c["dimJ2"], grad_res=c["state"]["grad_res"], delete=c["state"]["delete"], code=c["state"]["code"])
        it.restart, it.nb_newton_steps = c["state"]["restart"], c["state"]["nb_newton_steps"]
        its.append(it)
    st = lambda f: [c["state"][f] for c in cases]
    out = T.termination_batched_dev(solver, Ws, its, b.bufs(), T.make_tol(**tc.TOL), m=m, n=n, t_max=b.t_max, scaling=False,
                                    nb_iter=st("nb_iter"), error_code=st("error_code"), psi_error=st("psi_error"),
                                    delta_time=st("delta_time"), psi0=st("psi0"))
    assert same_bytes(out.sums, sums) and same_bytes(out.exit_code, codes) and same_bytes(out.progress, sums["progress"])
    assert [int(x) for x in out.exit_code] == [tc.oracle_exit(c) for c in cases]
    assert list(out.go_on) == [int(x == 0) for x in codes]


# ---- one full step of two reference problems: addition, solve, line-search set-up, this call ----------------------------------------
def oracle_records(runner):
    """The oracle's outer loop (oracle/enlsip_outer.py, LAPACK backend) with every call of check_termination_criteria recorded:
    its arguments, the point the iteration started from and the point new_point! left, and the exit code it returned."""
    import copy
    from oracle import enlsip_outer as eo
    recs, pts = [], []
    decide, new_point = eo.check_termination_criteria, eo.new_point

    def np_(x, r, c, rx, cx, J, A):
        new_point(x, r, c, rx, cx, J, A)
        pts.append(dict(x=x.copy(), rx=rx.copy(), cx=cx.copy(), J=J.copy(), A=A.copy()))

    def ct(it, prev, W, aC, x, cx, rx_sum, grad, max_iter, nb_iter, ea, er, ex, ec, error_code, dtime, smin, lmax, psi_error):
        code = decide(it, prev, W, aC, x, cx, rx_sum, grad, max_iter, nb_iter, ea, er, ex, ec, error_code, dtime, smin, lmax, psi_error)
        recs.append(dict(it=it.copy(), prev_x=prev.x.copy(), q=W.q, t=W.t, l=W.l, active=np.array(W.active, dtype=np.int64),
                         inactive=np.array(W.inactive, dtype=np.int64), aC=copy.deepcopy(aC), old=pts[-2], new=pts[-1], nb_iter=nb_iter,
                         error_code=error_code, psi_error=psi_error, code=code,
                         tol=dict(max_iter=max_iter, eps_abs=ea, eps_rel=er, eps_x=ex, eps_c=ec)))
        return code

    eo.check_termination_criteria, eo.new_point = ct, np_
    try:
        res = runner(eo.OracleBackend())
    finally:
        eo.check_termination_criteria, eo.new_point = decide, new_point
    return res, recs


def test_one_full_step_reproduces_the_oracles_exit_codes(solver):
    """HS65 (converges, 10300) and HS60 (abnormal, -10), each at the iteration where the oracle's outer loop terminates and at the
    one before it: four slots of one batch (n = m = 3, l = 7).  On the device, per slot: the additions after the previous
    iteration's step and the rebuild of the slot (working_set.add_constraints_batched_dev), the ragged solve on it (p and d), the
    line-search set-up on that p, x + alpha p, and termination.termination_batched_dev on the slot the addition built (the OLD slot),
    the p and d of the solve and prev_iter.x.  What the callbacks and the host stages give comes from the oracle's records:
    alpha, w and psi0 of compute_steplength, lambda of the multiplier estimate, and rx, cx, J at the new point."""
    import torch
    import hs65
    import hs_problems as hp
    from oracle import enlsip_outer as eo
    from enlsip_gn import termination as T
    from enlsip_gn import working_set as ws
    n, m, l, tm = 3, 3, 7, 3
    slots = []
    for runner, final in ((hs65.run, 10300), (lambda b: hp.run("hs60", b), -10)):
        res, recs = oracle_records(runner)
        assert res.exit_code == final and recs[-1]["code"] == final and recs[-2]["code"] == 0
        slots += [(recs[-3], recs[-2]), (recs[-2], recs[-1])]      # (the iteration before: its working set and step; the iteration)
    B = len(slots)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    old = [r["old"] for _, r in slots]
    new = [r["new"] for _, r in slots]
    for (before, r) in slots:      # the point an iteration starts from is the one the iteration before left
        assert np.array_equal(before["new"]["x"], r["old"]["x"]) and r["old"]["J"].shape == (m, n) and r["l"] == l
    # 1. the additions after the previous step, on the full cx of the iteration's starting point, and the rebuild of the slot
    Ws = [ws.WorkingSet(b["q"], b["t"], l, b["active"].copy(), b["inactive"][:l - b["q"]].copy()) for b, _ in slots]
    dA, dcx_all = up([o["A"].T for o in old]), up([o["cx"] for o in old])
    dAt, dcxa, dds = zeros(B, n * tm), zeros(B, tm), zeros(B, tm)
    added, status = ws.add_constraints_batched_dev(solver, Ws, [b["it"].index_alpha_upp for b, _ in slots], dA.data_ptr(),
                                                   dcx_all.data_ptr(), dAt.data_ptr(), dcxa.data_ptr(), dds.data_ptr(), n=n, t_max=tm,
                                                   scaling=False)
    assert not status.any()
    for W, (_, r) in zip(Ws, slots):      # no deletion in these iterations: the solve runs on the working set the walk left
        assert W.t == r["t"] and np.array_equal(W.active[:W.t], r["active"][:r["t"]])
    torch.cuda.synchronize()
    for k, (_, r) in enumerate(slots):
        assert np.allclose(dds[k, :r["t"]].cpu().numpy(), r["aC"].diag_scale[:r["t"]], rtol=1e-14)
    # 2. the solve on that slot: p and d stay on the device
    t = np.array([W.t for W in Ws], dtype=np.int64)
    dJ, drx = up([o["J"].T for o in old]), up([o["rx"] for o in old])
    dp, dd = zeros(B, n), zeros(B, m)
    solver.solve_batched_ragged_dev(B, m, n, tm, t, dJ.data_ptr(), m, m * n, drx.data_ptr(), dAt.data_ptr(), n, n * tm, dcxa.data_ptr(),
                                    dp=dp.data_ptr(), dd=dd.data_ptr())
    torch.cuda.synchronize()
    for k, (_, r) in enumerate(slots):      # Gauss-Newton steps at full dimension in all four iterations
        assert r["it"].code == 1 and np.allclose(dp[k].cpu().numpy(), r["it"].p, rtol=1e-9, atol=1e-12), k
    # 3. the line-search set-up on that p: its bound is the oracle's
    dJp, dAp = zeros(B, m), zeros(B, l)
    solver.jacobian_times_batched_dev(0, B, dp.data_ptr(), dJp.data_ptr())
    ina = np.zeros((B, l), dtype=np.int64)
    for k, W in enumerate(Ws):
        ina[k, :l - W.q] = W.inactive
    alpha_upp, _, _ = solver.linesearch_setup_batched_dev(B, m, n, l, dp.data_ptr(), dA.data_ptr(), l, l * n, dcx_all.data_ptr(), ina,
                                                          l - t, dAp.data_ptr(), index_del=[r["it"].index_del for _, r in slots],
                                                          dJp=dJp.data_ptr(), drx=drx.data_ptr())
    for k, (_, r) in enumerate(slots):
        W = types_ns(q=r["q"], t=r["t"], l=l, active=r["active"], inactive=r["inactive"])
        want, _ = eo.upper_bound_steplength(old[k]["A"], old[k]["cx"], r["it"].p, W, r["it"].index_del)
        assert np.isclose(alpha_upp[k], want, rtol=1e-9), (k, alpha_upp[k], want)
    # 4. the step, with the oracle's alpha; rx, cx, J at the new point are the callbacks' values from the oracle's run
    # dx_prev is prev_iter.x AS THE REFERENCE HOLDS IT at :2838: previous_iter is copied before iter.x is advanced (:2858-2860), so
    # it is the point the PREVIOUS iteration started from, two steps behind the new x, not the point this step started from
    dx_old = up([o["x"] for o in old])
    dx_prev = up([r["prev_x"] for _, r in slots])
    for (before, r) in slots:
        assert np.array_equal(r["prev_x"], before["old"]["x"])
    dx = dx_old + up([[r["it"].alpha] for _, r in slots]) * dp
    assert np.allclose(dx.cpu().numpy(), [p["x"] for p in new], rtol=1e-9, atol=1e-12)
    lam, w, psi0 = np.zeros((B, tm)), np.zeros((B, l)), np.zeros(B)
    for k, (_, r) in enumerate(slots):
        lam[k, :r["t"]] = r["it"].lam[:r["t"]]
        w[k] = r["it"].w
        act = r["active"][:r["t"]] - 1
        psi0[k] = 0.5 * (float(old[k]["rx"] @ old[k]["rx"]) + float(w[k][act] @ (old[k]["cx"][act] ** 2)))      # :2273
    dJn, drxn, dcxn = up([p["J"].T for p in new]), up([p["rx"] for p in new]), up([p["cx"] for p in new])
    dlam, dw, dgrad = up(lam), up(w), zeros(B, n)
    bufs = T.TerminationBuffers(dJ=dJn.data_ptr(), drx=drxn.data_ptr(), dcx_all=dcxn.data_ptr(), dx=dx.data_ptr(),
                                dx_prev=dx_prev.data_ptr(), dp=dp.data_ptr(), dd_gn=dd.data_ptr(), dlambda=dlam.data_ptr(),
                                dcx_active=dcxa.data_ptr(), ddiag_scale=dds.data_ptr(), dAt=dAt.data_ptr(), dw=dw.data_ptr(),
                                dgrad=dgrad.data_ptr())
    its = []
    for _, r in slots:
        it = ws.IterationRecord(dimJ2=r["it"].dimJ2, grad_res=r["it"].grad_res, delete=r["it"].delete, code=r["it"].code)
        it.restart, it.nb_newton_steps = r["it"].restart, r["it"].nb_newton_steps
        its.append(it)
    tols = [r["tol"] for _, r in slots]
    assert all(tl == tols[0] for tl in tols)
    out = T.termination_batched_dev(solver, Ws, its, bufs, T.make_tol(**tols[0]), m=m, n=n, t_max=tm, scaling=False,
                                    nb_iter=[r["nb_iter"] for _, r in slots], error_code=[r["error_code"] for _, r in slots],
                                    psi_error=[r["psi_error"] for _, r in slots], delta_time=-1.0, psi0=psi0)
    print("exit codes", list(out.exit_code), "oracle", [r["code"] for _, r in slots])
    assert [int(c) for c in out.exit_code] == [r["code"] for _, r in slots] == [0, 10300, 0, -10]
    for k, (_, r) in enumerate(slots):      # progress of :2280 and the gradient for the next multiplier estimate
        assert np.isclose(out.progress[k], r["it"].progress, rtol=1e-8, atol=1e-12), (k, out.progress[k], r["it"].progress)
        assert np.allclose(dgrad[k].cpu().numpy(), new[k]["J"].T @ new[k]["rx"], rtol=1e-12, atol=1e-14)


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)
