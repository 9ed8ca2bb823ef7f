"""The batched Newton direction at the panel, tile and pivot edges of its own kernels, on the GPU, against the references that
tests/test_newton_cases_host.py certifies (tests/newton_cases.py).

Per case and range: the kernel form; status equals the certified verdict on every member; rc == 1 exactly when a taken member is
flagged.  Every positive-definite member: rel(p, p_ref) <= C_EDGE u kappa against the high-precision reference (mpmath where
n <= 40, the longdouble restatement beyond) and rel(p, p_per_problem) <= 2 C_EDGE u kappa against enlsip_gn_newton_direction on a
second handle.  A failing or NaN member: p = 0.0 in every entry, status 1, and its positive-definite neighbours are bit for bit what
they are when its Gamma is replaced by a positive-definite one.  Untaken slots keep the sentinel bytes."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import newton_cases as nc  # noqa: E402
import newton_reference as nr  # noqa: E402
from oracle import gn_oracle as go, synth  # noqa: E402
from test_gpu_newton_batched import SENT, make_solver, per_problem, rel, snapshot  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = nc.cases()


def solve_case(s, c, members=None):
    ks = range(len(c["members"])) if members is None else members
    probs = [nc.member(c, k)[0] for k in ks]
    J = np.stack([np.ascontiguousarray(p[0].T) for p in probs])
    rx = np.stack([p[1] for p in probs])
    if nc.ragged(c) and members is None:
        At, cx, t = s.pack_ragged([p[2] for p in probs], [p[3] for p in probs], n=c["n"])
        return s.solve_batched_ragged(J, rx, At, cx, t)
    t = probs[0][2].shape[0]
    At = np.stack([np.ascontiguousarray(p[2]) for p in probs]) if t else None
    cx = np.stack([p[3] for p in probs]) if t else None
    return s.solve_batched(J, rx, At, cx)


def call(s, G, p0, cnt, take):
    n = G.shape[1]
    p = np.full((cnt, n), SENT, dtype=np.int64).view(np.float64)
    st = np.full(cnt, -77, dtype=np.int32)
    return s.newton_direction_batched(G[p0:p0 + cnt], p0, cnt, take=take[p0:p0 + cnt], out_p=p, out_status=st)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_case(c, monkeypatch):
    B, n = len(c["members"]), c["n"]
    want = [nc.expected_status(c, k) for k in range(B)]
    take = np.array([mb["take"] for mb in c["members"]], dtype=np.int64)
    G = np.stack([nc.member(c, k)[2] for k in range(B)])
    kappa = [nc.certificate(c, k)["kappa"] for k in range(B)]
    s, s1 = make_solver(monkeypatch), make_solver(monkeypatch)
    worst = [0.0, 0.0]
    try:
        solve_case(s, c)
        solve_case(s1, c)
        per = {k: per_problem(s1, k, G[k], n) for k in range(B) if not want[k]}
        full = None
        for p0, cnt in c["ranges"]:
            p, st, rc = call(s, G, p0, cnt, take)
            assert s.newton_form() == c["form"]
            full = p if (p0, cnt) == (0, B) else full
            assert rc == (1 if any(want[p0 + j] and take[p0 + j] for j in range(cnt)) else 0)
            for j in range(cnt):
                k = p0 + j
                if not take[k]:
                    assert st[j] == -77 and np.all(p[j].view(np.int64) == SENT)
                    continue
                assert st[j] == want[k], (c["id"], k, int(st[j]), want[k])
                if want[k]:
                    assert np.all(p[j] == 0.0) and not np.any(np.signbit(p[j]))
                    continue
                bound = nc.bound(kappa[k])
                assert per[k][1] == 0
                # (a wide rank-deficient working set has no high-precision reference, newton_cases.has_reference: per-problem only)
                e_ref, e_per = rel(p[j], nc.reference(c, k).p) if nc.has_reference(c) else 0.0, rel(p[j], per[k][0])
                worst = [max(worst[0], e_ref / bound), max(worst[1], e_per / (2 * bound))]
                print(f"{c['id']}[{k}] range ({p0},{cnt}): vs reference {e_ref:.2e} = {e_ref / (nc.U * kappa[k]):.2f} u kappa (bound {bound:.2e}); "
                      f"vs per-problem {e_per:.2e} (bound {2 * bound:.2e}); kappa {kappa[k]:.2e}")
                assert e_ref <= bound, (c["id"], k, e_ref, bound)
                assert e_per <= 2 * bound, (c["id"], k, e_per, 2 * bound)
        print(f"{c['id']}: worst ratio to the allowance: reference {worst[0]:.3f}, per-problem {worst[1]:.3f}")
        if any(want):
            G2 = G.copy()
            for k in range(B):
                if want[k]:
                    G2[k] = nc.partner_gamma(c, k)
            p2, st2, rc2 = call(s, G2, 0, B, take)
            assert rc2 == 0 and all(st2[k] == 0 for k in range(B) if take[k])
            for k in range(B):
                if take[k] and not want[k]:
                    assert np.array_equal(full[k], p2[k]), (c["id"], k)
                elif take[k]:
                    assert np.all(np.isfinite(p2[k])) and p2[k].any()
    finally:
        s.close()
        s1.close()


def test_ragged_members_against_uniform_batches(monkeypatch):
    c = nc.case("ragged-n40")
    B, n = len(c["members"]), c["n"]
    G = np.stack([nc.member(c, k)[2] for k in range(B)])
    s = make_solver(monkeypatch)
    try:
        solve_case(s, c)
        route = s.route()
        p, st, rc = s.newton_direction_batched(G)
        assert rc == 0 and not st.any()
    finally:
        s.close()
    for k in range(B):
        u = make_solver(monkeypatch)
        try:
            solve_case(u, c, members=[k] * B)
            same = u.route() == route
            pu, stu, rcu = u.newton_direction_batched(np.stack([G[k]] * B))
            assert rcu == 0
            for j in range(B):
                if same:
                    assert np.array_equal(pu[j], p[k]), (k, j, rel(pu[j], p[k]))
                else:
                    assert rel(pu[j], p[k]) <= 2 * nc.bound(nc.certificate(c, k)["kappa"]), (k, j)
            print(f"ragged-n40[{k}] t {c['members'][k]['t']}: {'same kernels, bit for bit' if same else 'other kernels, within the bound'}")
        finally:
            u.close()


@pytest.mark.parametrize("cid", ["edge-n70-t5", "fail-take-n134-t5"])
def test_dev_form_equals_host_form(cid, monkeypatch):
    import torch
    c = nc.case(cid)
    B, n = len(c["members"]), c["n"]
    prob0, count, g = 1, B - 1, 2
    take = np.array([mb["take"] for mb in c["members"]], dtype=np.int64)[prob0:]
    G = np.stack([nc.member(c, prob0 + j)[2] for j in range(count)])
    s = make_solver(monkeypatch)
    try:
        solve_case(s, c)
        ldg, sG = n + 3, (n + 3) * n + 5
        Gd = torch.zeros(count * sG, dtype=torch.float64, device="cuda:0")
        for j in range(count):
            Gd[j * sG:j * sG + ldg * n].view(n, ldg)[:, :n] = torch.from_numpy(np.ascontiguousarray(G[j].T)).to("cuda:0")
        pd = torch.full((count + 2 * g, n), SENT, dtype=torch.int64, device="cuda:0").view(torch.float64)
        sd = torch.full((count + 2 * g,), -77, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        rc = s.newton_direction_batched_dev(prob0, count, Gd.data_ptr(), ldg, sG, pd.data_ptr() + g * n * 8, sd.data_ptr() + g * 4, take=take)
        torch.cuda.synchronize()
        host, st, rch = s.newton_direction_batched(G, prob0, count, take=take)
        assert rc == rch
        pdev, sdev = pd.cpu().numpy(), sd.cpu().numpy()
        assert np.all(pdev[:g].view(np.int64) == SENT) and np.all(pdev[g + count:].view(np.int64) == SENT)
        assert np.all(sdev[:g] == -77) and np.all(sdev[g + count:] == -77)
        for j in range(count):
            if take[j]:
                assert np.array_equal(pdev[g + j], host[j]) and sdev[g + j] == st[j] == nc.expected_status(c, prob0 + j)
            else:
                assert np.all(pdev[g + j].view(np.int64) == SENT) and sdev[g + j] == -77
    finally:
        s.close()


def test_later_consumers_see_no_trace_of_the_call(monkeypatch):
    """resolve and the multiplier estimates after the call return the bytes they return on a handle that never took it"""
    B, m, n, t = 4, 128, 120, 68
    probs = [synth.make_problem(15100 + k, m, n, t) for k in range(B)]
    refs = [go.gn_subproblem(*p) for p in probs]
    G = np.stack([nr.make_gammas(15100 + k, p[0], p[2], r)[0] for k, (p, r) in enumerate(zip(probs, refs))])
    J = np.stack([np.ascontiguousarray(p[0].T) for p in probs])
    rx = np.stack([p[1] for p in probs])
    At = np.stack([np.ascontiguousarray(p[2]) for p in probs])
    cx = np.stack([p[3] for p in probs])
    s, s1 = make_solver(monkeypatch), make_solver(monkeypatch)
    try:
        s.solve_batched(J, rx, At, cx)
        s1.solve_batched(J, rx, At, cx)
        pn, st, rc = s.newton_direction_batched(G)
        assert rc == 0 and not st.any()
        for a, b in zip(snapshot(s, m, n, B), snapshot(s1, m, n, B)):
            assert np.array_equal(a, b)
        for k in range(B):
            (la, ga), (lb, gb) = s.first_lagrange(t, prob=k), s1.first_lagrange(t, prob=k)
            assert np.array_equal(la, lb) and ga == gb
            assert np.array_equal(s.second_lagrange(t, pn[k], prob=k), s1.second_lagrange(t, pn[k], prob=k))
            a = s.resolve(m, n, t, refs[k].rankA, max(refs[k].rankJ2 - 2, 0), -1, k)
            b = s1.resolve(m, n, t, refs[k].rankA, max(refs[k].rankJ2 - 2, 0), -1, k)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), k
    finally:
        s.close()
        s1.close()


@pytest.mark.parametrize("shape", nc.REFUSED_SHAPES, ids=[f"n{n}-t{t}" for n, t in nc.REFUSED_SHAPES])
def test_refused_after_the_distributed_constraint_stage(shape, monkeypatch):
    """kA >= 65 with n t beyond the LDS area of the constraint kernel: the working set is factored by the distributed stage, and
    the call answers -7 and writes nothing"""
    from enlsip_gn.api import GNError
    n, t = shape
    probs = [synth.make_problem(15300 + k, n + 8, n, t) for k in range(2)]
    s = make_solver(monkeypatch)
    try:
        s.solve_batched(np.stack([np.ascontiguousarray(p[0].T) for p in probs]), np.stack([p[1] for p in probs]),
                        np.stack([np.ascontiguousarray(p[2]) for p in probs]), np.stack([p[3] for p in probs]))
        assert "constraint_dist" in s.route()
        p = np.full((2, n), SENT, dtype=np.int64).view(np.float64)
        st = np.full(2, -77, dtype=np.int32)
        with pytest.raises(GNError, match="error -7"):
            s.newton_direction_batched(np.stack([np.eye(n)] * 2), out_p=p, out_status=st)
        assert np.all(p.view(np.int64) == SENT) and np.all(st == -77)
    finally:
        s.close()
