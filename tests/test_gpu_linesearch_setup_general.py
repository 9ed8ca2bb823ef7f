"""The general form of enlsip_gn_linesearch_setup_batched_dev (k_ls_product, k_ls_bound) past one 256-thread stride and up to the
cap n = 1024, and at l = 1024: the case tables of tests/general_form_cases.py (certified by
tests/test_general_form_cases_host.py) through check_batch, Call and the sentinel guards of
tests/test_gpu_linesearch_setup_batched.py, with their tolerances unchanged."""
import numpy as np
import pytest

import general_form_cases as G
import linesearch_cases as lc
import test_gpu_linesearch_setup_batched as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


@pytest.mark.parametrize("name", [s[0] for s in G.LS_SHAPES])
def test_random_batches(solver, name):
    b = G.ls_batch(name)
    L.check_batch(solver, name, b)
    assert solver.linesearch_form() == 0


def run_edges(solver, edges, n):
    """what test_named_edges_in_both_forms does with linesearch_cases.edge_cases(l), on any list of such edges"""
    l = edges[0][1].size
    rng = np.random.default_rng(5)
    real = [lc.realise(Ap, n, rng) for _, cx, Ap, *_ in edges]
    b = dict(A=np.stack([r[0] for r in real]), p=np.stack([r[1] for r in real]), cx=np.stack([e[1] for e in edges]),
             inactive=np.stack([e[3] for e in edges]), n_inactive=np.array([e[4] for e in edges], dtype=np.int64),
             index_del=np.array([e[5] for e in edges], dtype=np.int64), Jp=np.ones((len(edges), 3)), rx=np.ones((len(edges), 3)))
    c = L.Call(b)
    Ap, alpha, index, _ = c.run(solver)
    assert c.form == L.expected_form(n, l) == 0
    for k, (name, cx, Ap_want, lst, ni, idel, want) in enumerate(edges):
        assert np.array_equal(Ap[k], Ap_want, equal_nan=True), name      # the product realises the edge exactly
        got = (float(alpha[k]), int(index[k]))
        host = L.host_bound(Ap[k], cx, lst, ni, idel)
        oracle = lc.oracle_bound(Ap[k], cx, lst, ni, idel)
        assert L.same(got[0], host[0]) and got[1] == host[1], (name, got, host)
        assert L.same(got[0], oracle[0]) and got[1] == oracle[1], (name, got, oracle)
        assert want is None or (L.same(got[0], want[0]) and got[1] == want[1]), (name, got, want)


@pytest.mark.parametrize("n", G.LS_EDGE_N)
def test_named_edges_at_l_1024(solver, n):
    run_edges(solver, lc.edge_cases(G.CAP), n)


@pytest.mark.parametrize("n", G.LS_EDGE_N)
def test_designed_ties_across_strides(solver, n):
    """equal alpha at list positions i and i + 256 (one thread, the strict < keeps the first) and at 300 and 40 (two threads,
    the lower position wins in the reduction)"""
    run_edges(solver, G.ls_designed_ties(), n)


def test_refusal_past_the_cap(solver):
    """n = 1025 answers -3, writes nothing and leaves the form getter alone"""
    import torch
    from test_gpu_delete_constraints_batched import rc_of
    b = lc.random_batch(1, 3, 2, 3, 4)
    L.Call(b).run(solver)
    assert solver.linesearch_form() == 1
    B, n, l, m = 3, 1025, 5, 4
    b = lc.random_batch(2, B, n, l, m)
    c = L.Call(b)
    dev = {k: torch.from_numpy(v.copy()).to("cuda:0") for k, v in c.host.items()}
    torch.cuda.synchronize()
    rc = rc_of(lambda: solver.linesearch_setup_batched_dev(B, m, n, l, dev["p"].data_ptr(), dev["A"].data_ptr(), c.lda, c.strideA,
                                                           dev["cx"].data_ptr(), b["inactive"], b["n_inactive"],
                                                           dev["Ap"].data_ptr() + 8 * l, index_del=b["index_del"],
                                                           dJp=dev["Jp"].data_ptr(), drx=dev["rx"].data_ptr()))
    assert rc == -3 and solver.linesearch_form() == 1
    torch.cuda.synchronize()
    for k in c.host:
        assert dev[k].cpu().numpy().tobytes() == c.host[k].tobytes(), k
