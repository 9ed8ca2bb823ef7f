"""The general forms of enlsip_gn_delete_constraints_batched_dev / enlsip_gn_restore_constraints_batched_dev (k_delete_general,
k_restore_general) past one 256-thread stride and up to the cap t_max = 1024: the case tables of tests/general_form_cases.py
(certified by tests/test_general_form_cases_host.py), the reference and the NaN-guarded buffers of
tests/test_gpu_delete_constraints_batched.py.  Every comparison is exact and covers every byte of every buffer: nothing between
rows n and ldat, behind column t_max, in a problem that is not taken or in an input may change."""
import numpy as np
import pytest

import general_form_cases as G
from general_form_cases import D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def run_case(solver, c, n, t_max):
    """the delete, the restore of c["back"] and the restore of nothing, as test_decision_edit_and_restore checks them"""
    buf, t, q = c["buf"], c["t"], c["q"]
    B = len(t)
    buf.upload()
    s = solver.delete_constraints_batched_dev(B, n, t_max, t, q, c["scaling"], buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(),
                                              dgrad_res=buf.ptr("gres") if c["gres"] else 0,
                                              dsaved=buf.ptr("saved") if c["record"] else 0, take=c["take"])
    assert solver.deletion_form() == 0
    assert np.array_equal(s, c["s"]), (s, c["s"])
    after = buf.download()
    D.same_images(after, c["want"])
    if c["back"] is None:
        return
    orig, back = buf.images(), c["back"]
    t1 = t - (s != 0)
    solver.restore_constraints_batched_dev(B, n, t_max, t1, back, buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(), buf.ptr("saved"))
    assert solver.deletion_form() == 0
    got = buf.download()
    for nm in ("At", "cx", "lam", "ds"):
        for k in range(B):
            src = orig if back[k] else after
            assert got[nm][k].tobytes() == src[nm][k].tobytes(), (nm, k)
    assert got["saved"].tobytes() == after["saved"].tobytes() and got["gres"].tobytes() == after["gres"].tobytes()
    solver.restore_constraints_batched_dev(B, n, t_max, t1, np.zeros(B, dtype=np.int64), buf.ptr("lam"), buf.ptr("ds"),
                                           *buf.a_args(), 0)
    D.same_images(buf.download(), got)


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("n,t_max", G.DELETE_SHAPES)
def test_decision_edit_and_restore(solver, n, t_max, padded):
    for c in G.delete_cases(n, t_max, padded):
        run_case(solver, c, n, t_max)


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("t", G.DESIGNED_T)
def test_designed_rows_and_ties(solver, t, padded):
    """the deleted row fixed by construction at 1, 256, 257, 258, 512, 513, t - 1, t, and ties in different strides (the last wins)"""
    c = G.designed_delete_case(t, padded)
    run_case(solver, c, c["n"], t)


def test_refusal_past_the_cap(solver):
    """t_max = 1025 answers -3, writes nothing and leaves the form getter alone"""
    n, t_max, B = 5, 1025, 5
    t = np.array([1025, 0, 3, 1024, 1025], dtype=np.int64)
    q = np.zeros(B, dtype=np.int64)
    buf = D.Buffers(n, t_max, t, True, seed=1)
    before = buf.images()
    buf.upload()
    small = D.Buffers(n, 70, np.full(B, 70, dtype=np.int64), True, seed=2)
    small.upload()
    solver.delete_constraints_batched_dev(B, n, 70, small.t, q, True, small.ptr("lam"), small.ptr("ds"), *small.a_args())
    assert solver.deletion_form() == 0
    solver.delete_constraints_batched_dev(B, n, 4, np.full(B, 4, dtype=np.int64), q, True, small.ptr("lam"), small.ptr("ds"),
                                          small.ptr("At"), small.ldat, small.strideAt, small.ptr("cx"))
    assert solver.deletion_form() == 1      # the getter now differs from what a call at this shape would set
    rc = D.rc_of(lambda: solver.delete_constraints_batched_dev(B, n, t_max, t, q, True, buf.ptr("lam"), buf.ptr("ds"), *buf.a_args(),
                                                               dgrad_res=buf.ptr("gres"), dsaved=buf.ptr("saved")))
    assert rc == -3 and solver.deletion_form() == 1
    rc = D.rc_of(lambda: solver.restore_constraints_batched_dev(B, n, t_max, np.maximum(t - 1, 0), (t > 0).astype(np.int64), buf.ptr("lam"),
                                                                buf.ptr("ds"), *buf.a_args(), buf.ptr("saved")))
    assert rc == -3 and solver.deletion_form() == 1
    D.same_images(buf.download(), before)
