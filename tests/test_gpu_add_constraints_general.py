"""The general form of enlsip_gn_add_constraints_batched_dev (k_add_walk, k_add_gather) past one 256-thread stride and up to the
cap l = t_max = 1024: the case tables of tests/general_form_cases.py (certified by tests/test_general_form_cases_host.py), the
reference and the NaN-guarded buffers of tests/test_gpu_add_constraints_batched.py.  Every comparison is exact: the lists, t,
added, status and every byte of every buffer are those of the two host routines applied per problem, the documented summation
order of the column norms included; nothing between rows n and ldat, behind column t_max, in a problem that is not taken or in
an input may change."""
import numpy as np
import pytest

import general_form_cases as G
from general_form_cases import A, D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


def run_case(solver, c):
    """what run_and_compare of the call's test file asserts, on a case whose expected values are already built"""
    buf, q, t, act, ina = c["buf"], c["q"], c["t"], c["act"], c["ina"]
    buf.upload()
    before = (t.copy(), act.copy(), ina.copy())
    gt, gact, gina, gadd, gst = solver.add_constraints_batched_dev(c["B"], c["n"], c["l"], c["t_max"], q, t, act, ina, c["iau"],
                                                                   c["scaling"], *buf.args(), take=c["take"])
    assert solver.addition_form() == 0
    assert np.array_equal(t, before[0]) and np.array_equal(act, before[1]) and np.array_equal(ina, before[2])
    assert np.array_equal(gst, c["wst"]), np.flatnonzero(gst != c["wst"])
    assert np.array_equal(gt, c["wt"]) and np.array_equal(gadd, c["wadd"])
    assert np.array_equal(gact, c["wact"]) and np.array_equal(gina, c["wina"])
    assert not (c["wst"] == 2).any()
    A.same_images(buf.download(), c["want"], (c["n"], c["l"], c["scaling"]))


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("n,l", G.ADD_SHAPES)
def test_walk_and_rebuild(solver, n, l, padded):
    for c in G.add_shape_cases(n, l, padded):
        run_case(solver, c)


def test_walk_and_rebuild_at_the_cap(solver):
    """(n, l) = (1024, 1024), t_max = 1024: 16 tiles of A', 16 row chunks, 16 squares per column partial"""
    run_case(solver, G.add_full_case())


def test_rebuild_into_a_slot_that_ends_inside_a_tile(solver):
    run_case(solver, G.add_capped_case())


def test_refusal_past_the_cap(solver):
    """l = 1025 (with t_max = 1025 and with a legal t_max) answers -3, writes nothing and leaves the form getter alone"""
    n, l, B = 5, 1025, 5
    q, t, act, ina, iau, cx = A.problems(n, l, B, seed=1)
    buf = A.Buffers(n, l, 1025, cx, True, seed=1).upload()
    before = buf.images()
    qs, ts, acts, inas, iaus, cxs = A.problems(4, 6, B, seed=2)
    small = A.Buffers(4, 6, 4, cxs, True, seed=2).upload()
    solver.add_constraints_batched_dev(B, 4, 6, 4, qs, ts, acts, inas, iaus, True, *small.args())
    assert solver.addition_form() == 1
    for t_max in (1025, 5):
        a = list(buf.args())
        a[6] = buf.ldat * t_max + 5      # strideAt of this t_max
        rc = D.rc_of(lambda: solver.add_constraints_batched_dev(B, n, l, t_max, q, t, act, ina, iau, True, *a))
        assert rc == -3 and solver.addition_form() == 1, (t_max, rc)
    A.same_images(buf.download(), before)
