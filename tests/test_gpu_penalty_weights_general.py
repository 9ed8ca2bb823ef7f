"""The general form of enlsip_gn_penalty_weights_batched_dev (k_penalty<256, 1024>) past one 256-thread stride and up to the cap
t_max = 1024: the case tables of tests/general_form_cases.py (certified by tests/test_general_form_cases_host.py) through Call
of tests/test_gpu_penalty_weights_batched.py: w, K, the scalars and the branch bit for bit the host routine's, sentinel guards
around every buffer, behind t[k] and over the whole of a problem that is not taken, and no input written."""
import numpy as np
import pytest

import general_form_cases as G
import penalty_cases as pc
import test_gpu_penalty_weights_batched as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from enlsip_gn import GNSolver
    s = GNSolver(device=0)
    yield s
    s.close()


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("norm_code", [0, 2])
@pytest.mark.parametrize("l,t_max", G.PENALTY_SHAPES)
def test_five_problems(solver, l, t_max, norm_code, scaling):
    probs = G.penalty_problems(l, t_max, norm_code)
    c = G.penalty_call(probs, l, t_max, norm_code, scaling)
    w, K, scalars, branch = c.check(solver)
    assert c.form == 0
    if norm_code == 2 and not scaling:      # in place as well: step 1 has read what steps 3 and 4 overwrite
        wa, Ka, sa, ba = G.penalty_call(probs, l, t_max, norm_code, scaling).check(solver, alias=True)
        assert P.same(wa, w) and P.same(Ka, K) and P.same(sa, scalars) and np.array_equal(ba, branch)


def test_refusal_past_the_cap(solver):
    """t_max = 1025 with l = 1025 answers -3, writes nothing and leaves the form getter alone"""
    import torch
    from test_gpu_delete_constraints_batched import rc_of
    rng = np.random.default_rng(3)
    small = [pc.random_case(rng, k, l=4, t=2, m=3, norm_code=2) for k in range(3)]
    P.Call(small, 4, 2, 2, False).check(solver)
    assert solver.penalty_form() == 1
    l = t_max = 1025
    probs = [pc.random_case(rng, k, l=l, t=t, m=3, norm_code=2) for k, t in enumerate((1025, 0, 7))]
    c = P.Call(probs, l, t_max, 2, True)
    dev = {k: torch.from_numpy(v.copy()).to("cuda:0") for k, v in c.host.items()}
    torch.cuda.synchronize()
    at = lambda nm, per: dev[nm].data_ptr() + 8 * per
    rc = rc_of(lambda: solver.penalty_weights_batched_dev(c.B, l, t_max, c.t, c.dimA, c.active, 2, True, at("w_old", l), at("Ap", t_max),
                                                          at("ds", t_max), at("cx", l), at("K", 4 * l), c.sums, at("w", l)))
    assert rc == -3 and solver.penalty_form() == 1
    torch.cuda.synchronize()
    for k in c.host:
        assert dev[k].cpu().numpy().tobytes() == c.host[k].tobytes(), k
