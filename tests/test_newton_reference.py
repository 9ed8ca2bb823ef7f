"""The FP64 restatement of newton_search_direction's lines (tests/test_gpu_parity.py::_newton_reference) held to the mpmath
reference of tests/newton_reference.py on every case of its grid, the error expressed as a multiple of u * cond(sW22).  C_NEWTON,
the constant of the GPU tests' bound, is this measurement's worst multiple times 8.  CPU only."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import newton_reference as nr  # noqa: E402
from oracle import gn_oracle as go  # noqa: E402
from test_gpu_parity import _newton_reference  # noqa: E402  (a plain function; importing the module needs no GPU)


def rel(a, b):
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


def test_form_predicate_is_parsed():
    assert nr.newton_form_limit() == 64


@pytest.mark.parametrize("name", [g[0] for g in nr.GRID])
def test_fp64_oracle_against_mpmath(name):
    J, rx, A, cx = nr.make_case(name)
    n = J.shape[1]
    t = A.shape[0] if A.size else 0
    ref = go.gn_subproblem(J, rx, A, cx)
    Gam, Gbad = nr.make_gammas(500 + n, J, A, ref)
    hi = nr.NewtonReference(J, rx, A, cx, Gam, ref)
    if hi.undefined:            # n > t > rankA: the reference indexes out of bounds; nothing to compare
        assert t != ref.rankA and t < n
        return
    p64, e64 = _newton_reference(J, rx, A, cx, Gam)
    assert not hi.error and not e64
    mult = rel(p64, hi.p) / (nr.U * max(hi.cond, 1.0))
    print(f"{name}: rel {rel(p64, hi.p):.3e}  cond(sW22) {hi.cond:.3e}  multiple of u cond {mult:.3f}")
    assert mult <= nr.C_NEWTON / 8.0, (name, mult)
    if ref.rankA < n:
        bad = nr.NewtonReference(J, rx, A, cx, Gbad, ref)
        pb, eb = _newton_reference(J, rx, A, cx, Gbad)
        assert bad.error and eb and bad.lam_min < -1e-3 * bad.norm
        assert np.all(pb == 0.0) and np.all(bad.p == 0.0)


def test_grid_covers_the_branches():
    seen = set()
    for name, m, n, t, kind in nr.GRID:
        J, rx, A, cx = nr.make_case(name)
        r = go.gn_subproblem(J, rx, A, cx)
        seen.add("t0" if t == 0 else "rankA_eq_n" if r.rankA == n else "undefined" if (t != r.rankA and t < n)
                 else "E_reindexed" if t != r.rankA else "full")
        if m < n - r.rankA:
            seen.add("wide")
        if r.rankJ2 < min(m, n - r.rankA):
            seen.add("rankdefJ")
    assert seen >= {"t0", "rankA_eq_n", "undefined", "E_reindexed", "full", "wide", "rankdefJ"}, seen
