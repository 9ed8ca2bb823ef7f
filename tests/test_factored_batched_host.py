"""The batched constraint stage and the solve that goes on with it, host side (no GPU): the entry points are declared, exported and
bound, and the Python wrappers reject badly shaped arguments before anything reaches the library."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))

NAMES = ("enlsip_gn_factor_constraints_batched", "enlsip_gn_factor_constraints_batched_dev",
         "enlsip_gn_solve_factored_batched", "enlsip_gn_solve_factored_batched_dev", "enlsip_gn_get_constraint_refactored")


def test_symbols_declared_and_bound():
    from enlsip_gn import _lib as L
    hdr = (ROOT / "include" / "enlsip_gn.h").read_text()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.PROTOTYPES, name
    # parameter counts of the header (h included)
    for name, count in zip(NAMES, (12, 12, 23, 23, 2)):
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(args.split(",")) == count == len(L.PROTOTYPES[name][1]), name


def test_symbols_exported():
    from enlsip_gn import _lib as L
    lib = L.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT " + name + r"$", out, re.M), name


def unbound_solver():
    """A GNSolver without a handle or a library: any call into C raises AttributeError instead of the ValueError under test."""
    from enlsip_gn import GNSolver
    s = GNSolver.__new__(GNSolver)
    s._lib, s._h = None, None
    return s


def test_wrappers_reject_bad_shapes_before_calling_into_c():
    s = unbound_solver()
    B, t_max, n, m = 3, 4, 5, 7
    At, cx, t = np.zeros((B, t_max, n)), np.zeros((B, t_max)), np.array([4, 0, 2])
    J, rx = np.zeros((B, n, m)), np.zeros((B, m))
    with pytest.raises(ValueError, match="At must be"):
        s.factor_constraints_batched(m, At[0], cx, t)
    with pytest.raises(ValueError, match="cx must be"):
        s.factor_constraints_batched(m, At, cx[:, :3], t)
    with pytest.raises(ValueError, match="t must have 3 entries"):
        s.factor_constraints_batched(m, At, cx, t[:2])
    with pytest.raises(ValueError, match="0..t_max"):
        s.factor_constraints_batched(m, At, cx, np.array([5, 0, 0]))
    with pytest.raises(ValueError, match="0..t_max"):
        s.factor_constraints_batched(m, At, cx, np.array([-1, 0, 0]))
    with pytest.raises(ValueError, match="J must be"):
        s.solve_factored_batched(J[0], rx, At, cx, t)
    with pytest.raises(ValueError, match="columns per constraint"):
        s.solve_factored_batched(np.zeros((B, n + 1, m)), rx, At, cx, t)
    with pytest.raises(ValueError, match="At holds"):
        s.solve_factored_batched(J[:2], rx[:2], At, cx, t)
    with pytest.raises(ValueError, match="rx must be"):
        s.solve_factored_batched(J, rx[:, :6], At, cx, t)
    with pytest.raises(ValueError, match="refactor must have 3 entries"):
        s.solve_factored_batched(J, rx, At, cx, t, refactor=[1, 0])
    with pytest.raises(ValueError, match="t must have 3 entries"):
        s.factor_constraints_batched_dev(B, m, n, t_max, t[:2], 8, n, n * t_max, 8)
    with pytest.raises(ValueError, match="refactor must have 3 entries"):
        s.solve_factored_batched_dev(B, m, n, t_max, t, [1], 8, m, m * n, 8, 8, n, n * t_max, 8)
    # well-shaped arguments do reach the library
    with pytest.raises(AttributeError):
        s.factor_constraints_batched(m, At, cx, t)
    with pytest.raises(AttributeError):
        s.solve_factored_batched(J, rx, At, cx, t, refactor=[1, 0, 0])
