"""The changed-problems solve (enlsip_gn_solve_changed_batched), host side (no GPU): the entry points are declared, exported and
bound, and the Python wrappers reject badly shaped arguments before anything reaches the library."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))

NAMES = ("enlsip_gn_solve_changed_batched", "enlsip_gn_solve_changed_batched_dev", "enlsip_gn_get_jacobian_resolved")


def test_symbols_declared_and_bound():
    from enlsip_gn import _lib as L
    hdr = (ROOT / "include" / "enlsip_gn.h").read_text()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.PROTOTYPES, name
    # parameter counts of the header (h included)
    for name, count in zip(NAMES, (19, 19, 2)):
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(args.split(",")) == count == len(L.PROTOTYPES[name][1]), name


def test_header_cites_the_reference_lines_it_serves():
    hdr = (ROOT / "include" / "enlsip_gn.h").read_text()
    at = hdr.index("int enlsip_gn_solve_changed_batched(")
    comment = hdr[hdr.rindex("/*", 0, at):at]
    for cite in (":728-743", ":745-762", ":773-790", ":725", ":771"):
        assert cite in comment, cite


def test_symbols_exported():
    import __graft_entry__ as ge
    ge.build()
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
    s._lib, s._h, s._resident_m = None, None, None
    return s


def test_wrappers_reject_bad_shapes_before_calling_into_c():
    s = unbound_solver()
    B, t_max, n, m = 3, 4, 5, 7
    At, cx, t = np.zeros((B, t_max, n)), np.zeros((B, t_max)), np.array([4, 0, 2])
    ch = [1, 0, 0]
    with pytest.raises(ValueError, match="At must be"):
        s.solve_changed_batched(At[0], cx, t, ch, m=m)
    with pytest.raises(ValueError, match="cx must be"):
        s.solve_changed_batched(At, cx[:, :3], t, ch, m=m)
    with pytest.raises(ValueError, match="t must have 3 entries"):
        s.solve_changed_batched(At, cx, t[:2], ch, m=m)
    with pytest.raises(ValueError, match="0..t_max"):
        s.solve_changed_batched(At, cx, np.array([5, 0, 0]), ch, m=m)
    with pytest.raises(ValueError, match="changed must have 3 entries"):
        s.solve_changed_batched(At, cx, t, [1, 0], m=m)
    with pytest.raises(ValueError, match="changed must have 3 entries"):
        s.solve_changed_batched(At, cx, t, None, m=m)
    with pytest.raises(ValueError, match="t must have 3 entries"):
        s.solve_changed_batched_dev(B, m, n, t_max, t[:2], ch, 8, n, n * t_max, 8)
    with pytest.raises(ValueError, match="changed must have 3 entries"):
        s.solve_changed_batched_dev(B, m, n, t_max, t, [1], 8, n, n * t_max, 8)
    # without a row count (no ragged solve went through this object) the wrapper asks for it
    with pytest.raises(ValueError, match="pass m="):
        s.solve_changed_batched(At, cx, t, ch)
    # well-shaped arguments do reach the library
    with pytest.raises(AttributeError):
        s.solve_changed_batched(At, cx, t, ch, m=m)
    with pytest.raises(AttributeError):
        s.solve_changed_batched_dev(B, m, n, t_max, t, ch, 8, n, n * t_max, 8)
    with pytest.raises(AttributeError):
        s.jacobian_resolved()
