"""Host-side checks of the batched re-solve's mirror (no GPU): the DIM_HOLD constant, the request packing and the output layout of
GNSolver.resolve_batched, and the reference lines the header cites for the new entry points."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "enlsip_gn.h").read_text()


def test_dim_hold_equals_the_headers_constant():
    import enlsip_gn
    from enlsip_gn import _lib as L
    c = int(re.search(r"ENLSIP_GN_DIM_HOLD\s*=\s*(-?\d+)", HEADER).group(1))
    assert enlsip_gn.DIM_HOLD == L.DIM_HOLD == c == -2
    glue = (ROOT / "enlsip.jl_amd" / "julia" / "EnlsipHIP.jl").read_text()
    assert int(re.search(r"const DIM_HOLD\s*=\s*Int64\((-?\d+)\)", glue).group(1)) == c


def test_prototypes_of_the_new_entry_points():
    import ctypes as C
    from enlsip_gn import _lib as L
    for name in ("enlsip_gn_resolve_batched", "enlsip_gn_resolve_batched_dev"):
        res, args = L.PROTOTYPES[name]
        assert res is C.c_int and len(args) == 11 and args[1] is C.c_int64 and args[2] is C.c_int64
    assert len(L.PROTOTYPES["enlsip_gn_get_diagR_batched"][1]) == 6
    assert len(L.PROTOTYPES["enlsip_gn_get_resolve_form"][1]) == 2


def test_request_packing():
    from enlsip_gn import DIM_HOLD, GNSolver
    dA, dJ, cd = GNSolver.pack_resolve(5, [3, 2, DIM_HOLD, 0, 1], DIM_HOLD, [-1, 0, 1, 0, -1])
    for a in (dA, dJ, cd):
        assert a.dtype == np.int64 and a.shape == (5,) and a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"]
    assert list(dA) == [3, 2, -2, 0, 1] and list(dJ) == [-2] * 5 and list(cd) == [-1, 0, 1, 0, -1]
    dA, dJ, cd = GNSolver.pack_resolve(3, 4, 7)          # scalars broadcast, code defaults to -1
    assert list(dA) == [4] * 3 and list(dJ) == [7] * 3 and list(cd) == [-1] * 3
    with pytest.raises(ValueError):
        GNSolver.pack_resolve(3, [1, 2], 0)
    with pytest.raises(ValueError):
        GNSolver.pack_resolve(2, 0, 0, [2, -1])


def test_output_layout_and_null_outputs():
    from enlsip_gn import GNSolver
    from enlsip_gn import _lib as L
    import ctypes as C
    o = GNSolver.resolve_outputs(4, m=7, n=3, t_max=2)
    assert o["p"].shape == (4, 3) and o["b"].shape == (4, 2) and o["d"].shape == (4, 7)
    assert o["info"].shape == (4, 6) and o["info"].dtype == np.int64 and o["info"].itemsize * 6 == C.sizeof(L.Info)
    assert o["status"].shape == (4,) and o["status"].dtype == np.int32
    # slot j of every array starts j strides in: n, t_max, m doubles, one info record, one int
    assert o["p"].strides == (24, 8) and o["b"].strides == (16, 8) and o["d"].strides == (56, 8) and o["info"].strides == (48, 8)
    # what a call leaves alone stays recognisable
    assert np.all(np.isnan(o["p"])) and np.all(o["info"] == -1) and np.all(o["status"] == -1)
    o = GNSolver.resolve_outputs(4, 7, 3, 2, want=("d",))
    assert o["d"] is not None and all(o[k] is None for k in ("p", "b", "info", "status"))
    o = GNSolver.resolve_outputs(2, 7, 3, 0)
    assert o["b"].shape == (2, 0)


def test_header_cites_the_reference_lines_of_each_new_entry_point():
    text = HEADER[HEADER.index("the subspace re-solve over a range"):HEADER.index("int enlsip_gn_get_resolve_form")]
    for cite in ("src/enlsip_functions.jl:116-153", "src/enlsip_functions.jl:1249-1253", "src/enlsip_functions.jl:1118-1176"):
        assert cite in text, cite
    for name in ("enlsip_gn_resolve_batched", "enlsip_gn_resolve_batched_dev", "enlsip_gn_get_diagR_batched", "enlsip_gn_get_resolve_form"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", HEADER), name
    assert "ENLSIP_GN_ROUTE_RESOLVE" not in HEADER        # no new route bits: the form is reported by enlsip_gn_get_resolve_form


def test_what_is_determined_for_a_rank_deficient_member():
    """tests/test_gpu_resolve_batched.py compares a member with a rank-deficient A at the full dimJ2 and leaves the single entries
    of d out.  Shown here with the oracle alone: a 1e-15 relative perturbation of A leaves p (full dimJ2) and ||d|| where they are
    and moves the entries of d and a truncated-dimJ2 p by order one — the trailing columns of F_A.Q come from rounding-level
    reflectors, so J2 is fixed only up to a rotation."""
    import sys
    sys.path.insert(0, str(ROOT / "tests"))
    import test_gpu_resolve_batched as T
    from oracle import gn_oracle as go, synth
    for seed, m, n, t in ((9102, 256, 32, 4), (9104, 600, 40, 6)):
        prob = synth.make_rank_deficient_A(seed, m, n, t)
        ref = go.gn_subproblem(*prob)
        assert ref.rankA < t
        T.assert_deficient_member_is_compared_where_determined(prob, ref)
