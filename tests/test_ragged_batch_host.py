"""Ragged batches, host side (no GPU): the two entry points are declared, exported and bound, the Python wrapper packs
differently sized active Jacobians into the documented padded layout, and the Julia glue calls the ragged entry point."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "enlsip.jl_amd" / "python"))

NAMES = ("enlsip_gn_solve_batched_ragged", "enlsip_gn_solve_batched_ragged_dev")


def test_ragged_symbols_declared_and_bound():
    from enlsip_gn import _lib as L
    hdr = (ROOT / "include" / "enlsip_gn.h").read_text()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.PROTOTYPES, name
        assert L.PROTOTYPES[name][1][5] is not None      # t: a host array of int64


def test_ragged_symbols_exported():
    from enlsip_gn import _lib as L
    lib = L.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)],
                         capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT " + name + r"$", out, re.M), name


def test_version_bumped():
    from enlsip_gn import _lib as L
    assert L.load().enlsip_gn_version() >= 201


def test_pack_ragged_layout():
    from enlsip_gn import GNSolver
    n = 5
    rng = np.random.default_rng(0)
    As = [rng.standard_normal((3, n)), np.zeros((0, n)), rng.standard_normal((7, n)), rng.standard_normal((1, n))]
    cxs = [rng.standard_normal(A.shape[0]) for A in As]
    At, cx, t = GNSolver.pack_ragged(As, cxs)
    assert t.dtype == np.int64 and list(t) == [3, 0, 7, 1]
    assert At.shape == (4, 7, n) and cx.shape == (4, 7)
    assert At.flags.c_contiguous     # (batch, t_max, n) C-order = problem k's A' column-major n x t_max at k * n * t_max
    for k, A in enumerate(As):
        tk = A.shape[0]
        assert np.array_equal(At[k, :tk], A) and np.all(At[k, tk:] == 0.0)
        assert np.array_equal(cx[k, :tk], cxs[k]) and np.all(cx[k, tk:] == 0.0)
        # the memory the library reads for problem k: column j of A'_k = row j of A_k
        flat = At.reshape(-1)[k * 7 * n:(k + 1) * 7 * n].reshape(7, n)
        assert np.array_equal(flat[:tk], A)


def test_julia_glue_calls_the_ragged_entry_point():
    glue = (ROOT / "enlsip.jl_amd" / "julia" / "EnlsipHIP.jl").read_text()
    assert re.search(r"ccall\(\(:enlsip_gn_solve_batched_ragged, LIB\)", glue)
    assert re.search(r"function gn_search_direction_batched_hip\([^)]*As::Vector\{Matrix\{Float64\}\}", glue)


def test_pack_ragged_needs_n_when_it_cannot_be_inferred():
    import pytest
    from enlsip_gn import GNSolver
    with pytest.raises(ValueError, match="pass n"):
        GNSolver.pack_ragged([], [])
    with pytest.raises(ValueError, match="pass n"):
        GNSolver.pack_ragged([np.zeros(0), np.zeros(0)], [np.zeros(0), np.zeros(0)])
    At, cx, t = GNSolver.pack_ragged([np.zeros(0), np.zeros(0)], [np.zeros(0), np.zeros(0)], n=4)
    assert At.shape == (2, 0, 4) and cx.shape == (2, 0) and list(t) == [0, 0]
    with pytest.raises(ValueError, match="different column counts"):
        GNSolver.pack_ragged([np.ones((2, 3)), np.ones((1, 4))], [np.ones(2), np.ones(1)])
