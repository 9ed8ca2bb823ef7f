"""The host side of the batched working-set additions under the sanitizers: tests/addition_walk_check.cpp, a stand-alone program
with its own main that includes only the host-side headers (csrc/gn_violated_constraints.hpp, csrc/gn_batch_records.hpp), built
with -fsanitize=address,undefined.  It runs the walk and the rebuild at their edges (l = 1, q = l, full and empty lists, capacity
swaps, the one-pass cycle) on buffers of exactly their used size and pins the sizes and offsets of the new records, the checks
and the scratch layout.  Nothing is loaded into Python.  Where a GPU is present the program is built without the sanitizers
(they run on CPU-only machines) and the same assertions hold."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
GROUPS = ["walk_l_1", "walk_q_equals_l_full_active_list", "walk_empty_active_list_fills_up", "walk_capacity_swaps",
          "walk_status_1_leaves_the_lists", "walk_zero_entries", "gather_l_1_and_t_0", "gather_full_list_padded_leading_dimensions",
          "gather_zero_row_and_zero_entry", "record_AdditionMeta", "record_AdditionOut", "addition_take", "layout_addition",
          "addition_shape_checks", "addition_per_problem_checks"]


@pytest.fixture(scope="module")
def clang():
    c = CLANG if os.path.exists(CLANG) else shutil.which("clang++")
    if not c:
        pytest.skip("clang++ not found")
    return c


@pytest.fixture(scope="module")
def lines(clang, tmp_path_factory):
    import torch
    exe = tmp_path_factory.mktemp("addition_walk") / "addition_walk_check"
    san = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([clang, "-std=c++17", "-O1", "-g", *san, str(ROOT / "tests" / "addition_walk_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert "AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr
    return out.stdout.splitlines()


def test_the_walk_header_compiles_alone_without_hip(clang):
    subprocess.run([clang, "-std=c++17", "-Wall", "-Werror", "-Wno-pragma-once-outside-header", "-fsyntax-only", "-x", "c++",
                    str(ROOT / "enlsip.jl_amd" / "csrc" / "gn_violated_constraints.hpp")], check=True, capture_output=True, timeout=300)


def test_every_named_assertion_ran_and_held(lines):
    assert [ln for ln in lines if ln.startswith("FAIL")] == []
    assert [ln.split()[1] for ln in lines if ln.startswith("ok ")] == GROUPS
    assert lines[-1] == "0 failures"
