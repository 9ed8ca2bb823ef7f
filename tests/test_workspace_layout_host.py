"""The workspace layouts (csrc/gn_layout.hpp, gn_plan.hpp) on the CPU: tests/layout_check.cpp, a stand-alone program built with
-fsanitize=address,undefined, prints every array of every layout; nothing is loaded into Python.  Where a GPU is present the
program is built without the sanitizers (they run on CPU-only machines) and the same assertions hold.

tests/golden/workspace_layout.json holds the byte offsets of the main workspace (ws) and of the distributed constraint workspace
(cws) as the hand-written carve laid them out before the layouts existed ("Workspace layouts")."""
import json
import os
import shutil
import subprocess
from collections import defaultdict
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    import torch
    clang = CLANG if os.path.exists(CLANG) else shutil.which("clang++")
    if not clang:
        pytest.skip("clang++ not found")
    exe = tmp_path_factory.mktemp("layout") / "layout_check"
    san = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([clang, "-std=c++17", "-O1", "-g", *san, str(ROOT / "tests" / "layout_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert "AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    arrays, totals, pairs = defaultdict(list), {}, {}
    for line in out.stdout.splitlines():
        r = json.loads(line)
        key = (r["layout"], r["shape"])
        if "name" in r:
            arrays[key].append(r)
        elif "measured" in r:
            totals[key] = r
        else:
            pairs[r["shape"]] = r["pair"]
    return arrays, totals, pairs


# (batch, m, n, t, tile_rows, pairs forced): the smallest shapes that reach each branch of the plan geometry, and the benchmark's
PLAN_SHAPES = [(1, 1, 1, 0, 512, 0), (3, 33, 32, 1, 512, 0), (3, 512, 64, 8, 512, 0), (2, 4096, 512, 64, 512, 0), (2, 1056, 100, 0, 512, 1),
               (2, 1056, 100, 0, 256, 1), (1, 40000, 1024, 0, 512, 1), (2, 200, 128, 65, 512, 0), (1, 1024, 1024, 1024, 512, 0),
               (1, 3, 3, 0, 512, 0), (384, 4096, 512, 64, 512, 0), (1024, 512, 64, 8, 512, 0), (1, 262144, 1024, 0, 512, 0),
               (8192, 256, 32, 4, 512, 0)]
EXPECTED = ([(lay, ",".join(map(str, s))) for s in PLAN_SHAPES for lay in ("ws", "cws", "stage_in", "stage_out")] +
            [("tsqr", s) for s in ("1,1", "3,7", "8,1024")] + [("newton", s) for s in ("1,1,0", "5,3,2", "64,64,0")])


def test_every_layout_and_shape_is_reported(report):
    arrays, totals, _ = report
    assert sorted(arrays) == sorted(EXPECTED) and sorted(totals) == sorted(EXPECTED)
    assert len(arrays[("ws", "3,33,32,1,512,0")]) == 31 and len(arrays[("cws", "3,33,32,1,512,0")]) == 15


def test_measured_size_is_the_end_of_the_last_placed_array(report):
    arrays, totals, _ = report
    for key in EXPECTED:
        last = arrays[key][-1]
        assert totals[key]["measured"] == totals[key]["placed_end"] == last["offset"] + last["bytes"], key


def test_arrays_are_disjoint_inside_the_buffer_and_aligned(report):
    arrays, totals, _ = report
    for key in EXPECTED:
        end = 0
        for a in sorted(arrays[key], key=lambda a: a["offset"]):
            assert a["offset"] >= end, (key, a)                    # disjoint
            assert a["offset"] % a["align"] == 0, (key, a)         # aligned as requested
            end = a["offset"] + a["bytes"]
        assert end <= totals[key]["measured"], key                 # inside the buffer


def test_ws_and_cws_offsets_are_those_of_the_hand_written_carve(report):
    arrays, totals, pairs = report
    golden = json.loads((ROOT / "tests" / "golden" / "workspace_layout.json").read_text())
    assert len(golden) == len(PLAN_SHAPES)
    for g in golden:
        shape = ",".join(str(int(g[k])) for k in ("batch", "m", "n", "t", "tile_rows", "pair_forced"))
        assert pairs[shape] == g["pair"], shape
        for lay in ("ws", "cws"):
            got = {a["name"]: a["offset"] for a in arrays[(lay, shape)]}
            assert got == g[lay]["offsets"], (lay, shape)
            # the total may shrink by the removed slack, never grow
            assert totals[(lay, shape)]["measured"] <= g[lay]["parent_bytes"], (lay, shape)
