"""tests/layout_cases.py on the CPU: the builder inverts, everything that is not data is the fill NaN, each named layout has the
parity and alignment its table claims for every case, the restated guard of launch_jq1_v2 agrees with the source line evaluated
directly, expected_route under a layout moves only between the fast and the general J*Q1 kernel, and the oracle solves every
sampled problem at full rank within the conditioning the parity tolerance assumes."""
import re

import numpy as np
import pytest

import consumer_reference as cr
import dispatch_grid as dg
import layout_cases as lc
from oracle import gn_oracle as go

BASE = 7 << 20          # a 256-byte-aligned allocation
# tests/test_gpu_parity.py: forward error <= 1e-13 * cond, compared at TOL_P = 1e-11
KAPPA_MAX = 1e-11 / 1e-13

PAIRS = [(c, ln) for c in lc.ALL_CASES for ln in c.layouts]
IDS = [f"{c.name}-{ln}" for c, ln in PAIRS]


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("case,ln", PAIRS, ids=IDS)
def test_place_round_trip_and_fill(case, ln):
    probs = lc.problems(case)
    lay = lc.LAYOUTS[ln][0]
    pl = lc.place(probs, lay, case.t_max)
    assert (pl.B, pl.m, pl.n, pl.t_max) == (case.B, case.m, case.n, case.t_max) and tuple(pl.ts) == case.ts
    assert pl.ldj == case.m + lay.pad_j and pl.strideJ >= pl.ldj * case.n + lay.gap_j
    assert pl.ldat == case.n + lay.pad_at and pl.strideAt == pl.ldat * case.t_max + lay.gap_at
    assert pl.J.size == lay.off_j + case.B * pl.strideJ + lc.GUARD and pl.At.size == lay.off_at + case.B * pl.strideAt + lc.GUARD
    back = lc.unplace(pl)
    assert len(back) == case.B
    for k in (range(case.B) if case.B <= 200 else lc.sample(case)):
        for a, b in zip(back[k], probs[k]):
            assert same(np.asarray(a), np.asarray(b)), (case.name, ln, k)
    # everything that is not data is the fill, and no datum is
    mj, ma = lc.data_mask(pl)
    assert mj.sum() == case.B * case.m * case.n and ma.sum() == case.n * sum(case.ts)
    for buf, mask in ((pl.J, mj), (pl.At, ma)):
        bits = buf.view(np.uint64)
        assert np.all(bits[~mask] == lc.FILL) and not np.any(bits[mask] == lc.FILL) and np.all(np.isfinite(buf[mask]))
    assert np.all(np.isnan(pl.J[:lay.off_j])) and np.all(np.isnan(pl.J[-lc.GUARD:])) and np.all(np.isnan(pl.At[-lc.GUARD:]))
    for k, tk in enumerate(case.ts):
        assert np.all(pl.cx[k, tk:].view(np.uint64) == lc.FILL) and np.all(np.isfinite(pl.cx[k, :tk]))
    assert np.all(np.isfinite(pl.rx))


@pytest.mark.parametrize("case,ln", PAIRS, ids=IDS)
def test_named_layouts_have_the_parity_and_alignment_of_their_table(case, ln):
    lay, meets = lc.LAYOUTS[ln]
    ldj, sJ, ldat, sAt = lc.strides(lay, case.m, case.n, case.t_max)
    pl = lc.place(lc.problems(case)[:1] * 2, lay, case.t_max) if case.B > 200 else lc.place(lc.problems(case), lay, case.t_max)
    assert (pl.ldj, pl.strideJ, pl.ldat, pl.strideAt) == (ldj, sJ, ldat, sAt)
    assert case.m % 2 == 0                                           # what the table's parity column assumes
    want = {"tight": (0, 0, 0), "even": (0, 0, 0), "odd_ld": (1, 1, 0), "odd_stride": (0, 1, 0), "offset": (0, 0, 8),
            "offset2": (0, 0, 0)}[ln]
    addr = BASE + 8 * lay.off_j
    assert (ldj & 1, sJ & 1, addr & 15) == want, (case.name, ln, ldj, sJ, addr & 15)
    assert lc.v2_layout_ok(ldj, sJ, addr) == meets
    if ln == "offset2":
        assert addr % 16 == 0 and addr % lc.ALLOC_ALIGN == 16
    if ln != "tight":
        assert ldj > case.m and sJ > ldj * case.n and ldat > case.n and sAt > ldat * case.t_max and (BASE + 8 * lay.off_at) % 16 == 8
    # each pipeline half and each chunk starts where the guard answers as it does for the whole batch
    full = pl._replace(B=case.B)
    ok = {lc.v2_layout_ok(ldj, sJ, a) for a in lc.launch_bases(case, full, BASE)}
    assert ok == {meets}, (case.name, ln)
    assert len(lc.launch_bases(case, full, BASE)) == (2 if lc.seams(case) else 1)


def test_restated_guard_agrees_with_the_source_line():
    src = lc.v2_guard_source()
    cond = re.fullmatch(r"if \((.*)\) return false;", src).group(1)
    expr = cond.replace("||", " or ").replace("(size_t)a.J", "addr").replace("a.ldj", "ldj").replace("a.strideJ", "strideJ")
    assert "a." not in expr and "size_t" not in expr, expr
    seen = set()
    for ldj in (255, 256, 257, 263, 264):
        for sJ in (ldj * 128, ldj * 128 + 10, ldj * 128 + 11):
            for addr in (BASE + o for o in (0, 8, 16, 24, 4, 12, 256)):
                rejected = bool(eval(expr, {}, dict(ldj=ldj, strideJ=sJ, addr=addr)))
                assert lc.v2_layout_ok(ldj, sJ, addr) == (not rejected), (ldj, sJ, addr)
                seen.add(rejected)
    assert seen == {True, False}


def test_guard_regex_fails_loudly(monkeypatch, tmp_path):
    fake = tmp_path / "gn_kernels_q1_v2.hpp"
    fake.write_text("inline bool launch_jq1_v2(const JQ1Args& a) {\n    if ((a.ldj & 1) || ((size_t)a.J & 15)) return false;\n}\n")
    monkeypatch.setattr(lc, "CSRC", tmp_path)
    with pytest.raises(AssertionError, match="layout guard"):
        lc.v2_layout_ok(256, 256 * 128, BASE)


@pytest.mark.parametrize("case,ln", PAIRS, ids=IDS)
def test_expected_route_under_a_layout_moves_only_between_v2_and_mfma(case, ln):
    lay, meets = lc.LAYOUTS[ln]
    ldj, sJ, _, _ = lc.strides(lay, case.m, case.n, case.t_max)
    args = (case.B, case.m, case.n, case.t_max)
    tight = dg.expected_route(*args)
    got = dg.expected_route(*args, layout=(ldj, sJ, BASE + 8 * lay.off_j))
    v2 = {b for b in tight if b.startswith("jq1_v2_")}
    if meets or not v2:
        assert got == tight
    else:
        assert len(v2) == 1 and got == (tight - v2) | {"jq1_mfma"}
    assert dg.expected_route(*args, layout=None) == tight
    # the case's own route bits are what the grid expects of its shape on a tight buffer
    if len(set(case.ts)) == 1:
        assert case.route - {"pipeline_split"} <= tight, (case.name, sorted(case.route - tight))
        assert case.pipeline or ("pipeline_split" in case.route) == ("pipeline_split" in tight)
    dummy = lc.place(lc.problems(case)[:1], lay, case.t_max)._replace(B=case.B)
    assert {b for b in case.route if b.startswith("jq1_")} <= lc.expected_route(case, dummy, BASE) | v2


def test_every_jq1_kernel_a_default_handle_can_reach_has_a_case():
    reached = set().union(*(c.route for c in lc.JQ1_CASES))
    names = {b for b in dg.header_route_names() if b.startswith("jq1_")}
    assert names - reached == {"jq1_rows64", "jq1_plain"}            # leading dimensions beyond 2^23 / the get_JQ1 accessor
    assert {"pipeline_split", "chunked"} <= set().union(*(c.route for c in lc.BATCH_CASES))
    assert lc.BATCH_CASES[-1].B == dg.MAX_LAUNCH_BATCH + 1 and all(c.B >= dg.PIPELINE_MIN for c in lc.BATCH_CASES)


@pytest.mark.parametrize("case", lc.ALL_CASES, ids=[c.name for c in lc.ALL_CASES])
def test_oracle_solves_every_sampled_problem_well_conditioned(case):
    probs = lc.problems(case)
    smp = lc.sample(case)
    assert {0, case.B - 1} | set(lc.seams(case)) <= set(smp)
    for k in smp:
        J, rx, A, cx = probs[k]
        tk = case.ts[k]
        ref = go.gn_subproblem(J, rx, A, cx)
        assert ref.rankA == min(case.n, tk) and ref.rankJ2 == min(case.m, case.n - ref.rankA) and np.all(np.isfinite(ref.p)), (case.name, k)
        J2 = ref.F_A.rmul_Q(J)[:, ref.rankA:] if tk else J
        assert cr.kappa(J2) <= KAPPA_MAX and (tk == 0 or cr.kappa(A) <= KAPPA_MAX), (case.name, k, cr.kappa(J2), cr.kappa(A))
