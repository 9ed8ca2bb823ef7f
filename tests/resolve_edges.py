"""Edge cases of the batched re-solve family (gn_kernels_resolve_batched.hpp, gn_resolve_batched.inc), derived FROM the conditions
of its kernels and launch helpers in the manner of tests/dispatch_grid.py: the thresholds are parsed from the C++ sources, not copied.

`grid()` returns the named cases.  A case is one or more resident batches (shape, per-problem t_k, seed) and, per batch, ROUNDS of
explicit requests: one (dimA, dimJ2, code) per slot and call, written out, no positional pattern.  `covered(case)` restates from the
shapes and requests alone (A of full rank: rankA = min(n, t_k), kp = min(m, n - rankA)) which branches of the family the case
executes; tests/test_resolve_edges_host.py::test_grid_reaches_every_branch holds the union against BRANCHES and every case to the
branches it was written for.  The branches:

  head64 / head256            k_resolve_head in its one-wave / general form
  upper_t_1blk                wg_trsv_upper_t (code 1, R_A' p1 = b) with one diagonal block
  upper_t_nb64                ... t_k a multiple of the block width: the last diagonal block is exactly as wide
  upper_t_multi               ... a second block: the between-block update runs
  upper_t_partial             ... a partial block after a full one
  trsv_dimA_64 / _65          wg_trsv<false> of the head (code -1) at dimA = block width / + 1
  trsv_dimJ2_64 / _65         wg_trsv<false> of the tail at dimJ2 = block width / + 1
  tail_wave / tail_reg / tail_mem   k_resolve_tail<1, 64> / <8, 256> / <0, 256> (n beyond the register form: reflectors from memory)
  kp0                         t_k = n for every request of the call, so none has a kp above 0: no panel launch, no Qt'
  kp_eq_m                     kp = m < n2 (a wide problem: the last panel is narrow but carries a full T)
  kp_mixed                    one call whose problems end in different panels (the r0 >= kp return of k_caqr_vec_batched)
  passenger                   the plan's last panel is narrow and only d rode through it: diag(T) alone
  t_gt_n                      t_k > n (kA = n < t_k) in the head's general form

`problems(batch)` builds a batch's inputs and the oracle's solutions once for every test that needs them.

Test infrastructure: nothing here is on the product path."""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass, field
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "enlsip.jl_amd" / "csrc"


def _parse(file: str, pattern: str, *, after: str = "") -> tuple:
    txt = (CSRC / file).read_text()
    if after:
        assert after in txt, (file, after)
        txt = txt[txt.index(after):]
    mt = re.search(pattern, txt)
    assert mt, (file, pattern)
    return tuple(int(g) for g in mt.groups())


SMALL_N, SMALL_T = _parse("gn_resolve_batched.inc", r"bool resolve_small\(const Plan& P\) \{ return P\.n <= ([0-9]+) && P\.t <= ([0-9]+); \}")
TAIL_REG_N, = _parse("gn_resolve_batched.inc", r"else if \(hh->plan\.n <= ([0-9]+)\)", after="void resolve_tail_launch(")
_BLK_M1, BLK = _parse("gn_kernels_resolve_batched.hpp", r"nblk = \(dim \+ ([0-9]+)\) / ([0-9]+);", after="void wg_trsv_upper_t(")
assert _BLK_M1 == BLK - 1
_TRSV_M1, TRSV_BLK = _parse("gn_wg_linalg.hpp", r"nblk = \(dim \+ ([0-9]+)\) / ([0-9]+);", after="__device__ void wg_trsv(")
assert _TRSV_M1 == TRSV_BLK - 1 and TRSV_BLK == BLK          # the branch names below speak of one block width
PB, = _parse("gn_kernels_caqr.hpp", r"constexpr\s+int\s+PB\s*=\s*([0-9]+)")

BRANCHES = ("head64", "head256", "upper_t_1blk", "upper_t_nb64", "upper_t_multi", "upper_t_partial", "trsv_dimA_64", "trsv_dimA_65",
            "trsv_dimJ2_64", "trsv_dimJ2_65", "tail_wave", "tail_reg", "tail_mem", "kp0", "kp_eq_m", "kp_mixed", "passenger", "t_gt_n")

# tolerances of tests/test_gpu_resolve_batched.py::check_against_oracle (rel p with A of full rank / rank deficient, rel b, ||d||,
# |d[:dimJ2]|): the CPU tests hold the reference to a tenth of them
TOL = {"p": 1e-11, "p_deficient": 1e-9, "b": 1e-12, "dnorm": 1e-12, "dabs": 1e-10}


@dataclass(frozen=True)
class Batch:
    """one resident batch: problems synth.make_problem(seed + k, m, n, ts[k]); rounds[r][k] = (dimA, dimJ2, code) of slot k in call r"""
    name: str
    B: int
    m: int
    n: int
    ts: tuple
    seed: int
    rounds: tuple

    @property
    def t(self) -> int:
        return max(self.ts)

    @property
    def ragged(self) -> bool:
        return len(set(self.ts)) > 1

    def rankA(self, k: int) -> int:
        return min(self.n, self.ts[k])

    def kp(self, k: int) -> int:
        return min(self.m, self.n - self.rankA(k))

    @property
    def small(self) -> bool:
        return self.n <= SMALL_N and self.t <= SMALL_T

    @property
    def plan_panels(self) -> int:
        """panels of the sweep the solve launches: J2 as wide as the smallest t_k leaves it"""
        n2_launch = self.n - min(self.n, min(self.ts))
        return (min(self.m, n2_launch) + PB - 1) // PB

    @property
    def pair_variant(self) -> bool:
        """the general form with three panels or more: also run with panel pairs forced"""
        return not self.small and self.plan_panels >= 3


@dataclass(frozen=True)
class Case:
    name: str
    batches: tuple = field(default_factory=tuple)


def _check(b: Batch) -> Batch:
    assert len(b.ts) == b.B and b.rounds
    for rnd in b.rounds:
        assert len(rnd) == b.B, (b.name, rnd)
        for k, (dA, dJ, cd) in enumerate(rnd):
            assert cd in (1, -1, 0), (b.name, k)
            if cd == 0:
                continue
            assert 0 <= dA <= b.rankA(k) and 0 <= dJ <= b.kp(k), (b.name, k, dA, dJ)
            assert cd == -1 or b.rankA(k) == b.ts[k], (b.name, k)          # code 1 needs rankA == t_k
    return b


def grid() -> list:
    cases = []
    # ---- code1_blocks / codem1_blocks: ragged, m = 200, n = 140; kp_k = 140 - t_k
    ts = (63, 64, 65, 128, 130, 0, 64)
    kp = (77, 76, 75, 12, 10, 140, 76)
    code1 = (
        ((63, 77, 1), (64, 76, 1), (65, 75, 1), (128, 12, 1), (130, 10, 1), (0, 140, 1), (64, 76, 1)),      # full dimensions
        ((63, 0, 1), (64, 0, 1), (65, 0, 1), (128, 0, 1), (130, 0, 1), (0, 0, 1), (64, 0, 1)),
        ((63, 1, 1), (64, 1, 1), (65, 1, 1), (128, 1, 1), (130, 1, 1), (0, 1, 1), (64, 1, 1)),
        ((63, 63, 1), (64, 63, 1), (65, 63, 1), (128, 11, 1), (130, 9, 1), (0, 63, 1), (64, 63, 1)),
        ((63, 64, 1), (64, 64, 1), (65, 64, 1), (128, 6, 1), (130, 5, 1), (0, 64, 1), (64, 64, 1)),
        ((63, 65, 1), (64, 65, 1), (65, 65, 1), (128, 2, 1), (130, 2, 1), (0, 65, 1), (64, 65, 1)),
    )
    cases.append(Case("code1_blocks", (_check(Batch("code1_blocks", 7, 200, 140, ts, 12100, code1)),)))
    # dimA in {0, 1, 63, 64, 65, t_k} x dimJ2 in {0, 64, 65, kp}: each of the 24 pairs on a slot that admits it, one code 0 hole
    codem1 = (
        ((1, 0, -1), (1, 65, -1), (65, 64, -1), (1, 12, -1), (63, 10, -1), (0, 0, -1), (64, 65, -1)),
        ((1, 64, -1), (63, 65, -1), (65, 65, -1), (64, 0, -1), (65, 0, -1), (0, 64, -1), (64, 76, -1)),
        ((63, 0, -1), (64, 64, -1), (65, 75, -1), (65, 12, -1), (130, 0, -1), (0, 65, -1), (64, 64, -1)),
        ((63, 64, -1), (64, 65, -1), (0, 0, 0), (128, 12, -1), (130, 10, -1), (0, 140, -1), (63, 76, -1)),
        ((1, 77, -1), (0, 76, -1), (0, 75, -1), (0, 12, -1), (1, 10, -1), (0, 140, -1), (1, 76, -1)),
    )
    cases.append(Case("codem1_blocks", (_check(Batch("codem1_blocks", 7, 200, 140, ts, 12100, codem1)),)))
    assert kp == tuple(cases[0].batches[0].kp(k) for k in range(7))
    # ---- tail_mem: n beyond the register form of F_A.Q
    cases.append(Case("tail_mem", (
        _check(Batch("tail_mem_513", 2, 560, 513, (8, 8), 12200, (
            ((8, 505, 1), (8, 505, -1)),
            ((4, 300, -1), (8, 64, 1)),
        ))),
        _check(Batch("tail_mem_600", 2, 640, 600, (70, 70), 12210, (
            ((70, 530, 1), (70, 530, -1)),
            ((65, 129, -1), (70, 65, 1)),
        ))),
    )))
    # ---- kp_zero: t = n, no J2 at all
    cases.append(Case("kp_zero", (
        _check(Batch("kp_zero_wave", 2, 40, 12, (12, 12), 12300, (
            ((12, 0, 1), (12, 0, -1)),
            ((6, 0, -1), (12, 0, 1)),
        ))),
        _check(Batch("kp_zero_general", 2, 40, 70, (70, 70), 12331, (
            ((70, 0, 1), (70, 0, -1)),
            ((35, 0, -1), (70, 0, 1)),
        ))),
    )))
    # ---- wide: kp = m < n2
    cases.append(Case("wide", (
        _check(Batch("wide_20x100", 3, 20, 100, (4, 4, 4), 12400, (
            ((4, 0, -1), (4, 1, 1), (4, 20, -1)),
            ((4, 20, 1), (2, 1, -1), (0, 20, -1)),
        ))),
        _check(Batch("wide_33x80", 3, 33, 80, (10, 10, 10), 12410, (
            ((10, 0, -1), (10, 1, 1), (10, 33, -1)),
            ((10, 33, 1), (5, 1, -1), (0, 33, -1)),
        ))),
    )))
    # ---- t_gt_n: kA = n < t, code -1 only
    cases.append(Case("t_gt_n", (
        _check(Batch("t_gt_n_wave", 2, 60, 10, (12, 12), 12500, (
            ((10, 0, -1), (0, 0, -1)),
            ((0, 0, -1), (10, 0, -1)),
        ))),
        _check(Batch("t_gt_n_general", 2, 90, 66, (70, 70), 12510, (
            ((66, 0, -1), (0, 0, -1)),
            ((0, 0, -1), (66, 0, -1)),
        ))),
    )))
    # ---- mixed_kp: ragged, kp of 100, 97, 64, 32, 1 and 0 in one range; the third call leaves the two widest alone (two panels)
    cases.append(Case("mixed_kp", (
        _check(Batch("mixed_kp", 6, 300, 100, (0, 3, 36, 68, 99, 100), 12625, (
            ((0, 100, -1), (3, 97, -1), (36, 64, -1), (68, 32, -1), (99, 1, -1), (100, 0, -1)),
            ((0, 64, 1), (3, 65, 1), (36, 63, 1), (68, 32, 1), (99, 1, 1), (100, 0, 1)),
            ((0, 0, 0), (0, 0, 0), (18, 64, -1), (68, 1, -1), (99, 0, -1), (50, 0, -1)),
        ))),
    )))
    return cases


def covered(case: Case) -> set:
    """the branches (of BRANCHES) the calls of `case` execute, from its shapes and requests alone"""
    out = set()
    for b in case.batches:
        n2_launch = b.n - min(b.n, min(b.ts))
        kp_launch = min(b.m, n2_launch)
        narrow_last = kp_launch > 0 and kp_launch % PB != 0 and kp_launch == n2_launch       # d alone rode through the last panel
        for rnd in b.rounds:
            run = [(k, dA, dJ, cd) for k, (dA, dJ, cd) in enumerate(rnd) if cd != 0]
            if not run:
                continue
            out.add("head64" if b.small else "head256")
            out.add("tail_wave" if b.small else ("tail_reg" if b.n <= TAIL_REG_N else "tail_mem"))
            kps = [b.kp(k) for k, _, _, _ in run]
            if max(kps) == 0 and all(b.ts[k] == b.n for k, _, _, _ in run):
                out.add("kp0")
            ends = {(x + PB - 1) // PB for x in kps}
            if len(ends) > 1:
                out.add("kp_mixed")
            if narrow_last and max(ends) == b.plan_panels:
                out.add("passenger")
            for k, dA, dJ, cd in run:
                tk = b.ts[k]
                if b.kp(k) == b.m and b.m < b.n - b.rankA(k):
                    out.add("kp_eq_m")
                if tk > b.n and not b.small:
                    out.add("t_gt_n")
                if cd == 1 and tk > 0:
                    if tk <= BLK:
                        out.add("upper_t_1blk")
                    if tk % BLK == 0:
                        out.add("upper_t_nb64")
                    if tk > BLK:
                        out.add("upper_t_multi")
                        if tk % BLK:
                            out.add("upper_t_partial")
                if cd == -1 and dA in (BLK, BLK + 1):
                    out.add(f"trsv_dimA_{dA}")
                if dJ in (BLK, BLK + 1):
                    out.add(f"trsv_dimJ2_{dJ}")
    return out


def compared(b: Batch):
    """(round, slot, dimA, dimJ2, code) of every request of `b` that is answered and compared"""
    return [(r, k, dA, dJ, cd) for r, rnd in enumerate(b.rounds) for k, (dA, dJ, cd) in enumerate(rnd) if cd != 0]


@functools.lru_cache(maxsize=None)
def problems(b: Batch):
    """(probs, refs) of a batch: its inputs and the oracle's solutions, computed once and left unchanged"""
    from oracle import gn_oracle as go, synth
    probs = [synth.make_problem(b.seed + k, b.m, b.n, b.ts[k]) for k in range(b.B)]
    refs = [go.gn_subproblem(*p) for p in probs]
    for k, r in enumerate(refs):          # what covered() assumes
        assert r.rankA == b.rankA(k) and r.rankJ2 == b.kp(k), (b.name, k, r.rankA, r.rankJ2)
    return probs, refs
