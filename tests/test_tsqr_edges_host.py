"""CPU premises of tests/test_gpu_tsqr_edges.py (cases: tests/tsqr_edge_cases.py), from the oracle and NumPy alone:

* the oracle's unsharded solve finds the literal (rankA, code, n2, rankJ2) of the table;
* rank margin: the last kept diagonal entry of F_A and of F_J2 is at least 1e3 eps_rank dg[0] and the first dropped one at most
  1e-3 eps_rank dg[0] — conditions on the inputs, so a sharded factorisation cannot legitimately decide a rank differently;
* pivot margin: at each of the leading rankJ2 steps of the oracle's pivoted QR of J2 the chosen column's remaining norm exceeds
  the runner-up's by a relative 1e-8, so sharded and unsharded cannot legitimately pick different pivots;
* a NumPy restatement of the sharded algorithm (np.linalg.qr of [J2_g | d_temp_g] per block, zero fill below kp, LAPACK's pivoted
  QR of the stack) reproduces the oracle's pivots and stays below 1e-2 of each tolerance of check_against_oracle (p 1e-11, dlead
  1e-10, d_norm 1e-12): the GPU tolerance is never the binding one on the CPU side.  Where the pivoted QR of J2 truncates, dlead
  is compared on its leading rankJ2 entries only (tsqr_edge_cases.comparable): the rest is not determined by the inputs;
* for a rank-deficient A the pivots of J2 and the entries of Q'd are not determined by the inputs either: the same solve with the
  reflectors of F_A's dropped columns left out (as good a QR of A' as LAPACK's, to rounding) returns the same p and ||d||.

The margins and the restatement's errors are printed (pytest -s)."""
import numpy as np
import pytest

from oracle import gn_oracle as go

import tsqr_edge_cases as ec
import tsqr_magnitude_cases as mc

NAMES = list(ec.CASES) + [ec.GATE.name]

_cache = {}


def _solved(name):
    if name not in _cache:
        J, rx, A, cx = ec.build(name)
        _cache[name] = (J, rx, A, cx, go.gn_subproblem(J, rx, A, cx, ec.get(name).eps_rank))
    return _cache[name]


def restatement(J, rx, A, cx, blocks, eps_rank):
    """The sharded algorithm in NumPy: the constraint stage replicated, one unpivoted QR of [J2_g | d_temp_g] per row block, the
    triangles zero-filled below kp = min(m_g, n2) and stacked, LAPACK's pivoted QR and the rank test on the stack.  Returns a
    TSQRResult-like object for check_against_oracle."""
    from types import SimpleNamespace
    n = J.shape[1]
    t = A.shape[0]
    F_A = go.qr_colnorm(A.T)
    rankA = go.pseudo_rank(F_A.diagR(), eps_rank)
    code = 1 if rankA == t else -1
    b = -cx[F_A.p - 1]
    if code == 1:
        p1 = go._trtrs(F_A.R.T, b, lower=True)
    else:
        F_L = go.qr_colnorm(F_A.R.T)
        bq = F_L.Qt_mul(b)
        dp1 = go._trtrs(F_L.R[:rankA, :rankA], bq[:rankA], lower=False)
        p1 = np.concatenate([dp1, np.zeros(t - rankA)])[go.invperm(F_L.p)][:rankA]
    JQ1 = F_A.rmul_Q(J)
    d_temp = -JQ1[:, :rankA] @ p1 - rx
    J2 = JQ1[:, rankA:]
    n2 = n - rankA
    tris, zs, tail_sq = [], [], 0.0
    lo = 0
    for mg in blocks:
        Rg = np.linalg.qr(np.column_stack([J2[lo:lo + mg], d_temp[lo:lo + mg]]), mode="r")       # min(mg, n2 + 1) x (n2 + 1)
        kp = min(mg, n2)
        T = np.zeros((n2, n2))
        T[:kp] = np.triu(Rg[:kp, :n2])
        z = np.zeros(n2)
        z[:kp] = Rg[:kp, n2]
        tail_sq += float(Rg[kp:, n2] @ Rg[kp:, n2])
        tris.append(T)
        zs.append(z)
        lo += mg
    if n2 == 0:
        p2, dq, rankJ2, jp = np.zeros(0), np.zeros(0), 0, np.zeros(0, dtype=np.int64)
    else:
        F = go.qr_colnorm(np.concatenate(tris, axis=0))
        rankJ2 = go.pseudo_rank(F.diagR(), eps_rank)
        dq = F.Qt_mul(np.concatenate(zs))
        dp2 = go._trtrs(F.R[:rankJ2, :rankJ2], dq[:rankJ2], lower=False)
        p2 = np.concatenate([dp2, np.zeros(n2 - rankJ2)])[go.invperm(F.p)]
        jp = F.p
    p = F_A.Q_mul(np.concatenate([p1, p2]))
    d_norm = float(np.sqrt(tail_sq + float(dq @ dq)))
    return SimpleNamespace(p=p, dlead=dq[:n2].copy(), d_norm=d_norm, rankA=rankA, rankJ2=rankJ2, code=code, jpvtJ2=jp, n2=n2)


def errors_against(out, ref):
    """(rel p, rel dlead, rel d_norm) as check_against_oracle measures them (in-band inputs: plain norms)."""
    nl = ec.comparable(ref)["lead_rows"]
    nl = ref.p.size - ref.rankA if nl is None else nl
    err_p = float(np.linalg.norm(out.p - ref.p) / np.linalg.norm(ref.p))
    lead = np.abs(ref.d[:nl])
    err_l = float(np.abs(np.abs(out.dlead[:nl]) - lead).max() / lead.max()) if nl else 0.0
    nd = float(np.linalg.norm(ref.d))
    return err_p, err_l, abs(out.d_norm - nd) / nd


@pytest.mark.parametrize("name", NAMES)
def test_oracle_finds_the_literal_ranks(name):
    J, rx, A, cx, ref = _solved(name)
    c = ec.get(name)
    n = J.shape[1]
    assert (J.shape[0], A.shape[0]) == (sum(c.blocks), cx.size)
    assert (ref.rankA, ref.code, n - ref.rankA, ref.rankJ2) == c.expected, name
    assert np.all(np.isfinite(ref.p))


def _margin(dg, r, eps_rank):
    """(last kept / dg[0], first dropped / dg[0]) of a diagonal with pseudo-rank r; None where there is no such entry."""
    dg = np.abs(dg)
    kept = float(dg[r - 1] / dg[0]) if r > 0 else None
    dropped = float(dg[r:].max() / dg[0]) if r < dg.size else None
    return kept, dropped


@pytest.mark.parametrize("name", NAMES)
def test_rank_margins(name):
    J, rx, A, cx, ref = _solved(name)
    eps = ec.get(name).eps_rank
    for what, F, r in (("F_A", ref.F_A, ref.rankA), ("F_J2", ref.F_J2, ref.rankJ2)):
        dg = F.diagR()
        if dg.size == 0:
            continue
        kept, dropped = _margin(dg, r, eps)
        print(f"{name} {what}: rank {r} of {dg.size}, last kept {kept if kept is None else f'{kept:.2e}'}, "
              f"first dropped {dropped if dropped is None else f'{dropped:.2e}'} (of dg[0])", flush=True)
        assert kept is None or kept >= 1e3 * eps, (name, what, kept)
        assert dropped is None or dropped <= 1e-3 * eps, (name, what, dropped)


@pytest.mark.parametrize("name", NAMES)
def test_pivot_margins(name):
    """The remaining column norms at step k are those of rows k.. of the unpivoted QR of J2 with its columns in the oracle's pivot
    order."""
    J, rx, A, cx, ref = _solved(name)
    r = ref.rankJ2
    if r == 0:
        return
    J2 = ref.F_A.rmul_Q(J)[:, ref.rankA:]
    R = np.linalg.qr(J2[:, ref.jpvtJ2 - 1], mode="r")
    rem = np.sqrt(np.cumsum((R ** 2)[::-1], axis=0)[::-1])          # rem[k, j] = ||R[k:, j]||
    worst = np.inf
    for k in range(r):
        if k + 1 < R.shape[1]:
            worst = min(worst, float(rem[k, k] / rem[k, k + 1:].max()) - 1.0)
    print(f"{name}: smallest relative lead of a chosen pivot over its runner-up {worst:.2e} ({r} steps)", flush=True)
    assert worst > 1e-8, (name, worst)


@pytest.mark.parametrize("name", NAMES)
def test_numpy_restatement_of_the_sharded_algorithm(name):
    J, rx, A, cx, ref = _solved(name)
    c = ec.get(name)
    out = restatement(J, rx, A, cx, c.blocks, c.eps_rank)
    assert (out.rankA, out.code, out.n2, out.rankJ2) == c.expected, name
    assert np.array_equal(out.jpvtJ2[:ref.rankJ2], ref.jpvtJ2[:ref.rankJ2]), name
    err_p, err_l, err_d = errors_against(out, ref)
    print(f"{name}: restatement against the oracle: rel p {err_p:.2e}  lead {err_l:.2e}  d_norm {err_d:.2e}", flush=True)
    assert err_p <= 1e-2 * 1e-11, (name, err_p)
    assert err_l <= 1e-2 * 1e-10, (name, err_l)
    assert err_d <= 1e-2 * 1e-12, (name, err_d)
    mc.check_against_oracle(out, ref, f"{name} restatement", **ec.comparable(ref))      # the GPU test's own check
    if ref.rankJ2 < out.n2:
        # what lead_rows leaves out is not defined by the inputs: printed so that the reason stays visible
        nt = min(out.n2, ref.d.size)
        dust = float(np.abs(np.abs(out.dlead[ref.rankJ2:nt]) - np.abs(ref.d[ref.rankJ2:nt])).max() / np.abs(ref.d).max()) if nt > ref.rankJ2 else 0.0
        print(f"{name}: entries rankJ2.. of dlead, restatement against the oracle: {dust:.2e} of the largest entry", flush=True)


def test_in_place_offsets_have_both_parities():
    """The in-place cases start shards at odd and at even rows (8-byte and 16-byte aligned bases), and the gate case puts a 64-row
    block of an n = 128, kA = 64 problem with an even leading dimension at an odd row."""
    offs = [o for nm in ec.IN_PLACE for o in ec.offsets(ec.CASES[nm].blocks)[1:]]
    assert sorted(offs) == [513, 1024, 1100, 1800]
    assert any(o % 2 for o in offs) and any(o % 2 == 0 for o in offs)
    g = ec.GATE
    assert ec.offsets(g.blocks)[1] % 2 == 1 and g.blocks[1] % 32 == 0 and sum(g.blocks) % 2 == 0


@pytest.mark.parametrize("name", [nm for nm in NAMES if ec.get(nm).expected[1] == -1])
def test_rank_deficient_A_leaves_J2_defined_up_to_a_rotation(name):
    """Why tsqr_edge_cases.comparable compares neither pivots nor entries of dlead for code -1: with tau of F_A's dropped columns
    set to zero (their reflectors are built from rounding dust: |diag R| there is below 1e-15 of the first) the oracle's own
    arithmetic returns the same p and ||d|| to 1e-13, and whatever pivots and d the different basis of J2 gives."""
    import copy
    J, rx, A, cx, ref = _solved(name)
    eps = ec.get(name).eps_rank
    F_A = copy.deepcopy(ref.F_A)
    F_A.tau[ref.rankA:] = 0.0
    it = go.IterationRecord()
    p, F_J2 = go.gn_search_direction(J, rx, cx, F_A, ref.F_L11, ref.rankA, A.shape[0], eps, it)
    err_p = float(np.linalg.norm(p - ref.p) / np.linalg.norm(ref.p))
    nd = float(np.linalg.norm(ref.d))
    err_d = abs(float(np.linalg.norm(it.d_gn)) - nd) / nd
    n2 = J.shape[1] - ref.rankA
    same_pivots = bool(np.array_equal(F_J2.jpvt, ref.jpvtJ2))
    lead = float(np.abs(np.abs(it.d_gn[:n2]) - np.abs(ref.d[:n2])).max() / np.abs(ref.d[:n2]).max())
    print(f"{name}: without the dust reflectors of F_A: rel p {err_p:.2e}  d_norm {err_d:.2e}  same pivots {same_pivots}  "
          f"dlead differs by {lead:.2e} of its largest entry", flush=True)
    assert it.rankJ2 == ref.rankJ2
    assert err_p <= 1e-13 and err_d <= 1e-13, (name, err_p, err_d)
