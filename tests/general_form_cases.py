"""Case tables of the general (one 256-thread workgroup per problem) forms of four batched device-buffer calls, past one
256-thread stride and up to the cap of 1024: deletion / restore, additions / rebuild, line-search set-up, penalty weights.  Shared
by tests/test_general_form_cases_host.py, which certifies every table without a GPU, and the four tests/test_gpu_*_general.py.

Nothing here touches a GPU: the expected values come from the host routines and NumPy models the existing test files of each
call already use (their Buffers, host_model / model_delete, edit_cases, check_batch's inputs, Call)."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

import linesearch_cases as lc                               # noqa: E402
import penalty_cases as pc                                  # noqa: E402
import test_gpu_add_constraints_batched as A                # noqa: E402
import test_gpu_delete_constraints_batched as D             # noqa: E402

STRIDE = 256        # threads of a general-form workgroup: list position STRIDE is the first of a loop's second trip
CAP = 1024          # BATCH_MAX_T = LS_MAX_N

# ---- 1. deletion / restore -------------------------------------------------------------------------------------------------------------
DELETE_SHAPES = [(7, 257), (300, 70), (257, 513), (5, 1024), (260, 1024)]      # (n, t_max)
DELETE_BATCH = 7
DESIGNED_T = [257, 513, 1024]
DESIGNED_N = {257: 5, 513: 257, 1024: 5}      # the middle one walks the row loop r += 256 as well


def delete_cases(n, t_max, padded):
    """edit_cases of the call's test file at batch DELETE_BATCH: ragged t with 0 and t_max, scaling on and off, with the record
    and in the second-order form without it"""
    return D.edit_cases(n, t_max, padded, batch=DELETE_BATCH)


def designed_rows(t):
    return sorted({s for s in (1, 256, 257, 258, 512, 513, t - 1, t) if 1 <= s <= t})


def designed_ties(t):
    """positions (1-based) that hold the same v_i == e, in different strides: the last must win"""
    return [p for p in ([10, 300], [10, 300, 600], [255, 256, 257], [1, t]) if p[-1] <= t]


def designed_delete_case(t, padded):
    """One batch at t_max = t, every problem full (q = 0, no scaling, grad_res = 0): lambda is +1 except -1 at the designed row(s),
    so that row is the only candidate (v = -1 <= sqrt(eps) * 1) and the gate of :598 (0 > 10) lets it through.  A tie holds
    -1 at several positions.  The builder asserts that the host routine names the designed position."""
    n = DESIGNED_N[t]
    rows, ties = designed_rows(t), designed_ties(t)
    B = len(rows) + len(ties)
    tt = np.full(B, t, dtype=np.int64)
    q = np.zeros(B, dtype=np.int64)
    buf = D.Buffers(n, t, tt, padded, seed=t)
    buf.lam[:, :], buf.ds[:, :], buf.gres[:] = 1.0, 1.0, 0.0
    designed = np.zeros(B, dtype=np.int64)
    for k, s in enumerate(rows):
        buf.lam[k, s - 1] = -1.0
        designed[k] = s
    for k, pos in enumerate(ties, start=len(rows)):
        buf.lam[k, np.array(pos) - 1] = -1.0
        designed[k] = pos[-1]
    want = buf.images()
    s_want = np.array([D.host_s(0, buf.lam[k], False, buf.ds[k], 0.0) for k in range(B)], dtype=np.int64)
    assert np.array_equal(s_want, designed), (t, s_want, designed)
    D.model_delete(buf, want, s_want, tt, with_saved=True)
    back = s_want.copy()
    back[1::2] = 0      # a proper subset comes back, the row s = 1 (the longest shift) among it
    assert back.any() and (back == 0).any()
    return dict(buf=buf, t=tt, q=q, scaling=False, take=None, gres=True, record=True, s=s_want, want=want, back=back,
                designed=designed, ties=ties, n=n)


# ---- 2. additions / rebuild ------------------------------------------------------------------------------------------------------------
ADD_SHAPES = [(7, 257), (300, 70), (257, 300), (64, 1024), (1024, 65)]      # (n, l), t_max = min(n, l)
ADD_BATCH = 9
ADD_FULL = (1024, 1024)      # batch 3, scaled only
ADD_CAPPED = (320, 400, 300)      # (n, l, t_max): t_max < min(n, l) ends inside tile 4 (columns 256..299); rebuild only


def walk_trace(l, n, q, t, act, ina, cx, iau):
    """addition_walk (gn_violated_constraints.hpp) restated with a record of where it edits the lists.  Used only to CLASSIFY
    problems for the coverage conditions; the expected lists are the host routine's, and the certification asserts that the two
    agree.  Returns (t, act, ina, added, status, active insertion positions, inactive removal positions), positions 0-based."""
    act, ina, t = [int(v) for v in act], [int(v) for v in ina], int(t)
    bnd, cap, passes, status, added, i = min(l, n), (l + 1) ** 2, 0, 0, 0, 1
    ins, rem = [], []
    eps, delta = 2.0 ** -26, 0.1
    while i <= l - t:
        passes += 1
        if passes > cap:
            status = 2
            break
        k = ina[i - 1]
        if k == 0 or not (cx[k - 1] < eps or (k == iau and cx[k - 1] < delta)):
            i += 1
            continue
        if t >= bnd:
            worst_k, worst_val = 0, -np.inf
            for j in range(q + 1, t + 1):
                jj = act[j - 1]
                if jj != 0 and cx[jj - 1] > worst_val:
                    worst_val, worst_k = cx[jj - 1], j
            if not (worst_k > 0 and worst_val > cx[k - 1]):
                i += 1
                continue
            v = act[worst_k - 1]
            p = l - t
            while p > 0 and ina[p - 1] > v:
                p -= 1
            if p == i - 1:
                status = 1
                break
            ina[p + 1:l - t + 1] = ina[p:l - t]
            ina[p] = v
            del act[worst_k - 1]
            act.append(0)
            t -= 1
        v = ina[i - 1]
        p = t
        while p > 0 and act[p - 1] > v:
            p -= 1
        act[p + 1:t + 1] = act[p:t]
        act[p] = v
        ins.append(p)
        rem.append(i - 1)
        del ina[i - 1]
        ina.append(0)
        t += 1
        added = 1
    return t, np.array(act), np.array(ina), added, status, ins, rem


def add_case(n, l, t_max, B, padded, scaling, take, seed, t_cap=None):
    """problems() of the call's test file with two designed problems, its Buffers and its host_model.
    Problem 1 (where l > STRIDE): empty working set, only the LAST constraint violated: the walk removes inactive position
    l - 1 and nothing else.  Problem 2 (where min(n, l) > STRIDE): a working set of the first STRIDE constraints, below
    capacity, only the last constraint violated: it is inserted at active position STRIDE, the first of the second stride."""
    q, t, act, ina, iau, cx = A.problems(n, l, B, seed, t_cap)
    walked = lambda k: take is None or take[k] == 1
    if l > STRIDE and walked(1):
        q[1], t[1], iau[1] = 0, 0, 0
        act[1, :] = 0
        ina[1, :] = np.arange(1, l + 1)
        cx[1, :] = 1.0
        cx[1, l - 1] = -1.0
    if min(n, l) > STRIDE and t_cap is None and walked(2):
        tk = STRIDE
        q[2], t[2], iau[2] = 3, tk, 0
        act[2, :] = 0
        act[2, :tk] = np.arange(1, tk + 1)
        ina[2, :] = 0
        ina[2, :l - tk] = np.arange(tk + 1, l + 1)
        cx[2, :] = 1.0
        cx[2, l - 1] = -1.0
    buf = A.Buffers(n, l, t_max, cx, padded, seed + 1)
    want = buf.images()
    wt, wact, wina, wadd, wst = A.host_model(buf, want, q, t, act, ina, iau, take, scaling)
    return dict(n=n, l=l, t_max=t_max, B=B, scaling=scaling, take=take, q=q, t=t, act=act, ina=ina, iau=iau, buf=buf, want=want,
                wt=wt, wact=wact, wina=wina, wadd=wadd, wst=wst)


def add_shape_cases(n, l, padded):
    """the two runs of the existing test_walk_and_rebuild: no scaling with every problem walked, scaling with the mixed take"""
    t_max = min(n, l)
    return [add_case(n, l, t_max, ADD_BATCH, padded, scaling, take, seed=100 * n + l + int(scaling))
            for scaling, take in ((False, None), (True, A.mixed_take(ADD_BATCH, n + l)))]


def add_full_case():
    n, l = ADD_FULL
    return add_case(n, l, 1024, 3, True, True, None, seed=4)


def add_capped_case():
    n, l, t_max = ADD_CAPPED
    return add_case(n, l, t_max, 5, True, True, np.full(5, 2, dtype=np.int64), seed=6, t_cap=t_max)


def add_positions(c):
    """(largest active insertion position, largest inactive removal position) over the walked problems, 0-based, -1: none"""
    ins, rem = [-1], [-1]
    for k in range(c["B"]):
        if c["take"] is not None and c["take"][k] != 1:
            continue
        tr = walk_trace(c["l"], c["n"], int(c["q"][k]), int(c["t"][k]), c["act"][k], c["ina"][k], c["buf"].cx_all[k], int(c["iau"][k]))
        assert tr[0] == c["wt"][k] and np.array_equal(tr[1], c["wact"][k]) and np.array_equal(tr[2], c["wina"][k]), k
        assert (tr[3], tr[4]) == (c["wadd"][k], c["wst"][k]), k
        ins += tr[5]
        rem += tr[6]
    return max(ins), max(rem)


# ---- 3. line-search set-up -------------------------------------------------------------------------------------------------------------
# check_batch takes the exactly rounded value of every row's sum from mpmath, 4.4 ms per row of 1024 terms: the two large shapes
# run at batch 2 and 1 so that a test stays within seconds (the batch is cut, not the shape).
# (name, seed, B, n, l, m, n_inactive or None: random): seeds whose batches meet the input conditions of linesearch_cases.gap_report (certified on the host)
LS_SHAPES = [("n257_l3", 301, 5, 257, 3, 33, None), ("n1023_l257", 302, 2, 1023, 257, 7, 257), ("n1024_l5", 303, 5, 1024, 5, 1, None),
             ("n2_l1024", 304, 5, 2, 1024, 257, None), ("n1024_l1024", 305, 1, 1024, 1024, 1025, None)]
LS_EDGE_N = [3, 1024]


def ls_conditions(b, k):
    """the input conditions of linesearch_cases.gap_report that check_batch's comparison with the oracle rests on"""
    n = b["A"].shape[2]
    gap, margin, cond = lc.gap_report(b["A"][k], b["p"][k], b["cx"][k], b["inactive"][k], b["n_inactive"][k], b["index_del"][k])
    return gap > lc.GAP and margin > lc.GAP and 4 * n * lc.U * cond <= 1e-12


def ls_batch(name):
    """linesearch_cases.random_batch.  check_batch holds alpha_upp to 1e-12 of the oracle's, which is certain only while
    4 n u cond <= 1e-12 for the winning row (gap_report): at n = 1024 that asks for cond <= 2.2, which no random row of 1024
    terms has.  So where a problem misses the condition, the row that wins is given the signs of -p (its magnitudes stay):
    every product of its sum is then negative, cond = 1 exactly, its alpha only gets smaller and it still wins."""
    _, seed, B, n, l, m, ni = next(s for s in LS_SHAPES if s[0] == name)
    b = lc.random_batch(seed, B, n, l, m, ni)
    for k in range(B):
        if ls_conditions(b, k):
            continue
        A, p, cx, idel = b["A"][k], b["p"][k], b["cx"][k], int(b["index_del"][k])
        Ap = A @ p
        rows = [int(j) for j in b["inactive"][k][:b["n_inactive"][k]] if j and j != idel and cx[j - 1] > 0 and Ap[j - 1] < 0]
        if not rows:
            continue
        j = min(rows, key=lambda r: -cx[r - 1] / Ap[r - 1])
        A[j - 1] = -np.abs(A[j - 1]) * np.where(p < 0, -1.0, 1.0)
    return b


def ls_designed_ties(l=CAP):
    """Edge tuples in the format of linesearch_cases.edge_cases.  Every row is a candidate with alpha = 1 (cx = 1, Ap = -1) except
    two rows with alpha = 0.5 (cx = 1, Ap = -2).  The list is the rows in DESCENDING order, so the first list position never holds
    the lowest row.  same_thread: the two sit at list positions 40 and 40 + 256, which one thread of k_ls_bound visits in that
    order, and its strict < keeps the first.  two_threads: they sit at positions 300 and 40, in different threads; the lower
    position wins in the workgroup's reduction."""
    out = []
    for name, pa, pb in (("tie_same_thread_first_kept", 40, 40 + STRIDE), ("tie_two_threads_lower_position_wins", 300, 40)):
        cx, Ap = np.ones(l), -np.ones(l)
        lst = np.arange(l, 0, -1).astype(np.int64)
        for pos in (pa, pb):
            Ap[lst[pos] - 1] = -2.0
        first = int(lst[min(pa, pb)])
        out.append((name, cx, Ap, lst, l, 0, (0.5, first)))
    return out


# ---- 4. penalty weights ----------------------------------------------------------------------------------------------------------------
PENALTY_SHAPES = [(300, 257), (1024, 3), (1024, 513), (1024, 1024)]      # (l, t_max)
PENALTY_BATCH = 5


def penalty_take(scaling):
    """with scaling one problem is not taken"""
    return np.array([1, 1, 0, 1, 1], dtype=np.int64) if scaling else None


def penalty_call(probs, l, t_max, norm_code, scaling):
    import test_gpu_penalty_weights_batched as P      # its Call builds the device images and the host reference without a GPU
    return P.Call(probs, l, t_max, norm_code, scaling, take=penalty_take(scaling))


def penalty_coverage(probs, l, t_max, norm_code, scaling):
    """From the host routine's answers on the taken problems: (active entries at list position >= STRIDE whose column of K
    changes, problems whose column 0 of K changes: the `moved` branch of the max norm)"""
    call = penalty_call(probs, l, t_max, norm_code, scaling)
    far_moves = first_moved = 0
    for k, c in enumerate(probs):
        if call.take is not None and call.take[k] == 0:
            continue
        hK = call.reference(k)[3]
        changed = set(np.flatnonzero((hK.view(np.uint64) != c["K"].view(np.uint64)).any(axis=0)).tolist())
        if norm_code:
            far_moves += len(set((c["active"][STRIDE:c["t"]] - 1).tolist()) & changed)
        else:
            assert changed <= {0}
            first_moved += len(changed)
    return far_moves, first_moved


def penalty_covered(probs, l, t_max, norm_code):
    for scaling in (False, True):
        far_moves, first_moved = penalty_coverage(probs, l, t_max, norm_code, scaling)
        if (norm_code and t_max > STRIDE and not far_moves) or (not norm_code and not first_moved):
            return False
    return True


def penalty_problems(l, t_max, norm_code):
    """PENALTY_BATCH cases of penalty_cases.random_case at these sizes: t ragged with t_max (twice) and 0, several kinds of bias.
    A seeded search, judged by the host routine alone (penalty_covered), as penalty_cases.wanted does for the branches."""
    for attempt in range(50):
        rng = np.random.default_rng(7000 + 3 * l + t_max + norm_code + 100000 * attempt)
        ts = [t_max, 0, int(rng.integers(1, t_max + 1)), int(rng.integers(min(STRIDE, t_max - 1) + 1, t_max + 1)), t_max]
        kinds = [5, 0, 3, 4, 5] if norm_code else [3, 1, 3, 5, 0]
        probs = [pc.random_case(rng, kind, l=l, t=t, m=8, norm_code=norm_code) for kind, t in zip(kinds, ts)]
        if penalty_covered(probs, l, t_max, norm_code):
            return probs
    raise AssertionError(f"no batch meets the coverage conditions at l = {l}, t_max = {t_max}, norm_code = {norm_code}")
