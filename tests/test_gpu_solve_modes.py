"""Calls of different kinds, and refused calls, interleaved on ONE handle: no call may leave anything behind for the next one.

One long-lived handle walks the sequence below.  After every step that succeeds, all its outputs (p, b, d, the info records, the
three pivot arrays) must be bit for bit those of the same call on a handle created for that step alone, which gets the resident
state the step needs by the shortest sequence.  After a refused step only the return code is checked.

  1. ragged solve                                   6. changed-problems solve with profiling on (see below), profiling off again
  2. batched constraint stage                       7. batched constraint stage
  3. factored solve refused: wrong t[k], no flag    8. factored solve with two refactor flags
  4. ragged solve                                   9. (small shape) constraint stage + factored solve of one problem, a one-rank
  5. changed-problems solve, flags on the              TSQR solve of one problem, a uniform batched solve
     second half only                              10. the ragged solve of step 1: bit for bit the result of step 1

Step 6: profiling switches the pipeline off, so where the resident batch is split (the large shape) the call is refused with -1.
The small batch is never split: there the same call is a valid one and is compared like every other successful step."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

# (m, n, t_max, B, pipeline split): one stream / 130 >= pipeline_min = 128, so two halves of 65
SHAPES = [(48, 12, 4, 5, 0), (96, 72, 5, 130, 65)]


def rc_of(call):
    try:
        call()
    except Exception as e:      # GNError: "libenlsip_gn error <rc>: ..."
        return int(re.search(r"error (-?\d+)", str(e)).group(1))
    return 0


def same_single(got, want):
    """two GNResult / TSQRResult records, field by field"""
    from test_gpu_factored_batched import same
    for name, a in vars(got).items():
        b = getattr(want, name)
        assert (same(a, b) if isinstance(a, np.ndarray) else a == b), name


@pytest.mark.parametrize("m,n,t_max,B,split", SHAPES, ids=lambda v: str(v))
def test_interleaved_calls_leave_nothing_behind(m, n, t_max, B, split):
    from enlsip_gn import GNSolver
    from test_gpu_factored_batched import pack, same_outputs
    from test_gpu_ragged_batch import make_batch
    from test_gpu_solve_changed_batched import poisoned
    ts = [(3 + k) % (t_max + 1) for k in range(B)]
    Js, rxs, As, cxs = make_batch(m, n, ts, seed=23)
    As = [A if t else np.zeros((0, n)) for A, t in zip(As, ts)]
    J, rx, At, cx, t = pack(Js, rxs, As, cxs, t_max)
    # the sets the batch starts from: two problems of the second half with one row fewer (one more when they end with none)
    flags = np.zeros(B, dtype=np.int64)
    flags[[B - 2, B - 1] if split == 0 else [split + 1, B - 1]] = 1
    As0, cxs0 = list(As), list(cxs)
    for k in np.flatnonzero(flags):
        if ts[k]:
            As0[k], cxs0[k] = As[k][:-1], np.asarray(cxs[k])[:-1]
        else:
            As0[k], cxs0[k] = Js[k][:1], np.array([0.5])
    _, _, At0, cx0, t0 = pack(Js, rxs, As0, cxs0, t_max)
    assert int(flags.sum()) == 2 and all(t0[k] != t[k] for k in np.flatnonzero(flags))
    t_bad = t0.copy()
    t_bad[1] = (t0[1] + 1) % (t_max + 1)
    At1, cx1 = poisoned(At, cx, flags)

    made = []

    def fresh():
        made.append(GNSolver(device=0))
        return made[-1]

    s = fresh()
    try:
        # 1
        first = s.solve_batched_ragged(J, rx, At, cx, t)
        assert s.pipeline_split() == split
        same_outputs(first, fresh().solve_batched_ragged(J, rx, At, cx, t))
        # 2
        assert s.factor_constraints_batched(m, At0, cx0, t0) == fresh().factor_constraints_batched(m, At0, cx0, t0)
        # 3
        assert rc_of(lambda: s.solve_factored_batched(J, rx, At0, cx0, t_bad)) == -6
        # 4
        same_outputs(s.solve_batched_ragged(J, rx, At0, cx0, t0), fresh().solve_batched_ragged(J, rx, At0, cx0, t0))
        assert s.pipeline_split() == split
        # 5
        r = fresh()
        r.solve_batched_ragged(J, rx, At0, cx0, t0)
        same_outputs(s.solve_changed_batched(At1, cx1, t, flags), r.solve_changed_batched(At1, cx1, t, flags))
        assert s.jacobian_resolved() == r.jacobian_resolved() == 2
        # 6
        s.set_profiling(True)
        try:
            if split:
                assert rc_of(lambda: s.solve_changed_batched(At1, cx1, t, flags)) == -1
            else:
                got = s.solve_changed_batched(At1, cx1, t, flags)
        finally:
            s.set_profiling(False)
        if not split:
            r = fresh()
            r.solve_batched_ragged(J, rx, At, cx, t)
            r.set_profiling(True)
            same_outputs(got, r.solve_changed_batched(At1, cx1, t, flags))
        # 7
        assert s.factor_constraints_batched(m, At0, cx0, t0) == fresh().factor_constraints_batched(m, At0, cx0, t0)
        # 8
        r = fresh()
        r.factor_constraints_batched(m, At0, cx0, t0)
        same_outputs(s.solve_factored_batched(J, rx, At1, cx1, t, flags), r.solve_factored_batched(J, rx, At1, cx1, t, flags))
        assert s.constraint_refactored() == r.constraint_refactored() == 2 and s.pipeline_split() == split
        # 9
        if split == 0:
            import torch
            from enlsip_gn.tsqr import tsqr_solve_lib
            k1 = 0
            assert ts[k1] > 0
            r = fresh()
            for h in (s, r):
                h.factor_constraints(m, As[k1], cxs[k1])
            same_single(s.solve_factored(Js[k1], rxs[k1], ts[k1]), r.solve_factored(Js[k1], rxs[k1], ts[k1]))
            dev = torch.device("cuda:0")
            targs = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (J[k1], rx[k1], At[k1, :ts[k1]], cx[k1, :ts[k1]])]
            r = fresh()
            for h in (s, r):
                h._chk(h._lib.enlsip_gn_tsqr_set_exchange(h._h, None, None, 1, 0))
            same_single(tsqr_solve_lib(s, *targs), tsqr_solve_lib(r, *targs))
            Ju, rxu, Atu, cxu, _ = pack(*make_batch(m, n, [t_max] * B, seed=29), t_max)
            same_outputs(s.solve_batched(Ju, rxu, Atu, cxu), fresh().solve_batched(Ju, rxu, Atu, cxu))
        # 10
        same_outputs(s.solve_batched_ragged(J, rx, At, cx, t), first)
        assert s.pipeline_split() == split
    finally:
        for h in made:
            h.close()
