"""Ill-conditioned active-constraint Jacobians for the constraint stage, on every route (test infrastructure, CPU only: NumPy, the
oracle's seeded streams and tests/dispatch_grid.py; nothing here touches a GPU).

Every other generator of the suite draws A as a Gaussian matrix, on which dlaqp2's `temp2 <= sqrt(eps)` recompute branch
(oracle/lapack_semantics.py: geqp2) never runs with t <= n.  The kinds below make the pivoted QR of A' (and of R_A') work:

* leader_cluster  A[i] = s_i u + c_i w_i, (u, w_1 .. w_t) orthonormal, s = 2 on one seeded row and 1 elsewhere,
                  c_i = DELTA (1 + step perm(i)).  After the first pivot every remaining norm falls by ~DELTA, so all t - 1 are
                  recomputed, and the later pivots follow the order of the c_i with a relative lead of ~0.8 step: a recompute that
                  is skipped, or taken over the wrong rows, shows in jpvtA.  Needs t <= n - 1.
* graded          singular values 10^(-8 k / (kA - 1)) between random orthogonal factors (consumer_reference.conditioned_A).
* plateau         three plateaus of singular values, each at least 10x away from |R_00| sqrt(kA) eps_rank for eps_rank = 1e-3, 1e-6
                  and 1e-12, and an exactly dependent rest: the designed ranks are returned (tests/test_gpu_parity.py:
                  _plateau_problem, on the A side).
* dependent       the last q rows are combinations of the first t - q, cx consistent with them or not: rankA = min(n, t - q).
* row_scaled      Gaussian rows times 10^(-g i), also for the trapezoidal R of t > n.
* zero            A = 0: rankA = 0, the direction is the unconstrained minimiser.

`constraint_shapes()` derives, from dispatch_grid.expected_route, the smallest (n, t) of every set of constraint route bits, once
with t <= n - 1 and once with t > n where the set has such shapes; `cases()` puts the kinds on them; `j_side_cases()` are leader
clusters with J' = A and t = 0, where J2 = J and the cluster reaches the pivoted QR of R0 intact; `second_attempt_cases(batch)` are
dependent(q) problems whose second attempt (n2 = n - rankA) is routed to other kernels than the first, for a single problem and
for a launch of `batch`.  The premises of every
case are certified by tests/test_constraint_cases_host.py before tests/test_gpu_constraint_conditioning.py uses it."""
from __future__ import annotations

import functools
import math

import numpy as np

import consumer_reference as cr
import dispatch_grid as dg
from oracle import synth

DELTA = 1e-5                    # leader_cluster: distance of the cluster rows from u
STEP = 1e-6                     # leader_cluster: relative spacing of the c_i
EPS_RANKS = (1e-3, 1e-6, 1e-12)  # plateau
SQRT_EPS = math.sqrt(float(np.finfo(np.float64).eps))
T_MIN = 8                       # fewest constraints of a derived shape: below it a cluster has nothing to order
N_MAX, T_MAX = 720, 112         # the lattice constraint_shapes() searches: beyond every threshold of run_constraint_stage


def constraint_bits(route) -> frozenset:
    return frozenset(b for b in route if b.startswith("constraint_"))


def header_constraint_bits() -> list:
    return [b for b in dg.header_route_names() if b.startswith("constraint_")]


# ---- generators: A (t x n) and cx (t) ---------------------------------------------------------------------------------------------
def _perm(seed, stream, count):
    return np.argsort(synth.normal_stream(seed, stream, count), kind="stable")


def leader_cluster(seed, n, t, step=STEP, delta=DELTA):
    """(A, cx, leader): see the module head.  perm(i) is a seeded permutation of 0 .. t-1, `leader` the row with s = 2."""
    assert 2 <= t <= n - 1, "leader_cluster needs t + 1 orthonormal vectors of length n"
    Q = cr._orth(seed, 15, n, t + 1)
    u, W = Q[:, 0], Q[:, 1:]
    leader = int(_perm(seed, 16, t)[0])
    s = np.ones(t)
    s[leader] = 2.0
    c = delta * (1.0 + step * _perm(seed, 17, t).astype(np.float64))
    A = s[:, None] * u[None, :] + c[:, None] * W.T
    return A, synth.normal_stream(seed, 3, t), leader


def graded(seed, n, t, decades=8.0):
    k = min(n, t)
    sig = 10.0 ** (-decades * np.arange(k) / max(k - 1, 1))
    return cr.conditioned_A(seed, n, t, None, sigmas=sig), synth.normal_stream(seed, 3, t)


def plateau(seed, n, t):
    """(A, cx, designed): designed[i] = rankA at EPS_RANKS[i].  kA = min(n, t) >= 8."""
    k = min(n, t)
    assert k >= 8
    r1, r2, r3 = max(k // 3, 1), max(k // 4, 1), max(k // 5, 1)
    L = math.sqrt(k)
    sig = np.zeros(k)
    sig[:r1] = np.linspace(1.0, 0.5, r1)
    r00 = float(np.linalg.norm(cr.conditioned_A(seed, n, t, None, sigmas=sig), axis=1).max()) / math.sqrt(max(n, t))     # |R_00| (the largest row of A) in units of conditioned_A's scale
    sig[r1:r1 + r2] = r00 * L * 10 ** -4.3 * np.linspace(1.1, 0.9, r2)     # between L 1e-3 and L 1e-6, nearer the upper: late |R_ii| fall below their singular values
    sig[r1 + r2:r1 + r2 + r3] = r00 * L * 10 ** -7.7 * np.linspace(1.1, 0.9, r3)    # 50x below L 1e-6, far above L 1e-12
    return cr.conditioned_A(seed, n, t, None, sigmas=sig), synth.normal_stream(seed, 3, t), (r1, r1 + r2, r1 + r2 + r3)


def dependent(seed, n, t, q, consistent=True):
    """(A, cx, rank): rows t-q .. t-1 = W rows 0 .. t-q-1 (W seeded, scaled to keep the row norms); cx[t-q:] = W cx[:t-q] when
    consistent, seeded draws otherwise.  rank = min(n, t - q)."""
    assert 1 <= q <= t - 1
    base = synth.normal_stream(seed, 2, n * (t - q)).reshape((n, t - q), order="F").T
    W = synth.normal_stream(seed, 18, q * (t - q)).reshape((q, t - q), order="F") / math.sqrt(t - q)
    A = np.vstack([base, W @ base])
    cx = synth.normal_stream(seed, 3, t)
    if consistent:
        cx[t - q:] = W @ cx[:t - q]
    return A, cx, min(n, t - q)


def row_scaled(seed, n, t, decades=8.0):
    """Gaussian rows times 10^(-g i), g = decades / (t - 1)."""
    A = synth.normal_stream(seed, 2, n * t).reshape((n, t), order="F").T
    g = decades / max(t - 1, 1)
    return A * (10.0 ** (-g * np.arange(t)))[:, None], synth.normal_stream(seed, 3, t)


def zero(seed, n, t):
    return np.zeros((t, n)), synth.normal_stream(seed, 3, t)


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
def rows_of(n):
    """m of a case unless it says otherwise"""
    return n + 40


@functools.lru_cache(maxsize=None)
def constraint_shapes() -> tuple:
    """((n, t, bits), ...): per set of constraint route bits that a single problem reaches on the lattice n <= N_MAX, t <= T_MAX,
    the shape of smallest n t (then smallest n) with T_MIN <= t <= n - 1, and the one with t > n where the set has any."""
    best = {}
    for n in range(T_MIN, N_MAX + 1):
        for t in range(T_MIN, T_MAX + 1):
            if t == n:
                continue
            key = (constraint_bits(dg.expected_route(1, rows_of(n), n, t)), t > n)
            if key not in best or (n * t, n) < (best[key][0] * best[key][1], best[key][0]):
                best[key] = (n, t)
    out = [(n, t, bits) for (bits, _), (n, t) in best.items()]
    return tuple(sorted(out, key=lambda x: (x[0] * x[1], x[0])))


# further shapes beside the derived ones, with the bits they must reach (checked against expected_route by the host test): the
# upper edges of the wave forms, mid-range shapes of the LDS buckets and of the register and distributed forms, and t > n beside
# every form that has it
LISTED_SHAPES = {
    (24, 8): {"constraint_wave32"}, (32, 32): {"constraint_wave32"},
    (60, 40): {"constraint_wave64"}, (20, 50): {"constraint_wave64"},
    (100, 30): {"constraint_lds_r2"}, (40, 100): {"constraint_lds_r2"},
    (200, 30): {"constraint_lds_r4"}, (500, 16): {"constraint_lds_r8"}, (700, 10): {"constraint_lds_r16"},
    (513, 17): {"constraint_global", "constraint_lds_r16"},
    (129, 64): {"constraint_reg4", "constraint_lds_r1_512"}, (256, 33): {"constraint_reg4", "constraint_lds_r1_512"},
    (257, 32): {"constraint_reg8", "constraint_lds_r1_256"}, (512, 17): {"constraint_reg8", "constraint_lds_r1_256"},
    (127, 65): {"constraint_dist", "constraint_lds_r2"}, (80, 110): {"constraint_dist", "constraint_lds_r2"},
    (300, 70): {"constraint_dist", "constraint_lds_r8"},
}

# the forms of the constraint stage, each named by the bit that tells it from the others, in the order the full set of kinds
# (plateau, dependent, zero) is put on them
FORMS = ("constraint_wave32", "constraint_wave64", "constraint_lds_r2", "constraint_global", "constraint_reg4", "constraint_reg8",
         "constraint_dist")


def all_shapes() -> list:
    """[(n, t, bits)]: the derived shapes, then the listed ones that are not among them."""
    out = list(constraint_shapes())
    have = {(n, t) for n, t, _ in out}
    for (n, t) in LISTED_SHAPES:
        if (n, t) not in have:
            out.append((n, t, constraint_bits(dg.expected_route(1, rows_of(n), n, t))))
    return out


def admits_leader(n, t) -> bool:
    return 2 <= t <= n - 1


def form_shapes() -> dict:
    """{form bit: (n, t)}: per form its smallest derived shape with t <= n - 1."""
    out = {}
    for n, t, bits in constraint_shapes():
        for f in FORMS:
            if f in bits and t <= n - 1 and f not in out and (f != "constraint_lds_r2" or len(bits) == 1):
                out[f] = (n, t)
    return out


# ---- the case list ---------------------------------------------------------------------------------------------------------------
def _case(kind, n, t, bits, seed, *, m=None, eps_ranks=(SQRT_EPS,), ranks=None, **params):
    tag = "".join(f"-{k}{v}" for k, v in sorted(params.items()))
    return dict(id=f"{kind}-n{n}-t{t}{tag}", kind=kind, n=n, t=t, m=rows_of(n) if m is None else m, bits=set(bits), seed=seed,
                eps_ranks=tuple(eps_ranks), ranks=ranks, params=params)


def _seed(kind, n, t, extra=0):
    return 51000 + 7 * dg_hash(f"{kind}-{n}-{t}") % 20000 + extra


def dg_hash(s: str) -> int:
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % 1000003
    return h


@functools.lru_cache(maxsize=None)
def _cases() -> tuple:
    out = []
    for n, t, bits in all_shapes():
        if admits_leader(n, t):
            out.append(_case("leader_cluster", n, t, bits, _seed("leader", n, t)))
        out.append(_case("graded", n, t, bits, _seed("graded", n, t)))
        if not admits_leader(n, t):
            out.append(_case("row_scaled", n, t, bits, _seed("row_scaled", n, t)))
    forms = form_shapes()
    for f in FORMS:
        n, t = forms[f]
        bits = constraint_bits(dg.expected_route(1, rows_of(n), n, t))
        out.append(_case("row_scaled", n, t, bits, _seed("row_scaled", n, t)))
        designed = plateau(_seed("plateau", n, t), n, t)[2]
        out.append(_case("plateau", n, t, bits, _seed("plateau", n, t), eps_ranks=EPS_RANKS, ranks=designed))
        for q in sorted({2, t // 2, t - 1}):
            out.append(_case("dependent", n, t, bits, _seed("dependent", n, t, q), ranks=(min(n, t - q),), q=q, consistent=1))
        out.append(_case("dependent", n, t, bits, _seed("dependent", n, t, 977), ranks=(min(n, t - t // 2),), q=t // 2, consistent=0))
        out.append(_case("zero", n, t, bits, _seed("zero", n, t), ranks=(0,)))
    # t > n with a plateau and a defect: the trapezoidal R decides the rank from kA = n entries
    for n, t, bits in constraint_shapes():
        if t > n and ("constraint_wave64" in bits or "constraint_dist" in bits or bits == {"constraint_lds_r2"}):
            designed = plateau(_seed("plateau", n, t), n, t)[2]
            out.append(_case("plateau", n, t, bits, _seed("plateau", n, t), eps_ranks=EPS_RANKS, ranks=designed))
            q = t - n // 2
            out.append(_case("dependent", n, t, bits, _seed("dependent", n, t, q), ranks=(min(n, t - q),), q=q, consistent=1))
    ids = [c["id"] for c in out]
    assert len(ids) == len(set(ids)), ids
    return tuple(out)


def cases() -> list:
    return list(_cases())


def build(c):
    """(J, rx, A, cx) of a case: J and rx are the Gaussian draws of synth.make_problem, A and cx come from the case's kind."""
    n, t, seed, kind = c["n"], c["t"], c["seed"], c["kind"]
    J, rx, _, _ = synth.make_problem(seed, c["m"], n, 0)
    if kind == "leader_cluster":
        A, cx, _ = leader_cluster(seed, n, t)
    elif kind == "graded":
        A, cx = graded(seed, n, t)
    elif kind == "plateau":
        A, cx, _ = plateau(seed, n, t)
    elif kind == "dependent":
        A, cx, _ = dependent(seed, n, t, c["params"]["q"], bool(c["params"]["consistent"]))
    elif kind == "row_scaled":
        A, cx = row_scaled(seed, n, t)
    elif kind == "zero":
        A, cx = zero(seed, n, t)
    else:
        raise ValueError(kind)
    return J, rx, A, cx


def coverage(cs=None) -> dict:
    """{constraint bit: kinds that reach it}"""
    out = {b: set() for b in header_constraint_bits()}
    for c in (cases() if cs is None else cs):
        for b in c["bits"]:
            out[b].add(c["kind"])
    return out


# ---- the cluster on the J side --------------------------------------------------------------------------------------------------
def pivot_bits(route) -> frozenset:
    return frozenset(b for b in route if b.startswith("pivot_"))


def j_side_problem(seed, m, n):
    """(J m x n, rx): J' is a leader cluster (n rows of length m), so with t = 0 the pivoted QR of R0 meets it intact."""
    A, _, _ = leader_cluster(seed, m, n)
    return np.ascontiguousarray(A.T), synth.normal_stream(seed, 1, m)


@functools.lru_cache(maxsize=None)
def j_side_cases() -> tuple:
    """One leader cluster per pivot route a small shape reaches with t = 0, m = n + 8: the smallest n of pivot_wave32, pivot_wave64,
    pivot_wave2 (batch 2), the first LDS bucket, and pivot_blocks at kp = 91, 129 and 257 (one, two and three block sizes)."""
    out = []

    def add(tag, batch, n, want):
        m = n + 8
        got = pivot_bits(dg.expected_route(batch, m, n, 0))
        assert want <= got, (tag, n, got)
        out.append(dict(id=f"jside-{tag}-b{batch}-{m}x{n}", batch=batch, m=m, n=n, bits=set(got), seed=_seed("jside", n, batch)))

    def smallest(batch, bit):
        return next(n for n in range(T_MIN, N_MAX) if bit in dg.expected_route(batch, n + 8, n, 0))

    add("wave32", 1, smallest(1, "pivot_wave32"), {"pivot_wave32"})
    add("wave64", 1, smallest(1, "pivot_wave64"), {"pivot_wave64"})
    add("wave2", 2, smallest(2, "pivot_wave2"), {"pivot_wave2"})
    n_lds = next(n for n in range(T_MIN, N_MAX) if any(b.startswith("pivot_lds") for b in dg.expected_route(1, n + 8, n, 0))
                 and "pivot_blocks" not in dg.expected_route(1, n + 8, n, 0))
    add("lds", 1, n_lds, set())
    for kp in (91, 129, 257):
        add("blocks", 1, kp, {"pivot_blocks"})
    return tuple(out)


# ---- second attempt across a dispatch boundary ------------------------------------------------------------------------------------
RAGGED_EXTRA = (2, 0, 0, 1, 2)     # t_k - t of the ragged batch of five around a second-attempt case: member 2 is the deficient one,
                                   # and no member has fewer constraints than it, so the launch is planned for n2 = n - t


def j_bits(route) -> frozenset:
    """the bits of the Jacobian side: J*Q1, sweep, pivoted QR of R0"""
    return frozenset(b for b in route if b.startswith(("jq1_", "sweep_", "pivot_")))


@functools.lru_cache(maxsize=None)
def second_attempt_cases(batch=1) -> tuple:
    """dependent(q) problems, found on a small lattice from expected_route for a launch of `batch` problems: the first attempt is
    planned for n2 = n - t (the smallest t of the launch), the second runs with n2 = n - rankA = n - t + q.  One case per
    transition: the pivot form small wave (wave32, or wave2 in a batch) -> wave64, wave64 -> LDS, LDS -> blocks, the J*Q1 form
    fused -> rows, the passenger rule alone (the second attempt gains a narrow last panel and keeps its pivot form), and a
    control whose two attempts run the same kernels.
    t + max(RAGGED_EXTRA) stays within the reflector count of the row kernels, so that the J*Q1 predicates of a launch planned for
    t_max and of expected_route at t agree."""
    def has(r, prefix):
        return any(b.startswith(prefix) for b in r)

    small = ("pivot_wave32", "pivot_wave2")
    wants = {
        "wave_to_wave64": lambda a, b: any(x in a for x in small) and "pivot_wave64" in b,
        "wave64_to_lds": lambda a, b: "pivot_wave64" in a and has(b, "pivot_lds") and "pivot_blocks" not in b,
        "lds_to_blocks": lambda a, b: has(a, "pivot_lds") and "pivot_blocks" not in a and "pivot_blocks" in b,
        "fused_to_rows": lambda a, b: "jq1_fused_small" in a and "jq1_rows32" in b,
        "passenger": lambda a, b: "sweep_passenger" not in a and "sweep_passenger" in b and pivot_bits(a) == pivot_bits(b),
        "same_kernels": lambda a, b: a == b,        # the control: a second attempt that crosses nothing
    }
    found = {}
    for n in (24, 32, 40, 48, 64, 70, 72, 96, 100, 128):
        for m in (20, n + 40, 2 * n + 40):
            for t in (8, 12, 14):
                if t > n - 2 or t + max(RAGGED_EXTRA) > dg.Q1R_MAXK:
                    continue
                for q in (4, 7, t // 2, t - 1):
                    # the J side of the second attempt is that of a launch with t - q independent constraints
                    a, b = j_bits(dg.expected_route(batch, m, n, t)), j_bits(dg.expected_route(batch, m, n, t - q))
                    for name, pred in wants.items():
                        if name not in found and pred(a, b):
                            found[name] = dict(id=f"second-{name}-b{batch}-{m}x{n}-t{t}-q{q}", name=name, m=m, n=n, t=t, q=q,
                                               batch=batch, seed=_seed("second", n, t, q), first=a, second=b)
    missing = set(wants) - set(found)
    assert not missing, missing
    return tuple(found[k] for k in wants)


def build_second(c, deficient=True):
    """(J, rx, A, cx) of a second-attempt case; deficient = False: the same seeds with full-rank Gaussian rows in place of the
    q combinations (the batch partner of the bitwise test)."""
    J, rx, A0, cx0 = synth.make_problem(c["seed"], c["m"], c["n"], c["t"])
    if not deficient:
        return J, rx, A0, cx0
    A, cx, _ = dependent(c["seed"], c["n"], c["t"], c["q"], True)
    return J, rx, A, cx
