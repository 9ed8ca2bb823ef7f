"""The host rebuild enlsip_gn_gather_active_constraints (csrc/gn_violated_constraints.hpp, the routine the batched kernels run):
active_C.A = A[active, :], active_C.cx = cx[active] (src/enlsip_functions.jl:2854-2855) and evaluate_scaling!
(src/structures.jl:160-178), written as the n x t column-major A' block.  The gather is exact against NumPy indexing; the norms
and the scaled values are compared with np.longdouble (64-bit significand) within (n + 4) * 2^-53 relative: n rounded products
and n rounded additions in the sum of squares (2n * 2^-53, halved by the square root), the square root itself, and at most two
divisions (1 / row_i or x / row_i); the reference's own error, about n * 2^-64, is far below.  No GPU."""
import ctypes as C

import numpy as np
import pytest

U = 2.0 ** -53
SHAPES = [(1, 1), (3, 2), (5, 7), (64, 9), (65, 9), (130, 70), (257, 5)]      # (n, l)


def reference(rows, cxa, scaling):
    """(At rows, cx, diag_scale) in long double"""
    R = rows.astype(np.longdouble)
    nrm = np.sqrt((R * R).sum(axis=1))
    if not scaling:
        return R, cxa.astype(np.longdouble), nrm
    div = np.where(nrm < np.finfo(np.float64).eps, np.longdouble(1.0), nrm)
    return R / div[:, None], cxa.astype(np.longdouble) / div, 1.0 / div


def close(got, want, n, tag):
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    err = np.abs(got - want)
    assert np.all(err <= (n + 4) * U * np.abs(want)), (tag, float(np.max(err / np.maximum(np.abs(want), np.finfo(np.longdouble).tiny))))


def case(n, l, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((l, n)) * scale
    cx = rng.standard_normal(l)
    t = int(rng.integers(1, l + 1))
    active = np.zeros(l, dtype=np.int64)
    active[:t] = np.sort(rng.choice(np.arange(1, l + 1), size=t, replace=False))
    return A, cx, t, active


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("n,l", SHAPES)
def test_gather_and_scaling(n, l, scaling):
    from enlsip_gn import gather_active_constraints
    A, cx, t, active = case(n, l, 100 * n + l)
    At, ca, ds = gather_active_constraints(active, t, A, cx, scaling)
    rows = A[active[:t] - 1, :]
    if not scaling:      # copies
        assert At.tobytes() == np.ascontiguousarray(rows).tobytes() and ca.tobytes() == cx[active[:t] - 1].tobytes()
    wAt, wcx, wds = reference(rows, cx[active[:t] - 1], scaling)
    close(At, wAt, n, "At")
    close(ca, wcx, n, "cx")
    close(ds, wds, n, "diag_scale")


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "scaled"])
def test_zero_row_and_tiny_row(scaling):
    from enlsip_gn import gather_active_constraints
    n, l = 6, 4
    A = np.arange(1.0, l * n + 1).reshape(l, n)
    A[1, :] = 0.0
    A[2, :] = 1e-20      # norm below eps: the divisor is 1.0 under scaling
    cx = np.array([1.0, 2.0, 3.0, 4.0])
    active = np.array([1, 2, 3, 0])
    At, ca, ds = gather_active_constraints(active, 3, A, cx, scaling)
    if scaling:
        assert ds[1] == 1.0 and ds[2] == 1.0
        assert At[1].tobytes() == A[1].tobytes() and At[2].tobytes() == A[2].tobytes() and ca[1] == 2.0 and ca[2] == 3.0
        assert ds[0] == 1.0 / (1.0 / ds[0]) and abs(ds[0] * np.linalg.norm(A[0]) - 1.0) < 1e-14
    else:
        assert ds[1] == 0.0 and abs(ds[2] - 1e-20 * np.sqrt(6.0)) <= 10 * U * ds[2]
        assert At.tobytes() == A[:3].tobytes() and ca.tobytes() == cx[:3].tobytes()


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("e", [400, -400])
def test_rows_at_the_edges_of_the_magnitude_band(e, scaling):
    from enlsip_gn import gather_active_constraints
    n, l = 70, 5
    A, cx, t, active = case(n, l, 407 + e, scale=2.0 ** e)
    At, ca, ds = gather_active_constraints(active, t, A, cx, scaling)
    rows = A[active[:t] - 1, :]
    wAt, wcx, wds = reference(rows, cx[active[:t] - 1], scaling)
    assert np.isfinite(ds).all() and (ds > 0).all()
    close(At, wAt, n, "At")
    close(ca, wcx, n, "cx")
    close(ds, wds, n, "diag_scale")


def test_the_order_of_the_sum_is_the_documented_one():
    """64 strided partials in ascending j, then the butterfly x[s] += x[s ^ mask] for mask = 1, 2, 7, 15, 16, 32, one square root"""
    from enlsip_gn import gather_active_constraints
    for n in (1, 5, 64, 65, 200):
        rng = np.random.default_rng(n)
        A = rng.standard_normal((1, n)) * np.exp(rng.uniform(-8, 8, (1, n)))
        x = np.zeros(64)
        for j in range(n):
            x[j % 64] = x[j % 64] + A[0, j] * A[0, j]
        for mask in (1, 2, 7, 15, 16, 32):
            x = x + x[np.arange(64) ^ mask]
        assert len({v.tobytes() for v in x}) == 1
        _, _, ds = gather_active_constraints([1], 1, A, [0.0], False)
        assert ds[0].tobytes() == np.sqrt(x[0]).tobytes(), n


def test_no_constraint_and_padded_columns():
    from enlsip_gn import gather_active_constraints
    n, l = 5, 6
    A, cx, t, active = case(n, l, 3)
    At, ca, ds = gather_active_constraints(active, 0, A, cx, True)
    assert At.shape == (0, n) and ca.size == 0 and ds.size == 0
    ldat = n + 3
    for scaling in (False, True):
        out = (np.full((t, ldat), np.nan), np.full(t, np.nan), np.full(t, np.nan))
        At, ca, ds = gather_active_constraints(active, t, A, cx, scaling, ldat=ldat, out=out)
        assert np.isnan(At[:, n:]).all() and np.isfinite(At[:, :n]).all()      # nothing between rows n and ldat is written
        tight = gather_active_constraints(active, t, A, cx, scaling)
        assert At[:, :n].tobytes() == tight[0].tobytes() and ca.tobytes() == tight[1].tobytes() and ds.tobytes() == tight[2].tobytes()


def test_error_codes():
    import enlsip_gn._lib as L
    lib = L.load()
    n, l, t = 3, 4, 2
    A = np.asfortranarray(np.ones((l, n)))
    cx, act = np.ones(l), np.array([1, 3, 0, 0], dtype=np.int64)
    At, ca, ds = np.full((t, n), np.nan), np.full(t, np.nan), np.full(t, np.nan)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(l=l, n=n, t=t, act=act, A=A, lda=l, cx=cx, At=At, ldat=n, ca=ca, ds=ds):
        return lib.enlsip_gn_gather_active_constraints(l, n, t, p(act), p(A), lda, p(cx), 1, p(At), ldat, p(ca), p(ds))

    for kw in (dict(l=-1), dict(n=0), dict(t=-1), dict(t=5), dict(lda=3), dict(ldat=2)):
        assert call(**kw) == -2, kw
    for kw in (dict(act=None), dict(A=None), dict(cx=None), dict(At=None), dict(ca=None), dict(ds=None)):
        assert call(**kw) == -4, kw
    for bad in (5, -1):
        assert call(act=np.array([1, bad, 0, 0], dtype=np.int64)) == -5
    assert np.isnan(At).all() and np.isnan(ca).all() and np.isnan(ds).all()
    assert call() == 0 and np.isfinite(At).all()
