"""The dimension choice of the subspace-minimisation branch on the CPU: enlsip_gn_determine_solving_dim (the host instantiation of
enlsip.jl_amd/csrc/gn_subspace_choice.hpp, the routine the batched kernels run) against oracle.enlsip_outer.determine_solving_dim
(src/enlsip_functions.jl:1041-1113).

Decisions are thresholds, so a case counts only where the reference's own choice does not sit on one: it must be unchanged under
four relative perturbations of 1e-10 of y and diag(R).  Every case that passes that filter must match exactly."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import enlsip_outer as eo

NCASES = 4000


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import enlsip_gn._lib as L
    return L.load()


def make_case(i, rng):
    rankR = int(rng.integers(1, 70))
    grade = np.linspace(0.0, 1.0, rankR) if rankR > 1 else np.zeros(1)
    diag = 10.0 ** (-rng.uniform(0, 8) * grade) * rng.choice([-1.0, 1.0], rankR) * rng.uniform(0.5, 1.5, rankR)
    y = rng.standard_normal(rankR) * 10.0 ** (-rng.uniform(0, 4) * grade)
    mode = i % 4
    if mode == 0:
        prev = rankR
    elif mode == 2:
        prev = int(rng.integers(-1, 1))
    else:
        prev = int(rng.integers(1, rankR + 1))
    restart = i % 11 == 0
    alpha = (0.05, 0.5, 1.0)[i % 3]
    progress = rng.uniform(-0.1, 1.0) * float(y @ y) * (0.05 if i % 5 == 0 else 1.0)
    return prev, rankR, progress, diag, y, alpha, restart


def reference(prev, rankR, progress, diag, y, alpha, restart):
    nrm = float(np.linalg.norm(y))
    nrm_prev = float(np.linalg.norm(y[:max(prev, 0)]))
    return eo.determine_solving_dim(prev, rankR, nrm, progress, nrm_prev, np.diag(diag), y, alpha, restart)[0]


def library(prev, rankR, progress, diag, y, alpha, restart):
    from enlsip_gn import determine_solving_dim
    nrm = float(np.linalg.norm(y))
    nrm_prev = float(np.linalg.norm(y[:max(prev, 0)]))
    return determine_solving_dim(prev, rankR, nrm, progress, nrm_prev, diag, y, alpha, restart)


def test_matches_the_reference_on_4000_cases(lib, monkeypatch):
    reached = {"gn": 0, "sub": 0, "bad": 0, "not_bad": 0}
    gn_ref, sub_ref = eo.gn_previous_step, eo.subspace_min_previous_step

    def gn(*a):
        reached["gn"] += 1
        return gn_ref(*a)

    def sub(tau, rho, rho_prk, c1, pseudo_rk, previous_dimR, progress, plp, ppd, previous_alpha):
        reached["sub"] += 1
        bad = previous_alpha < 0.2 and progress <= 0.3 * plp ** 2 and progress <= 0.1 * ppd ** 2       # :879-881
        reached["bad" if bad else "not_bad"] += 1
        return sub_ref(tau, rho, rho_prk, c1, pseudo_rk, previous_dimR, progress, plp, ppd, previous_alpha)

    rng = np.random.default_rng(20261017)
    prng = np.random.default_rng(7)
    cases = [make_case(i, rng) for i in range(NCASES)]
    kept, full, truncated = [], 0, 0
    for case in cases:
        prev, rankR, progress, diag, y, alpha, restart = case
        want = reference(*case)
        stable = True
        for _ in range(4):
            y2 = y * (1.0 + 1e-10 * prng.uniform(-1, 1, rankR))
            d2 = diag * (1.0 + 1e-10 * prng.uniform(-1, 1, rankR))
            stable = stable and reference(prev, rankR, progress, d2, y2, alpha, restart) == want
        if stable:
            kept.append((case, want))
            full += want == rankR
            truncated += want < rankR
    # the branch census is taken on the unperturbed cases only
    monkeypatch.setattr(eo, "gn_previous_step", gn)
    monkeypatch.setattr(eo, "subspace_min_previous_step", sub)
    for case in cases:
        reference(*case)
    monkeypatch.undo()
    print(f"kept {len(kept)} of {NCASES}: {full} full-rank, {truncated} truncated choices; branches {reached}")
    assert len(kept) >= 0.99 * NCASES, len(kept)
    assert full > 0 and truncated > 0
    assert reached["gn"] > 0 and reached["sub"] > 0 and reached["bad"] > 0 and reached["not_bad"] > 0, reached
    wrong = [(case[:3], case[5:], want, library(*case)) for case, want in kept if library(*case) != want]
    assert not wrong, (len(wrong), wrong[:5])


@pytest.mark.parametrize("extra", [1, 3])
@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_previous_dimension_beyond_the_rank(lib, extra, alpha):
    """previous_dimR > rankR outside a restart: the reference indexes rho past its end (Julia throws, the Python restatement
    raises IndexError); the library reports 5 before the read.  In a restart nothing is read: min(rankR, previous_dimR)."""
    from enlsip_gn import determine_solving_dim
    rng = np.random.default_rng(3)
    for rankR in (1, 2, 7, 40):
        diag = rng.uniform(0.5, 1.5, rankR)
        y = rng.standard_normal(rankR)
        prev = rankR + extra
        nrm = float(np.linalg.norm(y))
        with pytest.raises(IndexError):
            eo.determine_solving_dim(prev, rankR, nrm, 0.5 * nrm ** 2, nrm, np.diag(diag), y, alpha, False)
        nd = C.c_int64(-7)
        rc = lib.enlsip_gn_determine_solving_dim(prev, rankR, nrm, 0.5 * nrm ** 2, nrm, diag.ctypes.data_as(C.c_void_p),
                                                 y.ctypes.data_as(C.c_void_p), alpha, 0, C.byref(nd))
        assert rc == 5 and nd.value == -7
        with pytest.raises(IndexError):
            determine_solving_dim(prev, rankR, nrm, 0.5 * nrm ** 2, nrm, diag, y, alpha, False)
        rc = lib.enlsip_gn_determine_solving_dim(prev, rankR, nrm, 0.5 * nrm ** 2, nrm, diag.ctypes.data_as(C.c_void_p),
                                                 y.ctypes.data_as(C.c_void_p), alpha, 1, C.byref(nd))
        assert rc == 0 and nd.value == min(rankR, prev)
        if extra == 1:      # further out the reference's eta (:1105-1107, discarded by its caller, not computed here) reads l_estim_sd[k]
            assert eo.determine_solving_dim(prev, rankR, nrm, 0.5 * nrm ** 2, nrm, np.diag(diag), y, alpha, True)[0] == nd.value


def test_short_step_one_beyond_the_rank_follows_the_reference(lib):
    """previous_dimR == rankR + 1 after a step shorter than 0.2 is the one case where the bad-step test decides whether the
    reference runs out of bounds: with it true, rho[rankR] is read (in bounds) and rankR returned; with it false the reference
    raises and the library reports 5."""
    rankR = 5
    diag = np.array([3.0, -2.0, 1.5, 1.0, 0.8])
    y = np.array([1.0, -0.5, 0.25, 0.3, -0.2])
    nrm = float(np.linalg.norm(y))
    bad = library(rankR + 1, rankR, -1.0, diag, y, 0.05, False)
    assert bad == reference(rankR + 1, rankR, -1.0, diag, y, 0.05, False) == rankR
    with pytest.raises(IndexError):
        reference(rankR + 1, rankR, 10.0 * nrm ** 2, diag, y, 0.05, False)
    with pytest.raises(IndexError):
        library(rankR + 1, rankR, 10.0 * nrm ** 2, diag, y, 0.05, False)


def test_rank_zero_and_argument_errors(lib):
    nd = C.c_int64(-7)
    for restart in (0, 1):
        assert lib.enlsip_gn_determine_solving_dim(3, 0, 1.0, 0.1, 1.0, None, None, 0.5, restart, C.byref(nd)) == 0
        assert nd.value == 0
        assert eo.determine_solving_dim(3, 0, 1.0, 0.1, 1.0, np.zeros((0, 0)), np.zeros(0), 0.5, bool(restart))[0] == 0
    one = np.ones(1)
    p = one.ctypes.data_as(C.c_void_p)
    assert lib.enlsip_gn_determine_solving_dim(1, 1, 1.0, 0.1, 1.0, p, p, 0.5, 0, None) < 0
    assert lib.enlsip_gn_determine_solving_dim(1, -1, 1.0, 0.1, 1.0, p, p, 0.5, 0, C.byref(nd)) < 0
    assert lib.enlsip_gn_determine_solving_dim(1, 1, 1.0, 0.1, 1.0, None, p, 0.5, 0, C.byref(nd)) < 0
    assert lib.enlsip_gn_determine_solving_dim(1, 1, 1.0, 0.1, 1.0, p, None, 0.5, 0, C.byref(nd)) < 0


def test_choice_does_not_depend_on_the_scale_of_its_data(lib):
    """y and diag(R) of a problem far from 1 (the rescue route's): sqrt(dsum) |R[i,i]| of :1081 would overflow, the library scales
    both by exact powers of two and picks what the reference picks on the data near 1"""
    rng = np.random.default_rng(11)
    for i in range(40):
        prev, rankR, _, diag, y, _, _ = make_case(4 * i + 1, rng)
        want = reference(prev, rankR, 0.0, diag, y, 0.5, False)
        for sy, sr in ((2.0 ** 600, 2.0 ** 600), (2.0 ** -600, 2.0 ** -500), (2.0 ** 600, 1.0)):
            assert library(prev, rankR, 0.0, diag * sr, y * sy, 0.5, False) == want


def test_python_mirror_of_the_abi(lib):
    import enlsip_gn._lib as L
    from enlsip_gn import GNSolver
    assert C.sizeof(L.SubspacePrev) == 48
    assert [f for f, _ in L.SubspacePrev._fields_] == ["previous_dimA", "previous_dimJ2", "restart", "previous_alpha",
                                                      "constraint_progress", "residual_progress"]
    assert GNSolver.PREV_DTYPE.itemsize == 48
    assert [GNSolver.PREV_DTYPE.fields[f][1] for f, _ in L.SubspacePrev._fields_] == [getattr(L.SubspacePrev, f).offset
                                                                                     for f, _ in L.SubspacePrev._fields_]
    for name, nargs in (("enlsip_gn_determine_solving_dim", 10), ("enlsip_gn_subspace_direction_batched", 10),
                        ("enlsip_gn_subspace_direction_batched_dev", 10), ("enlsip_gn_get_subspace_form", 2)):
        res, args = L.PROTOTYPES[name]
        assert res is C.c_int and len(args) == nargs, name
        assert hasattr(lib, name)
    pv = GNSolver.pack_subspace_prev(3, [1, 2, 3], 4, 0, 0.5, [0.1, 0.2, 0.3], -1.0)
    assert pv.shape == (3,) and pv.tobytes()[:8] == (1).to_bytes(8, "little") and pv["previous_dimJ2"].tolist() == [4, 4, 4]
    with pytest.raises(ValueError):
        GNSolver.pack_subspace_prev(3, [1, 2], 4, 0, 0.5, 0.1, -1.0)
    assert math.isclose(float(pv["constraint_progress"][2]), 0.3)
