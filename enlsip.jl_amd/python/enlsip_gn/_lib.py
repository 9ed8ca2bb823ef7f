"""ctypes binding of libenlsip_gn.so (include/enlsip_gn.h).

The product path is the HIP library: if it is missing or cannot be loaded this module raises —
there is no CPU fallback (the CPU oracle under /oracle is test infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_PKG_ROOT = Path(__file__).resolve().parents[2]          # .../enlsip.jl_amd
LIB_PATH = Path(os.environ.get("ENLSIP_GN_LIB", _PKG_ROOT / "lib" / "libenlsip_gn.so"))

FACTOR_A, FACTOR_L11, FACTOR_J2 = 0, 1, 2
FLAG_UPDATE_MFMA, FLAG_UPDATE_REFLECTORS = 1, 2
DIM_HOLD = -2            # ENLSIP_GN_DIM_HOLD: the held forms of resolve_batched
STAGE_NAMES = ("constraint", "jq1", "panel", "update", "pivot", "total")


class Opts(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_int32), ("panel_width", C.c_int32),
                ("tile_rows", C.c_int32), ("stream", C.c_void_p)]


class Info(C.Structure):
    _fields_ = [("rankA", C.c_int64), ("rankJ2", C.c_int64), ("code", C.c_int64),
                ("dimA", C.c_int64), ("dimJ2", C.c_int64), ("status", C.c_int64)]


class SubspacePrev(C.Structure):
    """enlsip_gn_subspace_prev: what choose_subspace_dimensions (src/enlsip_functions.jl:1118-1176) reads of previous_iter"""
    _fields_ = [("previous_dimA", C.c_int64), ("previous_dimJ2", C.c_int64), ("restart", C.c_int64),
                ("previous_alpha", C.c_double), ("constraint_progress", C.c_double), ("residual_progress", C.c_double)]


class TermState(C.Structure):
    """enlsip_gn_term_state: what check_termination_criteria (src/enlsip_functions.jl:2399-2517) reads of one problem's host records"""
    _fields_ = [("restart", C.c_int64), ("code", C.c_int64), ("del", C.c_int64), ("grad_res", C.c_double),
                ("nb_iter", C.c_int64), ("nb_newton_steps", C.c_int64), ("error_code", C.c_int64), ("psi_error", C.c_int64),
                ("delta_time", C.c_double), ("q", C.c_int64), ("t", C.c_int64), ("l", C.c_int64), ("dimJ2", C.c_int64),
                ("psi0", C.c_double)]


class TermTol(C.Structure):
    """enlsip_gn_term_tol: max_iter and the four tolerances of one call"""
    _fields_ = [("max_iter", C.c_int64), ("eps_abs", C.c_double), ("eps_rel", C.c_double), ("eps_x", C.c_double),
                ("eps_c", C.c_double)]


class TermSums(C.Structure):
    """enlsip_gn_term_sums: the scalars the device forms per problem"""
    _fields_ = [("rx_sum", C.c_double), ("grad_nrm", C.c_double), ("p_nrm", C.c_double), ("active_cx_nrm", C.c_double),
                ("n_inactive_nonpos", C.c_int64), ("n_inactive_le0", C.c_int64), ("sigma_min", C.c_double),
                ("lambda_abs_max", C.c_double), ("d1_sq", C.c_double), ("x_diff", C.c_double), ("x_nrm", C.c_double),
                ("Atcx_nrm", C.c_double), ("active_penalty_sum", C.c_double), ("whsum", C.c_double), ("progress", C.c_double)]


class DirState(C.Structure):
    """enlsip_gn_dir_state: what check_gn_direction (src/enlsip_functions.jl:943-1030) and the norms of :1222-1231 read of one
    problem's host records"""
    _fields_ = [("iter_number", C.c_int64), ("restart", C.c_int64), ("add", C.c_int64), ("del", C.c_int64), ("q", C.c_int64),
                ("t", C.c_int64), ("l", C.c_int64), ("rankA", C.c_int64), ("dimA", C.c_int64), ("dimJ2", C.c_int64),
                ("prev_code", C.c_int64), ("prev_dimJ2", C.c_int64), ("prev_t", C.c_int64), ("prev_beta", C.c_double),
                ("prev_progress", C.c_double), ("prev_predicted_reduction", C.c_double), ("prev_alpha", C.c_double)]


class DirSums(C.Structure):
    """enlsip_gn_dir_sums: the scalars the device forms per problem"""
    _fields_ = [("b1_sq", C.c_double), ("d_sq", C.c_double), ("d1_sq", C.c_double), ("d1_asprev_sq", C.c_double),
                ("active_c_sum", C.c_double), ("n_lm_ge", C.c_int64), ("n_lm_neg", C.c_int64), ("n_inactive_lt_delta", C.c_int64)]


# enlsip_gn_allgather_fn: int (*)(void* ctx, const void* dsend, void* drecv, size_t bytes_per_rank, void* hip_stream)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)
_i64 = C.c_int64
_h = C.c_void_p

# name -> (restype, argtypes); every symbol include/enlsip_gn.h declares
PROTOTYPES = {
    "enlsip_gn_version": (C.c_int, []),
    "enlsip_gn_create": (C.c_int, [C.POINTER(_h), C.POINTER(Opts)]),
    "enlsip_gn_destroy": (C.c_int, [_h]),
    "enlsip_gn_last_error": (C.c_char_p, [_h]),
    "enlsip_gn_synchronize": (C.c_int, [_h]),
    "enlsip_gn_solve": (C.c_int, [_h, _i64, _i64, _i64, C.c_void_p, _i64, C.c_void_p, C.c_void_p, _i64,
                                  C.c_void_p, C.c_double, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(Info), C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_factor_constraints": (C.c_int, [_h, _i64, _i64, _i64, C.c_void_p, _i64, C.c_void_p, C.c_double,
                                               C.POINTER(Info)]),
    "enlsip_gn_solve_factored": (C.c_int, [_h, _i64, _i64, _i64, C.c_void_p, _i64, C.c_void_p, C.c_double, _i64,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Info), C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "enlsip_gn_solve_batched": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, _i64, _i64, C.c_void_p,
                                          C.c_void_p, _i64, _i64, C.c_void_p, C.c_double, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "enlsip_gn_solve_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, _i64, _i64, C.c_void_p,
                                              C.c_void_p, _i64, _i64, C.c_void_p, C.c_double, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "enlsip_gn_solve_batched_ragged": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, _i64, _i64,
                                                 C.c_void_p, C.c_void_p, _i64, _i64, C.c_void_p, C.c_double, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]),
    "enlsip_gn_solve_batched_ragged_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, _i64, _i64,
                                                     C.c_void_p, C.c_void_p, _i64, _i64, C.c_void_p, C.c_double,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]),
    "enlsip_gn_factor_constraints_batched": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, _i64, _i64, C.c_void_p,
                                                       C.c_double, C.c_void_p]),
    "enlsip_gn_factor_constraints_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, _i64, _i64,
                                                           C.c_void_p, C.c_double, C.c_void_p]),
    "enlsip_gn_solve_factored_batched": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, _i64, _i64,
                                                   C.c_void_p, C.c_void_p, _i64, _i64, C.c_void_p, C.c_double, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_solve_factored_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, _i64, _i64,
                                                       C.c_void_p, C.c_void_p, _i64, _i64, C.c_void_p, C.c_double, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_get_constraint_refactored": (C.c_int, [_h, _ip]),
    "enlsip_gn_solve_changed_batched": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, _i64, _i64,
                                                  C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_solve_changed_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, _i64, _i64,
                                                      C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_get_jacobian_resolved": (C.c_int, [_h, _ip]),
    "enlsip_gn_factor_shape": (C.c_int, [_h, C.c_int, _i64, _ip, _ip]),
    "enlsip_gn_get_R": (C.c_int, [_h, C.c_int, _i64, C.c_void_p, _i64]),
    "enlsip_gn_get_diagR": (C.c_int, [_h, C.c_int, _i64, C.c_void_p]),
    "enlsip_gn_get_jpvt": (C.c_int, [_h, C.c_int, _i64, C.c_void_p]),
    "enlsip_gn_apply_qt": (C.c_int, [_h, C.c_int, _i64, C.c_void_p]),
    "enlsip_gn_apply_q": (C.c_int, [_h, C.c_int, _i64, C.c_void_p]),
    "enlsip_gn_get_JQ1": (C.c_int, [_h, _i64, C.c_void_p, _i64]),
    "enlsip_gn_resolve": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_gradient": (C.c_int, [_h, _i64, C.c_void_p]),
    "enlsip_gn_jacobian_times": (C.c_int, [_h, _i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_first_lagrange": (C.c_int, [_h, _i64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                           C.POINTER(C.c_double)]),
    "enlsip_gn_second_lagrange": (C.c_int, [_h, _i64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    "enlsip_gn_gradient_batched": (C.c_int, [_h, _i64, _i64, C.c_void_p]),
    "enlsip_gn_gradient_batched_dev": (C.c_int, [_h, _i64, _i64, C.c_void_p]),
    "enlsip_gn_jacobian_times_batched": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_jacobian_times_batched_dev": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_first_lagrange_batched": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                                   C.c_void_p, C.c_void_p]),
    "enlsip_gn_first_lagrange_batched_dev": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                                       C.c_void_p, C.c_void_p]),
    "enlsip_gn_second_lagrange_batched": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                                    C.c_void_p]),
    "enlsip_gn_second_lagrange_batched_dev": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                                        C.c_void_p]),
    "enlsip_gn_get_consumer_form": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "enlsip_gn_resolve_batched": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_resolve_batched_dev": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_get_diagR_batched": (C.c_int, [_h, C.c_int, _i64, _i64, C.c_void_p, _i64]),
    "enlsip_gn_get_resolve_form": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "enlsip_gn_get_resolve_q0_ms": (C.c_int, [_h, C.POINTER(C.c_float)]),
    "enlsip_gn_determine_solving_dim": (C.c_int, [_i64, _i64, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_double,
                                                  _i64, _ip]),
    "enlsip_gn_subspace_direction_batched": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p]),
    "enlsip_gn_subspace_direction_batched_dev": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_get_subspace_form": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "enlsip_gn_check_constraint_deletion": (C.c_int, [_i64, _i64, C.c_void_p, C.c_void_p, C.c_int, C.c_double, _ip]),
    "enlsip_gn_delete_constraints_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _i64, _i64, C.c_void_p,
                                                           C.c_void_p, C.c_void_p]),
    "enlsip_gn_restore_constraints_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.c_void_p, _i64, _i64, C.c_void_p, C.c_void_p]),
    "enlsip_gn_get_deletion_form": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "enlsip_gn_upper_bound_steplength": (C.c_int, [_i64, _i64, C.c_void_p, _i64, C.c_void_p, C.c_void_p, _dp, _ip]),
    "enlsip_gn_linesearch_setup_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, _i64, _i64, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_get_linesearch_form": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "enlsip_gn_penalty_weight_update": (C.c_int, [_i64, _i64, C.c_void_p, _i64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(C.c_int)]),
    "enlsip_gn_penalty_weights_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_get_penalty_form": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "enlsip_gn_merit_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_linesearch_coefficients": (C.c_int, [_i64, _i64, _i64, C.c_void_p, C.c_void_p, _i64, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                                    C.c_void_p]),
    "enlsip_gn_linesearch_fit": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                           C.POINTER(C.c_int)]),
    "enlsip_gn_minrn": (C.c_int, [C.c_double] * 9 + [_dp, _dp]),
    "enlsip_gn_check_reduction": (C.c_int, [C.c_double] * 5 + [C.POINTER(C.c_int)]),
    "enlsip_gn_linesearch_fit_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64] + [C.c_void_p] * 20),
    "enlsip_gn_evaluate_violated_constraints": (C.c_int, [_i64, _i64, _i64, _ip, C.c_void_p, C.c_void_p, C.c_void_p, _i64, _ip, _ip]),
    "enlsip_gn_gather_active_constraints": (C.c_int, [_i64, _i64, _i64, C.c_void_p, C.c_void_p, _i64, C.c_void_p, C.c_int,
                                                      C.c_void_p, _i64, C.c_void_p, C.c_void_p]),
    "enlsip_gn_add_constraints_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, _i64, _i64, C.c_void_p,
                                                        C.c_void_p, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_get_addition_form": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "enlsip_gn_minmax_lagrangian_mult": (C.c_int, [_i64, _i64, C.c_void_p, C.c_void_p, C.c_int, _dp, _dp]),
    "enlsip_gn_check_termination_criteria": (C.c_int, [C.POINTER(TermState), C.POINTER(TermSums), C.POINTER(TermTol), _ip]),
    "enlsip_gn_termination_sums": (C.c_int, [_i64, _i64, _i64, _i64, _i64, _i64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, _i64]
                                   + [C.c_void_p] * 10 + [_i64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.POINTER(TermSums)]),
    "enlsip_gn_termination_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64, _i64, C.c_void_p, C.POINTER(TermTol), C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, _i64, _i64] + [C.c_void_p] * 10
                                          + [_i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_get_termination_form": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "enlsip_gn_check_gn_direction": (C.c_int, [C.POINTER(DirState), C.POINTER(DirSums), _i64, _i64, _ip, _dp]),
    "enlsip_gn_direction_sums": (C.c_int, [_i64, _i64, _i64, C.POINTER(DirState)] + [C.c_void_p] * 7
                                 + [C.c_int, C.POINTER(DirSums), _ip]),
    "enlsip_gn_direction_check_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64, _i64] + [C.c_void_p] * 4 + [C.c_int]
                                              + [C.c_void_p] * 9),
    "enlsip_gn_get_direction_form": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "enlsip_gn_hessian_points": (C.c_int, [_i64, _i64, _i64, C.c_void_p, C.c_void_p]),
    "enlsip_gn_hessian_points_batched_dev": (C.c_int, [_h, _i64, _i64, _i64, _i64, C.c_void_p, C.c_void_p]),
    "enlsip_gn_hessian_sums": (C.c_int, [_i64] * 6 + [C.c_void_p] * 7 + [_i64]),
    "enlsip_gn_hessian_sums_batched_dev": (C.c_int, [_h] + [_i64] * 7 + [C.c_void_p] * 9 + [_i64, _i64]),
    "enlsip_gn_newton_direction": (C.c_int, [_h, _i64, C.c_void_p, _i64, C.c_void_p, _ip]),
    "enlsip_gn_newton_direction_batched": (C.c_int, [_h, _i64, _i64, C.c_void_p, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_newton_direction_batched_dev": (C.c_int, [_h, _i64, _i64, C.c_void_p, _i64, _i64, C.c_void_p, C.c_void_p,
                                                         C.c_void_p]),
    "enlsip_gn_get_newton_form": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "enlsip_gn_get_newton_stage_ms": (C.c_int, [_h, C.POINTER(C.c_float)]),
    "enlsip_gn_tsqr_local_dev": (C.c_int, [_h, _i64, _i64, _i64, C.c_void_p, _i64, C.c_void_p, C.c_void_p, _i64,
                                           C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, _dp, _ip]),
    "enlsip_gn_tsqr_combine_dev": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                             C.c_void_p, _dp, C.POINTER(Info), C.c_void_p]),
    "enlsip_gn_tsqr_local_scaled_dev": (C.c_int, [_h, _i64, _i64, _i64, C.c_void_p, _i64, C.c_void_p, C.c_void_p, _i64,
                                                  C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, _dp, _ip, _ip]),
    "enlsip_gn_tsqr_combine_scaled_dev": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                                    C.c_void_p, C.c_void_p, _dp, C.POINTER(Info), C.c_void_p]),
    "enlsip_gn_tsqr_get_scale": (C.c_int, [_h, _ip, _ip]),
    "enlsip_gn_tsqr_unique_id": (C.c_int, [C.c_void_p]),
    "enlsip_gn_tsqr_init_rccl": (C.c_int, [_h, C.c_void_p, C.c_int, C.c_int]),
    "enlsip_gn_tsqr_set_comm": (C.c_int, [_h, C.c_void_p, C.c_int, C.c_int]),
    "enlsip_gn_tsqr_set_exchange": (C.c_int, [_h, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "enlsip_gn_solve_tsqr": (C.c_int, [_h, _i64, _i64, _i64, C.c_void_p, _i64, C.c_void_p, C.c_void_p, _i64, C.c_void_p,
                                       C.c_double, C.c_void_p, C.c_void_p, _dp, C.POINTER(Info), C.c_void_p]),
    "enlsip_gn_tsqr_get_stage_ms": (C.c_int, [_h, C.POINTER(C.c_float)]),
    "enlsip_gn_tsqr_get_transport": (C.c_int, [_h, C.POINTER(C.c_int)]),
    "enlsip_gn_tsqr_get_exchange": (C.c_int, [_h, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "enlsip_gn_tsqr_products_msg_len": (_i64, [_i64]),
    "enlsip_gn_tsqr_products_local_dev": (C.c_int, [_h, _i64, _i64, C.c_void_p, _i64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]),
    "enlsip_gn_tsqr_products_combine_dev": (C.c_int, [_h, _i64, _i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_tsqr_products": (C.c_int, [_h, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "enlsip_gn_tsqr_first_lagrange": (C.c_int, [_h, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, _dp]),
    "enlsip_gn_tsqr_second_lagrange": (C.c_int, [_h, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    "enlsip_gn_tsqr_newton_direction": (C.c_int, [_h, C.c_void_p, _i64, C.c_void_p, C.POINTER(C.c_int64)]),
    "enlsip_gn_tsqr_newton_direction_dev": (C.c_int, [_h, C.c_void_p, _i64, C.c_void_p, C.c_void_p]),
    "enlsip_gn_set_profiling": (C.c_int, [_h, C.c_int]),
    "enlsip_gn_get_stage_ms": (C.c_int, [_h, C.POINTER(C.c_float)]),
    "enlsip_gn_get_update_stats": (C.c_int, [_h, C.POINTER(C.c_float), _ip, _dp]),
    "enlsip_gn_get_update_table": (C.c_int, [_h, C.c_int64, _dp, C.POINTER(C.c_float), _ip]),
    "enlsip_gn_get_launch_plan": (C.c_int, [_h, _ip, C.POINTER(C.c_int), _ip]),
    "enlsip_gn_get_update_totals": (C.c_int, [_h, C.POINTER(C.c_float), C.POINTER(C.c_float), _ip, _dp]),
    "enlsip_gn_measure_stream": (C.c_int, [_h, C.c_int64, C.c_int, _dp]),
    "enlsip_gn_debug_copy_W": (C.c_int, [_h, C.c_int64, _dp, _ip, C.c_int64]),
    "enlsip_gn_full_constraints_times": (C.c_int, [_h, _i64, _i64, C.c_void_p, _i64, C.c_void_p, C.c_void_p]),
    "enlsip_gn_matrix_times_QA": (C.c_int, [_h, _i64, _i64, C.c_void_p, _i64, C.c_void_p, _i64]),
    "enlsip_gn_get_route": (C.c_int, [_h, C.POINTER(C.c_uint64)]),
    "enlsip_gn_route_name": (C.c_char_p, [C.c_int]),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP library and bind every prototype.  Raises OSError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise OSError(f"{LIB_PATH} not found: build it with `python __graft_entry__.py` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
