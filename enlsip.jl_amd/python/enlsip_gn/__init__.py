"""enlsip_gn — host mirror of Enlsip.jl's Gauss-Newton subproblem interface over libenlsip_gn.so."""
from .api import GNSolver, GNResult, GNError, FactorView, SQRT_EPS, determine_solving_dim, check_constraint_deletion  # noqa: F401
from .api import upper_bound_steplength, penalty_weight_update  # noqa: F401
from .api import evaluate_violated_constraints, gather_active_constraints  # noqa: F401
from .api import linesearch_coefficients, linesearch_fit, minrn, check_reduction  # noqa: F401
from ._lib import FACTOR_A, FACTOR_L11, FACTOR_J2, FLAG_UPDATE_MFMA, FLAG_UPDATE_REFLECTORS, LIB_PATH, DIM_HOLD  # noqa: F401
from .termination import minmax_lagrangian_mult, check_termination_criteria, termination_sums  # noqa: F401
from .direction import check_gn_direction, direction_sums  # noqa: F401
