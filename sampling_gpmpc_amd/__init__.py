"""MI355X-native GP-posterior-sample rollout for sampling-based GP-MPC (drop-in for the hot path of
manish-pra/sampling-gpmpc: ``src/agent.py`` + ``src/GP_model.py`` + the forward-sampling harnesses)."""
from ._host_threads import limit_host_threads
limit_host_threads()        # pools larger than the cgroup's CPU quota freeze the launching thread (see _host_threads.py)
from .agent import Agent, random_vector_within_bounds                   # noqa: F401
from .environments import make_env, Pendulum, CarKinematicsModel        # noqa: F401
from .reachable_set import get_reachable_set_ball                       # noqa: F401
from . import _lib                                                      # noqa: F401
from .hulls import (HullSet, HullAccumulator, convex_hulls, merge_hulls, hull_area_ratio,  # noqa: F401
                    HullQuery, hull_query, tube_coverage)
from .small_ball import (SmallBall, reference_grid, posterior_on_grid, sup_deviation, small_ball_probability,  # noqa: F401
                         sup_deviation_quantile, required_samples)
from .mle import (MarginalLikelihood, FitResult, marginal_likelihood, pack_theta, unpack_theta, theta_from_params,  # noqa: F401
                  theta_to_params, fit_hyperparameters, restarts, rkhs_norm_and_beta)
from .moments import (MomentTube, chance_constraint_penalty, moment_rollout, moment_rollout_plan, moment_rollout_vjp,    # noqa: F401
                      moment_rollout_vjp_plan, plan_inputs, plan_inputs_plan)
from .tube_qp import TubeQP, TubeQPResult, tube_gram, tube_apply, tube_cost, solve_tube_qp  # noqa: F401
# the wrapper tube_rows.tube_rows is not re-exported: the name is the module's
from .tube_rows import TubeRows, TubeRowsResult, TubeCheck, ocp_rows, check_tube  # noqa: F401
from .closed_loop import ClosedLoop, SurrogateSolver, CondensedSolver  # noqa: F401
from .pathwise import (PathwiseSamples, draw_omega, rff_kernel_error, TubeStats, pathwise_tube_stats, merge_tube_stats,  # noqa: F401
                       tube_stats_of, pathwise_rollout_vjp, sampled_tube_penalty, plan_inputs_sampled, pathwise_rollout_cand_vjp,
                       plan_inputs_sampled_population)
from .weight_space import WeightSpaceSamples, learn_online  # noqa: F401
from .robust_tube import (RobustTube, robust_tube_rollout, robust_tube_rollout_plan, pairwise_lipschitz, estimate_lipschitz,  # noqa: F401
                          robust_tube_rollout_vjp, robust_tube_rollout_vjp_plan, plan_inputs_robust, plan_inputs_robust_plan)
from .optimistic import (OptimisticTube, optimistic_rollout, optimistic_rollout_plan, optimistic_rollout_vjp,  # noqa: F401
                         optimistic_rollout_vjp_plan, plan_inputs_optimistic, plan_inputs_optimistic_plan)
from .reconditioned import reconditioned_rollout, reconditioned_rollout_vjp, plan_inputs_reconditioned  # noqa: F401
from .terminal_set import (ContractionCheck, TerminalSet, contraction_rates, sample_terminal_jacobians, fit_terminal_set,  # noqa: F401
                           terminal_to_params)

__all__ = ["Agent", "make_env", "Pendulum", "CarKinematicsModel", "get_reachable_set_ball",
           "random_vector_within_bounds", "HullSet", "HullAccumulator", "convex_hulls", "merge_hulls", "hull_area_ratio",
           "HullQuery", "hull_query", "tube_coverage", "SmallBall", "reference_grid", "posterior_on_grid", "sup_deviation",
           "small_ball_probability", "sup_deviation_quantile", "required_samples", "MarginalLikelihood", "FitResult",
           "marginal_likelihood", "pack_theta", "unpack_theta", "theta_from_params", "theta_to_params", "fit_hyperparameters",
           "restarts", "rkhs_norm_and_beta", "MomentTube", "moment_rollout", "moment_rollout_plan", "moment_rollout_vjp", "moment_rollout_vjp_plan",
           "chance_constraint_penalty", "plan_inputs", "plan_inputs_plan", "TubeQP", "TubeQPResult",
           "tube_gram", "tube_apply", "tube_cost", "solve_tube_qp", "ClosedLoop", "SurrogateSolver", "CondensedSolver",
           "TubeRows", "TubeRowsResult", "TubeCheck", "ocp_rows", "check_tube", "PathwiseSamples", "draw_omega", "rff_kernel_error",
           "TubeStats", "pathwise_tube_stats", "merge_tube_stats", "tube_stats_of", "pathwise_rollout_vjp", "sampled_tube_penalty",
           "plan_inputs_sampled", "pathwise_rollout_cand_vjp", "plan_inputs_sampled_population", "RobustTube", "robust_tube_rollout", "robust_tube_rollout_plan", "robust_tube_rollout_vjp",
           "robust_tube_rollout_vjp_plan", "plan_inputs_robust", "plan_inputs_robust_plan", "pairwise_lipschitz",
           "estimate_lipschitz", "ContractionCheck", "TerminalSet", "contraction_rates", "sample_terminal_jacobians", "fit_terminal_set",
           "terminal_to_params", "OptimisticTube", "optimistic_rollout", "optimistic_rollout_plan", "optimistic_rollout_vjp",
           "optimistic_rollout_vjp_plan", "plan_inputs_optimistic", "plan_inputs_optimistic_plan", "reconditioned_rollout",
           "reconditioned_rollout_vjp", "plan_inputs_reconditioned", "WeightSpaceSamples", "learn_online"]
