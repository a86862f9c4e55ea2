"""lisp-mcmc_amd: MI355X-native drop-in for the walker-adaptive-steps path of afranson/Lisp-MCMC.

The package directory name carries a hyphen (it is the name the build contract fixes);
import it as `import lisp_mcmc_amd` (alias module at the repository root) or with
importlib.import_module("lisp-mcmc_amd").

  _capi    ctypes binding of libmhx.so (the C ABI of include/mhx.h)
  engine   Engine: batched chains, one engine per GPU
  walker   the reference's own names: walker_create, walker_adaptive_steps, walker_get, ...
  models   model designators that stand in for the reference's :function closures
"""
from . import _capi as capi  # noqa: F401
from ._capi import MhxError  # noqa: F401
from .engine import Engine, Group, band_count, loo_tail_length, comm_unique_id, partition, split_rhat, ensemble_pick, trace_rows, normeq_steps, hdi_span  # noqa: F401
from . import models  # noqa: F401
from . import sexpr  # noqa: F401
from . import distributed  # noqa: F401
from . import ingest  # noqa: F401
from .ingest import read_file_to_data, create_walker_data  # noqa: F401
from .saveload import walker_save, walker_load  # noqa: F401
from .walker import (  # noqa: F401
    Walker, WalkerStep, walker_create, walker_set_create, data_separated, planes_layout, mcmc_fit, walker_adaptive_steps,
    walker_adaptive_steps_full, walker_many_steps, walker_take_step, walker_get, walker_set_get,
    walker_modify, prior_bounds, log_prior_flat, request_stop, create_log_liklihood_function,
    walker_get_data_and_fit, walker_get_data_and_fit_no_stddev, walker_get_residuals,
    walker_set_get_data_and_fit, fit_linspace, walker_get_fit_credible, walker_set_get_fit_credible,
    walker_with_exp, walker_exp_get, walker_set_with_exp, walker_set_exp_get,
    make_histo, make_histo_x, histo_edges, walker_param_histo, walker_set_param_histo,
    walker_set_corner_grid,
    autocorr, walker_autocorr, walker_set_autocorr, walker_set_rhat, walker_set_ensemble_get,
    hdi, walker_set_hdi, walker_hdi, walker_set_quantiles,
    walker_set_waic, walker_waic, waic_compare, waic_merge,
    walker_set_loo, walker_loo, loo_compare,
    walker_set_score_data, walker_score_data, kfold_folds, walker_set_kfold_create, walker_set_kfold,
    walker_set_trace, walker_set_catepillar,
    walker_set_get_residuals, walker_set_goodness_of_fit, walker_goodness_of_fit, runs_z,
    walker_set_laplace, walker_laplace, laplace_summary, least_squares, walker_set_least_squares,
    candidate_grid, walker_set_search, walker_search, walker_set_chi2_map,
)

__all__ = ["capi", "MhxError", "Engine", "Group", "comm_unique_id", "partition", "models", "Walker", "WalkerStep", "walker_create",
           "walker_set_create", "data_separated", "planes_layout",
           "mcmc_fit", "walker_adaptive_steps", "walker_adaptive_steps_full",
           "walker_many_steps", "walker_take_step", "walker_get", "walker_set_get", "walker_modify",
           "prior_bounds", "log_prior_flat", "request_stop", "create_log_liklihood_function",
           "band_count", "walker_get_data_and_fit", "walker_get_data_and_fit_no_stddev",
           "walker_get_residuals", "walker_set_get_data_and_fit", "fit_linspace",
           "walker_get_fit_credible", "walker_set_get_fit_credible",
           "walker_with_exp", "walker_exp_get", "walker_set_with_exp", "walker_set_exp_get",
           "make_histo", "make_histo_x", "histo_edges", "walker_param_histo", "walker_set_param_histo",
           "walker_set_corner_grid",
           "autocorr", "walker_autocorr", "walker_set_autocorr", "walker_set_rhat", "split_rhat",
           "walker_set_ensemble_get", "ensemble_pick",
           "hdi", "hdi_span", "walker_set_hdi", "walker_hdi", "walker_set_quantiles",
           "walker_set_waic", "walker_waic", "waic_compare", "waic_merge",
           "walker_set_loo", "walker_loo", "loo_compare", "loo_tail_length",
           "walker_set_score_data", "walker_score_data", "kfold_folds", "walker_set_kfold_create",
           "walker_set_kfold",
           "trace_rows", "walker_set_trace", "walker_set_catepillar",
           "walker_set_get_residuals", "walker_set_goodness_of_fit", "walker_goodness_of_fit", "runs_z",
           "normeq_steps", "walker_set_laplace", "walker_laplace", "laplace_summary", "least_squares",
           "walker_set_least_squares",
           "candidate_grid", "walker_set_search", "walker_search", "walker_set_chi2_map"]
