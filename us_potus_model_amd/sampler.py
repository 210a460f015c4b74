"""Host-side mirror of the reference's sampler call surface, over libpotus_hmc.so.

The reference drives CmdStan from R (R is not available in this image, so the host side
above the C ABI is Python; R/potus_sampling.R is the same thin shim for R users):

    model <- cmdstanr::cmdstan_model("scripts/model/poll_model_2020.stan")   # final_2016.R:532
    fit   <- model$sample(data=, seed=1843, parallel_chains=, chains=,
                          iter_warmup=, iter_sampling=, refresh=)            # final_2016.R:533-541
    out   <- rstan::read_stan_csv(fit$output_files())                        # final_2016.R:543
    rstan::extract(out, pars = "mu_b")[[1]]                                  # final_2016.R:556,...

becomes

    model = PotusModel("full")                       # or "no_mode_adjustment" (final_2012.R:558)
    fit   = model.sample(data=, seed=1843, chains=, iter_warmup=, iter_sampling=, refresh=)
    fit.extract("mu_b")                              # [draws, S, T], chains merged

`sampling()` is the rstan::sampling() spelling (iter includes warmup; final_2016.R:525-529).
There is no CPU fallback: without the HIP library and an MI355X every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import _abi

_LIB = None
_HERE = Path(__file__).resolve().parent


class PotusError(RuntimeError):
    pass


def lib_path() -> Path:
    # POTUS_LIB selects a development build (e.g. the -DPOTUS_PROF one); default is the product library
    return Path(os.environ["POTUS_LIB"]) if os.environ.get("POTUS_LIB") else _HERE / "libpotus_hmc.so"


def load_library():
    """dlopen libpotus_hmc.so (built in-tree by __graft_entry__.build()). Fails loudly."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not p.exists():
        raise PotusError(f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(str(p))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.potus_version.restype = C.c_char_p
    L.potus_last_error.argtypes = [C.c_char_p, C.c_int]
    L.potus_default_opts.argtypes = [C.POINTER(_abi.PotusOpts)]
    L.potus_num_params.argtypes = [C.POINTER(_abi.PotusData), ip]
    L.potus_num_columns.argtypes = [C.POINTER(_abi.PotusData), ip]
    L.potus_column_name.argtypes = [C.POINTER(_abi.PotusData), C.c_int, C.c_char_p, C.c_int]
    L.potus_create.argtypes = [C.POINTER(_abi.PotusData), C.POINTER(_abi.PotusOpts), ip]
    L.potus_destroy.argtypes = [C.c_int]
    L.potus_log_prob_grad.argtypes = [C.c_int, dp, C.c_int, dp, dp]
    L.potus_init.argtypes = [C.c_int, dp]
    L.potus_run.argtypes = [C.c_int, C.c_int]
    L.potus_run_many.argtypes = [ip, C.c_int, C.c_int]
    L.potus_iterations_done.argtypes = [C.c_int, ip]
    L.potus_total_leapfrogs.argtypes = [C.c_int, C.POINTER(C.c_longlong)]
    L.potus_chain_status.argtypes = [C.c_int, ip, ip]
    L.potus_get_adaptation.argtypes = [C.c_int, dp, dp]
    L.potus_get_draws.argtypes = [C.c_int, dp, ip]
    L.potus_draws_device_ptr.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]
    L.potus_write_array.argtypes = [C.c_int, C.c_int, C.c_int, dp]
    L.potus_write_stan_csv.argtypes = [C.c_int, C.c_char_p, C.c_char_p]
    L.potus_last_run_timing.argtypes = [C.c_int, dp, C.POINTER(C.c_longlong)]
    L.potus_posterior_summary.argtypes = [C.c_int, dp, dp, dp, dp]
    L.potus_posterior_summary_many.argtypes = [ip, C.c_int, dp, dp, dp, dp]
    L.potus_backtest_scores.argtypes = [dp, C.c_int, C.c_int, C.c_int, dp, ip, dp]
    L.potus_write_array_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.potus_diagnostics.argtypes = [ip, C.c_int, C.c_int, C.c_int, dp, dp]
    L.potus_diagnostics_device.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int, dp, dp]
    if hasattr(L, "potus_check_convergence"):           # (development builds selected through POTUS_LIB may predate an export)
        L.potus_check_convergence.argtypes = [ip, C.c_int, C.c_double, C.c_double, ip, dp, dp]
    L.potus_get_dense_metric.argtypes = [C.c_int, C.c_int, dp]
    if hasattr(L, "potus_dense_pool_window"):
        L.potus_dense_pool_window.argtypes = [C.c_int, ip, dp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]
        L.potus_dense_pool_finish.argtypes = [C.c_int, C.c_double]
    L.potus_iterations_done.argtypes = [C.c_int, ip]
    L.potus_cus_per_chain.argtypes = [C.c_int, ip]
    L.potus_clusters_per_chain.argtypes = [C.c_int, ip]
    L.potus_plan_cus_per_chain.argtypes = [C.c_int] * 7 + [ip, ip]
    L.potus_plan_sides.argtypes = [C.c_int] * 7 + [ip]
    L.potus_twin_stats.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    if hasattr(L, "potus_sbc_ranks"):                   # simulation-based calibration (sbc.py)
        i32p = C.POINTER(C.c_int32)
        L.potus_set_datasets.argtypes = [C.c_int, C.c_int, i32p, i32p]
        L.potus_simulate_prior.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_int, dp, i32p, i32p]
        L.potus_constrain.argtypes = [C.c_int, dp, C.c_int, C.c_int, C.c_int, dp]
        L.potus_sbc_ranks.argtypes = [C.c_int, dp, C.c_int, C.c_int, C.c_int, i32p, i32p, ip]
    if hasattr(L, "potus_loo"):                         # PSIS-LOO (loo.py)
        L.potus_log_lik_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.potus_loo_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_longlong, dp, dp, dp]
        L.potus_loo.argtypes = [ip, C.c_int, C.c_int, dp, dp, dp]
    if hasattr(L, "potus_loo_moment_match"):            # moment matching for PSIS-LOO (loo.moment_match)
        i32p, mop = C.POINTER(C.c_int32), C.POINTER(_abi.PotusLooMmOpts)
        L.potus_default_loo_mm_opts.argtypes = [mop]
        L.potus_default_loo_mm_opts.restype = None
        L.potus_loo_moment_match.argtypes = [C.c_int, ip, C.c_int, mop, i32p, C.c_int, dp, dp, i32p, dp, dp]
        L.potus_loo_mm_timing.argtypes = [dp]
        L.potus_loo_mm_ratios_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, dp, dp, i32p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.potus_loo_mm_moments_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, dp, dp, dp]
        L.potus_psis_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_longlong, dp, C.c_void_p, dp]
        L.potus_R_loo_moment_match.argtypes = [ip, ip, ip, ip, dp, ip, dp, dp, ip, ip]
        L.potus_R_loo_moment_match.restype = None
    if hasattr(L, "potus_e_loo_device"):                # E_loo (loo.e_loo, loo.e_loo_shared)
        L.potus_e_loo_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, dp, dp, C.c_int, dp, dp]
        L.potus_e_loo_shared_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, dp, C.c_int, dp, dp, dp, dp]
        L.potus_e_loo_timing.argtypes = [dp]
        L.potus_poll_share_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.potus_e_loo.argtypes = [ip, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp]
        L.potus_R_loo_influence.argtypes = [ip, ip, ip, dp, dp, dp, dp, dp, dp, dp, ip]
        L.potus_R_loo_influence.restype = None
        L.potus_R_loo_predict.argtypes = [ip, ip, ip, dp, dp, ip]
        L.potus_R_loo_predict.restype = None
    if hasattr(L, "potus_ppc"):                         # posterior predictive checks (ppc.py)
        i32p, llp = C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
        L.potus_poll_rep_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.potus_ppc_pit_device.argtypes = [C.c_int, C.c_void_p, dp, C.c_void_p, C.c_int, C.c_int, C.c_longlong, dp]
        L.potus_ppc_groups_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, dp, dp, i32p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int,
                                              dp, llp]
        L.potus_ppc.argtypes = [ip, C.c_int, C.c_int, C.c_int, i32p, C.c_int, i32p, dp, dp, dp, llp]
        L.potus_ppc_timing.argtypes = [dp]
        L.potus_R_ppc.argtypes = [ip, ip, ip, ip, ip, dp, dp, dp, dp, ip]
        L.potus_R_ppc.restype = None
    if hasattr(L, "potus_outcomes"):                    # joint election outcomes (outcomes.py)
        i32p, llp = C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
        L.potus_outcomes.argtypes = [ip, C.c_int, C.c_int, C.c_int, i32p, C.c_int, dp, llp, llp, llp, llp, llp]
        L.potus_outcomes_device.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int, dp, i32p, C.c_int, dp, llp, llp, llp, llp, llp]
        L.potus_outcomes_timing.argtypes = [dp]
    if hasattr(L, "potus_monitor"):                     # the posterior summary table (monitor.py)
        L.potus_monitor.argtypes = [ip, C.c_int, C.c_int, C.c_int, dp, C.c_int, dp]
        L.potus_monitor_device.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int, dp, C.c_int, dp]
        L.potus_R_monitor.argtypes = [ip, ip, ip, dp, ip, dp, ip]
    if hasattr(L, "potus_scenario"):                    # conditional forecasts and the covariance of the state scores (scenario.py)
        i32p, llp = C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
        L.potus_scenario.argtypes = [ip, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int, i32p, C.c_int, llp, llp, dp, dp, llp, llp, llp]
        L.potus_scenario_device.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int, dp, C.c_int, dp, dp, i32p, C.c_int, llp, dp, dp, llp, llp, llp]
        L.potus_scenario_timing.argtypes = [dp]
        L.potus_R_scenario.argtypes = [ip, ip, ip, dp, dp, ip, dp, dp, dp, dp, dp, dp, ip]
    if hasattr(L, "potus_forecast_scores"):             # proper scoring rules of the joint forecast (scoring.py)
        i32p, llp = C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
        L.potus_forecast_scores_device.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int, dp, dp, C.c_int, dp, i32p, C.c_double, dp, dp]
        L.potus_forecast_scores.argtypes = [ip, C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, i32p, C.c_double, dp, dp, llp]
        L.potus_forecast_scores_datasets.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, i32p, C.c_double, dp, dp, i32p]
        L.potus_forecast_scores_timing.argtypes = [dp]
        L.potus_R_forecast_scores.argtypes = [ip, ip, ip, dp, dp, ip, dp, dp, dp, dp, ip]
        L.potus_R_forecast_scores.restype = None
    if hasattr(L, "potus_timeline"):                    # run dates as the data sets of one handle (timeline.py)
        i32p = C.POINTER(C.c_int32)
        L.potus_set_datasets_ex.argtypes = [C.c_int, C.c_int, i32p, i32p, i32p, i32p, dp, dp]
        L.potus_timeline.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, dp, dp, i32p]
        L.potus_timeline_scores_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.potus_timeline_timing.argtypes = [dp]
    if hasattr(L, "potus_grid_compare"):                # prior settings as the data sets of one handle (sensitivity.py)
        i32p = C.POINTER(C.c_int32)
        L.potus_set_datasets_grid.argtypes = [C.c_int, C.c_int, i32p, i32p, i32p, i32p, dp, dp, dp]
        L.potus_ecdf_distance_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, dp]
        L.potus_grid_compare.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, i32p]
        L.potus_grid_timing.argtypes = [dp]
        L.potus_R_set_datasets_grid.argtypes = [ip, ip, ip, ip, ip, ip, ip, dp, dp, dp, ip]
        L.potus_R_grid_compare.argtypes = [ip, ip, dp, dp, ip, ip]
    if hasattr(L, "potus_cv_lpd"):                      # exact cross-validation (crossval.py)
        i32p = C.POINTER(C.c_int32)
        L.potus_cv_log_lik_device.argtypes = [C.c_int, i32p, i32p, C.c_int, C.c_void_p, C.POINTER(C.c_longlong)]
        L.potus_cv_lpd.argtypes = [C.c_int, i32p, i32p, C.c_int, dp, i32p]
        L.potus_cv_timing.argtypes = [dp]
        L.potus_R_cv_lpd.argtypes = [ip, ip, ip, ip, dp, ip, ip]
    if hasattr(L, "potus_optimize"):                    # the posterior mode (Handle.optimize, PotusModel.optimize)
        i32p, oop = C.POINTER(C.c_int32), C.POINTER(_abi.PotusOptimizeOpts)
        L.potus_default_optimize_opts.argtypes = [oop]
        L.potus_default_optimize_opts.restype = None
        L.potus_optimize.argtypes = [C.c_int, oop, dp, C.c_int, dp, dp, dp, i32p, C.c_int, C.c_int, dp]
        L.potus_optimize_timing.argtypes = [dp]
        L.potus_R_optimize.argtypes = [ip, ip, dp, dp, dp, dp, dp, ip, ip, dp, ip]
        L.potus_R_optimize.restype = None
    if hasattr(L, "potus_laplace"):                     # the Laplace approximation (Handle.laplace, PotusModel.laplace)
        i32p, lop = C.POINTER(C.c_int32), C.POINTER(_abi.PotusLaplaceOpts)
        L.potus_default_laplace_opts.argtypes = [lop]
        L.potus_default_laplace_opts.restype = None
        L.potus_laplace.argtypes = [C.c_int, lop, dp, C.c_int, dp, C.c_int, dp, dp, dp, dp, dp]
        L.potus_laplace_write_array_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.potus_laplace_scores_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.potus_laplace_summary.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, dp, dp, i32p]
        L.potus_laplace_timing.argtypes = [dp]
        L.potus_R_laplace.argtypes = [ip, ip, dp, dp, dp, dp, dp, dp, dp, dp, ip]
        L.potus_R_laplace.restype = None
    if hasattr(L, "potus_pathfinder"):                  # Pathfinder (Handle.pathfinder, PotusModel.pathfinder)
        i32p, pop = C.POINTER(C.c_int32), C.POINTER(_abi.PotusPathfinderOpts)
        L.potus_default_pathfinder_opts.argtypes = [pop]
        L.potus_default_pathfinder_opts.restype = None
        L.potus_pathfinder.argtypes = [C.c_int, pop, dp, C.c_int, i32p, dp, i32p, dp, dp, dp, dp, dp]
        L.potus_pathfinder_path.argtypes = [C.c_int, pop, dp, dp, i32p, C.c_int, C.c_int, dp, dp, i32p, i32p, dp, i32p, dp, dp, dp, dp, dp, dp, dp, dp, dp]
        L.potus_pathfinder_write_array_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.potus_pathfinder_scores_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.potus_pathfinder_summary.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, dp, dp, i32p]
        L.potus_pathfinder_timing.argtypes = [dp]
        L.potus_R_pathfinder.argtypes = [ip, ip, dp, dp, ip, dp, ip, dp, dp, dp, ip]
        L.potus_R_pathfinder.restype = None
    if hasattr(L, "potus_advi"):                        # mean-field ADVI (Handle.variational, PotusModel.variational)
        i32p, vop = C.POINTER(C.c_int32), C.POINTER(_abi.PotusAdviOpts)
        L.potus_default_advi_opts.argtypes = [vop]
        L.potus_default_advi_opts.restype = None
        L.potus_advi.argtypes = [C.c_int, vop, dp, C.c_int, i32p, dp, dp, dp, dp, dp, dp, dp]
        L.potus_advi_write_array_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.potus_advi_scores_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.potus_advi_summary.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, dp, dp, i32p]
        L.potus_advi_timing.argtypes = [dp]
        L.potus_R_variational.argtypes = [ip, ip, dp, dp, ip, dp, dp, dp, dp, dp, dp, dp, ip]
        L.potus_R_variational.restype = None
    _LIB = L
    return L


EXPORTS = [
    "potus_version", "potus_last_error", "potus_default_opts", "potus_num_params", "potus_num_columns",
    "potus_column_name", "potus_create", "potus_destroy", "potus_cus_per_chain", "potus_clusters_per_chain", "potus_plan_cus_per_chain", "potus_plan_sides", "potus_twin_stats", "potus_log_prob_grad", "potus_init", "potus_run", "potus_run_many",
    "potus_iterations_done", "potus_total_leapfrogs", "potus_chain_status", "potus_get_adaptation",
    "potus_get_dense_metric", "potus_dense_timing", "potus_dense_adapt_timing", "potus_dense_pool_window", "potus_dense_pool_finish", "potus_dense_check", "potus_get_draws", "potus_draws_device_ptr", "potus_write_array", "potus_write_array_device", "potus_extract_matrix", "potus_write_stan_csv",
    "potus_last_run_timing", "potus_posterior_summary", "potus_posterior_summary_many", "potus_backtest_scores",
    "potus_diagnostics", "potus_diagnostics_device", "potus_check_convergence",
    "potus_set_datasets", "potus_simulate_prior", "potus_constrain", "potus_sbc_ranks",
    "potus_set_datasets_ex", "potus_timeline", "potus_timeline_scores_device", "potus_timeline_timing",
    "potus_set_datasets_grid", "potus_ecdf_distance_device", "potus_grid_compare", "potus_grid_timing",
    "potus_log_lik_device", "potus_loo_device", "potus_loo",
    "potus_default_loo_mm_opts", "potus_loo_moment_match", "potus_loo_mm_timing", "potus_loo_mm_ratios_device", "potus_loo_mm_moments_device",
    "potus_psis_device", "potus_R_loo_moment_match",
    "potus_e_loo_device", "potus_e_loo_shared_device", "potus_e_loo_timing", "potus_poll_share_device", "potus_e_loo", "potus_R_loo_influence", "potus_R_loo_predict",
    "potus_poll_rep_device", "potus_ppc_pit_device", "potus_ppc_groups_device", "potus_ppc", "potus_ppc_timing", "potus_R_ppc",
    "potus_cv_log_lik_device", "potus_cv_lpd", "potus_cv_timing",
    "potus_default_optimize_opts", "potus_optimize", "potus_optimize_timing",
    "potus_default_laplace_opts", "potus_laplace", "potus_laplace_write_array_device", "potus_laplace_scores_device", "potus_laplace_summary",
    "potus_laplace_timing", "potus_R_laplace",
    "potus_default_pathfinder_opts", "potus_pathfinder", "potus_pathfinder_path", "potus_pathfinder_write_array_device",
    "potus_pathfinder_scores_device", "potus_pathfinder_summary", "potus_pathfinder_timing", "potus_R_pathfinder",
    "potus_default_advi_opts", "potus_advi", "potus_advi_write_array_device", "potus_advi_scores_device", "potus_advi_summary",
    "potus_advi_timing", "potus_R_variational",
    "potus_outcomes", "potus_outcomes_device", "potus_outcomes_timing",
    "potus_monitor", "potus_monitor_device",
    "potus_scenario", "potus_scenario_device", "potus_scenario_timing",
    "potus_forecast_scores", "potus_forecast_scores_device", "potus_forecast_scores_datasets", "potus_forecast_scores_timing", "potus_R_forecast_scores",
    "potus_R_create", "potus_R_init", "potus_R_run", "potus_R_run_many", "potus_R_num_columns", "potus_R_saved_count",
    "potus_R_write_array", "potus_R_write_stan_csv", "potus_R_posterior_summary", "potus_R_diagnostics", "potus_R_check_convergence", "potus_R_backtest_scores", "potus_R_last_error", "potus_R_destroy",
    "potus_R_set_datasets", "potus_R_simulate_prior", "potus_R_sbc_ranks", "potus_R_constrain", "potus_R_loo", "potus_R_outcomes", "potus_R_monitor", "potus_R_scenario",
    "potus_R_set_datasets_ex", "potus_R_timeline", "potus_R_cv_lpd", "potus_R_optimize", "potus_R_set_datasets_grid", "potus_R_grid_compare",
]


# the nine hand-set prior scales of the data, in the order of potus_set_datasets_grid's scales[n][POTUS_N_SCALES]
SCALE_NAMES = ("sigma_c", "sigma_m", "sigma_pop", "sigma_measure_noise_national", "sigma_measure_noise_state", "sigma_e_bias",
               "random_walk_scale", "mu_b_T_scale", "polling_bias_scale")
N_SCALES = len(SCALE_NAMES)


def ecdf_distance_device(a, b, L=None):
    """potus_ecdf_distance_device: a [n_a, n_cols] and b [n_b, n_cols], float64 torch tensors on one GPU, draw-major.  Returns [n_cols, 3] =
    (w1, ks, cjs) per column (numpy)."""
    import torch
    L = L or load_library()
    if a.dtype != torch.float64 or b.dtype != torch.float64 or a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("ecdf_distance_device: two float64 blocks [n_a, n_cols] and [n_b, n_cols] are expected")
    a, b = a.contiguous(), b.contiguous()
    out = np.zeros((a.shape[1], 3))
    torch.cuda.current_stream(a.device).synchronize()
    _check(L, L.potus_ecdf_distance_device(a.device.index or 0, C.c_void_p(a.data_ptr()), a.shape[0], C.c_void_p(b.data_ptr()), b.shape[0], a.shape[1], _dp(out)))
    return out


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _check(L, rc):
    if rc != 0:
        buf = C.create_string_buffer(512)
        L.potus_last_error(buf, 512)
        raise PotusError(f"libpotus_hmc error {rc}: {buf.value.decode()}")


class Handle:
    """One sampler instance on one GPU (a set of chains)."""

    def __init__(self, data: dict, variant="full", **opts):
        self.L = load_library()
        self.data = data
        self.variant = variant
        self.n_datasets = 1                        # until set_datasets[_ex]
        self._d, self._keep = _abi.make_data(data, variant)
        o = _abi.PotusOpts()
        self.L.potus_default_opts(C.byref(o))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown sampler option {k!r}")
            setattr(o, k, v)
        self.opts = o
        h = C.c_int(-1)
        _check(self.L, self.L.potus_create(C.byref(self._d), C.byref(o), C.byref(h)))
        self.h = h.value
        D, nc = C.c_int(), C.c_int()
        _check(self.L, self.L.potus_num_params(C.byref(self._d), C.byref(D)))
        _check(self.L, self.L.potus_num_columns(C.byref(self._d), C.byref(nc)))
        self.D, self.n_cols = D.value, nc.value
        self.layout, ncols2 = _abi.column_layout(data, variant)
        assert ncols2 == self.n_cols
        k = C.c_int()
        _check(self.L, self.L.potus_cus_per_chain(self.h, C.byref(k)))
        self.cus_per_chain = k.value
        _check(self.L, self.L.potus_clusters_per_chain(self.h, C.byref(k)))
        self.clusters_per_chain = k.value          # 2: one cluster per end of the trajectory (opts twin)

    def close(self):
        if getattr(self, "h", None) is not None and self.h >= 0:
            self.L.potus_destroy(self.h)
            self.h = -1

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def log_prob_grad(self, q):
        q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float64)
        n = q.shape[0]
        assert q.shape[1] == self.D
        lp, g = np.zeros(n), np.zeros((n, self.D))
        _check(self.L, self.L.potus_log_prob_grad(self.h, _dp(q), n, _dp(lp), _dp(g)))
        return lp, g

    def init(self, q0=None):
        p = None
        if q0 is not None:
            q0 = np.ascontiguousarray(q0, dtype=np.float64).reshape(self.opts.chains, self.D)
            p = _dp(q0)
        _check(self.L, self.L.potus_init(self.h, p))

    def run(self, n_iter):
        _check(self.L, self.L.potus_run(self.h, int(n_iter)))

    def iterations_done(self):
        n = C.c_int()
        _check(self.L, self.L.potus_iterations_done(self.h, C.byref(n)))
        return n.value

    def total_leapfrogs(self):
        n = C.c_longlong()
        _check(self.L, self.L.potus_total_leapfrogs(self.h, C.byref(n)))
        return n.value

    def last_run_timing(self):
        ms, n = C.c_double(), C.c_longlong()
        _check(self.L, self.L.potus_last_run_timing(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def chain_status(self):
        ch = self.opts.chains
        st, dv = (C.c_int * ch)(), (C.c_int * ch)()
        _check(self.L, self.L.potus_chain_status(self.h, st, dv))
        return list(st), list(dv)

    def adaptation(self):
        ch = self.opts.chains
        eps, minv = np.zeros(ch), np.zeros((ch, self.D))
        _check(self.L, self.L.potus_get_adaptation(self.h, _dp(eps), _dp(minv)))
        return eps, minv

    def draws_saved(self):
        n = C.c_int()
        _check(self.L, self.L.potus_get_draws(self.h, None, C.byref(n)))
        return n.value

    def draws(self):
        """[chains, n_saved, 7 + D] on the unconstrained scale."""
        n = C.c_int()
        _check(self.L, self.L.potus_get_draws(self.h, None, C.byref(n)))
        out = np.zeros((self.opts.chains, n.value, _abi.N_SAMPLER_COLS + self.D))
        if n.value:
            _check(self.L, self.L.potus_get_draws(self.h, _dp(out), C.byref(n)))
        return out

    def posterior_summary(self, ev):
        """Device-side summaries of predicted_score over all saved draws (final_2016.R:708-762, 799-823).

        Returns dict(state=[T,S,4] (low, high, mean, prob), national=[T,4], electoral_votes=[T,5]
        (mean, median, high, low, P(>=270))); `ev` = electoral votes per state, in state order."""
        return posterior_summary([self], ev)

    def write_array_device(self, col_begin, col_end, out_tensor):
        """write_array straight into a torch tensor on this handle's GPU ([n_saved, chains, col_end - col_begin],
        float64, contiguous): the buffer an RCCL all-gather sends, no trip through the host."""
        _device_block(out_tensor, "write_array_device")                # (the library writes on its own stream)
        n = C.c_int()
        _check(self.L, self.L.potus_get_draws(self.h, None, C.byref(n)))
        if out_tensor.numel() != n.value * self.opts.chains * (col_end - col_begin):
            raise ValueError(f"tensor has {out_tensor.numel()} elements, {n.value} x {self.opts.chains} x {col_end - col_begin} expected")
        _check(self.L, self.L.potus_write_array_device(self.h, col_begin, col_end, C.c_void_p(out_tensor.data_ptr())))
        return out_tensor

    def twin_stats(self):
        """Twin mode: (leapfrogs counted in the trajectories, leaves integrated by the backward side, by the forward side)."""
        a, b, c = C.c_longlong(), C.c_longlong(), C.c_longlong()
        _check(self.L, self.L.potus_twin_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def dense_timing(self):
        """metric = dense_e: (milliseconds in k_dn_matvec, matrix passes, bytes of matrix streamed, leaf rounds) so far."""
        L = self.L
        L.potus_dense_timing.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        ms, n, b, r = C.c_double(), C.c_longlong(), C.c_longlong(), C.c_longlong()
        _check(L, L.potus_dense_timing(self.h, C.byref(ms), C.byref(n), C.byref(b), C.byref(r)))
        return ms.value, n.value, b.value, r.value

    def dense_adapt_timing(self):
        """metric = dense_e: dict(cov_ms, chol_ms, init_stepsize_ms, window_ends) of the warm-up's window ends so far."""
        L = self.L
        L.potus_dense_adapt_timing.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        _check(L, L.potus_dense_adapt_timing(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return dict(cov_ms=a.value, chol_ms=b.value, init_stepsize_ms=c.value, window_ends=n.value)

    def pool_window(self):
        """pooled_metric = 2: (pending, count, mean, m2) of a window end that waits for the host -- mean [D] and m2 [D, LD] are torch tensors ON the handle's
        GPU that alias the library's buffers (zero copy; m2[:, :D] is the matrix of centred outer products, both triangles)."""
        pend, cnt, pm, p2, ld = C.c_int(), C.c_double(), C.c_void_p(), C.c_void_p(), C.c_longlong()
        _check(self.L, self.L.potus_dense_pool_window(self.h, C.byref(pend), C.byref(cnt), C.byref(pm), C.byref(p2), C.byref(ld)))
        if not pend.value:
            return False, 0.0, None, None
        import torch

        class _Dev:                                        # __cuda_array_interface__: torch wraps the device pointer without copying
            def __init__(s_, ptr, shape):
                s_.__cuda_array_interface__ = {"shape": shape, "typestr": "<f8", "data": (ptr, False), "version": 2}
        dev = f"cuda:{self.opts.device}"
        mean = torch.as_tensor(_Dev(pm.value, (self.D,)), device=dev)
        m2 = torch.as_tensor(_Dev(p2.value, (self.D, ld.value)), device=dev)
        return True, cnt.value, mean, m2

    def pool_finish(self, n_total):
        _check(self.L, self.L.potus_dense_pool_finish(self.h, C.c_double(float(n_total))))

    def dense_check(self, chain=0, n_probe=2):
        """metric = dense_e: (max ||L L' x - M^-1 x|| / ||M^-1 x|| over n_probe random x, ||L' p - u|| / ||u|| of the momentum solve)."""
        L = self.L
        L.potus_dense_check.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        out = np.zeros(2)
        _check(L, L.potus_dense_check(self.h, int(chain), int(n_probe), _dp(out)))
        return float(out[0]), float(out[1])

    def dense_metric(self, chain=0):
        """metric = dense_e: the adapted D x D inverse metric of one chain."""
        out = np.zeros((self.D, self.D))
        _check(self.L, self.L.potus_get_dense_metric(self.h, int(chain), _dp(out)))
        return out

    def draws_device_ptr(self):
        p, n = C.c_void_p(), C.c_longlong()
        _check(self.L, self.L.potus_draws_device_ptr(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def write_array(self, col_begin, col_end, n_saved):
        out = np.zeros((n_saved, self.opts.chains, max(col_end - col_begin, 1)))
        if n_saved:
            _check(self.L, self.L.potus_write_array(self.h, col_begin, col_end, _dp(out)))
        return out

    def set_datasets(self, n_democrat_state, n_democrat_national):
        """potus_set_datasets: [n, N_state_polls] and [n, N_national_polls] poll outcomes, one data set per chains / n consecutive chains
        (before init(); one workgroup per chain, diagonal metric)."""
        Ns, Nn = int(self.data["N_state_polls"]), int(self.data["N_national_polls"])
        ys = np.ascontiguousarray(np.asarray(n_democrat_state, dtype=np.int32).reshape(-1, Ns) if Ns else np.zeros((0, 0), np.int32))
        yn = np.ascontiguousarray(np.asarray(n_democrat_national, dtype=np.int32).reshape(-1, Nn) if Nn else np.zeros((0, 0), np.int32))
        n = ys.shape[0] if Ns else yn.shape[0]
        if Ns and Nn and ys.shape[0] != yn.shape[0]:
            raise ValueError(f"{ys.shape[0]} state and {yn.shape[0]} national outcome vectors")
        _check(self.L, self.L.potus_set_datasets(self.h, n, _ip(ys), _ip(yn)))
        self.n_datasets = n

    def set_datasets_ex(self, n_democrat_state=None, n_democrat_national=None, n_two_share_state=None, n_two_share_national=None,
                        mu_b_prior=None, mu_b_T_scale=None, n=None, scales=None, _grid=False):
        """potus_set_datasets_ex: data sets that may differ in the poll outcomes and sizes ([n, N_state_polls], [n, N_national_polls];
        n_two_share = 0: the data set has not seen the poll), mu_b_prior [n, S] and mu_b_T_scale [n].  None = the handle's own for every data set."""
        what = "set_datasets_grid" if _grid else "set_datasets_ex"
        Ns, Nn, S = int(self.data["N_state_polls"]), int(self.data["N_national_polls"]), int(self.data["S"])
        given = [(a, w) for a, w in ((n_democrat_state, Ns), (n_two_share_state, Ns), (n_democrat_national, Nn), (n_two_share_national, Nn),
                                     (mu_b_prior, S), (mu_b_T_scale, 1), (scales, N_SCALES)) if a is not None and w]
        counts = {np.asarray(a).reshape(-1, w).shape[0] for a, w in given} | ({int(n)} if n is not None else set())
        if len(counts) != 1:
            raise ValueError(f"{what}: the arrays give {sorted(counts)} data sets (pass n when every array is None)")
        n = counts.pop()
        keep = []

        def ints(a, w):
            if a is None or not w:
                return None
            keep.append(np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(n, w)))
            return _ip(keep[-1])

        def dbls(a, w):
            if a is None:
                return None
            keep.append(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(n, w)))
            return _dp(keep[-1])
        args = (self.h, n, ints(n_democrat_state, Ns), ints(n_democrat_national, Nn), ints(n_two_share_state, Ns), ints(n_two_share_national, Nn),
                dbls(mu_b_prior, S), dbls(mu_b_T_scale, 1))
        _check(self.L, self.L.potus_set_datasets_grid(*args, dbls(scales, N_SCALES)) if _grid else self.L.potus_set_datasets_ex(*args))
        self.n_datasets = n

    def set_datasets_grid(self, scales=None, **datasets):
        """potus_set_datasets_grid: set_datasets_ex (same keywords) and scales [n, 9], the nine prior scales of every data set in the order of
        SCALE_NAMES.  None = the handle's own for every data set; mu_b_T_scale and scales together are refused."""
        self.set_datasets_ex(scales=scales, _grid=True, **datasets)

    def grid_compare(self, ev, base=0, days=None, ev_to_win=270):
        """potus_grid_compare: every data set against data set `base` over the post-warm-up draws, per day of `days` = (begin, end) (0-based,
        default: election day only): dict(distance [n, days, S + 2, 3] = (w1, ks, cjs) of the S state scores, the national vote and the
        electoral votes of a draw; n_draws [n]).  A data set with a failed chain has NaN, and so has every row if `base` failed."""
        S = int(self.data["S"])
        t0, t1 = self._day_range(days)
        n, nd = self.n_datasets, max(t1 - t0, 0)
        ev = np.ascontiguousarray(ev, dtype=np.float64).reshape(S)
        out, cnt = np.zeros((n, nd, S + 2, 3)), np.zeros(n, np.int32)
        _check(self.L, self.L.potus_grid_compare(self.h, int(base), t0, t1, _dp(ev), int(ev_to_win), _dp(out), _ip(cnt)))
        return dict(distance=out, n_draws=cnt)

    def grid_timing(self):
        ms = np.zeros(2)
        _check(self.L, self.L.potus_grid_timing(_dp(ms)))
        return dict(scores_ms=float(ms[0]), distance_ms=float(ms[1]))

    def _day_range(self, days):
        """days = (begin, end), 0-based; None: election day only."""
        T = int(self.data["T"])
        return (T - 1, T) if days is None else (int(days[0]), int(days[1]))

    def timeline(self, ev, days=None, ev_to_win=270):
        """potus_timeline: per data set of this handle and per day of `days` = (begin, end) (0-based, default: election day only) the summaries of
        posterior_summary over the data set's post-warm-up draws.  dict(state [n, days, S, 4], national [n, days, 4], electoral_votes [n, days, 5],
        n_draws [n]); a data set with a failed chain has n_draws = 0 and NaN."""
        S = int(self.data["S"])
        t0, t1 = self._day_range(days)
        n, nd = self.n_datasets, max(t1 - t0, 0)
        ev = np.ascontiguousarray(ev, dtype=np.float64).reshape(S)
        st, na, eo, cnt = np.zeros((n, nd, S, 4)), np.zeros((n, nd, 4)), np.zeros((n, nd, 5)), np.zeros(n, np.int32)
        _check(self.L, self.L.potus_timeline(self.h, t0, t1, _dp(ev), int(ev_to_win), _dp(st), _dp(na), _dp(eo), _ip(cnt)))
        return dict(state=st, national=na, electoral_votes=eo, n_draws=cnt)

    def timeline_scores_device(self, days=None):
        """potus_timeline_scores_device: predicted_score of the days (begin, end) as a torch tensor [n_datasets, draws per data set, days, S] on this handle's GPU."""
        import torch
        S = int(self.data["S"])
        t0, t1 = self._day_range(days)
        n = self.n_datasets
        per = (self.opts.chains // n) * self.post_warmup_saved()
        out = torch.empty((n, per, max(t1 - t0, 1), S), dtype=torch.float64, device=f"cuda:{self.opts.device}")
        torch.cuda.current_stream(out.device).synchronize()
        _check(self.L, self.L.potus_timeline_scores_device(self.h, t0, t1, C.c_void_p(out.data_ptr())))
        return out

    def timeline_timing(self):
        ms = np.zeros(2)
        _check(self.L, self.L.potus_timeline_timing(_dp(ms)))
        return dict(scores_ms=float(ms[0]), summary_ms=float(ms[1]))

    def optimize_opts(self, **opts):
        """potus_default_optimize_opts with the given fields replaced (jacobian, history_size, iter, path_offset, init_alpha, tol_*)."""
        o = _abi.PotusOptimizeOpts()
        self.L.potus_default_optimize_opts(C.byref(o))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown optimiser option {k!r}")
            setattr(o, k, v)
        return o

    def optimize(self, q0=None, paths=None, cols=None, opts=None, **fields):
        """potus_optimize: the mode of every path in one launch (batched L-BFGS, one workgroup per path).  q0 [paths, D] starts, or None for
        `paths` library starts (U(-init_radius, init_radius), Philox purpose 7).  On a handle with data sets path p uses data set
        p // (paths // n_datasets).  cols = (begin, end): also the CmdStan output row columns of every path's point, built with the path's
        own model.  fields: those of potus_optimize_opts (or opts: a filled struct).  Returns dict(q [paths, D], lp, grad_norm, return_code, iterations,
        grad_evals [paths] and, with cols, rows [paths, end - begin])."""
        o = opts if opts is not None else self.optimize_opts(**fields)
        p0 = None
        if q0 is not None:
            q0 = np.ascontiguousarray(np.atleast_2d(q0), dtype=np.float64)
            if q0.shape[1] != self.D or (paths is not None and int(paths) != q0.shape[0]):
                raise ValueError(f"optimize: q0 has shape {q0.shape}, [{paths if paths is not None else 'paths'}, {self.D}] expected")
            paths, p0 = q0.shape[0], _dp(q0)
        n = int(1 if paths is None else paths)
        q, lp, gn, info = np.zeros((max(n, 0), self.D)), np.zeros(max(n, 0)), np.zeros(max(n, 0)), np.zeros((max(n, 0), 3), np.int32)
        a, b = (0, 0) if cols is None else (int(cols[0]), int(cols[1]))
        rows = None if cols is None else np.zeros((max(n, 0), max(b - a, 1)))
        _check(self.L, self.L.potus_optimize(self.h, C.byref(o), p0, n, _dp(q), _dp(lp), _dp(gn), _ip(info), a, b, None if rows is None else _dp(rows)))
        out = dict(q=q, lp=lp, grad_norm=gn, return_code=info[:, 0].copy(), iterations=info[:, 1].copy(), grad_evals=info[:, 2].copy())
        if rows is not None:
            out["rows"] = rows[:, :b - a]
        return out

    def optimize_timing(self):
        """Milliseconds (HIP events) of k_opt_lbfgs in this thread's last optimize()."""
        ms = np.zeros(1)
        _check(self.L, self.L.potus_optimize_timing(_dp(ms)))
        return float(ms[0])

    def laplace_opts(self, **opts):
        """potus_default_laplace_opts with the given fields replaced (jacobian, draw_offset, h)."""
        o = _abi.PotusLaplaceOpts()
        self.L.potus_default_laplace_opts(C.byref(o))
        for k, v in opts.items():
            if k.startswith("pad") or not hasattr(o, k):
                raise TypeError(f"unknown Laplace option {k!r}")
            setattr(o, k, v)
        return o

    def laplace(self, mode, draws, u=None, precision=False, opts=None, **fields):
        """potus_laplace: the normal approximation around mode [modes, D] (or [D]): P = minus the Hessian of log_prob<jacobian> by central
        differences on the device, P = L L', `draws` draws x = mode + L^-T u per mode.  u [modes, draws, D]: the caller's standard normals, None:
        the library's (Philox purpose 8, draw n of a call is draw draw_offset + n).  On a handle with data sets mode m uses data set
        m // (modes // n_datasets).  fields: those of potus_laplace_opts (or opts: a filled struct).  Returns dict(q [modes, draws, D], lp,
        lp_approx [modes, draws], return_code, log_det, grad_norm, min_pivot [modes] and, with precision, precision [modes, D, D])."""
        o = opts if opts is not None else self.laplace_opts(**fields)
        mode = np.ascontiguousarray(np.atleast_2d(np.asarray(mode, dtype=np.float64)))
        if mode.ndim != 2 or mode.shape[1] != self.D:
            raise ValueError(f"laplace: mode has shape {mode.shape}, [modes, {self.D}] expected")
        m, n = mode.shape[0], int(draws)
        pu = None
        if u is not None:
            u = np.ascontiguousarray(np.asarray(u, dtype=np.float64))
            if u.shape == (n, self.D) and m == 1:
                u = u.reshape(1, n, self.D)
            if u.shape != (m, n, self.D):
                raise ValueError(f"laplace: u has shape {u.shape}, [{m}, {n}, {self.D}] expected")
            pu = _dp(u)
        k = max(n, 0)
        q, lp, la, info = np.zeros((m, k, self.D)), np.zeros((m, k)), np.zeros((m, k)), np.zeros((m, 4))
        prec = np.zeros((m, self.D, self.D)) if precision else None
        _check(self.L, self.L.potus_laplace(self.h, C.byref(o), _dp(mode), m, pu, n, _dp(q) if k else None, _dp(lp) if k else None,
                                            _dp(la) if k else None, _dp(info), None if prec is None else _dp(prec)))
        self._laplace_shape = (m, k)
        out = dict(q=q, lp=lp, lp_approx=la, return_code=info[:, 0].astype(np.int32), log_det=info[:, 1].copy(), grad_norm=info[:, 2].copy(),
                   min_pivot=info[:, 3].copy())
        if prec is not None:
            out["precision"] = prec
        return out

    def _laplace_block(self, what):
        shape = getattr(self, "_laplace_shape", None)
        if not shape or not shape[1]:
            raise PotusError(f"{what}: no Laplace draws on this handle (laplace(mode, draws >= 1) first)")
        return shape

    def laplace_rows_device(self, cols=None):
        """potus_laplace_write_array_device: the CmdStan output columns (begin, end) (default: all) of the last laplace() call's draws, a torch
        tensor [modes * draws, end - begin] on this handle's GPU -- what monitor_device takes."""
        import torch
        m, n = self._laplace_block("laplace_rows_device")
        a, b = (0, self.n_cols) if cols is None else (int(cols[0]), int(cols[1]))
        out = torch.empty((m * n, max(b - a, 1)), dtype=torch.float64, device=f"cuda:{self.opts.device}")
        torch.cuda.current_stream(out.device).synchronize()
        _check(self.L, self.L.potus_laplace_write_array_device(self.h, a, b, C.c_void_p(out.data_ptr())))
        return out

    def laplace_scores(self, days=None):
        """potus_laplace_scores_device: predicted_score of the days (begin, end) (0-based, default: election day) of the last laplace() call's
        draws, a torch tensor [modes, draws, days, S] on this handle's GPU; a mode's block is what outcomes_device / scenario_device take."""
        import torch
        m, n = self._laplace_block("laplace_scores")
        S = int(self.data["S"])
        t0, t1 = self._day_range(days)
        out = torch.empty((m, n, max(t1 - t0, 1), S), dtype=torch.float64, device=f"cuda:{self.opts.device}")
        torch.cuda.current_stream(out.device).synchronize()
        _check(self.L, self.L.potus_laplace_scores_device(self.h, t0, t1, C.c_void_p(out.data_ptr())))
        return out

    def laplace_summary(self, ev, days=None, ev_to_win=270):
        """potus_laplace_summary: timeline()'s outputs with the modes of the last laplace() call in the place of data sets:
        dict(state [modes, days, S, 4], national [modes, days, 4], electoral_votes [modes, days, 5], n_draws [modes])."""
        m, _ = self._laplace_block("laplace_summary")
        S = int(self.data["S"])
        t0, t1 = self._day_range(days)
        nd = max(t1 - t0, 0)
        ev = np.ascontiguousarray(ev, dtype=np.float64).reshape(S)
        st, na, eo, cnt = np.zeros((m, nd, S, 4)), np.zeros((m, nd, 4)), np.zeros((m, nd, 5)), np.zeros(m, np.int32)
        _check(self.L, self.L.potus_laplace_summary(self.h, t0, t1, _dp(ev), int(ev_to_win), _dp(st), _dp(na), _dp(eo), _ip(cnt)))
        return dict(state=st, national=na, electoral_votes=eo, n_draws=cnt)

    def laplace_timing(self):
        """Milliseconds (HIP events) of the stages of this thread's last laplace(): Hessian, factor, solve, lp__."""
        ms = np.zeros(4)
        _check(self.L, self.L.potus_laplace_timing(_dp(ms)))
        return dict(hessian_ms=float(ms[0]), factor_ms=float(ms[1]), solve_ms=float(ms[2]), lp_ms=float(ms[3]))

    def pathfinder_opts(self, **opts):
        """potus_default_pathfinder_opts with the given fields replaced: history_size, num_elbo_draws, num_draws, draw_offset, path_offset, and,
        for the L-BFGS run, max_lbfgs_iters (opt.iter), lbfgs_history_size (opt.history_size), init_alpha, tol_*."""
        o = _abi.PotusPathfinderOpts()
        self.L.potus_default_pathfinder_opts(C.byref(o))
        for k, v in opts.items():
            if k == "max_lbfgs_iters":
                o.opt.iter = int(v)
            elif k == "lbfgs_history_size":
                o.opt.history_size = int(v)
            elif k in ("init_alpha", "tol_obj", "tol_rel_obj", "tol_grad", "tol_rel_grad", "tol_param"):
                setattr(o.opt, k, float(v))
            elif k in ("history_size", "num_elbo_draws", "num_draws", "draw_offset", "path_offset"):
                setattr(o, k, int(v))
            else:
                raise TypeError(f"unknown Pathfinder option {k!r}")
        return o

    def _pathfinder_out(self, n, rows, m):
        return dict(info=np.zeros((n, 4), np.int32), elbo=np.zeros((n, rows)), kept=np.zeros((n, rows), np.int32), q=np.zeros((n, m, self.D)),
                    lp=np.zeros((n, m)), lq=np.zeros((n, m)))

    def _pathfinder_result(self, o, n, m):
        info = o.pop("info")
        self._pathfinder_shape = (n, m)
        o.update(return_code=info[:, 0].copy(), iterations=info[:, 1].copy(), best_iteration=info[:, 2].copy(), optimize_code=info[:, 3].copy())
        return o

    def pathfinder(self, q0=None, paths=None, trajectory=False, opts=None, **fields):
        """potus_pathfinder: an L-BFGS path per start (q0 [paths, D], or None for `paths` library starts), the normal approximation of every
        iterate, the ELBO of each, num_draws draws from the best one.  On a handle with data sets path p uses data set p // (paths // n_datasets).
        fields: see pathfinder_opts (or opts: a filled struct).  Returns dict(q [paths, draws, D], lp, lq [paths, draws], elbo, kept
        [paths, max_lbfgs_iters + 1] indexed by the iterate, return_code, iterations, best_iteration, optimize_code [paths] and, with
        trajectory, x, g [paths, max_lbfgs_iters + 1, D])."""
        o = opts if opts is not None else self.pathfinder_opts(**fields)
        p0 = None
        if q0 is not None:
            q0 = np.ascontiguousarray(np.atleast_2d(q0), dtype=np.float64)
            if q0.shape[1] != self.D or (paths is not None and int(paths) != q0.shape[0]):
                raise ValueError(f"pathfinder: q0 has shape {q0.shape}, [{paths if paths is not None else 'paths'}, {self.D}] expected")
            paths, p0 = q0.shape[0], _dp(q0)
        n, rows, m = int(1 if paths is None else paths), max(int(o.opt.iter), 0) + 1, max(int(o.num_draws), 0)
        r = self._pathfinder_out(max(n, 0), rows, m)
        tx, tg = (np.zeros((max(n, 0), rows, self.D)), np.zeros((max(n, 0), rows, self.D))) if trajectory else (None, None)
        _check(self.L, self.L.potus_pathfinder(self.h, C.byref(o), p0, n, _ip(r["info"]), _dp(r["elbo"]), _ip(r["kept"]), _dp(r["q"]) if m else None,
                                               _dp(r["lp"]) if m else None, _dp(r["lq"]) if m else None, None if tx is None else _dp(tx),
                                               None if tg is None else _dp(tg)))
        if trajectory:
            r.update(x=tx, g=tg)
        return self._pathfinder_result(r, n, m)

    def pathfinder_path(self, x, g, L=None, u_elbo=None, u_draws=None, want=None, opts=None, **fields):
        """potus_pathfinder_path: pathfinder() from the caller's trajectory x, g [paths, rows, D] (or [rows, D]) with lengths L [paths]
        (default rows - 1), no optimiser run.  u_elbo [paths, rows - 1, num_elbo_draws, D], u_draws [paths, num_draws, D]: the caller's
        standard normals.  want [paths]: the iterate whose mu, alpha [paths, D] and log_det [paths] are also returned, with phi [paths, draws, D] and
        lq_want [paths, draws], the draws that iterate gives from the final normals, and qtq [paths, 20, 20], Q'Q of its thin QR (NaN beyond 2j)."""
        o = opts if opts is not None else self.pathfinder_opts(**fields)
        x, g = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (x, g))
        if x.ndim == 2:
            x, g = x[None], g[None]
        if x.ndim != 3 or x.shape != g.shape or x.shape[2] != self.D:
            raise ValueError(f"pathfinder_path: x {x.shape} and g {g.shape}, [paths, rows, {self.D}] expected of both")
        n, rows, m, K = x.shape[0], x.shape[1], max(int(o.num_draws), 0), int(o.num_elbo_draws)
        Lv = np.ascontiguousarray(np.full(n, rows - 1) if L is None else np.asarray(L).reshape(-1), dtype=np.int32)
        if Lv.shape != (n,):
            raise ValueError(f"pathfinder_path: L has {Lv.size} entries, {n} expected")
        pe = pd = pw = None
        if u_elbo is not None:
            u_elbo = np.ascontiguousarray(np.asarray(u_elbo, dtype=np.float64))
            if u_elbo.size != n * (rows - 1) * K * self.D:
                raise ValueError(f"pathfinder_path: u_elbo has shape {u_elbo.shape}, [{n}, {rows - 1}, {K}, {self.D}] expected")
            pe = _dp(u_elbo)
        if u_draws is not None:
            u_draws = np.ascontiguousarray(np.asarray(u_draws, dtype=np.float64))
            if u_draws.size != n * m * self.D:
                raise ValueError(f"pathfinder_path: u_draws has shape {u_draws.shape}, [{n}, {m}, {self.D}] expected")
            pd = _dp(u_draws)
        r = self._pathfinder_out(n, rows, m)
        mu = al = ld = ph = lw = qq = None
        if want is not None:
            want = np.ascontiguousarray(np.broadcast_to(np.asarray(want), (n,)), dtype=np.int32)
            pw, mu, al, ld = _ip(want), np.zeros((n, self.D)), np.zeros((n, self.D)), np.zeros(n)
            ph, lw, qq = np.zeros((n, m, self.D)), np.zeros((n, m)), np.full((n, 20, 20), np.nan)
        _check(self.L, self.L.potus_pathfinder_path(self.h, C.byref(o), _dp(x), _dp(g), _ip(Lv), rows, n, pe, pd, pw, _ip(r["info"]), _dp(r["elbo"]),
                                                    _ip(r["kept"]), _dp(r["q"]) if m else None, _dp(r["lp"]) if m else None, _dp(r["lq"]) if m else None,
                                                    None if mu is None else _dp(mu), None if al is None else _dp(al), None if ld is None else _dp(ld),
                                                    _dp(ph) if ph is not None and m else None, _dp(lw) if lw is not None and m else None,
                                                    None if qq is None else _dp(qq)))
        if want is not None:
            r.update(mu=mu, alpha=al, log_det=ld, phi=ph, lq_want=lw, qtq=qq)
        return self._pathfinder_result(r, n, m)

    def _pathfinder_block(self, what):
        shape = getattr(self, "_pathfinder_shape", None)
        if not shape or not shape[1]:
            raise PotusError(f"{what}: no Pathfinder draws on this handle (pathfinder(...) with num_draws >= 1 first)")
        return shape

    def pathfinder_rows_device(self, cols=None):
        """potus_pathfinder_write_array_device: the CmdStan output columns (begin, end) (default: all) of the last pathfinder call's draws, a
        torch tensor [paths * draws, end - begin] on this handle's GPU."""
        import torch
        n, m = self._pathfinder_block("pathfinder_rows_device")
        a, b = (0, self.n_cols) if cols is None else (int(cols[0]), int(cols[1]))
        out = torch.empty((n * m, max(b - a, 1)), dtype=torch.float64, device=f"cuda:{self.opts.device}")
        torch.cuda.current_stream(out.device).synchronize()
        _check(self.L, self.L.potus_pathfinder_write_array_device(self.h, a, b, C.c_void_p(out.data_ptr())))
        return out

    def pathfinder_scores(self, days=None):
        """potus_pathfinder_scores_device: predicted_score of the days (begin, end) (0-based, default: election day) of the last pathfinder
        call's draws, a torch tensor [paths, draws, days, S] on this handle's GPU."""
        import torch
        n, m = self._pathfinder_block("pathfinder_scores")
        S = int(self.data["S"])
        t0, t1 = self._day_range(days)
        out = torch.empty((n, m, max(t1 - t0, 1), S), dtype=torch.float64, device=f"cuda:{self.opts.device}")
        torch.cuda.current_stream(out.device).synchronize()
        _check(self.L, self.L.potus_pathfinder_scores_device(self.h, t0, t1, C.c_void_p(out.data_ptr())))
        return out

    def pathfinder_summary(self, ev, days=None, ev_to_win=270):
        """potus_pathfinder_summary: laplace_summary with the paths of the last pathfinder call in the place of modes."""
        n, _ = self._pathfinder_block("pathfinder_summary")
        S = int(self.data["S"])
        t0, t1 = self._day_range(days)
        nd = max(t1 - t0, 0)
        ev = np.ascontiguousarray(ev, dtype=np.float64).reshape(S)
        st, na, eo, cnt = np.zeros((n, nd, S, 4)), np.zeros((n, nd, 4)), np.zeros((n, nd, 5)), np.zeros(n, np.int32)
        _check(self.L, self.L.potus_pathfinder_summary(self.h, t0, t1, _dp(ev), int(ev_to_win), _dp(st), _dp(na), _dp(eo), _ip(cnt)))
        return dict(state=st, national=na, electoral_votes=eo, n_draws=cnt)

    def pathfinder_timing(self):
        """Milliseconds (HIP events) of the stages of this thread's last pathfinder call: L-BFGS, alpha, ELBO, draws."""
        ms = np.zeros(4)
        _check(self.L, self.L.potus_pathfinder_timing(_dp(ms)))
        return dict(lbfgs_ms=float(ms[0]), alpha_ms=float(ms[1]), elbo_ms=float(ms[2]), draws_ms=float(ms[3]))

    def variational_opts(self, **opts):
        """potus_default_advi_opts with the given fields replaced: algorithm ("meanfield"; "fullrank" is refused by the library), iter,
        grad_samples, elbo_samples, eval_elbo, adapt_engaged, adapt_iter, output_samples, draw_offset, run_offset, eta, tol_rel_obj, elbo_offset."""
        o = _abi.PotusAdviOpts()
        self.L.potus_default_advi_opts(C.byref(o))
        for k, v in opts.items():
            if k == "algorithm":
                o.algorithm = _abi.ADVI_ALGORITHMS[v] if isinstance(v, str) else int(v)
            elif k in ("eta", "tol_rel_obj", "elbo_offset"):
                setattr(o, k, float(v))
            elif k in ("iter", "grad_samples", "elbo_samples", "eval_elbo", "adapt_engaged", "adapt_iter", "output_samples", "draw_offset", "run_offset"):
                setattr(o, k, int(v))
            else:
                raise TypeError(f"unknown ADVI option {k!r}")
        return o

    def variational(self, q0=None, runs=None, opts=None, **fields):
        """potus_advi: mean-field ADVI from every start (q0 [runs, D], or None for `runs` library starts).  On a handle with data sets run r
        uses data set r // (runs // n_datasets).  fields: see variational_opts (or opts: a filled struct).  Returns dict(mu, omega [runs, D],
        elbo [runs, iter // eval_elbo + 1] (the initial ELBO first, NaN behind the end), adapt_elbo [runs, 5], q [runs, draws, D], lp, lq
        [runs, draws], return_code, flags, iterations, eta_index, eta, model_passes, evaluations [runs])."""
        o = opts if opts is not None else self.variational_opts(**fields)
        p0 = None
        if q0 is not None:
            q0 = np.ascontiguousarray(np.atleast_2d(q0), dtype=np.float64)
            if q0.shape[1] != self.D or (runs is not None and int(runs) != q0.shape[0]):
                raise ValueError(f"variational: q0 has shape {q0.shape}, [{runs if runs is not None else 'runs'}, {self.D}] expected")
            runs, p0 = q0.shape[0], _dp(q0)
        n, m = int(1 if runs is None else runs), max(int(o.output_samples), 0)
        nn, trace = max(n, 0), max(int(o.iter), 0) // max(int(o.eval_elbo), 1) + 1
        info = np.zeros((nn, 6), np.int32)
        r = dict(mu=np.zeros((nn, self.D)), omega=np.zeros((nn, self.D)), elbo=np.zeros((nn, trace)), adapt_elbo=np.zeros((nn, 5)),
                 q=np.zeros((nn, m, self.D)), lp=np.zeros((nn, m)), lq=np.zeros((nn, m)))
        _check(self.L, self.L.potus_advi(self.h, C.byref(o), p0, n, _ip(info), _dp(r["mu"]), _dp(r["omega"]), _dp(r["elbo"]), _dp(r["adapt_elbo"]),
                                         _dp(r["q"]) if m else None, _dp(r["lp"]) if m else None, _dp(r["lq"]) if m else None))
        self._variational_shape = (n, m)
        eta = np.array([_abi.ADVI_ETAS[k] if k >= 0 else (float(o.eta) if not o.adapt_engaged else np.nan) for k in info[:, 3]])
        r.update(return_code=info[:, 0].copy(), flags=info[:, 1].copy(), iterations=info[:, 2].copy(), eta_index=info[:, 3].copy(), eta=eta,
                 model_passes=info[:, 4].copy(), evaluations=info[:, 5].copy())
        return r

    def _variational_block(self, what):
        shape = getattr(self, "_variational_shape", None)
        if not shape or not shape[1]:
            raise PotusError(f"{what}: no ADVI draws on this handle (variational(...) with output_samples >= 1 first)")
        return shape

    def variational_rows_device(self, cols=None):
        """potus_advi_write_array_device: the CmdStan output columns (begin, end) (default: all) of the last variational call's draws, a
        torch tensor [runs * draws, end - begin] on this handle's GPU."""
        import torch
        n, m = self._variational_block("variational_rows_device")
        a, b = (0, self.n_cols) if cols is None else (int(cols[0]), int(cols[1]))
        out = torch.empty((n * m, max(b - a, 1)), dtype=torch.float64, device=f"cuda:{self.opts.device}")
        torch.cuda.current_stream(out.device).synchronize()
        _check(self.L, self.L.potus_advi_write_array_device(self.h, a, b, C.c_void_p(out.data_ptr())))
        return out

    def variational_scores(self, days=None):
        """potus_advi_scores_device: predicted_score of the days (begin, end) (0-based, default: election day) of the last variational
        call's draws, a torch tensor [runs, draws, days, S] on this handle's GPU."""
        import torch
        n, m = self._variational_block("variational_scores")
        S = int(self.data["S"])
        t0, t1 = self._day_range(days)
        out = torch.empty((n, m, max(t1 - t0, 1), S), dtype=torch.float64, device=f"cuda:{self.opts.device}")
        torch.cuda.current_stream(out.device).synchronize()
        _check(self.L, self.L.potus_advi_scores_device(self.h, t0, t1, C.c_void_p(out.data_ptr())))
        return out

    def variational_summary(self, ev, days=None, ev_to_win=270):
        """potus_advi_summary: laplace_summary with the runs of the last variational call in the place of modes."""
        n, _ = self._variational_block("variational_summary")
        S = int(self.data["S"])
        t0, t1 = self._day_range(days)
        nd = max(t1 - t0, 0)
        ev = np.ascontiguousarray(ev, dtype=np.float64).reshape(S)
        st, na, eo, cnt = np.zeros((n, nd, S, 4)), np.zeros((n, nd, 4)), np.zeros((n, nd, 5)), np.zeros(n, np.int32)
        _check(self.L, self.L.potus_advi_summary(self.h, t0, t1, _dp(ev), int(ev_to_win), _dp(st), _dp(na), _dp(eo), _ip(cnt)))
        return dict(state=st, national=na, electoral_votes=eo, n_draws=cnt)

    def variational_timing(self):
        """Milliseconds (HIP events) of the stages of this thread's last variational call: adaptation, gradient segments, ELBO, draws."""
        ms = np.zeros(4)
        _check(self.L, self.L.potus_advi_timing(_dp(ms)))
        return dict(adapt_ms=float(ms[0]), grad_ms=float(ms[1]), elbo_ms=float(ms[2]), draws_ms=float(ms[3]))

    def simulate_prior(self, seed, n_sims, sim_offset=0):
        """potus_simulate_prior: (q [n_sims, D], n_democrat_state [n_sims, Ns], n_democrat_national [n_sims, Nn]) drawn from the prior
        predictive distribution of this handle's design (its poll outcomes are not used)."""
        Ns, Nn = int(self.data["N_state_polls"]), int(self.data["N_national_polls"])
        q = np.zeros((n_sims, self.D))
        ys, yn = np.zeros((n_sims, Ns), np.int32), np.zeros((n_sims, Nn), np.int32)
        _check(self.L, self.L.potus_simulate_prior(self.h, C.c_uint64(int(seed)), int(n_sims), int(sim_offset), _dp(q), _ip(ys), _ip(yn)))
        return q, ys, yn

    def constrain(self, q, col_begin=_abi.N_SAMPLER_COLS, col_end=None):
        """potus_constrain: output-row columns [col_begin, col_end) of unconstrained points q [n, D] (sampler columns are NaN)."""
        q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float64)
        assert q.shape[1] == self.D
        col_end = self.n_cols if col_end is None else int(col_end)
        out = np.zeros((q.shape[0], col_end - col_begin))
        _check(self.L, self.L.potus_constrain(self.h, _dp(q), q.shape[0], int(col_begin), col_end, _dp(out)))
        return out

    def sbc_ranks(self, truth, col_begin, col_end, thin=1):
        """potus_sbc_ranks: (less, equal) [n_datasets, col_end - col_begin] and L, the draws compared per data set."""
        nc = int(col_end) - int(col_begin)
        truth = np.ascontiguousarray(np.asarray(truth, dtype=np.float64).reshape(-1, nc))
        less, equal, L = np.zeros(truth.shape, np.int32), np.zeros(truth.shape, np.int32), C.c_int()
        _check(self.L, self.L.potus_sbc_ranks(self.h, _dp(truth), int(col_begin), int(col_end), int(thin), _ip(less), _ip(equal), C.byref(L)))
        return less, equal, L.value

    @property
    def n_polls(self):
        """Polls of the data: state polls, then national polls (the order of the logit_pi_democrat_* columns)."""
        return int(self.data["N_state_polls"]) + int(self.data["N_national_polls"])

    def post_warmup_saved(self):
        """Saved draws per chain that are not warm-up rows (save_warmup = 1 saves those too)."""
        n = self.draws_saved()
        return n - (min(n, self.opts.num_warmup) if self.opts.save_warmup else 0)

    def log_lik_device(self, poll_begin, poll_end, out, integrate=True):
        """potus_log_lik_device: per-poll log-likelihoods of the post-warm-up draws into a torch tensor on this handle's GPU
        ([poll_end - poll_begin, chains, draws], float64, contiguous).  integrate: each poll's own noise coordinate integrated out."""
        _device_block(out, "log_lik_device")
        want = (int(poll_end) - int(poll_begin)) * self.opts.chains * self.post_warmup_saved()
        if out.numel() != want:
            raise ValueError(f"tensor has {out.numel()} elements, {want} expected")
        _check(self.L, self.L.potus_log_lik_device(self.h, int(poll_begin), int(poll_end), int(bool(integrate)), C.c_void_p(out.data_ptr())))
        return out

    def loo_moment_match(self, loo, polls=None, model_handle=None, **opts):
        """loo.moment_match on this handle's draws: the Loo with the rows of the polls above the k-hat threshold moment-matched."""
        from .loo import moment_match
        return moment_match(self, loo, polls=polls, model_handle=model_handle, **opts)

    def poll_share_device(self, poll_begin, poll_end, integrate=True):
        """potus_poll_share_device: (a1, a2) = E_z[p], E_z[p^2] of the polls at the post-warm-up draws, two torch tensors [polls, chains,
        draws] on this handle's GPU; p = inv_logit(eta + sigma z), z the draw's own noise coordinate or (integrate) integrated out."""
        import torch
        shape = (int(poll_end) - int(poll_begin), self.opts.chains, self.post_warmup_saved())
        a1 = torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.opts.device}")
        a2 = torch.empty_like(a1)
        torch.cuda.current_stream(a1.device).synchronize()
        _check(self.L, self.L.potus_poll_share_device(self.h, int(poll_begin), int(poll_end), int(bool(integrate)), C.c_void_p(a1.data_ptr()), C.c_void_p(a2.data_ptr())))
        return a1, a2

    def poll_rep_device(self, poll_begin, poll_end, integrate=True, rep=0):
        """potus_poll_rep_device: replicated outcomes y_rep of the polls at the post-warm-up draws, a torch tensor [polls, chains, draws]
        (float64) on this handle's GPU; integrate: a fresh noise coordinate per cell (a new poll), else the draw's own (the same poll again)."""
        import torch
        shape = (int(poll_end) - int(poll_begin), self.opts.chains, self.post_warmup_saved())
        yr = torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.opts.device}")
        torch.cuda.current_stream(yr.device).synchronize()
        _check(self.L, self.L.potus_poll_rep_device(self.h, int(poll_begin), int(poll_end), int(bool(integrate)), int(rep), C.c_void_p(yr.data_ptr())))
        return yr

    def ppc(self, **kw):
        """ppc.check on this handle's draws: PIT, LOO-PIT and the grouped posterior predictive p-values."""
        from .ppc import check
        return check(self, **kw)

    def loo_predict(self, **kw):
        """loo.predict on this handle's draws: the leave-one-out predictive mean and sd of every poll's share (plain PSIS weights)."""
        from .loo import predict
        return predict(self, **kw)

    def loo_influence(self, ev, **kw):
        """loo.influence on this handle's draws: what leaving each poll out does to the forecast (plain PSIS weights)."""
        from .loo import influence
        return influence(self, ev, **kw)

    def _cv_masks(self, held_state, held_national):
        """The two masks as contiguous int32 [n_datasets, polls] arrays (None where the data have no such polls)."""
        n = self.n_datasets
        out = []
        for m, key in ((held_state, "N_state_polls"), (held_national, "N_national_polls")):
            w = int(self.data[key])
            a = np.ascontiguousarray(np.asarray(m).reshape(-1, w) != 0, dtype=np.int32) if w else np.zeros((n, 0), np.int32)
            if a.shape[0] != n:
                raise ValueError(f"cross-validation mask for {a.shape[0]} data sets, the handle holds {n}")
            out.append(a)
        return n, out[0], out[1]

    def cv_log_lik_device(self, held_state, held_national, integrate=True):
        """potus_cv_log_lik_device: log p(y | n, draw) of every (data set, poll) pair the masks [n_datasets, polls] name, over the data set's
        post-warm-up draws, as a torch tensor [pairs, draws per data set] on this handle's GPU; pairs by data set, then state polls, then
        national polls."""
        import torch
        n, ms, mn = self._cv_masks(held_state, held_national)
        np_ = C.c_longlong(0)
        _check(self.L, self.L.potus_cv_log_lik_device(self.h, _ip(ms), _ip(mn), int(bool(integrate)), None, C.byref(np_)))
        per = (self.opts.chains // n) * self.post_warmup_saved()
        out = torch.empty((np_.value, per), dtype=torch.float64, device=f"cuda:{self.opts.device}")
        if np_.value:                                      # (an empty tensor has no memory to point at)
            torch.cuda.current_stream(out.device).synchronize()
            _check(self.L, self.L.potus_cv_log_lik_device(self.h, _ip(ms), _ip(mn), int(bool(integrate)), C.c_void_p(out.data_ptr()), None))
        return out

    def cv_lpd(self, held_state, held_national, integrate=True):
        """potus_cv_lpd: (lpd [n_datasets, polls, 2] = log mean p and log mean p^2 of every pair the masks name over the data set's post-warm-up
        draws, NaN elsewhere; n_draws [n_datasets], 0 for a data set with a failed chain)."""
        n, ms, mn = self._cv_masks(held_state, held_national)
        lpd, cnt = np.zeros((n, self.n_polls, 2)), np.zeros(n, np.int32)
        _check(self.L, self.L.potus_cv_lpd(self.h, _ip(ms), _ip(mn), int(bool(integrate)), _dp(lpd), _ip(cnt)))
        return lpd, cnt

    def cv_timing(self):
        ms = np.zeros(2)
        _check(self.L, self.L.potus_cv_timing(_dp(ms)))
        return dict(loglik_ms=float(ms[0]), reduce_ms=float(ms[1]))

    def outcomes(self, ev, actual=None, days=None, ev_to_win=270):
        """Joint election outcomes of this handle's post-warm-up draws (us_potus_model_amd.outcomes)."""
        from .outcomes import outcomes
        return outcomes([self], ev, actual=actual, days=days, ev_to_win=ev_to_win)

    def scenario(self, ev=None, given=None, day=-1, days=None, ev_to_win=270, states=None):
        """Mean, covariance and joint outcomes of this handle's post-warm-up draws that meet a condition (us_potus_model_amd.scenario)."""
        from .scenario import scenario
        return scenario([self], ev=ev, given=given, day=day, days=days, ev_to_win=ev_to_win, states=states)

    def forecast_scores(self, ev, actual, **kw):
        """CRPS, energy, variogram and Dawid-Sebastiani scores of this handle's post-warm-up draws against the result (us_potus_model_amd.scoring.score)."""
        from .scoring import score
        return score([self], ev, actual, **kw)

    def monitor(self, pars=None, cols=None, probs=(0.025, 0.25, 0.5, 0.75, 0.975)):
        """The summary table of this handle's post-warm-up draws: mean, sd, mad, mcse, R-hat, ESS, quantiles (us_potus_model_amd.monitor)."""
        from .monitor import monitor
        return monitor([self], pars=pars, cols=cols, probs=probs)

    def write_stan_csv(self, directory, basename="poll_model_2020"):
        os.makedirs(directory, exist_ok=True)
        _check(self.L, self.L.potus_write_stan_csv(self.h, str(directory).encode(), basename.encode()))
        off = self.opts.chain_id_offset
        return [str(Path(directory) / f"{basename}-{off + c + 1}.csv") for c in range(self.opts.chains)]


def _handle_ids(handles):
    """(the handles as a list, their ids as the C int array a pooled entry point takes): one handle or a list / tuple of them."""
    hs = list(handles) if isinstance(handles, (list, tuple)) else [handles]
    return hs, (C.c_int * len(hs))(*[h.h for h in hs])


def _device_block(block, who, axes=None):
    """What a *_device entry point may be handed: a contiguous float64 torch tensor on a GPU, with the axes named (any shape when None).
    The library works on its own stream, so the tensor's current stream is synchronised here."""
    import torch
    if not (block.is_cuda and block.dtype == torch.float64 and block.is_contiguous() and (axes is None or block.dim() == len(axes))):
        raise TypeError(f"{who} needs a contiguous float64 {'' if axes is None else '[' + ', '.join(axes) + '] '}tensor on the GPU")
    torch.cuda.current_stream(block.device).synchronize()


def posterior_summary(handles, ev):
    """potus_posterior_summary_many: the summaries of final_2016.R:708-762, 799-823 over the pooled draws of every
    listed handle (the chains of one posterior, on one GPU or several)."""
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    S, T = int(h0.data["S"]), int(h0.data["T"])
    ev = np.ascontiguousarray(ev, dtype=np.float64).reshape(S)
    st, na, eo = np.zeros((S, T, 4)), np.zeros((T, 4)), np.zeros((T, 5))
    _check(h0.L, h0.L.potus_posterior_summary_many(ids, len(hs), _dp(ev), _dp(st), _dp(na), _dp(eo)))
    return dict(state=np.ascontiguousarray(st.transpose(1, 0, 2)), national=na, electoral_votes=eo)


def run_pooled(handles, n_iter, coll_device=None):
    """potus_run_many for dense samplers with pooled_metric = 2 (one posterior, its chains spread over several handles / GPUs / ranks): every window end is
    pooled over ALL of them before it is finished -- the handles of this process by adding their moments on the first handle's GPU, the ranks of an initialised
    torch.distributed group by all-reduces (RCCL over xGMI when coll_device is a GPU; parallel.pool_window_moments) -- so that every GPU ends up with the
    same inverse metric, estimated from the window draws of every chain of the job.  A declared deviation from Stan (potus_opts.pooled_metric)."""
    import torch
    from . import parallel
    left = int(n_iter)
    while left > 0:
        it0 = handles[0].iterations_done()
        run_many(handles, left)
        done = handles[0].iterations_done() - it0
        left -= done
        wins = [h.pool_window() for h in handles]
        if not any(w[0] for w in wins):
            if done == 0:
                break                                      # the sampler has run all its iterations
            continue
        if not all(w[0] for w in wins):
            raise PotusError("run_pooled: the handles do not share a warm-up schedule (a window end is pending on some of them only)")
        dev0 = wins[0][2].device
        cnt = float(sum(w[1] for w in wins))
        msum = sum((w[1] * w[2]).to(dev0) for w in wins)                       # sum of count x mean over this process's handles
        n_tot, gmean = parallel.pool_window_mean(cnt, msum, coll_device)       # ... and over the ranks
        for _, c, mean, m2 in wins:                                           # Chan: M2 += count (mean - pooled mean)(mean - pooled mean)'
            d = mean - gmean.to(mean.device)
            m2[:, :mean.numel()].addr_(d, d, alpha=c)
        total = wins[0][3]
        for w in wins[1:]:
            total += w[3].to(dev0)
        parallel.pool_window_m2(total, coll_device)                            # in place: the sum over the ranks
        for w in wins[1:]:
            w[3].copy_(total)
        torch.cuda.synchronize()
        for h in handles:
            h.pool_finish(n_tot)


def device_diagnostics(handles, col_begin, col_end):
    """potus_diagnostics: rank-normalised split R-hat and bulk ESS of columns [col_begin, col_end) of the output row over the pooled
    chains of the listed handles (one posterior), computed on the first handle's GPU.  Returns (rhat, ess_bulk), each [col_end - col_begin]."""
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    n = int(col_end) - int(col_begin)
    rhat, ess = np.zeros(n), np.zeros(n)
    _check(h0.L, h0.L.potus_diagnostics(ids, len(hs), int(col_begin), int(col_end), _dp(rhat), _dp(ess)))
    return rhat, ess


def _need_check_convergence(L):
    """A development build selected through POTUS_LIB may predate the export: say so up front, with the library's name, instead of an
    AttributeError in the middle of a run whose warm-up has already been paid for."""
    if not hasattr(L, "potus_check_convergence"):
        raise PotusError(f"{lib_path()} does not export potus_check_convergence (an older development build?): rhat_stop / check_convergence need it")


def check_convergence(handles, rhat_below=1.01, ess_at_least=400.0):
    """potus_check_convergence: (converged, rhat_max, ess_bulk_min) of lp__ and mu_b[:, T] over the post-warm-up draws the pooled chains of
    the handles have saved so far (the online early-stop check of SURVEY 8(f4); a deviation from Stan when acted upon)."""
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    _need_check_convergence(h0.L)
    conv, r, e = C.c_int(0), C.c_double(), C.c_double()
    _check(h0.L, h0.L.potus_check_convergence(ids, len(hs), C.c_double(rhat_below), C.c_double(ess_at_least), C.byref(conv), C.byref(r), C.byref(e)))
    return bool(conv.value), r.value, e.value


def device_diagnostics_of_block(block):
    """potus_diagnostics_device on a torch tensor [draws, chains, columns] (float64, contiguous, on a GPU) -- e.g. the result of the
    all-gather of potus_write_array_device blocks.  Returns (rhat, ess_bulk) as numpy arrays [columns]."""
    _device_block(block, "device_diagnostics_of_block", ("draws", "chains", "columns"))
    L = load_library()
    nd, nc, ncol = (int(x) for x in block.shape)
    rhat, ess = np.zeros(ncol), np.zeros(ncol)
    _check(L, L.potus_diagnostics_device(int(block.device.index or 0), C.c_void_p(block.data_ptr()), nd, nc, ncol, _dp(rhat), _dp(ess)))
    return rhat, ess


def backtest_scores(summary, ev, won, day=0):
    """final_2016.R:925-945: (EV-weighted Brier, unweighted Brier, states called correctly) from the `state` block of
    a posterior summary; `won` = 1 where the Democrat carried the state; day: 1-based, 0 = election day (the last)."""
    L = load_library()
    st = np.ascontiguousarray(np.asarray(summary["state"], dtype=np.float64).transpose(1, 0, 2))    # [S][T][4]: cell t + T*s
    S, T = st.shape[0], st.shape[1]
    ev = np.ascontiguousarray(ev, dtype=np.float64).reshape(S)
    w = (C.c_int * S)(*[int(x) for x in won])
    out = np.zeros(3)
    _check(L, L.potus_backtest_scores(_dp(st), T, S, int(day), _dp(ev), w, _dp(out)))
    return dict(ev_wtd_brier=float(out[0]), unwtd_brier=float(out[1]), states_correct=int(out[2]))


def plan_layout(chains, T, n_cus=256, cus_per_chain=0, twin=-1, metric="diag_e", one_workgroup_ok=True):
    """(workgroups per chain, clusters / workgroups per chain side count) as potus_create would first plan them for a device of
    n_cus compute units -- potus_plan_cus_per_chain + potus_plan_sides, no device needed."""
    L = load_library()
    k, low, sides = C.c_int(0), C.c_int(0), C.c_int(0)
    m = _abi.METRICS[metric] if isinstance(metric, str) else int(metric)
    _check(L, L.potus_plan_cus_per_chain(chains, T, n_cus, cus_per_chain, twin, m, int(bool(one_workgroup_ok)), C.byref(k), C.byref(low)))
    _check(L, L.potus_plan_sides(chains, k.value, n_cus, 1, cus_per_chain, twin, m, C.byref(sides)))
    K = k.value
    if sides.value == 1 and low.value:
        K = 16                                      # the smaller clusters were chosen for the sake of the second one
    return K, sides.value


def run_many(handles, n_iter):
    """potus_run_many: advance several handles (other posteriors, other GPUs) concurrently from one host thread."""
    if not handles:
        return
    hs, ids = _handle_ids(handles)
    _check(hs[0].L, hs[0].L.potus_run_many(ids, len(hs), int(n_iter)))


class StanFit:
    """What the scripts use of rstan's stanfit: extract(pars), model_name, sampler params."""

    def __init__(self, handle, model_name: str):
        # one handle, or one per device holding consecutive blocks of chains (PotusModel.sample(devices=...))
        self._hs = list(handle) if isinstance(handle, (list, tuple)) else [handle]
        self._h = self._hs[0]
        self.model_name = model_name  # out@model_name, final_2016.R:825
        # only the 7 sampler columns come to the host here (through write_array); the unconstrained draws
        # (chains x draws x D doubles: 1 GB for the 2016 run) stay on the device until unconstrained() asks for them
        self.n_saved = self._hs[0].draws_saved()
        self.chains = sum(h.opts.chains for h in self._hs)
        self._sampler = np.transpose(self._write_array(0, _abi.N_SAMPLER_COLS), (1, 0, 2))       # [chain, draw, 7]
        self._draws = None

    def _write_array(self, a, b):
        """[iter, chain, b - a] over all devices, chains in id order."""
        return np.concatenate([h.write_array(a, b, self.n_saved) for h in self._hs], axis=1)

    def sampler_params(self):
        """dict of [chains, draws] arrays: lp__, accept_stat__, ... (rstan::get_sampler_params)."""
        return {n: self._sampler[:, :, i] for i, n in enumerate(_abi.SAMPLER_COLS)}

    def unconstrained(self):
        """[chains, draws, D] on the unconstrained scale (copied from the devices on first use)."""
        if self._draws is None:
            self._draws = np.concatenate([h.draws() for h in self._hs], axis=0)
        return self._draws[:, :, _abi.N_SAMPLER_COLS:]

    def summary(self, ev):
        """Device-side posterior summaries over all chains of the fit (see posterior_summary)."""
        return posterior_summary(self._hs, ev)

    def loo(self, integrate=True, r_eff=None):
        """fit$loo(): PSIS-LOO of the polls over every chain of the fit, on the device (us_potus_model_amd.loo)."""
        from .loo import loo
        return loo(self._hs, integrate=integrate, r_eff=r_eff, name=self.model_name)

    def ppc(self, **kw):
        """Posterior predictive checks over every chain of the fit, on the device (us_potus_model_amd.ppc.check)."""
        from .ppc import check
        return check(self._hs, **kw)

    def outcomes(self, ev, actual=None, days=None, ev_to_win=270):
        """EV histogram, tipping point, joint win counts and p-values over every chain of the fit, on the device (us_potus_model_amd.outcomes)."""
        from .outcomes import outcomes
        return outcomes(self._hs, ev, actual=actual, days=days, ev_to_win=ev_to_win)

    def scenario(self, ev=None, given=None, day=-1, days=None, ev_to_win=270, states=None):
        """The forecast given an event, and the covariance / correlation of the state scores, over every chain of the fit (us_potus_model_amd.scenario)."""
        from .scenario import scenario
        return scenario(self._hs, ev=ev, given=given, day=day, days=days, ev_to_win=ev_to_win, states=states)

    def forecast_scores(self, ev, actual, **kw):
        """Proper scoring rules of the joint forecast against the result, over every chain of the fit (us_potus_model_amd.scoring.score)."""
        from .scoring import score
        return score(self._hs, ev, actual, **kw)

    def monitor(self, pars=None, cols=None, probs=(0.025, 0.25, 0.5, 0.75, 0.975)):
        """fit$summary() / print(stanfit) / rstan::monitor over every chain of the fit, on the device (us_potus_model_amd.monitor)."""
        from .monitor import monitor
        return monitor(self._hs, pars=pars, cols=cols, probs=probs)

    def extract(self, pars, permuted=False):
        """rstan::extract(out, pars=)[[1]]: array [draws, ...dims], chains merged.

        rstan additionally permutes the merged draws at random; the summaries the scripts
        take (means, quantiles, P(>0.5): final_2016.R:708-762) are permutation invariant, so
        the default keeps chain-major order.
        """
        single = isinstance(pars, str)
        names = [pars] if single else list(pars)
        out = {}
        for name in names:
            if name in _abi.SAMPLER_COLS:
                out[name] = self._sampler[:, :, _abi.SAMPLER_COLS.index(name)].reshape(-1)
                continue
            if name not in self._h.layout:
                raise KeyError(f"unknown parameter {name!r}")
            a, b, dims = self._h.layout[name]
            arr = self._write_array(a, b)                            # [iter, chain, n]
            arr = np.transpose(arr, (1, 0, 2)).reshape(self.chains * self.n_saved, b - a)
            if dims:
                arr = arr.reshape((arr.shape[0],) + tuple(reversed(dims))).transpose(
                    (0,) + tuple(range(len(dims), 0, -1)))            # column-major -> [draw, *dims]
            else:
                arr = arr[:, 0]
            out[name] = arr
        if permuted:
            perm = np.random.default_rng(self._h.opts.seed).permutation(self.chains * self.n_saved)
            out = {k: v[perm] for k, v in out.items()}
        return out[pars] if single else out

    def as_array(self, pars):
        """as.array(stanfit)[, , pars]: [iterations, chains, columns]."""
        a, b, _ = self._h.layout[pars]
        return self._write_array(a, b)

    def output_files(self, directory, basename=None):
        """fit$output_files(): writes CmdStan CSVs for rstan::read_stan_csv (final_2016.R:543)."""
        files = []
        for h in self._hs:                           # files are numbered by global chain id
            files += h.write_stan_csv(directory, basename or self.model_name.replace("_model", ""))
        return files


class Optimum:
    """What cmdstanr's fit$optimize() returns, for `paths` starts at once: q [paths, D] (unconstrained), lp, grad_norm, return_code
    (_abi.OPTIMIZE_CODES), iterations, grad_evals [paths]; `best` = the path with the highest lp among those that ended with a
    convergence code (1-5), else among all that have a point.  The constrained values are built on first use (Handle.constrain)."""

    def __init__(self, handle, res, jacobian):
        self._h, self.jacobian = handle, bool(jacobian)
        self.q, self.lp, self.grad_norm = res["q"], res["lp"], res["grad_norm"]
        self.return_code, self.iterations, self.grad_evals = res["return_code"], res["iterations"], res["grad_evals"]
        conv = (self.return_code >= 1) & (self.return_code <= 5)
        pool = conv if conv.any() else np.isfinite(self.lp)
        if not pool.any():
            raise PotusError("optimize: no path found a finite starting point (return code INIT on every path)")
        self.best = int(np.flatnonzero(pool)[np.argmax(self.lp[pool])])
        self._row = None

    @property
    def codes(self):
        return [_abi.OPTIMIZE_CODES.get(int(c), str(int(c))) for c in self.return_code]

    def mle(self, par, path=None):
        """fit$mle(par): the constrained values of one path (default: best), shaped as extract() shapes a single draw."""
        if par == "lp__":
            return float(self.lp[self.best if path is None else int(path)])
        if par not in self._h.layout:
            raise KeyError(f"unknown parameter {par!r}")
        if self._row is None:
            self._row = self._h.constrain(self.q, 0, self._h.n_cols)
        a, b, dims = self._h.layout[par]
        v = self._row[self.best if path is None else int(path), a:b]
        if not dims:
            return float(v[0])
        return v.reshape(tuple(reversed(dims))).transpose(tuple(range(len(dims) - 1, -1, -1))).copy()    # column-major -> dims

    def as_inits(self, chains):
        """[chains, D]: the best path's point for every chain (Handle.init(q0) / PotusModel.sample(inits=))."""
        return np.tile(self.q[self.best], (int(chains), 1))

    def close(self):
        self._h.close()


class Laplace:
    """What cmdstanr's model$laplace() returns for one mode: q [draws, D] (unconstrained draws of N(mode, P^-1), P = minus the Hessian of
    log_prob<jacobian> at the mode), lp (log_prob<jacobian = true> of every draw, as the sampler's lp__), lp_approx = -1/2 |u|^2,
    log_ratio = lp - lp(mode) - lp_approx (the log importance ratio of the draw up to a constant), log_det = log det P, grad_norm at the
    mode, return_code (_abi.LAPLACE_CODES).  The draws' rows stay on the handle: scores / summary / outcomes / scenario work on them there."""

    def __init__(self, handle, mode, res, lp_mode, jacobian):
        self._h, self.mode, self.jacobian = handle, np.asarray(mode, dtype=np.float64).reshape(-1), bool(jacobian)
        self.return_code = int(res["return_code"][0])
        if self.return_code != 0:
            raise PotusError(f"laplace: the mode has no Laplace approximation (return code {_abi.LAPLACE_CODES.get(self.return_code, self.return_code)}: "
                             "minus the Hessian is not positive definite there, or the point is not finite)")
        self.q, self.lp, self.lp_approx = res["q"][0], res["lp"][0], res["lp_approx"][0]
        self.log_det, self.grad_norm, self.min_pivot = float(res["log_det"][0]), float(res["grad_norm"][0]), float(res["min_pivot"][0])
        self.lp_mode = float(lp_mode)
        self.log_ratio = self.lp - self.lp_mode - self.lp_approx
        self._row = self._k = None

    def draws(self, par):
        """fit$draws(par): the constrained values of every draw, shaped as Optimum.mle shapes one, with a leading draw axis."""
        if par == "lp__":
            return self.lp.copy()
        if par == "lp_approx__":
            return self.lp_approx.copy()
        if par not in self._h.layout:
            raise KeyError(f"unknown parameter {par!r}")
        if self._row is None:
            self._row = self._h.laplace_rows_device().cpu().numpy()
        a, b, dims = self._h.layout[par]
        v = self._row[:, a:b]
        if not dims:
            return v[:, 0].copy()
        nd = len(dims)
        return v.reshape((v.shape[0],) + tuple(reversed(dims))).transpose((0,) + tuple(range(nd, 0, -1))).copy()    # column-major -> dims

    @property
    def pareto_k(self):
        """k-hat of the importance ratios: the library's PSIS (potus_loo_device) on a one-column block whose log-likelihood is -log_ratio."""
        if self._k is None:
            import torch
            from .loo import loo_of_block
            blk = torch.as_tensor(-self.log_ratio, device=f"cuda:{self._h.opts.device}").reshape(1, 1, -1).contiguous()
            self._k = float(loo_of_block(blk).pareto_k[0])
        return self._k

    def scores(self, days=None):
        """predicted_score of `days` = (begin, end) (0-based; default election day) of every draw: a torch tensor [draws, days, S] on the GPU."""
        return self._h.laplace_scores(days)[0]

    def summary(self, ev, days=None, ev_to_win=270):
        """timeline()'s summaries over the draws: dict(state [days, S, 4], national [days, 4], electoral_votes [days, 5], n_draws)."""
        r = self._h.laplace_summary(ev, days, ev_to_win)
        return dict(state=r["state"][0], national=r["national"][0], electoral_votes=r["electoral_votes"][0], n_draws=int(r["n_draws"][0]))

    def outcomes(self, ev, actual=None, days=None, ev_to_win=270, states=None):
        """Joint election outcomes over the draws (potus_outcomes_device on their scores)."""
        from .outcomes import outcomes_of_block
        return outcomes_of_block(self.scores(days).contiguous(), self._h.data["state_weights"], ev, actual=actual, ev_to_win=ev_to_win, states=states)

    def scenario(self, ev=None, given=None, day=-1, days=None, ev_to_win=270, states=None):
        """Conditional forecast over the draws (potus_scenario_device on their scores); `day` indexes the range `days`."""
        from .scenario import scenario_of_block
        return scenario_of_block(self.scores(days).contiguous(), self._h.data["state_weights"], ev=ev, given=given, day=day, ev_to_win=ev_to_win, states=states)

    def forecast_scores(self, ev, actual, days=None, **kw):
        """Proper scoring rules of the draws against the result (us_potus_model_amd.scoring.score_of_block on their scores)."""
        from .scoring import score_of_block
        T = int(self._h.data["T"])
        return score_of_block(self.scores(days).contiguous(), self._h.data["state_weights"], ev, actual, days=(T - 1, T) if days is None else days, **kw)

    def close(self):
        self._h.close()


class Pathfinder:
    """What cmdstanr's model$pathfinder(psis_resample = FALSE) returns: draws [paths * draws_per_path, D] (unconstrained, the pooled draws of
    every path, path-major), lp (log_prob<jacobian = true> of every draw, as the sampler's lp__), lq (the log density of the path's normal
    at the draw), log_ratio = lp - lq, and per path elbo (of its best iterate), best_iteration, iterations, return_code
    (_abi.PATHFINDER_CODES; a path without an ELBO has NaN draws).  The draws' rows stay on the handle for scores / summary / outcomes / scenario."""

    def __init__(self, handle, res):
        self._h, self.res = handle, res
        self.return_code, self.iterations, self.best_iteration = res["return_code"], res["iterations"], res["best_iteration"]
        self.paths, self.draws_per_path = res["q"].shape[0], res["q"].shape[1]
        if not (self.return_code == 0).any():
            raise PotusError("pathfinder: no path has an iterate with a finite ELBO (return code NO_ELBO on every path)")
        self.draws = res["q"].reshape(-1, res["q"].shape[2])
        self.lp, self.lq = res["lp"].reshape(-1), res["lq"].reshape(-1)
        self.log_ratio = self.lp - self.lq
        self.elbo = np.array([res["elbo"][p, l] if l > 0 else np.nan for p, l in enumerate(self.best_iteration)])
        self.elbo_path = res["elbo"]
        self._k = None

    @property
    def pareto_k(self):
        """k-hat of the importance ratios of the pooled draws: the library's PSIS (potus_loo_device), exactly as Laplace.pareto_k."""
        if self._k is None:
            import torch
            from .loo import loo_of_block
            lr = self.log_ratio[np.isfinite(self.log_ratio)]
            blk = torch.as_tensor(-lr, device=f"cuda:{self._h.opts.device}").reshape(1, 1, -1).contiguous()
            self._k = float(loo_of_block(blk).pareto_k[0])
        return self._k

    def inits(self, chains, seed=0):
        """[chains, D] starting points for sample(inits=...) / Handle.init: distinct draws spread evenly over the paths that have draws
        (chain c takes one from path c mod paths), chosen by numpy's default_rng(seed)."""
        ok = np.flatnonzero(self.return_code == 0)
        m = self.draws_per_path
        per = -(-int(chains) // ok.size)
        if per > m:
            raise ValueError(f"inits: {chains} chains from {ok.size} paths of {m} draws")
        rng = np.random.default_rng(seed)
        pick = {int(p): rng.choice(m, size=per, replace=False) for p in ok}
        return np.stack([self.draws[int(ok[c % ok.size]) * m + pick[int(ok[c % ok.size])][c // ok.size]] for c in range(int(chains))])

    def scores(self, days=None):
        """predicted_score of `days` = (begin, end) (0-based; default election day) of every draw: a torch tensor [paths * draws, days, S] on the GPU."""
        s = self._h.pathfinder_scores(days)
        return s.reshape((-1,) + tuple(s.shape[2:]))

    def summary(self, ev, days=None, ev_to_win=270):
        """timeline()'s summaries per path: dict(state [paths, days, S, 4], national [paths, days, 4], electoral_votes [paths, days, 5], n_draws [paths])."""
        return self._h.pathfinder_summary(ev, days, ev_to_win)

    def outcomes(self, ev, actual=None, days=None, ev_to_win=270, states=None):
        """Joint election outcomes over the pooled draws (potus_outcomes_device on their scores)."""
        from .outcomes import outcomes_of_block
        return outcomes_of_block(self.scores(days).contiguous(), self._h.data["state_weights"], ev, actual=actual, ev_to_win=ev_to_win, states=states)

    def scenario(self, ev=None, given=None, day=-1, days=None, ev_to_win=270, states=None):
        """Conditional forecast over the pooled draws (potus_scenario_device on their scores); `day` indexes the range `days`."""
        from .scenario import scenario_of_block
        return scenario_of_block(self.scores(days).contiguous(), self._h.data["state_weights"], ev=ev, given=given, day=day, ev_to_win=ev_to_win, states=states)

    def forecast_scores(self, ev, actual, days=None, **kw):
        """Proper scoring rules of the draws against the result (us_potus_model_amd.scoring.score_of_block on their scores)."""
        from .scoring import score_of_block
        T = int(self._h.data["T"])
        return score_of_block(self.scores(days).contiguous(), self._h.data["state_weights"], ev, actual, days=(T - 1, T) if days is None else days, **kw)

    def close(self):
        self._h.close()


class Variational:
    """What cmdstanr's model$variational(algorithm = "meanfield") returns: draws [runs * draws_per_run, D] (unconstrained, the pooled draws of
    every run, run-major), lp (log_prob<jacobian = true> of every draw, as the sampler's lp__), lq (the log density of the run's normal at the
    draw), log_ratio = lp - lq, and per run mean, sd = exp(omega) [runs, D], elbo (the last one evaluated), elbo_path, eta, iterations,
    return_code (_abi.ADVI_CODES; INIT and ADAPT_FAILED runs have NaN draws), flags.  The draws' rows stay on the handle for scores / summary /
    outcomes / scenario."""

    def __init__(self, handle, res):
        self._h, self.res = handle, res
        self.return_code, self.iterations, self.flags, self.eta = res["return_code"], res["iterations"], res["flags"], res["eta"]
        self.runs, self.draws_per_run = res["q"].shape[0], res["q"].shape[1]
        self.ok = ~np.isin(self.return_code, (5, 6))
        if not self.ok.any():
            raise PotusError("variational: no run has an approximation (return code INIT or ADAPT_FAILED on every run)")
        self.mean, self.sd = res["mu"], np.exp(res["omega"])
        self.draws = res["q"].reshape(-1, res["q"].shape[2])
        self.lp, self.lq = res["lp"].reshape(-1), res["lq"].reshape(-1)
        self.log_ratio = self.lp - self.lq
        self.elbo_path = res["elbo"]
        self.elbo = np.array([res["elbo"][r, k] for r, k in enumerate(res["evaluations"])])
        self._k = None

    @property
    def pareto_k(self):
        """k-hat of the importance ratios of the pooled draws: the library's PSIS (potus_loo_device), exactly as Laplace.pareto_k."""
        if self._k is None:
            import torch
            from .loo import loo_of_block
            lr = self.log_ratio[np.isfinite(self.log_ratio)]
            blk = torch.as_tensor(-lr, device=f"cuda:{self._h.opts.device}").reshape(1, 1, -1).contiguous()
            self._k = float(loo_of_block(blk).pareto_k[0])
        return self._k

    def inits(self, chains, seed=0):
        """[chains, D] starting points for sample(inits=...) / Handle.init: distinct draws spread evenly over the runs that have draws
        (chain c takes one from run c mod runs), chosen by numpy's default_rng(seed)."""
        ok = np.flatnonzero(self.ok)
        m = self.draws_per_run
        per = -(-int(chains) // ok.size)
        if per > m:
            raise ValueError(f"inits: {chains} chains from {ok.size} runs of {m} draws")
        rng = np.random.default_rng(seed)
        pick = {int(p): rng.choice(m, size=per, replace=False) for p in ok}
        return np.stack([self.draws[int(ok[c % ok.size]) * m + pick[int(ok[c % ok.size])][c // ok.size]] for c in range(int(chains))])

    def scores(self, days=None):
        """predicted_score of `days` = (begin, end) (0-based; default election day) of every draw: a torch tensor [runs * draws, days, S] on the GPU."""
        s = self._h.variational_scores(days)
        return s.reshape((-1,) + tuple(s.shape[2:]))

    def summary(self, ev, days=None, ev_to_win=270):
        """timeline()'s summaries per run: dict(state [runs, days, S, 4], national [runs, days, 4], electoral_votes [runs, days, 5], n_draws [runs])."""
        return self._h.variational_summary(ev, days, ev_to_win)

    def outcomes(self, ev, actual=None, days=None, ev_to_win=270, states=None):
        """Joint election outcomes over the pooled draws (potus_outcomes_device on their scores)."""
        from .outcomes import outcomes_of_block
        return outcomes_of_block(self.scores(days).contiguous(), self._h.data["state_weights"], ev, actual=actual, ev_to_win=ev_to_win, states=states)

    def scenario(self, ev=None, given=None, day=-1, days=None, ev_to_win=270, states=None):
        """Conditional forecast over the pooled draws (potus_scenario_device on their scores); `day` indexes the range `days`."""
        from .scenario import scenario_of_block
        return scenario_of_block(self.scores(days).contiguous(), self._h.data["state_weights"], ev=ev, given=given, day=day, ev_to_win=ev_to_win, states=states)

    def forecast_scores(self, ev, actual, days=None, **kw):
        """Proper scoring rules of the draws against the result (us_potus_model_amd.scoring.score_of_block on their scores)."""
        from .scoring import score_of_block
        T = int(self._h.data["T"])
        return score_of_block(self.scores(days).contiguous(), self._h.data["state_weights"], ev, actual, days=(T - 1, T) if days is None else days, **kw)

    def close(self):
        self._h.close()


class PotusModel:
    """cmdstanr::cmdstan_model() for the two poll models (final_2016.R:532, final_2012.R:558)."""

    def __init__(self, stan_file_or_variant="full"):
        v = str(stan_file_or_variant)
        if v.endswith(".stan"):
            v = "no_mode_adjustment" if "no_mode_adjustment" in v else "full"
        if v not in _abi.VARIANTS:
            raise ValueError(f"unknown model {stan_file_or_variant!r}")
        self.variant = v
        self.model_name = "poll_model_2020_model" if v == "full" else "poll_model_2020_no_mode_adjustment_model"

    def optimize(self, data, jacobian=False, init=2.0, paths=1, seed=1843, iter=2000, history_size=5, init_alpha=1e-3,
                 tol_obj=1e-12, tol_rel_obj=1e4, tol_grad=1e-8, tol_rel_grad=1e7, tol_param=1e-8, path_offset=0, device=0):
        """cmdstanr's model$optimize(data, jacobian = FALSE, algorithm = "lbfgs"): the posterior mode on the device, `paths` starts in one
        launch.  init: the radius of the uniform starts, or an array [paths, D] (or [D]) of unconstrained starting points.  path_offset: library start
        p is that of path path_offset + p, whatever the batch (timeline.modes: run date d with one path per date is path d)."""
        radius = 2.0 if not np.isscalar(init) else float(init)
        h = Handle(data, self.variant, chains=1, num_warmup=0, num_samples=0, seed=int(seed), init_radius=radius, device=int(device),
                   cus_per_chain=1, twin=0)                       # (a handle that will not sample: no draws array)
        try:
            q0 = None if np.isscalar(init) else np.atleast_2d(np.asarray(init, dtype=np.float64))
            res = h.optimize(q0, None if q0 is not None else int(paths), jacobian=int(bool(jacobian)), iter=int(iter), history_size=int(history_size),
                             init_alpha=float(init_alpha), tol_obj=float(tol_obj), tol_rel_obj=float(tol_rel_obj), tol_grad=float(tol_grad),
                             tol_rel_grad=float(tol_rel_grad), tol_param=float(tol_param), path_offset=int(path_offset))
            return Optimum(h, res, jacobian)
        except Exception:
            h.close()
            raise

    def laplace(self, data, mode=None, draws=1000, jacobian=True, seed=1843, h=None, u=None, draw_offset=0, device=0):
        """cmdstanr's model$laplace(data, mode =, draws =, jacobian = TRUE): draws from the normal approximation at the mode, on the device.
        mode: an Optimum (its best path; found with the same `jacobian`), an array [D] of unconstrained coordinates, or None -- then
        optimize(jacobian=jacobian) runs first with tol_grad = 1e-2 as its only stopping rule (CmdStan's default rules stop this model at
        |g| of 2-4, DESIGN.md section 4k, too far from the mode for a Hessian).  u [draws, D]: the caller's standard normals."""
        if isinstance(mode, Optimum):
            if mode.jacobian != bool(jacobian):
                raise ValueError(f"laplace: the mode was found with jacobian = {mode.jacobian}, the approximation is asked for jacobian = {bool(jacobian)}")
            q = mode.q[mode.best]
        elif mode is None:
            opt = self.optimize(data, jacobian=jacobian, seed=seed, tol_obj=0.0, tol_rel_obj=0.0, tol_grad=1e-2, tol_rel_grad=0.0, tol_param=0.0, device=device)
            try:
                q = opt.q[opt.best].copy()
            finally:
                opt.close()
        else:
            q = np.asarray(mode, dtype=np.float64).reshape(-1)
        hd = Handle(data, self.variant, chains=1, num_warmup=0, num_samples=0, seed=int(seed), device=int(device), cus_per_chain=1, twin=0)
        try:
            if q.shape != (hd.D,):
                raise ValueError(f"laplace: the mode has {q.size} coordinates, {hd.D} expected")
            fields = dict(jacobian=int(bool(jacobian)), draw_offset=int(draw_offset))
            if h is not None:
                fields["h"] = float(h)
            res = hd.laplace(q, int(draws), u=u, **fields)
            return Laplace(hd, q, res, hd.log_prob_grad(q)[0][0], jacobian)
        except Exception:
            hd.close()
            raise

    def pathfinder(self, data, paths=4, draws=1000, init=2.0, seed=1843, history_size=6, num_elbo_draws=25, max_lbfgs_iters=1000, device=0, **opt):
        """cmdstanr's model$pathfinder(data, num_paths = 4, draws = 1000, psis_resample = FALSE): `paths` L-BFGS paths, the ELBO of the normal
        around every iterate, `draws` draws IN ALL, dealt evenly to the paths from each path's best iterate.  init as in optimize(); opt: init_alpha, tol_*."""
        radius = 2.0 if not np.isscalar(init) else float(init)
        h = Handle(data, self.variant, chains=1, num_warmup=0, num_samples=0, seed=int(seed), init_radius=radius, device=int(device), cus_per_chain=1, twin=0)
        try:
            q0 = None if np.isscalar(init) else np.atleast_2d(np.asarray(init, dtype=np.float64))
            n = int(paths) if q0 is None else q0.shape[0]
            res = h.pathfinder(q0, None if q0 is not None else n, history_size=int(history_size), num_elbo_draws=int(num_elbo_draws),
                               num_draws=-(-int(draws) // n), max_lbfgs_iters=int(max_lbfgs_iters), **opt)
            return Pathfinder(h, res)
        except Exception:
            h.close()
            raise

    def variational(self, data, runs=1, seed=1843, init=2.0, algorithm="meanfield", iter=10000, grad_samples=1, elbo_samples=100, eta=None,
                    adapt_engaged=True, adapt_iter=50, tol_rel_obj=0.01, eval_elbo=100, output_samples=1000, device=0, **opt):
        """cmdstanr's model$variational(data, algorithm = "meanfield", ...) with its argument names: `runs` independent ADVI runs in one call
        (cmdstanr runs one), `output_samples` draws PER RUN.  init as in optimize(): a radius, or starts [runs, D].  eta: with adapt_engaged the
        adaptation chooses it; given and adapt_engaged = False it is the step size.  opt: elbo_offset, draw_offset, run_offset."""
        radius = 2.0 if not np.isscalar(init) else float(init)
        h = Handle(data, self.variant, chains=1, num_warmup=0, num_samples=0, seed=int(seed), init_radius=radius, device=int(device), cus_per_chain=1, twin=0)
        try:
            q0 = None if np.isscalar(init) else np.atleast_2d(np.asarray(init, dtype=np.float64))
            n = int(runs) if q0 is None else q0.shape[0]
            res = h.variational(q0, None if q0 is not None else n, algorithm=algorithm, iter=int(iter), grad_samples=int(grad_samples),
                                elbo_samples=int(elbo_samples), eta=1.0 if eta is None else float(eta), adapt_engaged=int(bool(adapt_engaged)),
                                adapt_iter=int(adapt_iter), tol_rel_obj=float(tol_rel_obj), eval_elbo=int(eval_elbo),
                                output_samples=int(output_samples), **opt)
            return Variational(h, res)
        except Exception:
            h.close()
            raise

    def sample(self, data, seed=1843, chains=4, parallel_chains=None, iter_warmup=1000, iter_sampling=1000,
               refresh=100, adapt_delta=0.8, max_treedepth=10, init=2.0, save_warmup=False, device=0,
               chain_id_offset=0, show_messages=False, inits=None, devices=None, metric="diag_e", cus_per_chain=0, twin=-1,
               metric_storage="f64", rhat_stop=None, ess_stop=400.0, pooled_metric=False):
        """`devices`: GPU ids; the chains are dealt to them in consecutive blocks and advance together under
        potus_run_many (one host thread).  Chain ids -- hence RNG streams and draws -- do not depend on the split.
        `rhat_stop` (off by default; a DEVIATION from Stan, which always runs iter_sampling iterations): after every `refresh` transitions
        of the sampling phase the pooled chains' rank-normalised split R-hat / bulk ESS of lp__ and mu_b[:, T] are taken on the device
        (potus_check_convergence) and sampling ends once every R-hat < rhat_stop and every bulk ESS >= ess_stop; the draws up to that
        point are those of the uninterrupted run.  `self.last_convergence` keeps the checks.
        `pooled_metric` (off by default; metric = "dense_e"; a DEVIATION from Stan): one inverse metric per GPU, adapted at every window end from
        the draws of all chains on it (potus_opts.pooled_metric)."""
        from . import parallel
        if rhat_stop is not None:
            _need_check_convergence(load_library())
        devs = [int(device)] if devices is None else [int(d) for d in devices]
        hs, first = [], 0
        for r, dev in enumerate(devs):
            off, n_loc = parallel.chain_block(int(chains), r, len(devs))
            if n_loc == 0:
                continue
            h = Handle(data, self.variant, chains=n_loc, chain_id_offset=int(chain_id_offset) + off,
                       num_warmup=int(iter_warmup), num_samples=int(iter_sampling), max_depth=int(max_treedepth),
                       delta=float(adapt_delta), init_radius=float(init), seed=int(seed), device=dev,
                       save_warmup=int(bool(save_warmup)), metric=_abi.METRICS[metric], cus_per_chain=int(cus_per_chain), twin=int(twin),
                       metric_storage={"f64": _abi.STORAGE_F64, "f32": _abi.STORAGE_F32}[metric_storage], pooled_metric=int(bool(pooled_metric)))
            h.init(None if inits is None else np.asarray(inits)[off:off + n_loc])
            hs.append(h)
        total = int(iter_warmup) + int(iter_sampling)
        chunk = max(1, int(refresh)) if refresh else total
        done = 0
        self.last_convergence = []
        while done < total:
            n = min(chunk, total - done)
            if done < iter_warmup:
                n = min(n, int(iter_warmup) - done)          # the first check falls on a whole chunk of sampling draws
            run_many(hs, n)
            done += n
            if show_messages:
                phase = "Warmup" if done <= iter_warmup else "Sampling"
                print(f"Iteration: {done:5d} / {total} [{100 * done // total:3d}%]  ({phase})", flush=True)
            if rhat_stop is not None and done > iter_warmup and done < total:
                conv, r, e = check_convergence(hs, float(rhat_stop), float(ess_stop))
                self.last_convergence.append({"iterations": done, "sampling_draws": done - int(iter_warmup), "rhat_max": r, "ess_bulk_min": e, "converged": conv})
                if conv:
                    if show_messages:
                        print(f"Stopped after {done - int(iter_warmup)} sampling iterations: R-hat {r:.4f} < {rhat_stop}, bulk ESS {e:.0f} >= {ess_stop}", flush=True)
                    break
        self.last_handle = hs[0]
        self.last_handles = hs
        return StanFit(hs, self.model_name)


def sampling(model: PotusModel, data, chains=4, iter=2000, warmup=None, refresh=None, seed=1843, control=None,
             **kw):
    """rstan::sampling(model, data=, chains=, iter=, warmup=, refresh=) (final_2016.R:525-529)."""
    warmup = iter // 2 if warmup is None else warmup
    control = control or {}
    return model.sample(data, seed=seed, chains=chains, iter_warmup=warmup, iter_sampling=iter - warmup,
                        refresh=refresh if refresh is not None else max(iter // 10, 1),
                        adapt_delta=control.get("adapt_delta", 0.8), max_treedepth=control.get("max_treedepth", 10),
                        metric=control.get("metric", "diag_e"), **kw)
