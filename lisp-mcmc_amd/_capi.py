"""ctypes binding of libmhx.so -- exactly the entry points include/mhx.h declares.

There is no CPU fallback: if the HIP library is missing or no gfx950 device is usable,
loading or mhx_create fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MHX_LIBRARY") or os.path.join(_HERE, "libmhx.so")  # MHX_LIBRARY: a tuning build

f64p = C.POINTER(C.c_double)
i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)
u8p = C.POINTER(C.c_uint8)
u64p = C.POINTER(C.c_uint64)

OK, EINVAL, ENOMEM, EDEVICE, ESTATE, EUNSUPPORTED, ECOMM = 0, -1, -2, -3, -4, -5, -6
MODEL_POLY, MODEL_GAUSS_PEAKS, MODEL_LORENTZ_PEAKS, MODEL_LORDER_MIXED = 0, 1, 2, 3
MODEL_EXP_DECAY, MODEL_SINUSOID, MODEL_PVOIGT2, MODEL_EXPR = 4, 5, 6, 7
LIK_NORMAL, LIK_NORMAL_CUTOFF, LIK_POISSON, LIK_EXPR = 0, 1, 2, 3
ADAPT_FAITHFUL, ADAPT_POOLED = 0, 1
SIGMA_NONE, SIGMA_SHARED, SIGMA_PER_CHAIN, SIGMA_PER_POINT = 0, 1, 2, 3
CHAIN_RUNNING, CHAIN_DONE, CHAIN_FP_TRAP, CHAIN_STOPPED = 0, 1, 2, 3
L_OK, L_CAUGHT, L_INVALID, L_EMPTY = 0, 1, 2, 3
AUTOCORR_NONFINITE, AUTOCORR_CONSTANT, AUTOCORR_OPEN, MAX_AUTOCORR_LAG = 1, 2, 4, 1023
WAIC_NONFINITE, WAIC_ONE_STEP, WAIC_BLOCK = 1, 2, 256
LOO_NONFINITE, LOO_SHORT, LOO_FLAT, LOO_EMPTY, LOO_BLOCK, LOO_MAX_TAIL = 1, 2, 4, 8, 256, 1024
HELDOUT_NONFINITE, HELDOUT_NO_POINTS, HELDOUT_BLOCK = 1, 2, 256
RESID_NONFINITE, RESID_BLOCK = 1, 256
NORMEQ_NONFINITE, NORMEQ_BLOCK = 1, 1024
CAND_KEEP_MAX = 16
FITPCT_NONFINITE, FITPCT_ONE_STEP, FITPCT_EMPTY, FITPCT_BLOCK = 1, 2, 4, 128
HDI_NONFINITE, MAX_HDI_MASSES, MAX_HDI_LADDER = 1, 8, 4096
TRACE_STEPS, TRACE_UNIQUE, TRACE_FORWARD, TRACE_PROB = 0, 1, 2, -1


class Config(C.Structure):
    _fields_ = [("n_chains", C.c_int64), ("n_params", C.c_int32), ("n_functions", C.c_int32),
                ("device", C.c_int32), ("adapt_mode", C.c_int32), ("seed", C.c_uint64),
                ("chain_offset", C.c_int64), ("history_capacity", C.c_int32),
                ("poisson_logfact_double", C.c_int32)]


class RunOpts(C.Structure):
    _fields_ = [("n", C.c_int64), ("temperature", C.c_double), ("auto_mode", C.c_int32),
                ("max_walker_length", C.c_int64), ("l_matrix", f64p),
                ("l_matrix_per_chain", C.c_int32)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, f64p, C.c_size_t, C.c_int)

# name -> (restype, argtypes): every symbol of include/mhx.h
SIGNATURES = {
    "mhx_version": (C.c_int, []),
    "mhx_build_id": (C.c_char_p, []),
    "mhx_last_error": (C.c_char_p, []),
    "mhx_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "mhx_create": (C.c_int, [C.POINTER(Config), C.POINTER(C.c_void_p)]),
    "mhx_destroy": (None, [C.c_void_p]),
    "mhx_set_function": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, C.c_int, i32p, C.c_int]),
    "mhx_set_dataset": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p, f64p, C.c_size_t, C.c_int]),
    "mhx_set_dataset_cols": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(f64p), C.c_int, f64p, f64p,
                                       C.c_size_t, C.c_int]),
    "mhx_set_dataset_planes": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p, f64p, C.c_int, C.c_size_t,
                                         C.c_int]),
    "mhx_set_bounds": (C.c_int, [C.c_void_p, C.c_int, i32p, f64p, f64p, C.c_int]),
    "mhx_set_function_expr": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_char_p),
                                        i32p, C.c_int]),
    "mhx_set_expr_recognition": (C.c_int, [C.c_void_p, C.c_int]),
    "mhx_expr_classify": (C.c_int, [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, i32p, i32p, i32p, i32p]),
    "mhx_set_prior_expr": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_char_p),
                                     i32p, C.c_int]),
    "mhx_set_likelihood_expr": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p]),
    "mhx_init_chains": (C.c_int, [C.c_void_p, f64p, C.c_int]),
    "mhx_logpost": (C.c_int, [C.c_void_p, f64p, C.c_size_t, f64p, f64p]),
    "mhx_step_injected": (C.c_int, [C.c_void_p, f64p, C.c_int, f64p, f64p, f64p, u8p]),
    "mhx_run_opts_default": (None, [C.POINTER(RunOpts)]),
    "mhx_adaptive_begin": (C.c_int, [C.c_void_p, C.POINTER(RunOpts)]),
    "mhx_adaptive_advance": (C.c_int, [C.c_void_p, C.c_int64, i64p]),
    "mhx_adaptive_steps_full": (C.c_int, [C.c_void_p, C.POINTER(RunOpts)]),
    "mhx_adaptive_steps": (C.c_int, [C.c_void_p, C.c_int64]),
    "mhx_many_steps": (C.c_int, [C.c_void_p, C.c_int64, f64p, C.c_int]),
    "mhx_request_stop": (C.c_int, [C.c_void_p]),
    "mhx_set_allreduce": (C.c_int, [C.c_void_p, ALLREDUCE_FN, C.c_void_p, C.c_int]),
    "mhx_get_state": (C.c_int, [C.c_void_p, f64p, f64p, f64p, f64p, i64p, i64p]),
    "mhx_get_chain_status": (C.c_int, [C.c_void_p, i32p, i64p]),
    "mhx_get_lmatrix": (C.c_int, [C.c_void_p, f64p]),
    "mhx_get_temperature": (C.c_int, [C.c_void_p, f64p]),
    "mhx_get_acceptance": (C.c_int, [C.c_void_p, C.c_int, f64p]),
    "mhx_get_trace": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, f64p, f64p, C.POINTER(C.c_int)]),
    "mhx_get_proposal_factor": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, f64p,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mhx_set_history": (C.c_int, [C.c_void_p, C.c_int64, f64p, f64p, C.c_int]),
    "mhx_walker_modify": (C.c_int, [C.c_void_p, C.c_int, C.c_int64]),
    "mhx_get_pooled": (C.c_int, [C.c_void_p, f64p, f64p, i32p, u64p]),
    "mhx_get_counters": (C.c_int, [C.c_void_p, u64p, u64p]),
    "mhx_kernel_name": (C.c_char_p, [C.c_void_p]),
    "mhx_kernel_timing": (C.c_int, [C.c_void_p, C.c_int, f64p, u64p, f64p]),
    "mhx_take_step": (C.c_int, [C.c_void_p, f64p, C.c_int, C.c_double]),
    "mhx_get_chain": (C.c_int, [C.c_void_p, C.c_int64, f64p, f64p, f64p, f64p, i64p, i64p]),
    "mhx_comm_get_unique_id": (C.c_int, [u8p]),
    "mhx_comm_init_rank": (C.c_int, [C.c_void_p, u8p, C.c_int, C.c_int]),
    "mhx_group_partition": (C.c_int, [C.c_int64, C.c_int, C.c_int, i64p, i64p]),
    "mhx_group_create": (C.c_int, [C.POINTER(Config), i32p, C.c_int, C.POINTER(C.c_void_p)]),
    "mhx_group_destroy": (None, [C.c_void_p]),
    "mhx_group_size": (C.c_int, [C.c_void_p]),
    "mhx_group_engine": (C.c_void_p, [C.c_void_p, C.c_int]),
    "mhx_group_chain_range": (C.c_int, [C.c_void_p, C.c_int, i64p, i64p]),
    "mhx_group_set_function": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, C.c_int, i32p, C.c_int]),
    "mhx_group_set_dataset": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p, f64p, C.c_size_t, C.c_int]),
    "mhx_group_set_dataset_cols": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(f64p), C.c_int, f64p, f64p,
                                             C.c_size_t, C.c_int]),
    "mhx_group_set_dataset_planes": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p, f64p, C.c_int,
                                               C.c_size_t, C.c_int]),
    "mhx_group_set_bounds": (C.c_int, [C.c_void_p, C.c_int, i32p, f64p, f64p, C.c_int]),
    "mhx_group_set_function_expr": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p,
                                              C.POINTER(C.c_char_p), i32p, C.c_int]),
    "mhx_group_set_expr_recognition": (C.c_int, [C.c_void_p, C.c_int]),
    "mhx_group_set_prior_expr": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p,
                                           C.POINTER(C.c_char_p), i32p, C.c_int]),
    "mhx_group_set_likelihood_expr": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p]),
    "mhx_group_init_chains": (C.c_int, [C.c_void_p, f64p, C.c_int]),
    "mhx_group_adaptive_begin": (C.c_int, [C.c_void_p, C.POINTER(RunOpts)]),
    "mhx_group_adaptive_advance": (C.c_int, [C.c_void_p, C.c_int64, i64p]),
    "mhx_group_adaptive_steps_full": (C.c_int, [C.c_void_p, C.POINTER(RunOpts)]),
    "mhx_group_request_stop": (C.c_int, [C.c_void_p]),
    "mhx_group_get_state": (C.c_int, [C.c_void_p, f64p, f64p, f64p, f64p, i64p, i64p]),
    "mhx_group_get_counters": (C.c_int, [C.c_void_p, u64p, u64p]),
    "mhx_percentile_rank": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, i64p, i32p]),
    "mhx_get_percentiles": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, C.c_int, f64p, i32p]),
    "mhx_get_covariances": (C.c_int, [C.c_void_p, C.c_int, f64p, i32p, i32p]),
    "mhx_get_proposal_factors": (C.c_int, [C.c_void_p, C.c_int, f64p, i32p, i32p]),
    "mhx_get_window_best": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p]),
    "mhx_get_history_capacity": (C.c_int, [C.c_void_p, i32p]),
    "mhx_get_summary_timing": (C.c_int, [C.c_void_p, f64p]),
    "mhx_group_get_percentiles": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, C.c_int, f64p, i32p]),
    "mhx_group_get_covariances": (C.c_int, [C.c_void_p, C.c_int, f64p, i32p, i32p]),
    "mhx_group_get_proposal_factors": (C.c_int, [C.c_void_p, C.c_int, f64p, i32p, i32p]),
    "mhx_group_get_window_best": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p]),
    "mhx_band_count": (C.c_int, [C.c_int64, i64p]),
    "mhx_eval_function": (C.c_int, [C.c_void_p, C.c_int, f64p, C.c_int64, f64p, C.c_int, C.c_int64,
                                    f64p]),
    "mhx_get_fit_bands": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p, C.c_int, C.c_int64, f64p,
                                    f64p, i32p, i32p]),
    "mhx_group_get_fit_bands": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p, C.c_int, C.c_int64,
                                          f64p, f64p, i32p, i32p]),
    "mhx_get_derived": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p),
                                  i32p, C.c_int, C.c_int, i32p, i32p, C.c_int, f64p, f64p, f64p,
                                  f64p, f64p, i32p, i32p]),
    "mhx_group_get_derived": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int,
                                        C.POINTER(C.c_char_p), i32p, C.c_int, C.c_int, i32p, i32p,
                                        C.c_int, f64p, f64p, f64p, f64p, f64p, i32p, i32p]),
    "mhx_get_histograms": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, C.c_int, f64p, C.c_int,
                                     i32p, i32p, i32p, i32p]),
    "mhx_get_pair_grids": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, i32p, i32p, C.c_int, C.c_int,
                                     f64p, C.c_int, i32p, i32p, i32p, i32p]),
    "mhx_group_get_histograms": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, C.c_int, f64p, C.c_int,
                                           i32p, i32p, i32p, i32p]),
    "mhx_group_get_pair_grids": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, i32p, i32p, C.c_int,
                                           C.c_int, f64p, C.c_int, i32p, i32p, i32p, i32p]),
    "mhx_get_autocorr": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, C.c_int, f64p, f64p, f64p, f64p,
                                   f64p, i32p, i32p, i32p]),
    "mhx_group_get_autocorr": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, C.c_int, f64p, f64p, f64p,
                                         f64p, f64p, i32p, i32p, i32p]),
    "mhx_split_rhat": (C.c_int, [f64p, f64p, i32p, C.c_int64, C.c_int, f64p]),
    "mhx_get_ensemble_percentiles": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, u8p, i32p, i32p, C.c_int,
                                               f64p, i64p, i32p, i32p]),
    "mhx_group_get_ensemble_percentiles": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, u8p, i32p, i32p,
                                                     C.c_int, f64p, i64p, i32p, i32p]),
    "mhx_ensemble_pick": (C.c_int, [u64p, C.c_int, C.c_int64, i32p, i64p, i64p]),
    "mhx_get_waic": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p, f64p, f64p, i32p, f64p, f64p, f64p,
                               i32p, i32p]),
    "mhx_group_get_waic": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p, f64p, f64p, i32p, f64p, f64p,
                                     f64p, i32p, i32p]),
    "mhx_loo_tail_length": (C.c_int, [C.c_int64, C.c_int32, i32p]),
    "mhx_get_loo": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, f64p, f64p, f64p, i32p, i32p,
                              i32p, f64p, f64p, f64p, f64p, f64p]),
    "mhx_group_get_loo": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, f64p, f64p, f64p, i32p,
                                    i32p, i32p, f64p, f64p, f64p, f64p, f64p]),
    "mhx_get_heldout": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p, C.c_int, C.c_int64, f64p, C.c_int, f64p,
                                  C.c_int, u8p, C.c_int, f64p, i32p, f64p, f64p, i32p, i32p]),
    "mhx_group_get_heldout": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p, C.c_int, C.c_int64, f64p, C.c_int,
                                        f64p, C.c_int, u8p, C.c_int, f64p, i32p, f64p, f64p, i32p, i32p]),
    "mhx_get_residuals": (C.c_int, [C.c_void_p, C.c_int, f64p, C.c_double, f64p, f64p, f64p, f64p, f64p,
                                    f64p, i64p, i32p, i32p, i32p, i32p]),
    "mhx_group_get_residuals": (C.c_int, [C.c_void_p, C.c_int, f64p, C.c_double, f64p, f64p, f64p, f64p,
                                          f64p, f64p, i64p, i32p, i32p, i32p, i32p]),
    "mhx_get_normal_equations": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p, C.c_int, f64p, f64p, f64p, f64p,
                                           i32p]),
    "mhx_group_get_normal_equations": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p, C.c_int, f64p, f64p, f64p,
                                                 f64p, i32p]),
    "mhx_get_candidate_scores": (C.c_int, [C.c_void_p, C.c_int, f64p, C.c_int64, C.c_int, C.c_int, f64p, i32p,
                                           f64p, i32p]),
    "mhx_group_get_candidate_scores": (C.c_int, [C.c_void_p, C.c_int, f64p, C.c_int64, C.c_int, C.c_int, f64p,
                                                 i32p, f64p, i32p]),
    "mhx_get_fit_percentiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p, C.c_int, C.c_int64, i32p, i32p,
                                          C.c_int, f64p, f64p, f64p, i32p, i32p]),
    "mhx_group_get_fit_percentiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p, C.c_int, C.c_int64, i32p,
                                                i32p, C.c_int, f64p, f64p, f64p, i32p, i32p]),
    "mhx_get_traces": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, i32p, C.c_int, C.c_int,
                                 f64p, f64p, f64p, i32p, i32p, i32p]),
    "mhx_group_get_traces": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, i32p, C.c_int,
                                       C.c_int, f64p, f64p, f64p, i32p, i32p, i32p]),
    "mhx_trace_rows": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, i64p]),
    "mhx_hdi_span": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, i64p]),
    "mhx_get_hdi": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, i32p, i32p, C.c_int, C.c_int, f64p, f64p, i32p,
                              f64p, i32p, i32p]),
    "mhx_group_get_hdi": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, i32p, i32p, C.c_int, C.c_int, f64p, f64p,
                                    i32p, f64p, i32p, i32p]),
    "mhx_get_derived_hdi": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), i32p,
                                      C.c_int, C.c_int, i32p, i32p, C.c_int, C.c_int, f64p, f64p, i32p, f64p, i32p,
                                      i32p]),
    "mhx_group_get_derived_hdi": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p),
                                            i32p, C.c_int, C.c_int, i32p, i32p, C.c_int, C.c_int, f64p, f64p, i32p,
                                            f64p, i32p, i32p]),
}

_lib = None


class MhxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmhx error %d: %s" % (code, msg))
        self.code = code


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64.so (SONAME
    libamdhip64.so.7, the name libmhx.so needs); if this process may also use torch
    (bench.py: torch.distributed / RCCL), load that copy first so libmhx.so binds to it instead
    of /opt/rocm's - two live HIP runtimes in one process cannot both see the GPU.  Without
    torch installed nothing happens and libmhx.so uses the ROCm installation's runtime."""
    import importlib.util
    import sys
    if os.environ.get("MHX_NO_TORCH_HIP"):
        return
    if "torch" in sys.modules:
        return  # already loaded: the loader will reuse it by SONAME
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    cand = os.path.join(libdir, "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            return
        # ... and the RCCL that was built against THAT runtime, should libmhx need one
        # (mhx_comm_init_rank / mhx_group_create load it lazily)
        rccl = os.path.join(libdir, "librccl.so")
        if os.path.exists(rccl):
            os.environ.setdefault("MHX_RCCL_LIBRARY", rccl)


def lib():
    """Load libmhx.so (built by lisp-mcmc_amd/csrc/Makefile or __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `make -C lisp-mcmc_amd/csrc` (hipcc, gfx950). "
                "There is no CPU fallback." % LIB_PATH)
        _share_hip_runtime_with_torch()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = header and library disagree
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != OK:
        raise MhxError(rc, lib().mhx_last_error().decode("utf-8", "replace"))


def as_f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(f64p)


def as_i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(i32p)
