"""MI355X-native batched lunar-ascent trajectory optimiser.

The package holds only the hot path of Ben-Bussch/Lunar_Module_Ascent_Trajectory_Optimiser
(the NLP solve behind Launch_Optimiser.py:177): csrc/ (HIP kernels + C ABI, include/ascent.h)
and the host-side mirror of the reference's problem-definition surface.
"""
from .params import AscentParams, sweep_isp_drymass, sweep_config4, isp_drymass_gradient, PARAM_FIELDS  # noqa: F401
from .solver import (solve_batch, solve_batch_torch, last_kernel_ms, eval_nodes, kkt_step, BatchResult,  # noqa: F401
                     TRAJ_FIELDS, blob_rows, dense_records, coast_batch, kkt_solve, default_path,
                     param_sensitivity, final_time, fly_batch, FlightResult, FLIGHT_ROWS,
                     flight_jacobian, FlightJacobian, JACOBIAN_ROWS, trim_batch, TrimResult, TRIM_ROWS,
                     disperse_batch, DispersionResult, guidance_gains, GuidanceResult, GUIDE_ROWS, GUIDE_FF_ROWS,
                     DispersionHistory, HISTORY_ROWS, linear_corridor, LinearCorridor, LINCOV_COLS, navigation_filter, NavigationFilter, NAVFILTER_ROWS,
                     sample_quantiles, quantile_chunks)

__all__ = ["AscentParams", "sweep_isp_drymass", "sweep_config4", "solve_batch", "eval_nodes", "kkt_step",
           "BatchResult", "TRAJ_FIELDS", "PARAM_FIELDS", "blob_rows", "param_sensitivity", "final_time",
           "isp_drymass_gradient", "fly_batch", "FlightResult", "FLIGHT_ROWS",
           "flight_jacobian", "FlightJacobian", "JACOBIAN_ROWS", "trim_batch", "TrimResult", "TRIM_ROWS",
           "disperse_batch", "DispersionResult", "guidance_gains", "GuidanceResult", "GUIDE_ROWS", "GUIDE_FF_ROWS",
           "DispersionHistory", "HISTORY_ROWS", "linear_corridor", "LinearCorridor", "LINCOV_COLS", "navigation_filter", "NavigationFilter", "NAVFILTER_ROWS",
           "sample_quantiles", "quantile_chunks"]
