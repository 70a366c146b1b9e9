// Host interface of the navigation filter (ascent_navfilter.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"
#include "ascent_host.hpp"

namespace ascent {

// The arrays of ascent_navigation_filter (include/ascent.h), device pointers; null where the caller gave none.  blob [21K+10][batch],
// sigma_nav [7][batch], sigma_u [K][batch], filter_q [7][batch], meas_h [n_meas][7][batch], meas_sigma [n_meas][batch];
// gain_l [n_meas][7][K][batch], pfilt [28][K][batch] or null, summary [ASCENT_NAVFILTER_ROWS][batch].
struct NavFilterIO {
  const double *blob, *sigma_nav, *sigma_u, *filter_q, *meas_h, *meas_sigma;
  int n_meas, meas_stride;
  double *gain_l, *pfilt, *summary;
};

// The arrays of ascent_covariance_filtered_batch: those of the parent call (ascent_lincov.hpp: LincovIO) without the feed-forward,
// sigma_nav [7][batch], the filter's gain_l, meas_h and meas_sigma as above; nav_cov [ASCENT_NAV_COV_ROWS][NJ][batch], nav_jac
// [7][ASCENT_LINCOV_COLS][NJ][batch] or null.
struct FilteredIO {
  const double *blob, *sigma, *sigma_u;
  const double *gain_u, *gain_t, *stretch_max;
  const double *sigma_nav, *gain_l, *meas_h, *meas_sigma;
  int n_meas, meas_stride, node_stride;
  double *nominal, *cov, *nav_cov, *jac, *nav_jac;
};

// io: device pointers, ws of lincov_ws_bytes (ascent_lincov.hpp).  Options already checked by the caller.  Each only enqueues two
// kernels on c.stream: f_fly, then n_filter / l_lincov_filtered.  Return ASCENT_OK / ASCENT_E_HIP.
int navfilter_run(const Call &c, int substeps, const NavFilterIO &io, double *ws);
int lincov_filtered_run(const Call &c, int substeps, const FilteredIO &io, double *ws);

}  // namespace ascent
