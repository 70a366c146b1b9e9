// Host interface of the linear covariance corridor (ascent_lincov.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"
#include "ascent_host.hpp"

namespace ascent {

// Device workspace (bytes) of lincov_run: the nominal trajectory and f_fly's summary rows (flight_ws_bytes).  The step records,
// the state sensitivity and Q live in LDS only.
size_t lincov_ws_bytes(int K, long batch);

// The arrays of ascent_covariance_history_batch (include/ascent.h), host or device pointers alike; null where the caller gave none.
// blob [21K+10][batch], sigma [24][batch], sigma_u [K][batch], gain_u [7][K][batch], gain_t [7][batch], stretch_max [batch],
// ff_u [K][batch], ff_t [batch], ff_know [16][batch], sigma_nav [ASCENT_NAV_ROWS][batch]; nominal [10][NJ][batch], cov
// [ASCENT_LINCOV_COV_ROWS][NJ][batch], jac [10][ASCENT_LINCOV_COLS][NJ][batch] or null, NJ = history_nodes(K, node_stride).
struct LincovIO {
  const double *blob, *sigma, *sigma_u;
  const double *gain_u, *gain_t, *stretch_max;
  const double *ff_u, *ff_t, *ff_know, *sigma_nav;
  int node_stride;
  double *nominal, *cov, *jac;
  const double *nav_phi, *nav_q;      // ascent_covariance_drifting_batch: [ASCENT_NAV_ROWS][batch] each, both or neither
};

// io: device pointers, ws of lincov_ws_bytes.  Options already checked by the caller.  Only enqueues two kernels on c.stream:
// f_fly, then l_lincov (with io.nav_phi: l_lincov_drifting).  Returns ASCENT_OK / ASCENT_E_HIP.
int lincov_run(const Call &c, int substeps, const LincovIO &io, double *ws);

}  // namespace ascent
