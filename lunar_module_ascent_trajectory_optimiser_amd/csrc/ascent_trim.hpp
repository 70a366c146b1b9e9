// Host interface of the flight Jacobian and the trim (ascent_trim.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"
#include "ascent_host.hpp"

namespace ascent {

// Device workspace (bytes) of jac_run / trim_run for `batch` NLPs on K intervals: the flown trajectory the Jacobian is
// linearised about and f_fly's summary rows; the trim adds the Jacobian itself and its per-problem state.  The step records
// (112 doubles per step) live in LDS only.
size_t jac_ws_bytes(int K, long batch);
size_t trim_ws_bytes(int K, long batch);

// include/ascent.h: ascent_flight_jacobian.  Device pointers: c.dp[batch], dblob [21K+10][batch], djac [9][24][batch], djac_u
// [9][K][batch] or null, ws of jac_ws_bytes.  Options already checked by the caller.  Only enqueues two kernels on c.stream
// (f_fly, j_jac).  Returns ASCENT_OK / ASCENT_E_HIP.
int jac_run(const Call &c, int substeps, const double *dblob, double *djac, double *djac_u, double *ws);

// include/ascent.h: ascent_trim_batch.  Device pointers: dblob_out [21K+10][batch] (working copy and result), dsummary
// [ASCENT_TRIM_ROWS][batch], ws of trim_ws_bytes.  terminal: ascent_opts.terminal itself, 0 / 1.  rounds 1..32, tol > 0.  Only
// enqueues: one copy, one memset and 3 rounds + 2 kernels.
int trim_run(const Call &c, int terminal, int substeps, int rounds, double tol, const double *dblob, double *dblob_out,
             double *dsummary, double *ws);

}  // namespace ascent
