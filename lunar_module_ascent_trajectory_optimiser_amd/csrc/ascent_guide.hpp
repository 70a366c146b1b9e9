// Host interface of the guidance gains (ascent_guide.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"
#include "ascent_host.hpp"

namespace ascent {

// Device workspace (bytes) of gains_run: the nominal trajectory and f_fly's summary rows (jac_ws_bytes of ascent_trim.hpp).  The
// step records, P and Lambda live in LDS only.
size_t gains_ws_bytes(int K, long batch);

// include/ascent.h: ascent_guidance_gains.  Device pointers: c.dp[batch], dblob [21K+10][batch], dweights [6][batch], dgain_u
// [7][K][batch], dgain_t [7][batch], dsummary [ASCENT_GUIDE_ROWS][batch], djac [9][24][batch] and djac_u [9][K][batch] both or
// neither, ws of gains_ws_bytes.  Options already checked by the caller.  Only enqueues two kernels on c.stream (f_fly, g_gains).
// Returns ASCENT_OK / ASCENT_E_HIP.
int gains_run(const Call &c, int substeps, const double *dblob, const double *dweights, double *dgain_u, double *dgain_t,
              double *dsummary, double *djac, double *djac_u, double *ws);

// include/ascent.h: ascent_guidance_feedforward.  As gains_run, plus dff_dir [16][batch], dff_know [16][batch] or null (needed
// with djac), dff_u [K][batch], dff_t [batch], dsummary [ASCENT_GUIDE_FF_ROWS][batch], djac_nav [9][ASCENT_NAV_ROWS][batch] or null
// (only with djac).  Same workspace; enqueues f_fly and g_gains_ff.
int gains_ff_run(const Call &c, int substeps, const double *dblob, const double *dweights, const double *dff_dir,
                 const double *dff_know, double *dgain_u, double *dgain_t, double *dff_u, double *dff_t, double *dsummary,
                 double *djac, double *djac_u, double *djac_nav, double *ws);

}  // namespace ascent
