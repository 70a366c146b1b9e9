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

// The arrays of ascent_guidance_gains and ascent_guidance_feedforward (include/ascent.h), host or device pointers alike.
// blob [21K+10][batch], weights [6][batch], gain_u [7][K][batch], gain_t [7][batch], summary [ASCENT_GUIDE_ROWS |
// ASCENT_GUIDE_FF_ROWS][batch], jac [9][24][batch] or null, jac_u [9][K][batch] or null (only with jac).  The feed-forward call
// (ff_dir not null) adds ff_dir [16][batch], ff_know [16][batch] or null (needed with jac), ff_u [K][batch], ff_t [batch],
// jac_nav [9][ASCENT_NAV_ROWS][batch] or null (only with jac); all five are null in a gains call.
struct GainsIO {
  const double *blob, *weights, *ff_dir, *ff_know;
  double *gain_u, *gain_t, *ff_u, *ff_t, *summary, *jac, *jac_u, *jac_nav;
};

// io: device pointers, ws of gains_ws_bytes.  Options already checked by the caller.  Only enqueues two kernels on c.stream:
// f_fly, then g_gains, or g_gains_ff where io.ff_dir is given.  Returns ASCENT_OK / ASCENT_E_HIP.
int gains_run(const Call &c, int substeps, const GainsIO &io, double *ws);

}  // namespace ascent
