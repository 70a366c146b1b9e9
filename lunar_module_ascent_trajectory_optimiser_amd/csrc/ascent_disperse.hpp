// Host interface of the Monte Carlo dispersion (ascent_disperse.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"
#include "ascent_host.hpp"

namespace ascent {

// Device workspace (bytes) of disperse_run: the nominal trajectory and f_fly's summary rows, and ceil(samples / 256) partial
// records of 73 doubles per problem.  Nothing of size samples * K exists.
size_t disperse_ws_bytes(int K, long batch, int samples);

// include/ascent.h: ascent_disperse_batch.  Device pointers: c.dp[batch], dblob [21K+10][batch], dxi [24 + K][samples] ([24][samples]
// with dsigma_u null), dsigma [24][batch], dsigma_u [K][batch] or null, dstats [ASCENT_DISPERSE_STAT_ROWS][batch], dsamples
// [9][samples][batch] or null, ws of disperse_ws_bytes.  Options already checked by the caller.  Only enqueues on c.stream: f_fly,
// f_disperse (one launch per 2^22 workgroups) and f_disperse_stats.  Returns ASCENT_OK / ASCENT_E_HIP.
int disperse_run(const Call &c, int substeps, int samples, const double *dblob, const double *dxi, const double *dsigma,
                 const double *dsigma_u, double *dstats, double *dsamples, double *ws);

// include/ascent.h: ascent_disperse_guided_batch.  As disperse_run, plus dgain_u [7][K][batch], dgain_t [7][batch] or null,
// dsmax [batch] or null; dsamples [12][samples][batch] or null.  Same workspace, same three enqueues with f_disperse_guided in
// f_disperse's place.
int disperse_guided_run(const Call &c, int substeps, int samples, const double *dblob, const double *dxi, const double *dsigma,
                        const double *dsigma_u, const double *dgain_u, const double *dgain_t, const double *dsmax, double *dstats,
                        double *dsamples, double *ws);

// include/ascent.h: ascent_disperse_navigated_batch.  As disperse_guided_run, plus dff_u [K][batch], dff_t [batch], dff_know
// [16][batch], dxi_nav [ASCENT_NAV_ROWS][samples], dsigma_nav [ASCENT_NAV_ROWS][batch], each or null.  Same workspace, same three
// enqueues with f_disperse_navigated in f_disperse_guided's place.
int disperse_navigated_run(const Call &c, int substeps, int samples, const double *dblob, const double *dxi, const double *dsigma,
                           const double *dsigma_u, const double *dgain_u, const double *dgain_t, const double *dsmax,
                           const double *dff_u, const double *dff_t, const double *dff_know, const double *dxi_nav,
                           const double *dsigma_nav, double *dstats, double *dsamples, double *ws);

}  // namespace ascent
