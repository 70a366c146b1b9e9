// Host interface of the Monte Carlo dispersion (ascent_disperse.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"
#include "ascent_host.hpp"

namespace ascent {

// Device workspace (bytes) of disperse_run: the nominal trajectory and f_fly's summary rows, and ceil(samples / 256) partial
// records of 73 doubles per problem.  Nothing of size samples * K exists.  node_stride > 0 (the history call): also
// ceil(samples / 256) * NJ partial records of 42 doubles per problem, NJ = history_nodes(K, node_stride).
size_t disperse_ws_bytes(int K, long batch, int samples, int node_stride = 0);
int history_nodes(int K, int node_stride);      // K / node_stride, and the last node where that leaves it out

// The three dispersion calls of include/ascent.h differ in what they are given, not in what is done with it
enum DisperseKind { DISPERSE_OPEN = 0 /* ascent_disperse_batch */, DISPERSE_GUIDED /* .._guided_batch */, DISPERSE_NAVIGATED /* .._navigated_batch */ };

// The arrays of a dispersion call, host or device pointers alike; null where the caller gave none or the kind has none.
// blob [21K+10][batch], xi [24 + K][samples] ([24][samples] with sigma_u null), sigma [24][batch], sigma_u [K][batch];
// guided and navigated: gain_u [7][K][batch], gain_t [7][batch], stretch_max [batch];
// navigated: ff_u [K][batch], ff_t [batch], ff_know [16][batch], xi_nav [ASCENT_NAV_ROWS][samples], sigma_nav [ASCENT_NAV_ROWS][batch];
// stats [ASCENT_DISPERSE_STAT_ROWS][batch], samples_out [9 (open) | ASCENT_GUIDED_SAMPLE_ROWS][samples][batch];
// the history call (hist not null; samples_out then always ASCENT_GUIDED_SAMPLE_ROWS): node_stride, hist
// [ASCENT_HISTORY_ROWS][NJ][batch], hist_samples [ASCENT_HISTORY_QUANTITIES][NJ][samples][batch];
// the drifting call (ascent_disperse_drifting_batch; nav_phi not null, with hist and gain_u): nav_phi and nav_q
// [ASCENT_NAV_ROWS][batch], xi_drift [ASCENT_NAV_ROWS][K][samples].
struct DisperseIO {
  const double *blob, *xi, *sigma, *sigma_u;
  const double *gain_u, *gain_t, *stretch_max;
  const double *ff_u, *ff_t, *ff_know, *xi_nav, *sigma_nav;
  double *stats, *samples_out;
  int node_stride;
  double *hist, *hist_samples;
  const double *nav_phi, *nav_q, *xi_drift;
};

// io: device pointers, ws of disperse_ws_bytes.  Options already checked by the caller.  Only enqueues on c.stream: f_fly, the
// kind's kernel -- f_disperse, f_disperse_guided or f_disperse_navigated, one launch per 2^22 workgroups -- and f_disperse_stats.
// With io.hist: f_disperse<FORM, true> (open), f_history_guided (guided and navigated alike) or, with io.nav_phi, f_history_drifting
// in the kernel's place, and f_history_stats last.
// Returns ASCENT_OK / ASCENT_E_HIP.
int disperse_run(const Call &c, DisperseKind kind, int substeps, int samples, const DisperseIO &io, double *ws);

}  // namespace ascent
