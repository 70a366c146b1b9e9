// Host interface of the post-optimal sensitivity kernel (ascent_sens.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"
#include "ascent_host.hpp"

namespace ascent {

// dJ*/dp of every NLP at its solution blob (envelope theorem; include/ascent.h: ascent_param_sensitivity).  Device pointers:
// c.dp[batch], dblob [21K+10][batch], dgrad [16][batch].  Options already checked by the caller (schemes 0/1/2, formulation 1 with
// scheme 0 only).  terminal: ascent_opts.terminal itself, 0/1/2 (the chain rule of terminal 1 is the kernel's own; c.dp are the
// caller's parameters).  Only enqueues on c.stream.  Returns ASCENT_OK / ASCENT_E_HIP.
int sens_run(const Call &c, int terminal, const double *dblob, double *dgrad);

// problems per workgroup of sens_run for a batch (a power of two, 1 .. 64; the rest of the workgroup's lanes split the steps)
int sens_problems_per_group(long batch);

}  // namespace ascent
