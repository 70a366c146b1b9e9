// Host interface of the order statistics of sample rows (ascent_quantile.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"

namespace ascent {

constexpr int QUANTILE_MAX_PROBS = 16, QUANTILE_MAX_LIMITS = 16;

// The arrays of a selection, device pointers but for probs (include/ascent.h: ascent_sample_quantiles).  values
// [Q][G][samples][batch]; a sample is valid where its rows q < V are finite; limits [n_limits][Q][batch] or null;
// count [G][batch] or null, quant [n_probs][Q][G][batch], below [n_limits][Q][G][batch] or null.
struct QuantileIO {
  const double *values;
  int Q, G, V, samples;
  long batch;
  double probs[QUANTILE_MAX_PROBS];
  int n_probs;
  const double *limits;
  int n_limits;
  double *count, *quant, *below;
};

// Only enqueues on the stream: q_sort (the rows of a tile of problems sorted in LDS) where the padded samples of one problem
// fit a workgroup's LDS, q_select (one workgroup per row, radix select from memory) above that.  Arguments already checked.
// Returns ASCENT_OK / ASCENT_E_HIP.
int quantile_run(const QuantileIO &io, hipStream_t stream, char *err, size_t errlen);

}  // namespace ascent
