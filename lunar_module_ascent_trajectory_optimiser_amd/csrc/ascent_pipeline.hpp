// Host interface of the split pipeline (ascent_pipeline.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"
#include "ascent_host.hpp"

namespace ascent {

struct PipelineStats {
  int launches = 0;
};

// bytes of workspace the pipeline needs for `batch` problems on K = n_nodes-1 steps
size_t pipeline_ws_bytes(int K, long batch);

// Solve one grid level; all pointers are device pointers.  Synchronises c.stream once per interior-point iteration
// (it reads three counters to steer the lanes' state machines).  `wide` picks the 16-lane sweeps.  Returns ASCENT_OK or ASCENT_E_HIP.
int pipeline_run(const Call &c, double *ws, const SolveIO &io, bool wide, PipelineStats *stats);

// One round of the pipeline's kernels at a caller-supplied iterate (the parity surface behind ascent_kkt_step /
// ascent_eval_nodes): mu and delta_w per problem; `wide` picks the 16-lane sweeps.  Without io.step only the
// node evaluation (q_trial_eval) runs.  Output pointers may be null.  All device pointers; asynchronous on c.stream.
int pipeline_probe(const Call &c, double *ws, const ProbeIO &io, bool wide);

}  // namespace ascent
