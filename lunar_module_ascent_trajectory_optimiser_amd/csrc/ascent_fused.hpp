// Host interface of the fused one-lane-per-NLP kernels (ascent_fused.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"
#include "ascent_host.hpp"

namespace ascent {

// bytes of workspace for `batch` problems on K = n_nodes-1 steps (one tile of 64 NLPs per wavefront)
size_t fused_ws_bytes(int K, long batch);

// One grid level: k_solve runs the whole interior-point loop of every NLP.  All device pointers (blob / traj layouts of
// include/ascent.h); asynchronous on c.stream.  Returns ASCENT_OK or ASCENT_E_HIP.
int fused_run(const Call &c, double *ws, const SolveIO &io);

// Parity surfaces: one Newton step at a caller-supplied iterate, mu and delta_w (k_kkt_step; io.inertia[p] = 1 where the
// factorisation was refused), and the defects, Jacobian and Hessian blocks of every collocation step (k_eval_nodes).
int fused_probe(const Call &c, double *ws, const ProbeIO &io);
int fused_eval_nodes(const Call &c, const ProbeIO &io);

}  // namespace ascent
