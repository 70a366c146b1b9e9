// Host interface of the fused one-lane-per-NLP kernels (ascent_fused.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"

namespace ascent {

// bytes of workspace for `batch` problems on K = n_nodes-1 steps (one tile of 64 NLPs per wavefront)
size_t fused_ws_bytes(int K, long batch);

// One grid level: k_solve runs the whole interior-point loop of every NLP.  All device pointers (blob / traj layouts of
// include/ascent.h); asynchronous on `stream`.  Returns ASCENT_OK or ASCENT_E_HIP.
int fused_run(const ascent_params *dp, long batch, int K, double *ws, const double *dguess, int warm, int max_iter, double tol,
              double mu0, double *dtraj, double *dtf, int *dstatus, int *diters, double *dblob, hipStream_t stream, char *err,
              size_t errlen);

// Parity surfaces: one Newton step at a caller-supplied iterate, mu and delta_w (k_kkt_step; dinertia[p] = 1 where the
// factorisation was refused), and the defects, Jacobian and Hessian blocks of every collocation step (k_eval_nodes).
int fused_probe(const ascent_params *dp, long batch, int K, double *ws, const double *diterate, const double *dmu, const double *ddw,
                double *dstep, int *dinertia, hipStream_t stream, char *err, size_t errlen);
int fused_eval_nodes(const ascent_params *dp, long batch, int K, const double *diterate, double *ddefects, double *djac, double *dhess,
                     hipStream_t stream, char *err, size_t errlen);

}  // namespace ascent
