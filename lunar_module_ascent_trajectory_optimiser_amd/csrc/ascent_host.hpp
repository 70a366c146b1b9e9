// Host plumbing shared by the C ABI (ascent_solver.hip) and the host functions of the kernel families: the error macro, the
// descriptor of a call that every family host function takes first, and the requests of a solve and of a parity probe.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdio>
#include "ascent.h"

// a failed HIP call: its text and HIP's message go to (err, errlen), ASCENT_E_HIP to the caller
#define ASC_CHK(err, errlen, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { snprintf(err, errlen, "%s: %s", #call, hipGetErrorString(e_)); return ASCENT_E_HIP; } } while (0)

namespace ascent {

// What every family host function is told about a call.  dp: device pointer.  K: intervals of the grid the call works on.
// term: what the kernels see of ascent_opts.terminal, 2 or 0 (terminal 1 reaches them as transformed parameters).
struct Call {
  const ascent_params *dp;
  long batch;
  int K;
  int scheme, form, mp, term;
  hipStream_t stream;
  char *err;
  size_t errlen;
};

// o == nullptr: a call without options (the coast arc)
inline Call call_of(const ascent_params *dp, long batch, const ascent_opts *o, hipStream_t stream, char *err, size_t errlen) {
  if (!o) return Call{dp, batch, 0, 0, 0, 0, 0, stream, err, errlen};
  return Call{dp, batch, o->n_nodes - 1, (int)o->scheme, (int)o->formulation, (int)o->move_penalty, o->terminal == 2 ? 2 : 0, stream, err, errlen};
}

// One grid level of a solve (the *_run functions); device pointers, blob / traj layouts of include/ascent.h.  guess may be
// null when warm == 0; traj and blob may be null.
struct SolveIO {
  const double *guess;
  int warm, max_iter;
  double tol, mu0;
  double *traj, *tf;
  int *status, *iters;
  double *blob;
};

// One round at a caller-supplied iterate (the *_probe* functions of the parity surfaces); device pointers.  mu, dw: per
// problem.  step / inertia: the Newton step in the blob layout and its flag, or null for no step.  defects, jac, hess: the node
// rows in the layout of ascent_eval_nodes, or null.  records: the dense stage records, or null.
struct ProbeIO {
  const double *iterate, *mu, *dw;
  double *step;
  int *inertia;
  double *defects, *jac, *hess;
  double *records;
};

}  // namespace ascent
