// Host interface of the dense-block solver path (ascent_dense.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"
#include "ascent_host.hpp"

namespace ascent {

// bytes of workspace for `batch` problems on K = n_nodes-1 steps
size_t dense_ws_bytes(int K, long batch);
size_t dense_pcr_ws_bytes(int K, long batch);     // with the PCR variant's block images

// Solve one grid level (schemes 0/1/2; c.term 0/2).  The host reads one counter per burst of four rounds.  pcr: the Newton
// systems are solved by parallel cyclic reduction over the nodes (workspace dense_pcr_ws_bytes) instead of the serial Riccati
// recursion.  c.mp: the objective gains params.dcost * sum_k |u_k - u_{k-1}| (the reference's MV DCOST, LO:99; both Newton
// solvers).  Returns ASCENT_OK / ASCENT_E_HIP / ASCENT_E_NOTERM.
int dense_run(const Call &c, double *ws, const SolveIO &io, bool pcr);

// Parity surface: one Newton step at a caller-supplied iterate (io.step; io.inertia receives 0 / nonzero), and/or the dense stage
// records of every step as d_eval leaves them, io.records[batch][K][6][64] (grids Ja, Jb, Haa, Hab, Hbb and the vector grid).
int dense_probe(const Call &c, double *ws, const ProbeIO &io, bool pcr);

// Kepler-exact coast arc from every NLP's burnout state (scaled x, y, xdot, ydot: dstate4[4][batch]) to the next apoapsis:
// dcoast[4][nc+1][batch], dtheta2[batch] (duration / T_scale), dapsides[2][batch] (periapsis, apoapsis altitude in m).
int coast_run(const Call &c, const double *dstate4, int nc, double *dcoast, double *dtheta2, double *dapsides);

}  // namespace ascent
