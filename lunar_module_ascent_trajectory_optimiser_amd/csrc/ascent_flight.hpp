// Host interface of the flight-verification kernels (ascent_flight.hip), used by the C ABI in ascent_solver.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ascent.h"
#include "ascent_host.hpp"

namespace ascent {

// Fly every NLP's control with RK4 and compare with its solution blob (include/ascent.h: ascent_fly_batch).  Device pointers:
// c.dp[batch], dblob [21K+10][batch], dtraj [10(K+1)][batch] or null, dlocal [7K][batch] or null, dsummary
// [ASCENT_FLIGHT_ROWS][batch].  Options already checked by the caller (formulation 0 / 1, substeps 0 .. ASCENT_FLIGHT_MAX_SUBSTEPS).
// Only enqueues two kernels on c.stream (f_fly, f_local; they write disjoint rows).  Returns ASCENT_OK / ASCENT_E_HIP.
int flight_run(const Call &c, int substeps, const double *dblob, double *dtraj, double *dlocal, double *dsummary);

// The serial fly-out alone (f_fly; summary rows 0..5 and 9 only): the linearisation point of the flight Jacobian and every
// round of the trim (ascent_trim.hip).
int flight_fly_only(const Call &c, int substeps, const double *dblob, double *dtraj, double *dsummary);

// The head of every workspace that starts with a fly-out (the flight Jacobian, the trim, the guidance gains, the dispersion):
// flight_fly_only's trajectory [ASCENT_TRAJ_FIELDS (K + 1)][batch], its summary [ASCENT_FLIGHT_ROWS][batch], then the caller's own.
struct FlightWs { double *traj, *fsum, *rest; };
inline FlightWs flight_ws(double *ws, int K, long batch) {
  FlightWs w;
  w.traj = ws;
  w.fsum = w.traj + (size_t)ASCENT_TRAJ_FIELDS * (K + 1) * (size_t)batch;
  w.rest = w.fsum + (size_t)ASCENT_FLIGHT_ROWS * (size_t)batch;
  return w;
}
inline size_t flight_ws_bytes(int K, long batch) {
  return ((size_t)ASCENT_TRAJ_FIELDS * (K + 1) + ASCENT_FLIGHT_ROWS) * (size_t)batch * sizeof(double);
}

}  // namespace ascent
