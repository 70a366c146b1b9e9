// Device helpers of the flight verification (ascent_flight.hip) shared with the flight Jacobian and the trim
// (ascent_trim.hip) and the dispersion (ascent_disperse.hip): the substep rule, the right-hand side, one RK4 collocation step,
// the two-body apsides, a node of a flown trajectory, the wavefront sum, and the two NaN rules every family member follows:
// finite1 and the NaN-propagating maximum.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "ascent.h"
#include "ascent_device.hpp"

namespace ascent {

ASC_DEV bool finite1(double a) { return fabs(a) <= 1.79769313486231570815e308; }      // false for NaN, +-inf
// the maximum that a NaN wins (fmax drops it): an unconverged blob shows as NaN, not as its largest finite value
ASC_DEV double max_nan(double a, double b) { return (a != a || b != b) ? NAN : fmax(a, b); }

// substeps per collocation step: the caller's, or (0) dt / 0.5 s rounded up, 1 .. ASCENT_FLIGHT_MAX_SUBSTEPS; whatever the
// blob holds, the loops below are bounded by it
ASC_DEV int flight_substeps(double dt, int substeps) {
  if (substeps > 0) return substeps;
  if (!finite1(dt)) return 1;
  const double q = ceil(dt / 0.5);
  return q >= (double)ASCENT_FLIGHT_MAX_SUBSTEPS ? ASCENT_FLIGHT_MAX_SUBSTEPS : q >= 1.0 ? (int)q : 1;
}

template <int FORM>
ASC_DEV void flight_f(const Der &d, const double *z, double u, double *F) {
  double ax, ay;
  accel<0>(d, z[IX], z[IY], z[IA], z[IM], 0.0, 0.0, ax, ay, nullptr, nullptr);
  rhs_f<FORM>(d, z, u, ax, ay, F);
}

// one collocation step: m classical RK4 steps of size hs under the held control u
template <int FORM>
ASC_DEV void fly_step(const Der &d, double *z, double u, double hs, int m) {
  if (FORM == 1) { z[IA] = 0.5 * d.aub * (u + 1.0); z[IW] = 0.0; }
  for (int j = 0; j < m; j++) {
    double k1[7], k2[7], k3[7], k4[7], w[7];
    flight_f<FORM>(d, z, u, k1);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) w[i] = z[i] + 0.5 * hs * k1[i];
    flight_f<FORM>(d, w, u, k2);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) w[i] = z[i] + 0.5 * hs * k2[i];
    flight_f<FORM>(d, w, u, k3);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) w[i] = z[i] + hs * k3[i];
    flight_f<FORM>(d, w, u, k4);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) z[i] += hs * (1.0 / 6.0) * (k1[i] + 2.0 * (k2[i] + k3[i]) + k4[i]);
  }
}

// periapsis / apoapsis altitude above R0 (m) of the two-body orbit through a scaled state, the library's one definition (the
// flight summary, the trim and k_coast call it): eccentricity vector; periapsis from the semi-latus rectum, h^2 / (GM (1 + e)) --
// a (1 - e) carries the rounding of a, 1 / (1 - e) times larger: 4e-9 m at e = 0.9 --; apoapsis a (1 + e) with the semi-major
// axis from the vis-viva equation, +inf for specific energy >= 0
ASC_DEV void apsides_of(const ascent_params &prm, double x, double y, double vx, double vy, double &peri, double &apo) {
  const double S = prm.r_peri, GM = prm.G * prm.M;
  const double X = x * S, Y = y * S + prm.R0, VX = vx * S, VY = vy * S;
  const double r = sqrt(X * X + Y * Y), v2 = VX * VX + VY * VY, rv = X * VX + Y * VY;
  const double ex = (v2 / GM - 1.0 / r) * X - rv / GM * VX, ey = (v2 / GM - 1.0 / r) * Y - rv / GM * VY;
  const double e = sqrt(ex * ex + ey * ey);
  const double h = X * VY - Y * VX;
  peri = h * h / (GM * (1.0 + e)) - prm.R0;
  apo = 0.5 * v2 - GM / r >= 0.0 ? INFINITY : (1.0 + e) / (2.0 / r - v2 / GM) - prm.R0;
}

// the 7-state of node k in a trajectory of ascent_fly_batch's layout (fields x y xdot ydot ax ay angle angledot u mass)
ASC_DEV void load_node(const double *__restrict__ tr, size_t B, int nt, int k, double *z) {
  z[IX] = tr[((size_t)0 * nt + k) * B];
  z[IY] = tr[((size_t)1 * nt + k) * B];
  z[IVX] = tr[((size_t)2 * nt + k) * B];
  z[IVY] = tr[((size_t)3 * nt + k) * B];
  z[IA] = tr[((size_t)6 * nt + k) * B];
  z[IW] = tr[((size_t)7 * nt + k) * B];
  z[IM] = tr[((size_t)9 * nt + k) * B];
}

// sum over the 64 lanes of a wavefront
ASC_DEV double wave_sum(double v) {          // butterfly: every lane ends with the same bits
  ASC_UNROLL
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

}  // namespace ascent
