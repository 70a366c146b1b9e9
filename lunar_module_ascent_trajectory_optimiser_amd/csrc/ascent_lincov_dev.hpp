// Device helper shared by the linear covariance sweeps (ascent_lincov.hip: l_lincov, l_lincov_drifting; ascent_navfilter.hip:
// l_lincov_filtered): the radius of a nominal node, whose bits nominal_out shares with hist_out.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "ascent_device.hpp"

namespace ascent {

// the nominal node in metres about the centre and its radius rr: the operations of f_history_stats' altitude (ascent_disperse.hip:
// altitude_of), none contracted, so that rr - R0 in nominal_out has the bits of hist_out.  The altitude's gradient is formed from
// the same three values
struct Radius { double X, Y, rr; };

ASC_DEV Radius nominal_radius(double x, double y, double r_peri, double R0) {
#pragma clang fp contract(off)
  const double X = x * r_peri, Y = y * r_peri + R0;
  return {X, Y, sqrt(X * X + Y * Y)};
}

}  // namespace ascent
