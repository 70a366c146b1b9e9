// Device helpers of the flight Jacobian (ascent_trim.hip: j_jac) shared with the guidance gains (ascent_guide.hip: g_gains): the
// shape of a workgroup and of a step record, one RK4 collocation step with a tangent column carried along, the gradient of the
// two-body apsides, and the two ends of the Jacobian's sweep: the rows of Lambda_K it starts from (lambda_apsis_rows) and the chain
// rule from its accumulators to the 24 columns (jac_columns), with that rule's transpose for a direction of the parameters
// (tangent_coefficients).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "ascent.h"
#include "ascent_device.hpp"
#include "ascent_flight_dev.hpp"

namespace ascent {

constexpr int JB = 256;                    // j_jac, g_gains: threads per workgroup
constexpr int CH = 16;                     // steps per chunk = groups per workgroup
constexpr int NCOL = 16;                   // tangent columns per step = lanes per group
constexpr int REC = 7 * NCOL;              // doubles per step record
constexpr int C_U = 7, C_DT = 8, C_DER = 9, C_ALPHA = 14, C_MRATE = 15;      // C_DER + ACC_RHO0 .. ACC_MS, then alpha | angle_ub, mrate
constexpr int NACC = 8;                    // accumulators of the sweep: columns C_DT .. C_MRATE
constexpr int JROWS = 9, JCOLS = 24;

// f(z, u) and its tangent dF = f_z dz + (the column's own forcing): (fx, fy) picked from d accel / d Der for the columns
// C_DER .. C_DER + 4, cw on the angledot row (alpha for the control column, u for the alpha column), cm on the mass row (mrate)
template <int FORM>
ASC_DEV void stage(const Der &d, const double *z, const double *dz, double u, int col, double cw, double cm, double *F, double *dF) {
  double ax, ay, G[8], dax[ACC_NDER], day[ACC_NDER];
  accel<1>(d, z[IX], z[IY], z[IA], z[IM], 0.0, 0.0, ax, ay, G, nullptr);
  accel_dder(d, z[IX], z[IY], z[IA], z[IM], dax, day);
  rhs_f<FORM>(d, z, u, ax, ay, F);
  double fx = 0.0, fy = 0.0;
  ASC_UNROLL
  for (int j = 0; j < ACC_NDER; j++) {
    const bool s = col == C_DER + j;
    fx = s ? dax[j] : fx;
    fy = s ? day[j] : fy;
  }
  dF[IX] = dz[IVX];
  dF[IY] = dz[IVY];
  dF[IVX] = G[0] * dz[IX] + G[1] * dz[IY] + G[2] * dz[IA] + G[3] * dz[IM] + fx;
  dF[IVY] = G[4] * dz[IX] + G[5] * dz[IY] + G[6] * dz[IA] + G[7] * dz[IM] + fy;
  dF[IA] = FORM == 1 ? 0.0 : dz[IW];
  dF[IW] = FORM == 1 ? 0.0 : cw;
  dF[IM] = cm;
}

// fly_step (ascent_flight_dev.hpp) with one tangent column carried along: z the same arithmetic, dz the exact derivative of it
template <int FORM>
ASC_DEV void fly_step_tangent(const Der &d, double *z, double *dz, double u, double hs, int m, int col) {
  double cw = 0.0, cm = col == C_MRATE ? 1.0 : 0.0;
  const double dhs = col == C_DT ? 1.0 / m : 0.0;      // hs = dt / m
  if (FORM == 1) {
    z[IA] = 0.5 * d.aub * (u + 1.0); z[IW] = 0.0;
    dz[IA] = col == C_U ? 0.5 * d.aub : col == C_ALPHA ? 0.5 * (u + 1.0) : 0.0;
    dz[IW] = 0.0;
  } else {
    cw = col == C_U ? d.alpha : col == C_ALPHA ? u : 0.0;
  }
  for (int j = 0; j < m; j++) {
    double k1[7], k2[7], k3[7], k4[7], w[7], d1[7], d2[7], d3[7], d4[7], dw[7];
    stage<FORM>(d, z, dz, u, col, cw, cm, k1, d1);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) { w[i] = z[i] + 0.5 * hs * k1[i]; dw[i] = dz[i] + 0.5 * (hs * d1[i] + dhs * k1[i]); }
    stage<FORM>(d, w, dw, u, col, cw, cm, k2, d2);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) { w[i] = z[i] + 0.5 * hs * k2[i]; dw[i] = dz[i] + 0.5 * (hs * d2[i] + dhs * k2[i]); }
    stage<FORM>(d, w, dw, u, col, cw, cm, k3, d3);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) { w[i] = z[i] + hs * k3[i]; dw[i] = dz[i] + (hs * d3[i] + dhs * k3[i]); }
    stage<FORM>(d, w, dw, u, col, cw, cm, k4, d4);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) {
      const double ks = k1[i] + 2.0 * (k2[i] + k3[i]) + k4[i], ds = d1[i] + 2.0 * (d2[i] + d3[i]) + d4[i];
      z[i] += hs * (1.0 / 6.0) * ks;
      dz[i] += (1.0 / 6.0) * (hs * ds + dhs * ks);
    }
  }
}

// Gradients of apsides_of's periapsis / apoapsis altitude with respect to (X, Y, VX, VY, GM) in SI units at a scaled state;
// returns false where the specific energy is >= 0 (the apoapsis gradient is then NaN).  With E = v^2/2 - GM/r, h = X VY - Y VX,
// a = -GM / (2 E) and the eccentricity vector (ex, ey) = (v^2/GM - 1/r) r - (r.v/GM) v of apsides_of: periapsis a (1 - e),
// apoapsis a (1 + e); E >= 0: periapsis h^2 / (GM (1 + e)).  e and its gradient come from the vector, de = (ex dex + ey dey) / e
// (accurate to about eps / e; e^2 = 1 + 2 E h^2 / GM^2 loses eps / e^2).  At e exactly 0 the apsides have a kink (e = |(ex, ey)|)
// and no gradient: de is set to 0, so that both rows are the gradient of a - R0, the mean of the one-sided derivatives.
ASC_DEV bool apsides_grad(const ascent_params &prm, double x, double y, double vx, double vy, double *gp, double *ga) {
  const double S = prm.r_peri, GM = prm.G * prm.M;
  const double X = x * S, Y = y * S + prm.R0, VX = vx * S, VY = vy * S;
  const double r = sqrt(X * X + Y * Y), v2 = VX * VX + VY * VY, rv = X * VX + Y * VY;
  const double E = 0.5 * v2 - GM / r, h = X * VY - Y * VX;
  const double ir3 = 1.0 / (r * r * r);
  const double c = v2 / GM - 1.0 / r, d = rv / GM;      // (ex, ey) = c (X, Y) - d (VX, VY)
  const double ex = c * X - d * VX, ey = c * Y - d * VY;
  const double e = sqrt(ex * ex + ey * ey);
  const double dE[5] = {GM * X * ir3, GM * Y * ir3, VX, VY, -1.0 / r};
  const double dh[5] = {VY, -VX, -Y, X, 0.0};
  const double dc[5] = {X * ir3, Y * ir3, 2.0 * VX / GM, 2.0 * VY / GM, -v2 / (GM * GM)};
  const double dd[5] = {VX / GM, VY / GM, X / GM, Y / GM, -rv / (GM * GM)};
  double de[5];
  ASC_UNROLL
  for (int i = 0; i < 5; i++) {
    const double dex = dc[i] * X - dd[i] * VX + (i == 0 ? c : 0.0) - (i == 2 ? d : 0.0);
    const double dey = dc[i] * Y - dd[i] * VY + (i == 1 ? c : 0.0) - (i == 3 ? d : 0.0);
    de[i] = e > 0.0 ? (ex * dex + ey * dey) / e : 0.0;
  }
  if (E >= 0.0) {
    const double q = 1.0 / (GM * (1.0 + e));
    ASC_UNROLL
    for (int i = 0; i < 5; i++) { gp[i] = 2.0 * h * q * dh[i] - h * h * q / (1.0 + e) * de[i]; ga[i] = NAN; }
    gp[4] -= h * h * q / GM;
    return false;
  }
  const double a = -GM / (2.0 * E);
  double da[5];
  ASC_UNROLL
  for (int i = 0; i < 5; i++) da[i] = GM / (2.0 * E * E) * dE[i];
  da[4] -= 1.0 / (2.0 * E);
  ASC_UNROLL
  for (int i = 0; i < 5; i++) { gp[i] = (1.0 - e) * da[i] - a * de[i]; ga[i] = (1.0 + e) * da[i] + a * de[i]; }
  return true;
}

// the direct dependence of an apsis row on G, M, R0 and r_peri (the sweep carries only what passes through the flown state)
struct ApsisDirect { double G, M, R0, S; };

// Lambda_K is the Jacobian of the nine end quantities with respect to the flown last state zK: the identity for the seven states
// -- the caller's L[i] = q == i, for every thread, and dir = 0 -- and here, for the lanes of the sweeping wavefront, rows q = 7 / 8:
// the gradient of the periapsis / apoapsis altitude and its direct terms.  (The identity stays outside and the gradient is
// taken by every lane that calls: with either inside the branch j_jac is no longer the parent's instruction stream.)
ASC_DEV void lambda_apsis_rows(const ascent_params &prm, const double *zK, int q, double *L, ApsisDirect &dir) {
  double gp[5], ga[5];
  apsides_grad(prm, zK[IX], zK[IY], zK[IVX], zK[IVY], gp, ga);
  if (q == 7 || q == 8) {
    const double *gq = q == 7 ? gp : ga;
    const double S = prm.r_peri;
    L[IX] = S * gq[0]; L[IY] = S * gq[1]; L[IVX] = S * gq[2]; L[IVY] = S * gq[3];
    dir.S = zK[IX] * gq[0] + zK[IY] * gq[1] + zK[IVX] * gq[2] + zK[IVY] * gq[3];
    dir.R0 = gq[1] - 1.0;
    dir.G = prm.M * gq[4];
    dir.M = prm.G * gq[4];
  }
}

// The chain rule d(dt, Der)/d(params, t_f) (derive of ascent_device.hpp) at the end of the sweep: one row of the Jacobian, o[24] =
// [z_0 | the 16 fields | t_f], from its row L0 of Lambda_0, its accumulators A[NACC] (columns C_DT .. C_MRATE summed over the
// steps) and its direct terms.  tf: the blob's, K: intervals.
template <int FORM>
ASC_DEV void jac_columns(const ascent_params &prm, const Der &d, double tf, int K, const double *L0, const double *A,
                         const ApsisDirect &dir, double *o) {
  const double S = prm.r_peri, R0 = prm.R0;
  const double aDT = A[0], aRHO0 = A[1 + ACC_RHO0], aGAM = A[1 + ACC_GAM], aTHR = A[1 + ACC_THR], aM0 = A[1 + ACC_M0],
               aMS = A[1 + ACC_MS], aAL = A[C_ALPHA - C_DT], aMR = A[C_MRATE - C_DT];
  ASC_UNROLL
  for (int i = 0; i < 7; i++) o[i] = L0[i];
  const double S3 = S * S * S;
  o[7 + 0] = aGAM * prm.M / S3 + dir.G;                             // G
  o[7 + 1] = aGAM * prm.G / S3 + dir.M;                             // M
  o[7 + 2] = aRHO0 / S + dir.R0;                                    // R0
  o[7 + 3] = aTHR / S;                                              // Ft
  o[7 + 4] = aM0;                                                   // M0
  o[7 + 5] = aMR / prm.fuel_mass;                                   // mdot
  o[7 + 6] = -aMR * d.mrate / prm.fuel_mass;                        // fuel_mass
  o[7 + 7] = aMS;                                                   // mass_scalar
  o[7 + 8] = FORM == 1 ? 0.0 : aAL / 3.0;                           // ang_acc_max
  o[7 + 9] = -aRHO0 * R0 / (S * S) - 3.0 * aGAM * d.gam / S - aTHR * d.thr / S + dir.S;     // r_peri
  o[7 + 10] = 0.0;                                                  // r_apo
  o[7 + 11] = aDT * (tf / K);                                       // T_scale
  o[7 + 12] = FORM == 1 ? aAL : 0.0;                                // angle_ub
  o[7 + 13] = 0.0; o[7 + 14] = 0.0; o[7 + 15] = 0.0;                // tf_lb, tf_ub, dcost
  o[23] = aDT * (d.T / K);                                          // t_f
}

// The transpose of the rule above without its direct terms: what a unit step along the direction dd of the 16 fields does to
// (dt, Der), coef[NACC] in the order of the accumulators -- column by column the factors of jac_columns.
template <int FORM>
ASC_DEV void tangent_coefficients(const ascent_params &prm, const Der &d, double tf, int K, const double *dd, double *coef) {
  const double S = prm.r_peri, S3 = S * S * S;
  coef[0] = dd[11] * (tf / K);
  coef[1 + ACC_RHO0] = dd[2] / S - dd[9] * prm.R0 / (S * S);
  coef[1 + ACC_GAM] = dd[0] * prm.M / S3 + dd[1] * prm.G / S3 - dd[9] * 3.0 * d.gam / S;
  coef[1 + ACC_THR] = dd[3] / S - dd[9] * d.thr / S;
  coef[1 + ACC_M0] = dd[4];
  coef[1 + ACC_MS] = dd[7];
  coef[C_ALPHA - C_DT] = FORM == 1 ? dd[12] : dd[8] / 3.0;
  coef[C_MRATE - C_DT] = dd[5] / prm.fuel_mass - dd[6] * d.mrate / prm.fuel_mass;
}

}  // namespace ascent
