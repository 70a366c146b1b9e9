// Flight verification (include/ascent.h: ascent_fly_batch): the ODEs of the model integrated under the control of a
// solution blob, beside what the NLP says about the same trajectory.
//
// Model: z = (x, y, xdot, ydot, angle, angledot, mass), dz/dt = f(z, u) per second (rhs_f, accel<0> of ascent_device.hpp; the
// defect of every scheme is z_k - z_{k-1} - Phi with Phi ~ dt f, dt = tf T / K).  Node 0 is the zero initial state; step k
// (node k-1 -> k) flies with the blob's u_k held constant -- what all three defects assume (ascent_sens.hip).  Formulation 1:
// the angle itself is held at (angle_ub/2)(u_k + 1) over step k and angledot stays 0.  The terminal mode and the move penalty
// do not enter the ODEs.  Integrator: classical RK4, every collocation step cut into m equal substeps (flight_substeps).
//
// f_fly    serial in time, one lane per NLP (64 NLPs per wavefront): with problem-fastest rows the wavefront's load of u_k and
//          its stores of the ten trajectory rows of a node are contiguous 512-byte runs.  The next step's control is loaded
//          before the current step is integrated.  Latency-bound: 4 m K dependent right-hand sides per lane.  Owns summary
//          rows 0..5 and 9.
// f_local  no dependency between steps: start from the NLP's z_{k-1}, integrate step k with the same RK4 and m, eta_k = flown
//          - z_k.  A workgroup of LB threads covers PB consecutive NLPs (PB a power of two, sens_problems_per_group); thread t
//          takes NLP t % PB and the steps k = t / PB + 1, + LB/PB, ...  Owns summary rows 6..8: the maxima over the steps are
//          reduced over the lanes of one NLP with cross-lane shuffles, then over the waves in LDS, in a fixed order (results
//          depend on the batch size only through PB, never on timing).
// flight_ws (ascent_flight.hpp) is the head of every workspace that starts with a fly-out; finite1 and max_nan, the family's two
// NaN rules, are in ascent_flight_dev.hpp.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>

#include "ascent.h"
#include "ascent_device.hpp"
#include "ascent_flight.hpp"
#include "ascent_flight_dev.hpp"
#include "ascent_sens.hpp"

namespace ascent {
namespace {

constexpr int FW = 64;                     // f_fly: threads per workgroup (one wavefront)
constexpr int LB = 256;                    // f_local: threads per workgroup
constexpr int LNW = LB / 64;

template <int FORM>
__global__ __launch_bounds__(FW) void f_fly(const ascent_params *__restrict__ P, long batch, int K, int substeps,
                                            const double *__restrict__ blob, double *__restrict__ traj,
                                            double *__restrict__ summary) {
  const long p = (long)blockIdx.x * FW + threadIdx.x;
  if (p >= batch) return;
  const size_t B = (size_t)batch;
  const int nt = K + 1;
  const double *b = blob + p;
  const ascent_params prm = P[p];
  const Der d = derive(prm);
  const double tf = b[(size_t)(21 * K + S_TH) * B];
  const double dt = (tf * d.T) / K;
  const int m = flight_substeps(dt, substeps);
  const double hs = dt / m;
  double z[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (traj) {
    double ax, ay;
    accel<0>(d, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, ax, ay, nullptr, nullptr);
    const double v[10] = {0.0, 0.0, 0.0, 0.0, ax, ay, 0.0, 0.0, 0.0, 0.0};
    ASC_UNROLL
    for (int f = 0; f < 10; f++) traj[((size_t)f * nt) * B + p] = v[f];
  }
  double u = b[(size_t)(7 * K) * B];
  for (int k = 0; k < K; k++) {
    const double un = b[(size_t)(7 * K + (k + 1 < K ? k + 1 : k)) * B];
    fly_step<FORM>(d, z, u, hs, m);
    if (traj) {
      double ax, ay;
      accel<0>(d, z[IX], z[IY], z[IA], z[IM], 0.0, 0.0, ax, ay, nullptr, nullptr);
      const double v[10] = {z[IX], z[IY], z[IVX], z[IVY], ax, ay, z[IA], z[IW], u, z[IM]};
      ASC_UNROLL
      for (int f = 0; f < 10; f++) traj[((size_t)f * nt + k + 1) * B + p] = v[f];
    }
    u = un;
  }
  double zn[4];
  ASC_UNROLL
  for (int i = 0; i < 4; i++) zn[i] = b[(size_t)(7 * (K - 1) + i) * B];
  const double S = prm.r_peri;
  const double dx = z[IX] - zn[IX], dy = z[IY] - zn[IY], dvx = z[IVX] - zn[IVX], dvy = z[IVY] - zn[IVY];
  double pf, af, pn, an;
  apsides_of(prm, z[IX], z[IY], z[IVX], z[IVY], pf, af);
  apsides_of(prm, zn[IX], zn[IY], zn[IVX], zn[IVY], pn, an);
  summary[(size_t)0 * B + p] = S * sqrt(dx * dx + dy * dy);
  summary[(size_t)1 * B + p] = S * sqrt(dvx * dvx + dvy * dvy);
  summary[(size_t)2 * B + p] = pf;
  summary[(size_t)3 * B + p] = af;
  summary[(size_t)4 * B + p] = pn;
  summary[(size_t)5 * B + p] = an;
  summary[(size_t)9 * B + p] = (double)m;
}

// running maxima over the steps.  Position error with the step where it is attained (k = 0: none yet): the larger value wins,
// the lower step among equals, and a NaN beats every number (an unconverged blob shows as NaN, not as its largest finite
// error).  Velocity error: the value alone, same rule.
ASC_DEV void max_at(double &v, int &k, double w, int l) {         // (v, k) <- the winner of (v, k) and (w, l)
  if (l == 0) return;
  bool take = k == 0;
  if (!take) {
    const bool vn = v != v, wn = w != w;
    take = vn != wn ? wn : (vn || v == w) ? l < k : w > v;
  }
  if (take) { v = w; k = l; }
}

template <int FORM>
__global__ __launch_bounds__(LB) void f_local(const ascent_params *__restrict__ P, long batch, int K, int pb, int substeps,
                                              const double *__restrict__ blob, double *__restrict__ local,
                                              double *__restrict__ summary) {
  __shared__ double rpos[LNW][64], rvel[LNW][64];
  __shared__ int rk[LNW][64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int slot = t / pb, nslot = LB / pb;
  const long p = (long)blockIdx.x * pb + (t & (pb - 1));
  const bool on = p < batch;
  double mpv = -1.0, mv = -1.0;
  int mpk = 0;
  if (on) {
    const size_t B = (size_t)batch;
    const double *b = blob + p;
    const Der d = derive(P[p]);
    const double tf = b[(size_t)(21 * K + S_TH) * B];
    const double dt = (tf * d.T) / K;
    const int m = flight_substeps(dt, substeps);
    const double hs = dt / m;
    for (int k = slot; k < K; k += nslot) {       // step k + 1
      double z[7], zb[7];
      ASC_UNROLL
      for (int i = 0; i < 7; i++) z[i] = k ? b[(size_t)(7 * (k - 1) + i) * B] : 0.0;
      ASC_UNROLL
      for (int i = 0; i < 7; i++) zb[i] = b[(size_t)(7 * k + i) * B];
      const double u = b[(size_t)(7 * K + k) * B];
      fly_step<FORM>(d, z, u, hs, m);
      double eta[7];
      ASC_UNROLL
      for (int i = 0; i < 7; i++) eta[i] = z[i] - zb[i];
      if (local) {
        ASC_UNROLL
        for (int i = 0; i < 7; i++) local[(size_t)(7 * k + i) * B + p] = eta[i];
      }
      const double ep = sqrt(eta[IX] * eta[IX] + eta[IY] * eta[IY]), ev = sqrt(eta[IVX] * eta[IVX] + eta[IVY] * eta[IVY]);
      max_at(mpv, mpk, ep, k + 1);
      mv = max_nan(mv, ev);
    }
  }
  // the lanes of one NLP in a wave (lane = j + PB * i), then the waves, in a fixed order
  for (int off = 32; off >= pb; off >>= 1) {
    const double ov = __shfl_xor(mpv, off), ow = __shfl_xor(mv, off);
    const int ok = __shfl_xor(mpk, off);
    max_at(mpv, mpk, ov, ok);
    mv = max_nan(mv, ow);
  }
  if (lane < pb) { rpos[wv][lane] = mpv; rvel[wv][lane] = mv; rk[wv][lane] = mpk; }
  __syncthreads();
  if (t < pb && on) {
    for (int w = 1; w < LNW; w++) {
      max_at(mpv, mpk, rpos[w][t], rk[w][t]);
      mv = max_nan(mv, rvel[w][t]);
    }
    const double S = P[p].r_peri;
    const size_t B = (size_t)batch;
    summary[(size_t)6 * B + p] = S * mpv;
    summary[(size_t)7 * B + p] = S * mv;
    summary[(size_t)8 * B + p] = (double)mpk;
  }
}

}  // namespace

int flight_fly_only(const Call &c, int substeps, const double *dblob, double *dtraj, double *dsummary) {
  const dim3 gfly((unsigned)((c.batch + FW - 1) / FW)), bfly(FW);
  if (c.form == 1)
    hipLaunchKernelGGL((f_fly<1>), gfly, bfly, 0, c.stream, c.dp, c.batch, c.K, substeps, dblob, dtraj, dsummary);
  else
    hipLaunchKernelGGL((f_fly<0>), gfly, bfly, 0, c.stream, c.dp, c.batch, c.K, substeps, dblob, dtraj, dsummary);
  ASC_CHK(c.err, c.errlen, hipGetLastError());
  return ASCENT_OK;
}

int flight_run(const Call &c, int substeps, const double *dblob, double *dtraj, double *dlocal, double *dsummary) {
  if (const int rc = flight_fly_only(c, substeps, dblob, dtraj, dsummary)) return rc;
  const int pb = sens_problems_per_group(c.batch);      // the same split of a workgroup between NLPs and steps as s_sens
  const dim3 gloc((unsigned)((c.batch + pb - 1) / pb)), bloc(LB);
  if (c.form == 1)
    hipLaunchKernelGGL((f_local<1>), gloc, bloc, 0, c.stream, c.dp, c.batch, c.K, pb, substeps, dblob, dlocal, dsummary);
  else
    hipLaunchKernelGGL((f_local<0>), gloc, bloc, 0, c.stream, c.dp, c.batch, c.K, pb, substeps, dblob, dlocal, dsummary);
  ASC_CHK(c.err, c.errlen, hipGetLastError());
  return ASCENT_OK;
}

}  // namespace ascent
