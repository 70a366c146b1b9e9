// Flight Jacobian and trim (include/ascent.h: ascent_flight_jacobian, ascent_trim_batch).
//
// The map: F(z_0, p, t_f, u_1..u_K) -> the flown state at the last node exactly as f_fly computes it (ascent_flight.hip): K
// collocation steps of m classical RK4 substeps each, the control held over a step, m as flight_substeps picks it at the blob
// and then held fixed.  The Jacobian is that of the discrete map (the tangent of every RK4 stage, not the variational ODE
// integrated separately), linearised about the states f_fly itself wrote into the workspace trajectory.
//
// j_jac    one workgroup of JB = 256 threads per NLP; the grid is worked through in chunks of CH = 16 steps, last chunk first.
//   evaluation  group g (16 lanes) takes step g of the chunk: every lane carries the 7-state through the step's m substeps
//          (redundant across the group, uniform inside it) and one tangent column of the step map z_k = S(z_{k-1}, u_k, dt; Der):
//          columns 0..6 Phi_k = dz_k/dz_{k-1}, 7 the control, 8 dt, 9..15 the Der constants the right-hand side reads (rho0, gam,
//          thr, M0, ms, alpha, mrate; formulation 1 does not read alpha and takes angle_ub, which enters through the reset of
//          the angle, in its place).  d f/d z from accel<1>, d f/d Der from accel_dder.
//   staging     the 16 step records of a chunk (7 x 16 doubles each, 14 KB) go to LDS as rec[step][state][column] and never to
//          HBM.  A wave stores 4 steps x 16 columns of one state row at a time: doubles 112 g + 16 i + col; 112 = 16 mod 32,
//          so the two steps of each half wave fill 32 different 8-byte slots -- no bank conflict.  The sweep reads one address
//          per instruction for the whole wave (a broadcast).
//   sweep       wave 0, lane q = row q of Lambda (9 rows: the 7 flown states, periapsis, apoapsis): Lambda_K = I / grad apsides,
//          Lambda_{k-1} = Lambda_k Phi_k; Lambda_k g_k goes to jac_u, Lambda_k Gamma_k is summed into 8 accumulators, steps in
//          descending order -- a fixed order, so a problem gives the same bits alone as inside any batch.
//   epilogue    chain rule d(dt, Der)/d(params, t_f) (derive of ascent_device.hpp) plus the direct dependence of the apsis rows
//          on G, M, R0, r_peri; Lambda_0 gives the z_0 columns.  Lambda_K's apsis rows and the epilogue are lambda_apsis_rows and
//          jac_columns of ascent_tangent_dev.hpp, shared with g_gains.
// t_update one wavefront per NLP, lanes over the steps: the conditions c = (e3, g1, g2) of terminal_eval at the flown last
//          node, A = grad c [J_tf | J_u], the 3 x 3 normal matrix A W A' (per-lane partial sums over k = lane, lane + 64, ..,
//          then a butterfly of cross-lane shuffles: a fixed order), delta = -W A' (A W A')^-1 c, the update in place.
// t_final  the state rows of the trimmed blob from the last fly-out, and the summary.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>

#include "ascent.h"
#include "ascent_device.hpp"
#include "ascent_flight.hpp"
#include "ascent_flight_dev.hpp"
#include "ascent_tangent_dev.hpp"
#include "ascent_trim.hpp"

namespace ascent {
namespace {

constexpr int TW = 64;                     // t_update / t_final: one wavefront per NLP
// per-problem state of the trim between its kernels, rows of [ST_ROWS][batch]
constexpr int ST_FLAG = 0 /* 0 active, 1 converged, 2 non-finite or singular */, ST_ROUNDS = 1, ST_C0 = 2, ST_NFREE = 3, ST_ROWS = 4;

template <int FORM>
__global__ __launch_bounds__(JB) void j_jac(const ascent_params *__restrict__ P, long batch, int K, int substeps,
                                            const double *__restrict__ blob, const double *__restrict__ traj,
                                            const double *__restrict__ skip, double *__restrict__ jac, double *__restrict__ jac_u) {
  __shared__ double rec[CH * REC];
  const long p = blockIdx.x;
  const size_t B = (size_t)batch;
  if (skip && skip[p] != 0.0) return;         // a frozen problem of the trim (uniform over the workgroup)
  const int t = threadIdx.x, g = t >> 4, col = t & (NCOL - 1);
  const int nt = K + 1;
  const double *b = blob + p, *tr = traj + p;
  const ascent_params prm = P[p];
  const Der d = derive(prm);
  const double tf = b[(size_t)(21 * K + S_TH) * B];
  const double dt = (tf * d.T) / K;
  const int m = flight_substeps(dt, substeps);
  const double hs = dt / m;

  // the sweep's state, wave 0: lane q holds row q of Lambda, its accumulators and (rows 7, 8) the direct parameter terms
  double L[7], A[NACC];
  ApsisDirect dir = {0.0, 0.0, 0.0, 0.0};
  ASC_UNROLL
  for (int i = 0; i < 7; i++) L[i] = t == i ? 1.0 : 0.0;
  ASC_UNROLL
  for (int a = 0; a < NACC; a++) A[a] = 0.0;
  if (t < TW) {
    double zK[7];
    load_node(tr, B, nt, K, zK);
    lambda_apsis_rows(prm, zK, t, L, dir);
  }

  const int nch = (K + CH - 1) / CH;
  for (int c = nch - 1; c >= 0; c--) {
    const int k = c * CH + g + 1;             // this group's step: node k-1 -> k
    if (k <= K) {
      double z[7], dz[7];
      load_node(tr, B, nt, k - 1, z);
      const double u = b[(size_t)(7 * K + k - 1) * B];
      ASC_UNROLL
      for (int i = 0; i < 7; i++) dz[i] = col == i ? 1.0 : 0.0;
      fly_step_tangent<FORM>(d, z, dz, u, hs, m, col);
      ASC_UNROLL
      for (int i = 0; i < 7; i++) rec[g * REC + i * NCOL + col] = dz[i];
    }
    __syncthreads();
    if (t < TW) {
      const int top = K - c * CH < CH ? K - c * CH : CH;
      for (int s = top - 1; s >= 0; s--) {
        const double *R = rec + s * REC;
        double o[NCOL];
        ASC_UNROLL
        for (int cc = 0; cc < NCOL; cc++) {
          double a = 0.0;
          ASC_UNROLL
          for (int i = 0; i < 7; i++) a += L[i] * R[i * NCOL + cc];
          o[cc] = a;
        }
        if (jac_u && t < JROWS) jac_u[((size_t)t * K + (c * CH + s)) * B + p] = o[C_U];
        ASC_UNROLL
        for (int a = 0; a < NACC; a++) A[a] += o[C_DT + a];
        ASC_UNROLL
        for (int i = 0; i < 7; i++) L[i] = o[i];
      }
    }
    __syncthreads();
  }

  if (t < JROWS) {
    double o[JCOLS];
    jac_columns<FORM>(prm, d, tf, K, L, A, dir, o);
    ASC_UNROLL
    for (int cc = 0; cc < JCOLS; cc++) jac[((size_t)t * JCOLS + cc) * B + p] = o[cc];
  }
}

ASC_DEV double wave_max_nan(double v) {
  ASC_UNROLL
  for (int off = 32; off >= 1; off >>= 1) v = max_nan(v, __shfl_xor(v, off));
  return v;
}
ASC_DEV bool finite3(double a, double b, double c) {
  const double big = 1.79769313486231570815e308;
  return fabs(a) <= big && fabs(b) <= big && fabs(c) <= big;
}

// one round of the trim: after f_fly and j_jac of the current control
__global__ __launch_bounds__(TW) void t_update(const ascent_params *__restrict__ P, long batch, int K, int terminal, double tol,
                                               int first, double *__restrict__ blob, const double *__restrict__ traj,
                                               const double *__restrict__ jac, const double *__restrict__ jac_u,
                                               double *__restrict__ st) {
  const long p = blockIdx.x;
  const size_t B = (size_t)batch;
  const int lane = threadIdx.x, nt = K + 1;
  if (st[(size_t)ST_FLAG * B + p] != 0.0) return;
  double *b = blob + p;
  const Der d = derive_t(P[p], terminal);
  double zK[7];
  load_node(traj + p, B, nt, K, zK);
  const Terminal tm = terminal_eval(d, zK);
  const double c[3] = {tm.e3, tm.g1, tm.g2};
  const bool fin = finite3(c[0], c[1], c[2]);
  const double cn = fin ? fmax(fabs(c[0]), fmax(fabs(c[1]), fabs(c[2]))) : NAN;
  double nf = 0.0;
  for (int k = lane; k < K; k += TW) nf += fabs(b[(size_t)(7 * K + k) * B]) < 0.999 ? 1.0 : 0.0;
  nf = wave_sum(nf);
  if (lane == 0) {
    if (first) st[(size_t)ST_C0 * B + p] = cn;
    st[(size_t)ST_NFREE * B + p] = nf;
  }
  if (!fin) { if (lane == 0) st[(size_t)ST_FLAG * B + p] = 2.0; return; }
  if (cn <= tol) { if (lane == 0) st[(size_t)ST_FLAG * B + p] = 1.0; return; }
  // grad c (3 x 4 on x, y, xdot, ydot)
  const double gc[3][4] = {{tm.e3g[0], tm.e3g[1], tm.e3g[2], tm.e3g[3]}, {tm.g1g[0], tm.g1g[1], 0.0, 0.0}, {0.0, 0.0, tm.g2g[0], tm.g2g[1]}};
  double at[3];
  {
    double j[4];
    ASC_UNROLL
    for (int q = 0; q < 4; q++) j[q] = jac[((size_t)q * JCOLS + 23) * B + p];
    ASC_UNROLL
    for (int r = 0; r < 3; r++) at[r] = gc[r][0] * j[0] + gc[r][1] * j[1] + gc[r][2] * j[2] + gc[r][3] * j[3];
  }
  double n[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};       // 11 12 13 22 23 33
  for (int k = lane; k < K; k += TW) {
    if (!(fabs(b[(size_t)(7 * K + k) * B]) < 0.999)) continue;
    double j[4], a[3];
    ASC_UNROLL
    for (int q = 0; q < 4; q++) j[q] = jac_u[((size_t)q * K + k) * B + p];
    ASC_UNROLL
    for (int r = 0; r < 3; r++) a[r] = gc[r][0] * j[0] + gc[r][1] * j[1] + gc[r][2] * j[2] + gc[r][3] * j[3];
    n[0] += a[0] * a[0]; n[1] += a[0] * a[1]; n[2] += a[0] * a[2];
    n[3] += a[1] * a[1]; n[4] += a[1] * a[2]; n[5] += a[2] * a[2];
  }
  ASC_UNROLL
  for (int i = 0; i < 6; i++) n[i] = wave_sum(n[i]);
  n[0] += at[0] * at[0]; n[1] += at[0] * at[1]; n[2] += at[0] * at[2];
  n[3] += at[1] * at[1]; n[4] += at[1] * at[2]; n[5] += at[2] * at[2];
  // (A W A') y = c by L D L' without pivoting (the matrix is symmetric positive definite or the problem is frozen)
  const double d1 = n[0];
  bool ok = d1 > 1e-300;
  const double l21 = n[1] / d1, l31 = n[2] / d1;
  const double d2 = n[3] - l21 * n[1];
  ok = ok && d2 > 1e-300;
  const double s32 = n[4] - l21 * n[2], l32 = s32 / d2;
  const double d3 = n[5] - l31 * n[2] - l32 * s32;
  ok = ok && d3 > 1e-300;
  const double w1 = c[0], w2 = c[1] - l21 * w1, w3 = c[2] - l31 * w1 - l32 * w2;
  const double y3 = w3 / d3, y2 = w2 / d2 - l32 * y3, y1 = w1 / d1 - l21 * y2 - l31 * y3;
  if (!ok || !finite3(y1, y2, y3)) { if (lane == 0) st[(size_t)ST_FLAG * B + p] = 2.0; return; }
  for (int k = lane; k < K; k += TW) {
    const double u = b[(size_t)(7 * K + k) * B];
    if (!(fabs(u) < 0.999)) continue;
    double j[4], a[3];
    ASC_UNROLL
    for (int q = 0; q < 4; q++) j[q] = jac_u[((size_t)q * K + k) * B + p];
    ASC_UNROLL
    for (int r = 0; r < 3; r++) a[r] = gc[r][0] * j[0] + gc[r][1] * j[1] + gc[r][2] * j[2] + gc[r][3] * j[3];
    const double un = u - (a[0] * y1 + a[1] * y2 + a[2] * y3);
    b[(size_t)(7 * K + k) * B] = fmin(1.0, fmax(-1.0, un));
  }
  if (lane == 0) {
    b[(size_t)(21 * K + S_TH) * B] -= at[0] * y1 + at[1] * y2 + at[2] * y3;
    st[(size_t)ST_ROUNDS * B + p] += 1.0;
  }
}

// after the last fly-out: the flown states into the trimmed blob, and the summary rows
__global__ __launch_bounds__(TW) void t_final(const ascent_params *__restrict__ P, long batch, int K, int terminal, double tol,
                                              const double *__restrict__ blob_in, double *__restrict__ blob,
                                              const double *__restrict__ traj, const double *__restrict__ st,
                                              double *__restrict__ summary) {
  const long p = blockIdx.x;
  const size_t B = (size_t)batch;
  const int lane = threadIdx.x, nt = K + 1;
  double *b = blob + p;
  const double *bi = blob_in + p, *tr = traj + p;
  const ascent_params prm = P[p];
  const Der d = derive_t(prm, terminal);
  double du = 0.0, viol = 0.0;
  for (int k = lane; k < K; k += TW) {
    double z[7];
    load_node(tr, B, nt, k + 1, z);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) b[(size_t)(7 * k + i) * B] = z[i];
    du = fmax(du, fabs(b[(size_t)(7 * K + k) * B] - bi[(size_t)(7 * K + k) * B]));
    viol = max_nan(viol, fmax(-z[IA], z[IA] - d.aub));
  }
  du = wave_max_nan(du);
  viol = wave_max_nan(viol);
  if (lane != 0) return;
  double zK[7];
  load_node(tr, B, nt, K, zK);
  const Terminal tm = terminal_eval(d, zK);
  const bool fin = finite3(tm.e3, tm.g1, tm.g2);
  const double cn = fin ? fmax(fabs(tm.e3), fmax(fabs(tm.g1), fabs(tm.g2))) : NAN;
  const double flag = st[(size_t)ST_FLAG * B + p];
  double peri, apo;
  apsides_of(prm, zK[IX], zK[IY], zK[IVX], zK[IVY], peri, apo);
  summary[(size_t)0 * B + p] = (flag == 2.0 || !fin) ? 2.0 : cn <= tol ? 0.0 : 1.0;
  summary[(size_t)1 * B + p] = st[(size_t)ST_ROUNDS * B + p];
  summary[(size_t)2 * B + p] = cn;
  summary[(size_t)3 * B + p] = st[(size_t)ST_C0 * B + p];
  summary[(size_t)4 * B + p] = (b[(size_t)(21 * K + S_TH) * B] - bi[(size_t)(21 * K + S_TH) * B]) * d.T;
  summary[(size_t)5 * B + p] = du;
  summary[(size_t)6 * B + p] = st[(size_t)ST_NFREE * B + p];
  summary[(size_t)7 * B + p] = peri;
  summary[(size_t)8 * B + p] = apo;
  summary[(size_t)9 * B + p] = viol;
}

struct TrimWs { double *traj, *fsum, *jac, *jac_u, *st; };
TrimWs carve(double *ws, int K, long batch) {
  const FlightWs f = flight_ws(ws, K, batch);
  double *jac_u = f.rest + (size_t)JROWS * JCOLS * (size_t)batch;
  return TrimWs{f.traj, f.fsum, f.rest, jac_u, jac_u + (size_t)JROWS * K * (size_t)batch};
}

}  // namespace

size_t jac_ws_bytes(int K, long batch) { return flight_ws_bytes(K, batch); }
size_t trim_ws_bytes(int K, long batch) {
  return jac_ws_bytes(K, batch) + ((size_t)JROWS * JCOLS + (size_t)JROWS * K + ST_ROWS) * (size_t)batch * sizeof(double);
}

static int jac_launch(const Call &c, int substeps, const double *dblob, const double *dtraj, const double *dskip, double *djac,
                      double *djac_u) {
  const dim3 grid((unsigned)c.batch), block(JB);
  if (c.form == 1)
    hipLaunchKernelGGL((j_jac<1>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, dblob, dtraj, dskip, djac, djac_u);
  else
    hipLaunchKernelGGL((j_jac<0>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, dblob, dtraj, dskip, djac, djac_u);
  ASC_CHK(c.err, c.errlen, hipGetLastError());
  return ASCENT_OK;
}

int jac_run(const Call &c, int substeps, const double *dblob, double *djac, double *djac_u, double *ws) {
  const FlightWs w = flight_ws(ws, c.K, c.batch);
  if (const int rc = flight_fly_only(c, substeps, dblob, w.traj, w.fsum)) return rc;
  return jac_launch(c, substeps, dblob, w.traj, nullptr, djac, djac_u);
}

int trim_run(const Call &c, int terminal, int substeps, int rounds, double tol, const double *dblob, double *dblob_out,
             double *dsummary, double *ws) {
  const ascent_params *dp = c.dp;
  const long batch = c.batch;
  const int K = c.K;
  hipStream_t stream = c.stream;
  const TrimWs w = carve(ws, K, batch);
  const size_t B = (size_t)batch;
  ASC_CHK(c.err, c.errlen, hipMemcpyAsync(dblob_out, dblob, (21 * (size_t)K + NSC) * B * sizeof(double), hipMemcpyDeviceToDevice, stream));
  ASC_CHK(c.err, c.errlen, hipMemsetAsync(w.st, 0, (size_t)ST_ROWS * B * sizeof(double), stream));
  const dim3 grid((unsigned)batch), block(TW);
  for (int r = 0; r < rounds; r++) {
    if (const int rc = flight_fly_only(c, substeps, dblob_out, w.traj, w.fsum)) return rc;
    if (const int rc = jac_launch(c, substeps, dblob_out, w.traj, w.st, w.jac, w.jac_u)) return rc;
    hipLaunchKernelGGL(t_update, grid, block, 0, stream, dp, batch, K, terminal, tol, r == 0 ? 1 : 0, dblob_out, w.traj, w.jac, w.jac_u, w.st);
    ASC_CHK(c.err, c.errlen, hipGetLastError());
  }
  if (const int rc = flight_fly_only(c, substeps, dblob_out, w.traj, w.fsum)) return rc;
  hipLaunchKernelGGL(t_final, grid, block, 0, stream, dp, batch, K, terminal, tol, dblob, dblob_out, w.traj, w.st, dsummary);
  ASC_CHK(c.err, c.errlen, hipGetLastError());
  return ASCENT_OK;
}

}  // namespace ascent
