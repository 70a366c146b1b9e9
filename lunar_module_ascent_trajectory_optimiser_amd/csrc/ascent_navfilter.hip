// Navigation filter (include/ascent.h: ascent_navigation_filter, ascent_covariance_filtered_batch): the design of a linear Kalman
// filter along a flown solution, and the true covariance of the guided flight whose knowledge error is that filter's estimation
// error -- the linear covariance corridor (ascent_lincov.hip) with the error e = z-hat - z estimated instead of driven.
//
// The model is ascent_lincov.hip's: the derivative of the flight about the nominal flight f_fly writes, the records
// [Phi_k | g_k | Gamma_k] of fly_step_tangent.  M scalar measurements h_i . z + sigma_i v, constant along the flight, are taken at
// the nodes j with j % meas_stride == 0 and processed one after the other; nothing is inverted.
//   n_filter            P-hat_0 = diag(sigma_nav^2), P-hat_k^- = Phi_k P-hat_{k-1} Phi_k' + sigma_u,k^2 g_k g_k' + diag(filter_q^2), and per
//                       measurement s = h' P h + sigma^2, l = P h / s, P <- (I - l h') P (I - l h')' + sigma^2 l l'
//   l_lincov_filtered   the gains l_{k,i} are given.  w = [dz; e] (14):
//                         corr_k = K_k . (dz_{k-1} + e_{k-1}), du_k = -corr_k + eps_k
//                         dz_k   = Phi_k dz_{k-1} + g_k du_k + Gamma_k dp + (dz_k/dt_f) dt_f  [+ gamma_K tau, tau = -k_t . (dz_{K-1} + e_{K-1})]
//                         e_k^-  = Phi_k e_{k-1} - g_k eps_k - Gamma_k dp - (dz_k/dt_f) dt_f
//                         e     <- e + l_{k,i} (-h_i . e + sigma_i v_{k,i})
//                       carried as X (14 x 22: the columns z_0 (7) | the 8 tangent coefficients | e_0 (7), expanded to the 32 columns
//                       at a history node as l_lincov does) and Q (14 x 14, the covariance of w under eps and v).
//
// Both kernels: one workgroup of JB = 256 threads per problem, chunks of CH = 16 steps in ascending order, evaluation and LDS
// staging of the step records as l_lincov / j_jac; beside its record a group stages K_k, sigma_u,k^2, u_k, the nominal node and,
// at a measurement node, the gains l_{k,.}.  The state of a sweep lives in LDS in two copies; every phase -- a step, or the update
// by one measurement -- reads one copy, writes the other and ends in a barrier.
//   n_filter
//     lanes 0..48     entry (i, j) of P-hat: both halves formed by the lane itself and averaged, as g_gains keeps its P; in an update
//                     phase every lane forms s for itself (the same operations in the same order: the same bits), the lanes of
//                     column 0 store the gain
//   l_lincov_filtered   (256 threads: the kernel holds 312 / 316 registers, and a fifth wavefront would halve the budget; ascent_lincov.hip)
//     lanes 0..104    entry (a, b), a <= b, of Q, stored to (a, b) and (b, a): F Q F' + sigma_u^2 [g; -g][g; -g]' with
//                     F = [A_k, -g_k K_k'; 0, Phi_k] (the stretch of the last step on both upper blocks); in an update phase
//                     U Q U' + sigma^2 [0; l][0; l]' with U = diag(I, I - l h'), written out in the rows h' Q of the block of e (exact for
//                     any l, not only the design's); a row of Q at a time -- unrolled, the 196 loads were hoisted and the kernel spilled
//     lanes 128..204  rows i and 7 + i of the columns c and c + 11 of X (they share corr_c)
//     lanes 224..231  the noise helpers Cov(dz_k, corr_k) (7) and Var(corr_k), from Q_{k-1}; in an update phase they look at the gains
//   A history node adds two phases (l_lincov's node_phase): lanes 0..9 expand their row of y_j and lanes 64..70 their row of e_j to
//   the 32 columns; then lanes 0..54 sum their entry of cov_j and lanes 64..91 their entry of the covariance of e_j over the
//   columns in ascending order and add the noise part last.
// A gain K_k or l_{k,i} that is not finite, a measurement row or sigma_nav that is not finite, or a sigma_i that is not > 0 raises
// a flag of the workgroup: NaN rows from that node on (from the first node for the constant arrays).
// The order of every addition is fixed: a problem gives the same bits alone as inside any batch, and a node's rows do not depend
// on the node stride or on which optional outputs were asked for.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>

#include "ascent.h"
#include "ascent_device.hpp"
#include "ascent_disperse.hpp"
#include "ascent_flight.hpp"
#include "ascent_flight_dev.hpp"
#include "ascent_lincov_dev.hpp"
#include "ascent_navfilter.hpp"
#include "ascent_tangent_dev.hpp"

namespace ascent {
namespace {

constexpr int MM = ASCENT_NAVFILTER_MAX_MEAS;
constexpr int NW = 14;                                     // w = [dz; e]
constexpr int XF = 22, X_COEF = 7, X_E0 = X_COEF + NACC;   // columns of X
static_assert(X_E0 + 7 == XF, "compressed columns");
constexpr int LC = ASCENT_LINCOV_COLS, HQ = ASCENT_HISTORY_QUANTITIES, NCOV = ASCENT_LINCOV_COV_ROWS, NNAV = ASCENT_NAV_COV_ROWS;
constexpr int C_E0 = ASCENT_DISPERSE_COLS;                 // the columns of e_0 among the 32
static_assert(C_E0 + 8 == LC && NNAV == 28, "layout");
constexpr int NQL = NW * (NW + 1) / 2;                     // lanes of Q
constexpr int T_X = 128, NXL = 7 * (XF / 2), T_H = 224, T_E = 64;
static_assert(NQL <= T_X && T_X + NXL <= T_H && T_H + 8 <= JB && T_E + NNAV <= T_X, "lane map");
constexpr int ST_SU2 = 7, ST_U = 8, ST = 9;                // staged per step: K_k (7), sigma_u,k^2, u_k

// what a workgroup holds of its problem's nominal flight
struct Flight {
  ascent_params prm;
  Der d;
  double tf, dt, hs;
  int m;
};

ASC_DEV Flight flight_of(const ascent_params *__restrict__ P, long p, size_t B, int K, int substeps, const double *__restrict__ b) {
  Flight F;
  F.prm = P[p];
  F.d = derive(F.prm);
  F.tf = b[(size_t)(21 * K + S_TH) * B];
  F.dt = (F.tf * F.d.T) / K;
  F.m = flight_substeps(F.dt, substeps);
  F.hs = F.dt / F.m;
  return F;
}

// the staged arrays of a chunk
struct Staged {
  double *rec, (*stp)[ST], (*stl)[7 * MM], (*nod)[7];      // stl, nod: null in n_filter
};

// group g evaluates step k (node k-1 -> k) and stages its record and what the sweep reads of it (l_lincov's stage_step)
template <int FORM>
ASC_DEV void stage_step(const Staged &L, const Flight &F, const double *__restrict__ b, const double *__restrict__ tr, const double *gain_u,
                        const double *sigma_u, const double *gain_l, int n_meas, int meas_stride, size_t B, long p, int K, int k, int g,
                        int col) {
  if (k > K) return;
  const int nt = K + 1;
  double z[7], dz[7];
  load_node(tr, B, nt, k - 1, z);
  const double u = b[(size_t)(7 * K + k - 1) * B];
  if (col < 7) {
    L.stp[g][col] = gain_u ? gain_u[((size_t)col * K + k - 1) * B + p] : 0.0;
  } else if (col == ST_SU2) {
    const double su = sigma_u ? sigma_u[(size_t)(k - 1) * B + p] : 0.0;
    L.stp[g][ST_SU2] = su * su;
  } else if (col == ST_U) {
    L.stp[g][ST_U] = u;
  } else if (col == NCOL - 1 && L.nod) {      // the nominal node the step ends at, f_fly's
    double zk[7];
    load_node(tr, B, nt, k, zk);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) L.nod[g][i] = zk[i];
  }
  if (gain_l && k % meas_stride == 0)         // the gains of a measurement node; elsewhere they are never read
    for (int e = col; e < 7 * n_meas; e += NCOL) L.stl[g][e] = gain_l[((size_t)e * K + k - 1) * B + p];
  ASC_UNROLL
  for (int i = 0; i < 7; i++) dz[i] = col == i ? 1.0 : 0.0;
  fly_step_tangent<FORM>(F.d, z, dz, u, F.hs, F.m, col);
  ASC_UNROLL
  for (int i = 0; i < 7; i++) L.rec[g * REC + i * NCOL + col] = dz[i];
}

// entry t of a packed upper triangle of order n, row by row: (a, b), a <= b
ASC_DEV void upper_entry(int t, int n, int &a, int &b) {
  a = 0;
  while (t >= n - a) { t -= n - a; a++; }
  b = a + t;
}

struct FilterArgs {
  const double *sigma_nav, *sigma_u, *filter_q, *meas_h, *meas_sigma;
  int n_meas, meas_stride;
  double *gain_l, *pfilt, *summary;
};

template <int FORM>
__global__ __launch_bounds__(JB) void n_filter(const ascent_params *__restrict__ P, long batch, int K, int substeps,
                                               const double *__restrict__ blob, const double *__restrict__ traj, FilterArgs A) {
  __shared__ double rec[CH * REC];
  __shared__ double Ps[2][49], stp[CH][ST], hms[MM][7], sgm[MM], q2s[7];
  const Staged L{rec, stp, nullptr, nullptr};
  const long p = blockIdx.x;
  const size_t B = (size_t)batch;
  const int t = threadIdx.x, g = t >> 4, col = t & (NCOL - 1);
  const double *b = blob + p, *tr = traj + p;
  const Flight F = flight_of(P, p, B, K, substeps, b);
  if (t < 49) {
    const double sn = A.sigma_nav[(size_t)(t / 7) * B + p];
    Ps[0][t] = t / 7 == t % 7 ? sn * sn : 0.0;
  }
  if (t >= 64 && t < 64 + 7 * A.n_meas) hms[0][t - 64] = A.meas_h[(size_t)(t - 64) * B + p];
  if (t >= 128 && t < 128 + A.n_meas) sgm[t - 128] = A.meas_sigma[(size_t)(t - 128) * B + p];
  if (t >= 192 && t < 192 + 7) {
    const double q = A.filter_q ? A.filter_q[(size_t)(t - 192) * B + p] : 0.0;
    q2s[t - 192] = q * q;
  }
  int cp = 0, bad = finite1(F.tf) ? 0 : 1;    // the first node from which the rows are NaN (0: none); the same in every lane
  for (int e = 0; e < 7; e++)                 // sigma_nav and filter_q enter P-hat before the first node; h and sigma_i at a measurement
    if (!finite1(A.sigma_nav[(size_t)e * B + p]) || (A.filter_q && !finite1(A.filter_q[(size_t)e * B + p]))) bad = 1;
  int qi = 0, qj = 0;
  if (t < 28) upper_entry(t, 7, qi, qj);

  const int nch = (K + CH - 1) / CH;
  for (int c = 0; c < nch; c++) {
    stage_step<FORM>(L, F, b, tr, nullptr, A.sigma_u, nullptr, 0, 1, B, p, K, c * CH + g + 1, g, col);
    __syncthreads();
    const int top = K - c * CH < CH ? K - c * CH : CH;
    for (int s = 0; s < top; s++) {
      const int j = c * CH + s + 1;
      const double *R = rec + s * REC;
      if (t < 49) {                           // the propagation: both halves of entry (i, jj)
        const int i = t / 7, jj = t - i * 7;
        const double *Po = Ps[cp];
        double nij = 0.0, nji = 0.0;
        ASC_UNROLL
        for (int l = 0; l < 7; l++) {
          double wi = 0.0, wj = 0.0;
          ASC_UNROLL
          for (int mm = 0; mm < 7; mm++) {
            const double pl = Po[l * 7 + mm];
            wj += pl * R[jj * NCOL + mm];
            wi += pl * R[i * NCOL + mm];
          }
          nij += R[i * NCOL + l] * wj;
          nji += R[jj * NCOL + l] * wi;
        }
        const double su2 = stp[s][ST_SU2];
        const double gg = su2 != 0.0 ? su2 * (R[i * NCOL + C_U] * R[jj * NCOL + C_U]) : 0.0;
        const double qq = i == jj ? q2s[i] : 0.0;
        Ps[cp ^ 1][t] = 0.5 * (((nij + gg) + qq) + ((nji + gg) + qq));
      }
      __syncthreads();
      cp ^= 1;
      if (j % A.meas_stride == 0) {
        for (int i = 0; i < A.n_meas; i++) {
          const double *Pc = Ps[cp], *h = hms[i];
          const double sg = sgm[i];
          double sv = 0.0;                    // s = h' P h + sigma^2, by every lane
          ASC_UNROLL
          for (int a = 0; a < 7; a++) {
            double w = 0.0;
            ASC_UNROLL
            for (int bb = 0; bb < 7; bb++) w += Pc[a * 7 + bb] * h[bb];
            sv += h[a] * w;
          }
          sv += sg * sg;
          if (!bad && !(sg > 0.0 && sv > 0.0 && finite1(sv))) bad = j;
          if (t < 49) {
            const int a = t / 7, bb = t - a * 7;
            double pa = 0.0, pb = 0.0;
            ASC_UNROLL
            for (int l = 0; l < 7; l++) {
              pa += Pc[a * 7 + l] * h[l];
              pb += Pc[bb * 7 + l] * h[l];
            }
            const double la = pa / sv, lb = pb / sv;
            double ma[7], mb[7], h1 = 0.0, h2 = 0.0;
            ASC_UNROLL
            for (int l = 0; l < 7; l++) {
              ma[l] = (a == l ? 1.0 : 0.0) - la * h[l];
              mb[l] = (bb == l ? 1.0 : 0.0) - lb * h[l];
            }
            ASC_UNROLL
            for (int l = 0; l < 7; l++) {
              double wa = 0.0, wb = 0.0;
              ASC_UNROLL
              for (int mm = 0; mm < 7; mm++) {
                const double pl = Pc[l * 7 + mm];
                wb += pl * mb[mm];
                wa += pl * ma[mm];
              }
              h1 += ma[l] * wb;
              h2 += mb[l] * wa;
            }
            const double r = (sg * sg) * (la * lb);
            Ps[cp ^ 1][t] = bad ? NAN : 0.5 * ((h1 + r) + (h2 + r));
            if (bb == 0) A.gain_l[((size_t)(i * 7 + a) * K + j - 1) * B + p] = bad ? NAN : la;
          }
          __syncthreads();
          cp ^= 1;
        }
        if (bad == j && t < 7 * A.n_meas)     // the failing node: also the gains of the measurements before the failing one
          A.gain_l[((size_t)t * K + j - 1) * B + p] = NAN;
      } else if (t < 7 * A.n_meas) {
        A.gain_l[((size_t)t * K + j - 1) * B + p] = bad ? NAN : 0.0;
      }
      if (A.pfilt && t < 28) A.pfilt[((size_t)t * K + j - 1) * B + p] = bad ? NAN : Ps[cp][qi * 7 + qj];
    }
    __syncthreads();                          // the records and the staged steps are rewritten by the next chunk
  }
  if (t == 0) {
    A.summary[0 * B + p] = bad ? 2.0 : 0.0;
    A.summary[1 * B + p] = (double)bad;
    A.summary[2 * B + p] = (double)(K / A.meas_stride);
    A.summary[3 * B + p] = (double)F.m;
  }
}

struct FilteredArgs {
  const double *sigma, *sigma_u, *gain_u, *gain_t, *stretch_max, *sigma_nav, *gain_l, *meas_h, *meas_sigma;
  int n_meas, meas_stride, stride, nj;
  double *nominal, *cov, *nav_cov, *jac, *nav_jac;
};

// row a of F_k = [A_k, -g_k K_k'; 0, Phi_k], A_k = Phi_k - g_k K_k'; on a stretched last step - gamma_K k_t' on both upper blocks
ASC_DEV void f_row(const double *R, const double *kv, const double *kt, bool last, double dt, int a, double *f) {
  const bool up = a < 7;
  const int i = up ? a : a - 7;
  const double gi = R[i * NCOL + C_U], ti = dt * R[i * NCOL + C_DT];
  ASC_UNROLL
  for (int l = 0; l < 7; l++) {
    const double ph = R[i * NCOL + l];
    double v = -gi * kv[l];
    if (last) v -= ti * kt[l];
    f[l] = up ? ph + v : 0.0;
    f[7 + l] = up ? v : ph;
  }
}

// entry (a, l) of F_k, the operations of f_row
ASC_DEV double f_entry(const double *R, const double *kv, const double *kt, bool last, double dt, int a, int l) {
  const bool up = a < 7, left = l < 7;
  const int i = up ? a : a - 7, lc = left ? l : l - 7;
  const double ph = R[i * NCOL + lc];
  double v = -R[i * NCOL + C_U] * kv[lc];
  if (last) v -= (dt * R[i * NCOL + C_DT]) * kt[lc];
  return up ? (left ? ph + v : v) : (left ? 0.0 : ph);
}

template <int FORM>
__global__ __launch_bounds__(JB) void l_lincov_filtered(const ascent_params *__restrict__ P, long batch, int K, int substeps,
                                                        const double *__restrict__ blob, const double *__restrict__ traj, FilteredArgs A) {
  __shared__ double rec[CH * REC];
  __shared__ double Xs[2][NW * XF], Qs[2][NW * NW], stp[CH][ST], stl[CH][7 * MM], nod[CH][7], cors[XF], nks[8], Ss[(HQ + 7) * LC], sgs[LC],
      kts[7], hms[MM][7], sgm[MM];
  __shared__ int flag;                        // raised: NaN rows from this node on
  const Staged L{rec, stp, stl, nod};
  const long p = blockIdx.x;
  const size_t B = (size_t)batch;
  const int t = threadIdx.x, g = t >> 4, col = t & (NCOL - 1);
  const double *b = blob + p, *tr = traj + p;
  const Flight F = flight_of(P, p, B, K, substeps, b);
  const double smax = A.gain_t && A.stretch_max ? A.stretch_max[p] : 0.0;
  const bool stretch = smax > 0.0;
  // X_0 = [I, 0, 0; 0, 0, I], Q_0 = 0, and what every step shares; the barrier after the first evaluation publishes them
  for (int e = t; e < NW * XF; e += JB) {
    const int r = e / XF, cc = e - r * XF;
    Xs[0][e] = (r < 7 ? cc == r : cc == X_E0 + r - 7) ? 1.0 : 0.0;
  }
  if (t < NW * NW) Qs[0][t] = 0.0;
  if (t < LC) sgs[t] = t < C_E0 ? A.sigma[(size_t)t * B + p] : t < C_E0 + 7 ? A.sigma_nav[(size_t)(t - C_E0) * B + p] : 0.0;
  if (t < 7) kts[t] = stretch ? A.gain_t[(size_t)t * B + p] : 0.0;
  if (t >= 64 && t < 64 + 7 * A.n_meas) hms[0][t - 64] = A.meas_h[(size_t)(t - 64) * B + p];
  if (t >= 128 && t < 128 + A.n_meas) sgm[t - 128] = A.meas_sigma[(size_t)(t - 128) * B + p];
  if (t == JB - 1) {                          // the constant arrays, by one lane
    int bad = 0;
    for (int e = 0; e < 7 * A.n_meas; e++) bad |= !finite1(A.meas_h[(size_t)e * B + p]);
    for (int e = 0; e < A.n_meas; e++) {
      const double sg = A.meas_sigma[(size_t)e * B + p];
      bad |= !(sg > 0.0 && finite1(sg));
    }
    for (int e = 0; e < 7; e++) bad |= !finite1(A.sigma_nav[(size_t)e * B + p]);
    flag = bad;
  }
  int qa = 0, qb = 0;
  if (t < NQL) upper_entry(t, NW, qa, qb);
  const int xq = t - T_X, xi = xq / (XF / 2), xc0 = xq - xi * (XF / 2);      // the lanes of X

  int cp = 0;
  const int nch = (K + CH - 1) / CH;
  for (int c = 0; c < nch; c++) {
    stage_step<FORM>(L, F, b, tr, A.gain_u, A.sigma_u, A.gain_l, A.n_meas, A.meas_stride, B, p, K, c * CH + g + 1, g, col);
    __syncthreads();
    const int top = K - c * CH < CH ? K - c * CH : CH;
    for (int s = 0; s < top; s++) {
      const int j = c * CH + s + 1;
      const double *R = rec + s * REC, *kv = stp[s];
      const bool last = stretch && j == K;
      const double dt = F.dt;
      {
        const double *Xo = Xs[cp], *Qo = Qs[cp];
        double *Xn = Xs[cp ^ 1], *Qn = Qs[cp ^ 1];
        if (t < NQL) {
          double fb[NW], acc = 0.0;
          f_row(R, kv, kts, last, dt, qb, fb);
#pragma unroll 1
          for (int l = 0; l < NW; l++) {      // (a row of Q at a time: unrolled, the 196 loads are hoisted and the kernel spills)
            double w = 0.0;
            ASC_UNROLL
            for (int mm = 0; mm < NW; mm++) w += Qo[l * NW + mm] * fb[mm];
            acc += f_entry(R, kv, kts, last, dt, qa, l) * w;
          }
          const double su2 = kv[ST_SU2];
          const double ga = qa < 7 ? R[qa * NCOL + C_U] : -R[(qa - 7) * NCOL + C_U], gb = qb < 7 ? R[qb * NCOL + C_U] : -R[(qb - 7) * NCOL + C_U];
          const double v = acc + (su2 != 0.0 ? su2 * (ga * gb) : 0.0);
          Qn[qa * NW + qb] = v;
          Qn[qb * NW + qa] = v;
        } else if (t >= T_X && t < T_X + NXL) {
          ASC_UNROLL
          for (int hh = 0; hh < 2; hh++) {
            const int xc = xc0 + hh * (XF / 2);
            double xz[7], xe[7], corr = 0.0, az = 0.0, ae = 0.0;
            ASC_UNROLL
            for (int l = 0; l < 7; l++) { xz[l] = Xo[l * XF + xc]; xe[l] = Xo[(7 + l) * XF + xc]; }
            ASC_UNROLL
            for (int l = 0; l < 7; l++) corr += kv[l] * xz[l];
            ASC_UNROLL
            for (int l = 0; l < 7; l++) corr += kv[l] * xe[l];
            ASC_UNROLL
            for (int l = 0; l < 7; l++) { az += R[xi * NCOL + l] * xz[l]; ae += R[xi * NCOL + l] * xe[l]; }
            az -= R[xi * NCOL + C_U] * corr;
            if (xc >= X_COEF && xc < X_E0) {
              const double f = R[xi * NCOL + C_DT + (xc - X_COEF)];
              az += f;
              ae -= f;
            }
            if (last) {
              double tau = 0.0;
              ASC_UNROLL
              for (int l = 0; l < 7; l++) tau -= kts[l] * xz[l];
              ASC_UNROLL
              for (int l = 0; l < 7; l++) tau -= kts[l] * xe[l];
              az += (dt * R[xi * NCOL + C_DT]) * tau;
            }
            Xn[xi * XF + xc] = az;
            Xn[(7 + xi) * XF + xc] = ae;
            if (xi == 0) {
              cors[xc] = corr;
              if (!finite1(corr)) flag = 1;
            }
          }
        } else if (t >= T_H && t < T_H + 8) {
          const int q = t - T_H;
          double a = 0.0;
#pragma unroll 1
          for (int l = 0; l < NW; l++) {
            double w = 0.0;
            ASC_UNROLL
            for (int mm = 0; mm < NW; mm++) w += Qo[l * NW + mm] * kv[mm < 7 ? mm : mm - 7];
            a += (q < 7 ? f_entry(R, kv, kts, last, dt, q, l) : kv[l < 7 ? l : l - 7]) * w;
          }
          nks[q] = a;
        }
      }
      __syncthreads();
      cp ^= 1;
      if (j % A.meas_stride == 0) {
        for (int i = 0; i < A.n_meas; i++) {
          const double *Xo = Xs[cp], *Qo = Qs[cp], *h = hms[i], *lg = stl[s] + 7 * i;
          double *Xn = Xs[cp ^ 1], *Qn = Qs[cp ^ 1];
          if (t < NQL) {
            const double sg = sgm[i];
            double hqa = 0.0, hqb = 0.0, hqh = 0.0;
            ASC_UNROLL
            for (int l = 0; l < 7; l++) {
              double w = 0.0;
              ASC_UNROLL
              for (int mm = 0; mm < 7; mm++) w += Qo[(7 + l) * NW + 7 + mm] * h[mm];
              hqh += h[l] * w;
              hqa += h[l] * Qo[(7 + l) * NW + qa];
              hqb += h[l] * Qo[(7 + l) * NW + qb];
            }
            const double ua = qa < 7 ? 0.0 : lg[qa < 7 ? 0 : qa - 7], ub = qb < 7 ? 0.0 : lg[qb < 7 ? 0 : qb - 7];
            const double v = ((Qo[qa * NW + qb] - ua * hqb) - ub * hqa) + (ua * ub) * (hqh + sg * sg);
            Qn[qa * NW + qb] = v;
            Qn[qb * NW + qa] = v;
          } else if (t >= T_X && t < T_X + NXL) {
            ASC_UNROLL
            for (int hh = 0; hh < 2; hh++) {
              const int xc = xc0 + hh * (XF / 2);
              double hx = 0.0;
              ASC_UNROLL
              for (int l = 0; l < 7; l++) hx += h[l] * Xo[(7 + l) * XF + xc];
              Xn[xi * XF + xc] = Xo[xi * XF + xc];
              Xn[(7 + xi) * XF + xc] = Xo[(7 + xi) * XF + xc] - lg[xi] * hx;
            }
          } else if (t >= T_H && t < T_H + 7) {
            if (!finite1(lg[t - T_H])) flag = 1;
          }
          __syncthreads();
          cp ^= 1;
        }
      }
      if (j % A.stride == 0 || j == K) {      // a history node (uniform)
        const int ni = (j + A.stride - 1) / A.stride - 1;
        const bool ok = finite1(F.tf) && flag == 0;
        const double *Xn = Xs[cp], *Qn = Qs[cp], *zn = nod[s];
        // the altitude's gradient at the nominal node: (gax, gay) on (x, y), and the unit vector (ex, ey) of its direct terms
        const double S = F.prm.r_peri;
        const Radius rad = nominal_radius(zn[IX], zn[IY], S, F.prm.R0);
        const double ex = rad.X / rad.rr, ey = rad.Y / rad.rr, gax = S * ex, gay = S * ey;
        if (t < HQ || (t >= T_E && t < T_E + 7)) {
          const bool nav = t >= T_E;
          const int r = nav ? HQ + t - T_E : t;                  // the row of Ss
          double cx[XF], o[LC];
          ASC_UNROLL
          for (int cc = 0; cc < XF; cc++) {
            const double xr = Xn[(nav ? 7 + t - T_E : t < 7 ? t : 0) * XF + cc], al = gax * Xn[IX * XF + cc] + gay * Xn[IY * XF + cc], cr = cors[cc];
            cx[cc] = nav || t < 7 ? xr : t == 7 ? al : t == 8 ? -cr : cr;
          }
          const ApsisDirect dir = {0.0, 0.0, t == 7 ? ey - 1.0 : 0.0, t == 7 ? zn[IX] * ex + zn[IY] * ey : 0.0};
          jac_columns<FORM>(F.prm, F.d, F.tf, K, cx, cx + X_COEF, dir, o);
          ASC_UNROLL
          for (int a = 0; a < 7; a++) o[C_E0 + a] = cx[X_E0 + a];
          o[LC - 1] = 0.0;
          if (!ok) {
            ASC_UNROLL
            for (int cc = 0; cc < LC; cc++) o[cc] = NAN;
          }
          double *out = nav ? A.nav_jac : A.jac;
          const int orow = nav ? t - T_E : t;
          ASC_UNROLL
          for (int cc = 0; cc < LC; cc++) {
            Ss[r * LC + cc] = o[cc];
            if (out) out[(((size_t)orow * LC + cc) * A.nj + ni) * B + p] = o[cc];
          }
          if (!nav) {
            const double nom = t < 7 ? zn[t] : t == 7 ? rad.rr - F.prm.R0 : t == 8 ? kv[ST_U] : 0.0;
            A.nominal[((size_t)t * A.nj + ni) * B + p] = nom;
          }
        }
        __syncthreads();
        if (t < NCOV) {
          int a, bq;
          upper_entry(t, HQ, a, bq);
          double acc = 0.0;
          for (int cc = 0; cc < LC; cc++) {
            const double sg = sgs[cc];
            if (sg != 0.0) acc += (Ss[a * LC + cc] * Ss[bq * LC + cc]) * (sg * sg);
          }
          // the noise part, as l_lincov's: rows 0..6 Q_j's block of dz, 7 the altitude's gradient on it, 8 / 9 through the helpers
          const double su2 = kv[ST_SU2];
          const int ar = a < 7 ? a : 0;
          const double qal = gax * Qn[ar * NW + IX] + gay * Qn[ar * NW + IY];
          const double n8 = (su2 != 0.0 ? su2 * R[ar * NCOL + C_U] : 0.0) - nks[ar];
          const double n8x = (su2 != 0.0 ? su2 * R[IX * NCOL + C_U] : 0.0) - nks[IX], n8y = (su2 != 0.0 ? su2 * R[IY * NCOL + C_U] : 0.0) - nks[IY];
          double n;
          if (bq < 7) n = Qn[a * NW + bq];
          else if (a < 7) n = bq == 7 ? qal : bq == 8 ? n8 : nks[a];
          else if (a == 7)
            n = bq == 7 ? gax * (gax * Qn[IX * NW + IX] + gay * Qn[IX * NW + IY]) + gay * (gax * Qn[IY * NW + IX] + gay * Qn[IY * NW + IY])
                : bq == 8 ? gax * n8x + gay * n8y : gax * nks[IX] + gay * nks[IY];
          else if (a == 8) n = bq == 8 ? nks[7] + su2 : -nks[7];
          else n = nks[7];
          acc += n;
          A.cov[((size_t)t * A.nj + ni) * B + p] = ok ? acc : NAN;
        } else if (t >= T_E && t < T_E + NNAV) {
          int a, bq;
          upper_entry(t - T_E, 7, a, bq);
          double acc = 0.0;
          for (int cc = 0; cc < LC; cc++) {
            const double sg = sgs[cc];
            if (sg != 0.0) acc += (Ss[(HQ + a) * LC + cc] * Ss[(HQ + bq) * LC + cc]) * (sg * sg);
          }
          acc += Qn[(7 + a) * NW + 7 + bq];
          A.nav_cov[((size_t)(t - T_E) * A.nj + ni) * B + p] = ok ? acc : NAN;
        }
        __syncthreads();                      // cors, nks and Ss are rewritten by the next step
      }
    }
    __syncthreads();                          // the records and the staged steps are rewritten by the next chunk
  }
}

}  // namespace

int navfilter_run(const Call &c, int substeps, const NavFilterIO &io, double *ws) {
  const FlightWs w = flight_ws(ws, c.K, c.batch);
  if (const int rc = flight_fly_only(c, substeps, io.blob, w.traj, w.fsum)) return rc;
  const FilterArgs a{io.sigma_nav, io.sigma_u, io.filter_q, io.meas_h, io.meas_sigma, io.n_meas, io.meas_stride, io.gain_l, io.pfilt, io.summary};
  const dim3 grid((unsigned)c.batch), block(JB);
  if (c.form == 1) hipLaunchKernelGGL((n_filter<1>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, io.blob, w.traj, a);
  else hipLaunchKernelGGL((n_filter<0>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, io.blob, w.traj, a);
  ASC_CHK(c.err, c.errlen, hipGetLastError());
  return ASCENT_OK;
}

int lincov_filtered_run(const Call &c, int substeps, const FilteredIO &io, double *ws) {
  const FlightWs w = flight_ws(ws, c.K, c.batch);
  if (const int rc = flight_fly_only(c, substeps, io.blob, w.traj, w.fsum)) return rc;
  const FilteredArgs a{io.sigma, io.sigma_u, io.gain_u, io.gain_t, io.stretch_max, io.sigma_nav, io.gain_l, io.meas_h, io.meas_sigma,
                       io.n_meas, io.meas_stride, io.node_stride, history_nodes(c.K, io.node_stride), io.nominal, io.cov, io.nav_cov, io.jac,
                       io.nav_jac};
  const dim3 grid((unsigned)c.batch), block(JB);
  if (c.form == 1) hipLaunchKernelGGL((l_lincov_filtered<1>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, io.blob, w.traj, a);
  else hipLaunchKernelGGL((l_lincov_filtered<0>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, io.blob, w.traj, a);
  ASC_CHK(c.err, c.errlen, hipGetLastError());
  return ASCENT_OK;
}

}  // namespace ascent
