// Linear covariance corridor (include/ascent.h: ascent_covariance_history_batch, ascent_covariance_drifting_batch): the first-order
// dispersion of a flown solution at every history node, in one deterministic forward sweep per problem -- what
// ascent_disperse_history_batch and ascent_disperse_drifting_batch sample.
//
// The model is the derivative of that call's flight about the nominal flight f_fly writes (clips ignored, substeps held, blob
// fixed in scaled units).  Constants c (32 columns): dz_0 (7) | the 16 fields | t_f | the knowledge bias nu (7) | the error e of
// theta-hat = w . dp + e.  Step k, from the records [Phi_k | g_k | Gamma_k] of fly_step_tangent:
//   corr_k = K_k . (dz_{k-1} + nu) + f_k theta-hat,   du_k = -corr_k + eps_k,   eps_k = sigma_u,k xi_k
//   dz_k = Phi_k dz_{k-1} + g_k du_k + Gamma_k dp + (dz_k/dt_f) dt_f  [+ gamma_K tau on step K, tau = -k_t . (dz_{K-1} + nu) - f_t theta-hat]
// The ten quantities y_j of a node are dz_j, the altitude (its gradient at the nominal node and its direct dependence on R0 and
// r_peri), du_j and corr_j.  Outputs per node: S_j = dy_j/dc (10 x 32) and cov_j = S_j diag(sigma^2) S_j' + N_j with the white
// noise N_j = Y_j Q_{j-1} Y_j' + sigma_u,j^2 y_j y_j', Q_k = A_k Q_{k-1} A_k' + sigma_u,k^2 g_k g_k', A_k = Phi_k - g_k K_k' (- gamma_K k_t').
// Drifting (ascent_covariance_drifting_batch): the eight knowledge errors are first-order Gauss-Markov sequences
// n_k = Phi_n n_{k-1} + q omega_{k-1}, Phi_n = diag(phi).  The columns nu and theta-hat stay the derivative with respect to n_0:
// their forcing at step k is scaled by the running product phi^k.  theta-hat = w . dp + n_7 then has two responses, so the sweep
// carries one more column: the response to the constant part w . dp, forced by f_k unscaled, which the parameter columns take
// their (theta-hat column) w_c from; with phi_7 = 1 it has the bits of the column theta-hat.  The driving noise enters the noise
// part beside Q: D_k = Phi_n D_{k-1} Phi_n + diag(q^2) (8, diagonal), C_k = A_k C_{k-1} Phi_n + B_k D_k (7 x 8, the covariance of
// dz_k and n_k), Q_k = A_k Q_{k-1} A_k' + M + M' + B_k D_k B_k' + sigma_u,k^2 g_k g_k', M = A_k C_{k-1} Phi_n B_k',
// B_k = -g_k kappa_k' (- gamma_K (k_t, f_t)' on a stretched last step), kappa_k = (K_k, f_k).
//
// Both kernels: one workgroup of JB = 256 threads per problem, chunks of CH = 16 steps in ascending order; evaluation and LDS
// staging of the step records exactly as j_jac (ascent_trim.hip).  Beside its record every group stages what the sweep reads of
// its step: K_k, f_k, sigma_u,k^2, u_k and the nominal node k -- no global load on the serial path.  The sensitivity is carried
// in the compressed column space X (7 x 23): z_0 (7) | the 8 tangent coefficients of tangent_coefficients / jac_columns | nu (7) |
// theta-hat, and Q (7 x 7); both stay in LDS across the chunks, each in two copies that alternate with the parity of the step, so
// a step is one phase and one barrier.  Without gain_u the same arithmetic runs on zero gains: all-zero gains give the bits of
// gain_u null.  Two more phases at a history node (node_phase): lanes 0..9 expand their row of y_j to the 32 columns --
// jac_columns for the fields and t_f, + (theta-hat column) w_c for a parameter column (the transpose of the E w_c rule of
// ascent_guidance_feedforward), the altitude's direct terms -- into LDS and jac_hist_out, and write the nominal row; then lanes
// 0..54 sum their covariance entry over the 32 columns in ascending order and add the noise part last.
// Every expression of the sweep but one is written once (stage_step, x_entry, closed_row, helper_entry, node_phase); a kernel is
// its lane map, its stores and, in the drifting one, the lanes of C, D and phi^k.  The one: the two halves of a Q entry stand in
// both kernels' Q lanes.  As one function called from both, l_lincov_drifting held 416 / 420 registers for 396 / 400 and its step
// 150 AGPR moves for 92, and its stride-10 calls were 1.7 to 3.5 % slower.
//   l_lincov
//     lanes 0..160    entry (i, c) of X: its own copy of corr_c, then row i of the step; lanes of row 0 store corr
//     lanes 161..168  the noise helpers A_k Q_{k-1} K_k (7) and K_k' Q_{k-1} K_k, two copies by parity as well
//     lanes 192..240  entry (i, j) of Q: both halves N_ij and N_ji computed by the lane itself and averaged, as g_gains keeps P,
//                     so Q stays exactly symmetric
//   l_lincov_drifting   (compiled with a fifth wavefront for C, 320 threads, the kernel was held to 256 registers and used 580
//                     bytes of scratch, so the workgroup stays 256 threads and Q is kept on the 28 entries of its upper triangle)
//     lanes 0..167    X (7 x 24) as l_lincov, the forcing of the columns nu and theta-hat times phi^k
//     lanes 168..223  entry (i, a) of C; the eight lanes of row 0 are the helpers as well, now the whole Cov(dz_k, corr_k) (7) and
//                     Var(corr_k): l_lincov's A Q K and K' Q K plus the terms through C_{k-1} Phi_n and D_k, and each carries
//                     phi^k and D_k of one channel
//     lanes 228..255  entry (i, j), i <= j, of Q: both halves as l_lincov forms them, the terms of C and D formed once and added
//                     to both, the average stored to (i, j) and (j, i), so Q stays exactly symmetric
//   C, D and phi^k are in LDS in two copies by the parity of the step, like X and Q; a lane that needs D_k forms it from D_{k-1}.
//   With every channel frozen (phi = 1, q = 0) the terms of C and D are not formed at all, and phi^k = 1 leaves every product
//   alone: the bits of l_lincov.  A phi outside [0, 1] or a q that is negative or not finite gives NaN rows at every node.
// The order of every addition is fixed: a problem gives the same bits alone as inside any batch, and a node's rows do not depend
// on the stride or on whether the Jacobian was asked for.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>

#include "ascent.h"
#include "ascent_device.hpp"
#include "ascent_disperse.hpp"
#include "ascent_flight.hpp"
#include "ascent_flight_dev.hpp"
#include "ascent_lincov.hpp"
#include "ascent_lincov_dev.hpp"
#include "ascent_tangent_dev.hpp"

namespace ascent {
namespace {

constexpr int XC = 23, XCD = XC + 1;                       // columns of X; with the column of theta-hat's constant part
constexpr int X_COEF = 7, X_NU = X_COEF + NACC, X_TH = X_NU + 7, X_TW = XC;
static_assert(X_TH + 1 == XC, "compressed columns");
constexpr int LC = ASCENT_LINCOV_COLS, HQ = ASCENT_HISTORY_QUANTITIES, NCOV = ASCENT_LINCOV_COV_ROWS;
static_assert(LC == ASCENT_DISPERSE_COLS + ASCENT_NAV_ROWS && NCOV == HQ * (HQ + 1) / 2, "lincov layout");
constexpr int T_NK = 7 * XC, T_Q = 192;                    // l_lincov: first lane of the noise helpers and of Q
static_assert(T_NK + 8 <= T_Q && T_Q + 49 <= JB, "lane map");
constexpr int T_C = 7 * XCD, T_QU = 228;                   // l_lincov_drifting: first lane of C and of the upper triangle of Q
static_assert(T_C + 56 <= T_QU && T_QU + 28 == JB, "lane map of the drifting sweep");
constexpr int ST_F = 7, ST_SU2 = 8, ST_U = 9, ST = 10;     // staged per step: K_k (7), f_k, sigma_u,k^2, u_k

struct LincovArgs {
  const double *sigma, *sigma_u, *gain_u, *gain_t, *stretch_max, *ff_u, *ff_t, *ff_know, *sigma_nav;
  int stride, nj;
  double *nominal, *cov, *jac;
};

struct DriftCov { const double *phi, *q; };

// the LDS arrays both sweeps keep, X with XCOLS columns.  Each is a __shared__ array of its kernel (ASC_SWEEP_LDS), not a member of
// one __shared__ struct: as members the compiler could not tell their stores and loads apart, and every covariance call was 1.4 to
// 8 % slower
template <int XCOLS>
struct Sweep {
  double *rec, (*Xs)[7 * XCOLS], (*Qs)[49], (*nks)[8], (*stp)[ST], (*nod)[7], *cors, *Ss, *sgs, *kts, *wks;
};
#define ASC_SWEEP_LDS(XCOLS, L)                                                                                               \
  __shared__ double rec[CH * REC];                                                                                            \
  __shared__ double Xs[2][7 * XCOLS], Qs[2][49], nks[2][8], stp[CH][ST], nod[CH][7], cors[XCOLS], Ss[HQ * LC], sgs[LC], kts[8], wks[16]; \
  const Sweep<XCOLS> L{rec, Xs, Qs, nks, stp, nod, cors, Ss, sgs, kts, wks}

// what a workgroup holds of its problem's nominal flight
struct Flight {
  ascent_params prm;
  Der d;
  double tf, dt, hs;
  int m;
  bool stretch;                               // the flight's rule: gain_t and stretch_max given, stretch_max > 0
};

ASC_DEV Flight flight_of(const ascent_params *__restrict__ P, long p, size_t B, int K, int substeps, const double *__restrict__ b,
                         const LincovArgs &A) {
  Flight F;
  F.prm = P[p];
  F.d = derive(F.prm);
  F.tf = b[(size_t)(21 * K + S_TH) * B];
  F.dt = (F.tf * F.d.T) / K;
  F.m = flight_substeps(F.dt, substeps);
  F.hs = F.dt / F.m;
  const double smax = A.gain_t && A.stretch_max ? A.stretch_max[p] : 0.0;
  F.stretch = smax > 0.0;
  return F;
}

// X_0 = [I | 0], Q_0 = 0, and what every step shares; the barrier after the first evaluation publishes them
template <int XCOLS>
ASC_DEV void prologue(const Sweep<XCOLS> &L, const LincovArgs &A, size_t B, long p, int t, bool stretch) {
  if (t < 7 * XCOLS) L.Xs[0][t] = t / XCOLS == t % XCOLS ? 1.0 : 0.0;
  if (t < 49) L.Qs[0][t] = 0.0;
  if (t < LC) L.sgs[t] = t < ASCENT_DISPERSE_COLS ? A.sigma[(size_t)t * B + p]
                                                  : A.sigma_nav ? A.sigma_nav[(size_t)(t - ASCENT_DISPERSE_COLS) * B + p] : 0.0;
  if (t < 7) L.kts[t] = stretch ? A.gain_t[(size_t)t * B + p] : 0.0;
  if (t == 7) L.kts[7] = stretch && A.ff_t ? A.ff_t[p] : 0.0;
  if (t < 16) L.wks[t] = A.ff_know ? A.ff_know[(size_t)t * B + p] : 0.0;
}

// group g evaluates step k (node k-1 -> k) and stages its record and what the sweep reads of it
template <int FORM, int XCOLS>
ASC_DEV void stage_step(const Sweep<XCOLS> &L, const LincovArgs &A, const Flight &F, const double *__restrict__ b, const double *__restrict__ tr,
                        size_t B, long p, int K, int k, int g, int col) {
  if (k > K) return;
  const int nt = K + 1;
  double z[7], dz[7];
  load_node(tr, B, nt, k - 1, z);
  const double u = b[(size_t)(7 * K + k - 1) * B];
  if (col < 7) {
    L.stp[g][col] = A.gain_u ? A.gain_u[((size_t)col * K + k - 1) * B + p] : 0.0;
  } else if (col == ST_F) {
    L.stp[g][ST_F] = A.ff_u ? A.ff_u[(size_t)(k - 1) * B + p] : 0.0;
  } else if (col == ST_SU2) {
    const double su = A.sigma_u ? A.sigma_u[(size_t)(k - 1) * B + p] : 0.0;
    L.stp[g][ST_SU2] = su * su;
  } else if (col == ST_U) {
    L.stp[g][ST_U] = u;
  } else if (col == NCOL - 1) {               // the nominal node the step ends at, f_fly's
    double zk[7];
    load_node(tr, B, nt, k, zk);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) L.nod[g][i] = zk[i];
  }
  ASC_UNROLL
  for (int i = 0; i < 7; i++) dz[i] = col == i ? 1.0 : 0.0;
  fly_step_tangent<FORM>(F.d, z, dz, u, F.hs, F.m, col);
  ASC_UNROLL
  for (int i = 0; i < 7; i++) L.rec[g * REC + i * NCOL + col] = dz[i];
}

// entry (xi, xc) of X_k from copy Xo of X_{k-1}; corr is the lane's own copy of corr_c.  pw is phi^k of the column's channel,
// read with DRIFT only: it scales the forcing of the columns nu and theta-hat, and column X_TW is forced by f_k unscaled
template <int XCOLS, bool DRIFT>
ASC_DEV double x_entry(const double *R, const double *kv, const double *kts, const double *Xo, bool last, double dt, int xi, int xc,
                       double pw, double &corr) {
  double x[7], a = 0.0;
  corr = 0.0;
  ASC_UNROLL
  for (int l = 0; l < 7; l++) x[l] = Xo[l * XCOLS + xc];
  ASC_UNROLL
  for (int l = 0; l < 7; l++) corr += kv[l] * x[l];
  if constexpr (DRIFT) {
    if (xc >= X_NU && xc < X_TH) corr += kv[xc - X_NU] * pw;
    if (xc == X_TH) corr += kv[ST_F] * pw;
    if (xc == X_TW) corr += kv[ST_F];
  } else {
    if (xc >= X_NU && xc < X_TH) corr += kv[xc - X_NU];
    if (xc == X_TH) corr += kv[ST_F];
  }
  ASC_UNROLL
  for (int l = 0; l < 7; l++) a += R[xi * NCOL + l] * x[l];
  a -= R[xi * NCOL + C_U] * corr;
  if (xc >= X_COEF && xc < X_NU) a += R[xi * NCOL + C_DT + (xc - X_COEF)];
  if (last) {
    double tau = 0.0;
    ASC_UNROLL
    for (int l = 0; l < 7; l++) tau -= kts[l] * x[l];
    if constexpr (DRIFT) {
      if (xc >= X_NU && xc < X_TH) tau -= kts[xc - X_NU] * pw;
      if (xc == X_TH) tau -= kts[7] * pw;
      if (xc == X_TW) tau -= kts[7];
    } else {
      if (xc >= X_NU && xc < X_TH) tau -= kts[xc - X_NU];
      if (xc == X_TH) tau -= kts[7];
    }
    a += (dt * R[xi * NCOL + C_DT]) * tau;
  }
  return a;
}

// row i of A_k = Phi_k - g_k K_k' (- gamma_K k_t' on a stretched last step)
ASC_DEV void closed_row(const double *R, const double *kv, const double *kt, bool last, double dt, int i, double *a) {
  const double gi = R[i * NCOL + C_U], ti = dt * R[i * NCOL + C_DT];
  ASC_UNROLL
  for (int l = 0; l < 7; l++) {
    double v = R[i * NCOL + l] - gi * kv[l];
    if (last) v -= ti * kt[l];
    a[l] = v;
  }
}

// the noise helper q: row q of A_k Q_{k-1} K_k for q < 7 (ar is that row of A_k), K_k' Q_{k-1} K_k for q = 7
ASC_DEV double helper_entry(const double *R, const double *kv, const double *kts, const double *Qo, bool last, double dt, int q,
                            double *ar) {
  double v[7], a = 0.0;
  ASC_UNROLL
  for (int l = 0; l < 7; l++) {
    double w = 0.0;
    ASC_UNROLL
    for (int mm = 0; mm < 7; mm++) w += Qo[l * 7 + mm] * kv[mm];
    v[l] = w;
  }
  closed_row(R, kv, kts, last, dt, q < 7 ? q : 0, ar);
  ASC_UNROLL
  for (int l = 0; l < 7; l++) a += (q < 7 ? ar[l] : kv[l]) * v[l];
  return a;
}

// the two phases of history node i, rows then covariance, after step s of the chunk wrote copy cp of X and Q (the helpers are in
// the other).  X_W is the column the parameter columns take their w_c from; without ok the rows are NaN, the structurally zero
// columns included
template <int FORM, int XCOLS, int X_W>
ASC_DEV void node_phase(const Sweep<XCOLS> &L, const LincovArgs &A, const Flight &F, int K, size_t B, long p, int t, int s, int cp, int i,
                        bool ok) {
  const double *R = L.rec + s * REC, *kv = L.stp[s], *Xn = L.Xs[cp], *Qn = L.Qs[cp], *zn = L.nod[s];
  // the altitude's gradient at the nominal node: (gax, gay) on (x, y), and the unit vector (ex, ey) of its direct terms
  const double S = F.prm.r_peri;
  const Radius rad = nominal_radius(zn[IX], zn[IY], S, F.prm.R0);
  const double ex = rad.X / rad.rr, ey = rad.Y / rad.rr, gax = S * ex, gay = S * ey;
  if (t < HQ) {
    double c[XCOLS], o[LC];
    ASC_UNROLL
    for (int cc = 0; cc < XCOLS; cc++) {
      const double xr = Xn[(t < 7 ? t : 0) * XCOLS + cc], al = gax * Xn[IX * XCOLS + cc] + gay * Xn[IY * XCOLS + cc], cr = L.cors[cc];
      c[cc] = t < 7 ? xr : t == 7 ? al : t == 8 ? -cr : cr;
    }
    const ApsisDirect dir = {0.0, 0.0, t == 7 ? ey - 1.0 : 0.0, t == 7 ? zn[IX] * ex + zn[IY] * ey : 0.0};
    jac_columns<FORM>(F.prm, F.d, F.tf, K, c, c + X_COEF, dir, o);
    if (A.ff_know) {
      ASC_UNROLL
      for (int cc = 0; cc < 16; cc++) o[7 + cc] += c[X_W] * L.wks[cc];
    }
    ASC_UNROLL
    for (int a = 0; a < ASCENT_NAV_ROWS; a++) o[ASCENT_DISPERSE_COLS + a] = c[X_NU + a];
    if (!ok) {
      ASC_UNROLL
      for (int cc = 0; cc < LC; cc++) o[cc] = NAN;
    }
    ASC_UNROLL
    for (int cc = 0; cc < LC; cc++) {
      L.Ss[t * LC + cc] = o[cc];
      if (A.jac) A.jac[(((size_t)t * LC + cc) * A.nj + i) * B + p] = o[cc];
    }
    const double nom = t < 7 ? zn[t] : t == 7 ? rad.rr - F.prm.R0 : t == 8 ? kv[ST_U] : 0.0;
    A.nominal[((size_t)t * A.nj + i) * B + p] = nom;
  }
  __syncthreads();
  if (t < NCOV) {
    int a = 0, rem = t;
    while (rem >= HQ - a) { rem -= HQ - a; a++; }
    const int bq = a + rem;                   // entry (a, bq), a <= bq
    double acc = 0.0;
    for (int cc = 0; cc < LC; cc++) {
      const double sg = L.sgs[cc];
      if (sg != 0.0) acc += (L.Ss[a * LC + cc] * L.Ss[bq * LC + cc]) * (sg * sg);
    }
    // the noise part: rows 0..6 Q_j, 7 the altitude's gradient on it, 8 / 9 through the helpers' covariances with corr_j and eps_j
    const double *nk = L.nks[cp ^ 1];
    const double su2 = kv[ST_SU2];
    const int ar = a < 7 ? a : 0;
    const double qa = gax * Qn[ar * 7 + IX] + gay * Qn[ar * 7 + IY];
    const double n8 = (su2 != 0.0 ? su2 * R[ar * NCOL + C_U] : 0.0) - nk[ar];
    const double n8x = (su2 != 0.0 ? su2 * R[IX * NCOL + C_U] : 0.0) - nk[IX], n8y = (su2 != 0.0 ? su2 * R[IY * NCOL + C_U] : 0.0) - nk[IY];
    double n;
    if (bq < 7) n = Qn[a * 7 + bq];
    else if (a < 7) n = bq == 7 ? qa : bq == 8 ? n8 : nk[a];
    else if (a == 7)
      n = bq == 7 ? gax * (gax * Qn[IX * 7 + IX] + gay * Qn[IX * 7 + IY]) + gay * (gax * Qn[IY * 7 + IX] + gay * Qn[IY * 7 + IY])
          : bq == 8 ? gax * n8x + gay * n8y : gax * nk[IX] + gay * nk[IY];
    else if (a == 8) n = bq == 8 ? nk[7] + su2 : -nk[7];
    else n = nk[7];
    acc += n;
    A.cov[((size_t)t * A.nj + i) * B + p] = ok ? acc : NAN;
  }
}

template <int FORM>
__global__ __launch_bounds__(JB) void l_lincov(const ascent_params *__restrict__ P, long batch, int K, int substeps,
                                               const double *__restrict__ blob, const double *__restrict__ traj, LincovArgs A) {
  ASC_SWEEP_LDS(XC, L);
  const long p = blockIdx.x;
  const size_t B = (size_t)batch;
  const int t = threadIdx.x, g = t >> 4, col = t & (NCOL - 1);
  const double *b = blob + p, *tr = traj + p;
  const Flight F = flight_of(P, p, B, K, substeps, b, A);
  prologue(L, A, B, p, t, F.stretch);

  const int nch = (K + CH - 1) / CH;
  for (int c = 0; c < nch; c++) {
    stage_step<FORM>(L, A, F, b, tr, B, p, K, c * CH + g + 1, g, col);
    __syncthreads();
    const int top = K - c * CH < CH ? K - c * CH : CH;
    for (int s = 0; s < top; s++) {
      const int kk = c * CH + s, par = kk & 1;            // step kk + 1 reads copy par and writes the other
      const double *R = L.rec + s * REC, *kv = L.stp[s], *Qo = L.Qs[par];
      const bool last = F.stretch && kk + 1 == K;
      if (t < T_NK) {
        const int xi = t / XC, xc = t - xi * XC;
        double corr;
        L.Xs[par ^ 1][t] = x_entry<XC, false>(R, kv, L.kts, L.Xs[par], last, F.dt, xi, xc, 0.0, corr);
        if (xi == 0) L.cors[xc] = corr;
      } else if (t >= T_NK && t < T_NK + 8) {
        double ar[7];
        L.nks[par][t - T_NK] = helper_entry(R, kv, L.kts, Qo, last, F.dt, t - T_NK, ar);
      } else if (t >= T_Q && t < T_Q + 49) {
        const int q = t - T_Q, qi = q / 7, qj = q - qi * 7;
        // both halves; the same lines stand in l_lincov_drifting (header: the piece left unshared)
        double ai[7], aj[7], nij = 0.0, nji = 0.0;
        closed_row(R, kv, L.kts, last, F.dt, qi, ai);
        closed_row(R, kv, L.kts, last, F.dt, qj, aj);
        ASC_UNROLL
        for (int l = 0; l < 7; l++) {
          double wi = 0.0, wj = 0.0;
          ASC_UNROLL
          for (int mm = 0; mm < 7; mm++) {
            const double ql = Qo[l * 7 + mm];
            wj += ql * aj[mm];
            wi += ql * ai[mm];
          }
          nij += ai[l] * wj;
          nji += aj[l] * wi;
        }
        const double su2 = kv[ST_SU2];
        const double gg = su2 != 0.0 ? su2 * (R[qi * NCOL + C_U] * R[qj * NCOL + C_U]) : 0.0;
        L.Qs[par ^ 1][q] = 0.5 * ((nij + gg) + (nji + gg));
      }
      __syncthreads();
      const int j = kk + 1;
      if (j % A.stride == 0 || j == K)                    // a history node (uniform)
        node_phase<FORM, XC, X_TH>(L, A, F, K, B, p, t, s, par ^ 1, (j + A.stride - 1) / A.stride - 1, finite1(F.tf));
    }
    __syncthreads();                          // the records and the staged steps are rewritten by the next chunk
  }
}

// D_k of a channel from D_{k-1}; not contracted, so that every lane that forms it has the same bits
ASC_DEV double drift_var(double phi, double dold, double q2) {
#pragma clang fp contract(off)
  return (phi * dold) * phi + q2;
}

// what the Q lanes and the helpers share of the drifting terms: c1 = C_{k-1} Phi_n kappa, c2 = C_{k-1} Phi_n (k_t, f_t) (7 each),
// skk = kappa' D_k kappa, skt = kappa' D_k (k_t, f_t), stt = (k_t, f_t)' D_k (k_t, f_t); c2, skt and stt only on a stretched last step
struct DriftTerms { double c1[7], c2[7], skk, skt, stt; };

ASC_DEV void drift_terms(const double *Co, const double *Do, const double *phs, const double *q2s, const double *kv, const double *kts,
                         bool last, DriftTerms &T) {
  static_assert(ST_F == 7, "kappa_k = (K_k, f_k) is the head of a staged step");
  double kp[8], tp[8];
  T.skk = T.skt = T.stt = 0.0;
  ASC_UNROLL
  for (int a = 0; a < 8; a++) {
    const double ka = kv[a], ta = last ? kts[a] : 0.0, dk = drift_var(phs[a], Do[a], q2s[a]);      // (kv[7] is f_k: ST_F = 7)
    kp[a] = phs[a] * ka;
    tp[a] = phs[a] * ta;
    T.skk += (ka * ka) * dk;
    T.skt += (ka * ta) * dk;
    T.stt += (ta * ta) * dk;
  }
  ASC_UNROLL
  for (int l = 0; l < 7; l++) {
    double a1 = 0.0, a2 = 0.0;
    ASC_UNROLL
    for (int a = 0; a < 8; a++) {
      a1 += Co[l * 8 + a] * kp[a];
      a2 += Co[l * 8 + a] * tp[a];
    }
    T.c1[l] = a1;
    T.c2[l] = a2;
  }
}

template <int FORM>
__global__ __launch_bounds__(JB) void l_lincov_drifting(const ascent_params *__restrict__ P, long batch, int K, int substeps,
                                                        const double *__restrict__ blob, const double *__restrict__ traj, LincovArgs A,
                                                        DriftCov G) {
  ASC_SWEEP_LDS(XCD, L);
  __shared__ double Cs[2][56], Ds[2][8], pws[2][8], phs[8], q2s[8];
  __shared__ int flags[2];                   // any channel drifting; any phi or q out of range
  const long p = blockIdx.x;
  const size_t B = (size_t)batch;
  const int t = threadIdx.x, g = t >> 4, col = t & (NCOL - 1);
  const double *b = blob + p, *tr = traj + p;
  const Flight F = flight_of(P, p, B, K, substeps, b, A);
  prologue(L, A, B, p, t, F.stretch);
  if (t >= T_C && t < T_C + 56) Cs[0][t - T_C] = 0.0;
  if (t >= T_C && t < T_C + 8) {
    const int a = t - T_C;
    const double ph = G.phi ? G.phi[(size_t)a * B + p] : 1.0, q = G.q ? G.q[(size_t)a * B + p] : 0.0;
    phs[a] = ph;
    q2s[a] = q * q;
    Ds[0][a] = 0.0;
    pws[0][a] = 1.0;
  }
  if (t == JB - 1) {                         // the two flags, by one lane in ascending channel order
    int drift = 0, bad = 0;
    for (int a = 0; a < 8; a++) {
      const double ph = G.phi ? G.phi[(size_t)a * B + p] : 1.0, q = G.q ? G.q[(size_t)a * B + p] : 0.0;
      drift |= !(ph == 1.0 && q == 0.0);
      bad |= !(ph >= 0.0 && ph <= 1.0) || !(q >= 0.0 && q <= 1.7976931348623157e308);
    }
    flags[0] = drift;
    flags[1] = bad;
  }

  const int nch = (K + CH - 1) / CH;
  for (int c = 0; c < nch; c++) {
    stage_step<FORM>(L, A, F, b, tr, B, p, K, c * CH + g + 1, g, col);
    __syncthreads();
    const bool drift = flags[0] != 0, ok = finite1(F.tf) && flags[1] == 0;
    const int top = K - c * CH < CH ? K - c * CH : CH;
    for (int s = 0; s < top; s++) {
      const int kk = c * CH + s, par = kk & 1;            // step kk + 1 reads copy par and writes the other
      const double *R = L.rec + s * REC, *kv = L.stp[s], *kts = L.kts, *Qo = L.Qs[par], *Co = Cs[par], *Do = Ds[par];
      const double dt = F.dt;
      const bool last = F.stretch && kk + 1 == K;
      if (t < T_C) {
        const int xi = t / XCD, xc = t - xi * XCD;
        const int ch = xc >= X_NU && xc <= X_TH ? xc - X_NU : 0;
        const double pw = pws[par][ch] * phs[ch];          // phi^k of the column's channel (used by the columns nu and theta-hat only)
        double corr;
        L.Xs[par ^ 1][t] = x_entry<XCD, true>(R, kv, kts, L.Xs[par], last, dt, xi, xc, pw, corr);
        if (xi == 0) L.cors[xc] = corr;
      } else if (t >= T_QU) {
        int qi = 0, qj = t - T_QU;
        while (qj >= 7 - qi) { qj -= 7 - qi; qi++; }
        qj += qi;                             // entry (qi, qj), qi <= qj
        // both halves, l_lincov's lines
        double ai[7], aj[7], nij = 0.0, nji = 0.0;
        closed_row(R, kv, kts, last, dt, qi, ai);
        closed_row(R, kv, kts, last, dt, qj, aj);
        ASC_UNROLL
        for (int l = 0; l < 7; l++) {
          double wi = 0.0, wj = 0.0;
          ASC_UNROLL
          for (int mm = 0; mm < 7; mm++) {
            const double ql = Qo[l * 7 + mm];
            wj += ql * aj[mm];
            wi += ql * ai[mm];
          }
          nij += ai[l] * wj;
          nji += aj[l] * wi;
        }
        const double su2 = kv[ST_SU2];
        const double gg = su2 != 0.0 ? su2 * (R[qi * NCOL + C_U] * R[qj * NCOL + C_U]) : 0.0;
        double hij = nij + gg, hji = nji + gg;
        if (drift) {                          // M + M' + B D B' of the entry
          DriftTerms T;
          drift_terms(Co, Do, phs, q2s, kv, kts, last, T);
          const int lo = qi, hi = qj;
          double l1 = 0.0, l2 = 0.0, h1 = 0.0, h2 = 0.0;
          ASC_UNROLL
          for (int l = 0; l < 7; l++) {
            l1 += ai[l] * T.c1[l];
            l2 += ai[l] * T.c2[l];
            h1 += aj[l] * T.c1[l];
            h2 += aj[l] * T.c2[l];
          }
          const double gl = R[lo * NCOL + C_U], gh = R[hi * NCOL + C_U];
          double e = T.skk * (gl * gh) - (l1 * gh + h1 * gl);
          if (last) {
            const double tl = dt * R[lo * NCOL + C_DT], th = dt * R[hi * NCOL + C_DT];
            e += T.skt * (gl * th + tl * gh) + T.stt * (tl * th) - (l2 * th + h2 * tl);
          }
          hij += e;
          hji += e;
        }
        const double qn = 0.5 * (hij + hji);
        L.Qs[par ^ 1][qi * 7 + qj] = qn;
        L.Qs[par ^ 1][qj * 7 + qi] = qn;
      } else if (t >= T_C && t < T_C + 56) {
        const int q = t - T_C, ci = q >> 3, ca = q & 7;
        double v = 0.0;
        if (drift) {
          double ar[7], ac = 0.0;
          closed_row(R, kv, kts, last, dt, ci, ar);
          ASC_UNROLL
          for (int l = 0; l < 7; l++) ac += ar[l] * Co[l * 8 + ca];
          double bia = -R[ci * NCOL + C_U] * kv[ca];
          if (last) bia -= (dt * R[ci * NCOL + C_DT]) * kts[ca];
          v = ac * phs[ca] + bia * drift_var(phs[ca], Do[ca], q2s[ca]);
        }
        Cs[par ^ 1][q] = v;
      }
      if (t >= T_C && t < T_C + 8) {          // the helpers: the lanes of row 0 of C
        const int q = t - T_C;
        double ar[7];
        double a = helper_entry(R, kv, kts, Qo, last, dt, q, ar);
        if (drift) {
          DriftTerms T;
          drift_terms(Co, Do, phs, q2s, kv, kts, last, T);
          double ac1 = 0.0, k1 = 0.0, k2 = 0.0;
          ASC_UNROLL
          for (int l = 0; l < 7; l++) {
            ac1 += ar[l] * T.c1[l];
            k1 += kv[l] * T.c1[l];
            k2 += kv[l] * T.c2[l];
          }
          if (q < 7) {
            double e = ac1 - R[q * NCOL + C_U] * (k1 + T.skk);
            if (last) e -= (dt * R[q * NCOL + C_DT]) * (k2 + T.skt);
            a += e;
          } else {
            a += 2.0 * k1 + T.skk;
          }
        }
        L.nks[par][q] = a;
        pws[par ^ 1][q] = pws[par][q] * phs[q];
        Ds[par ^ 1][q] = drift_var(phs[q], Do[q], q2s[q]);
      }
      __syncthreads();
      const int j = kk + 1;
      if (j % A.stride == 0 || j == K)                    // a history node (uniform); no final time, or a phi or q out of range: NaN rows
        node_phase<FORM, XCD, X_TW>(L, A, F, K, B, p, t, s, par ^ 1, (j + A.stride - 1) / A.stride - 1, ok);
    }
    __syncthreads();                          // the records and the staged steps are rewritten by the next chunk
  }
}

// the sweep of one formulation: l_lincov, with io.nav_phi l_lincov_drifting
template <int FORM>
void launch_sweep(const Call &c, int substeps, const LincovIO &io, const double *traj, const LincovArgs &a) {
  const dim3 grid((unsigned)c.batch), block(JB);
  if (io.nav_phi)
    hipLaunchKernelGGL((l_lincov_drifting<FORM>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, io.blob, traj, a,
                       DriftCov{io.nav_phi, io.nav_q});
  else hipLaunchKernelGGL((l_lincov<FORM>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, io.blob, traj, a);
}

}  // namespace

size_t lincov_ws_bytes(int K, long batch) { return flight_ws_bytes(K, batch); }

int lincov_run(const Call &c, int substeps, const LincovIO &io, double *ws) {
  const FlightWs w = flight_ws(ws, c.K, c.batch);
  if (const int rc = flight_fly_only(c, substeps, io.blob, w.traj, w.fsum)) return rc;
  const LincovArgs a{io.sigma, io.sigma_u, io.gain_u, io.gain_t, io.stretch_max, io.ff_u, io.ff_t, io.ff_know, io.sigma_nav,
                     io.node_stride, history_nodes(c.K, io.node_stride), io.nominal, io.cov, io.jac};
  if (c.form == 1) launch_sweep<1>(c, substeps, io, w.traj, a);
  else launch_sweep<0>(c, substeps, io, w.traj, a);
  ASC_CHK(c.err, c.errlen, hipGetLastError());
  return ASCENT_OK;
}

}  // namespace ascent
