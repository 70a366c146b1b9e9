// Guidance gains (include/ascent.h: ascent_guidance_gains): the neighbouring-optimal feedback about a flown solution.
//
// The linearisation is j_jac's (ascent_trim.hip): about the states f_fly wrote into the workspace trajectory, the step records
// [Phi_k | g_k | Gamma_k] from fly_step_tangent.  Deviations obey dz_k = Phi_k dz_{k-1} + g_k du_k + [k = K] gamma_K tau with
// gamma_K = dt dz_K/d dt (tau: the relative stretch of the last step), and the cost is
//   1/2 sum_i q_i (c_i' dz_K)^2 + 1/2 r_u sum_k du_k^2 + 1/2 r_t tau^2,   c_i = grad (e3, g1, g2) of terminal_eval at z_K.
//
// g_gains  one workgroup of JB = 256 threads per NLP, chunks of CH = 16 steps, last chunk first; evaluation and LDS staging
//          exactly as j_jac.  Wave 0 then takes the chunk's steps in descending order, P (7 x 7), Lambda (9 x 7) and the 9 x 8
//          accumulators in LDS between the chunks:
//   A      lane (i, j) < 49: M = P Phi;  lanes 49..55 / 56..62: w_u = P g, w_t = P gamma
//   B      every lane, redundantly (LDS broadcasts): S = R + B' P B (at most 2 x 2: the column g if |u_k| < 0.999, the column
//          gamma if k = K and stretch_max > 0), G = S^-1 (w' Phi) -- a division, or the closed-form 2 x 2 inverse on the last
//          step --; lane j < 7 stores G_j.  A non-finite S, a pivot or a determinant <= 0 freezes the problem.
//   C      lane (i, j) < 49: P <- 1/2 (N_ij + N_ji), N = Phi' M - G' S G, both halves computed by the lane itself, so P stays
//          exactly symmetric;  lane q < 9: row q of Lambda <- Lambda (Phi - g K' - gamma k_t'), Lambda g to jac_u, Lambda Gamma
//          into the accumulators -- j_jac's sweep with the gain terms taken off.
//          The phases of one wavefront are ordered by LDS's in-order execution; wave_sync keeps the compiler from reordering them.
//   The two ends of the Jacobian part are j_jac's own functions (ascent_tangent_dev.hpp): lambda_apsis_rows starts Lambda_K,
//   jac_columns is the epilogue's chain rule; the trim depends on j_jac's bits, and both kernels keep the parent text's.
// The order of every addition is fixed: a problem gives the same bits alone as inside any batch.
//
// g_gains_ff  the same sweep with a thrust (parameter) feed-forward (include/ascent.h: ascent_guidance_feedforward): one body,
//          gains_body<FORM, FF>, so the P-part above is one source text and its gains are g_gains' bits.  The deviation state is
//          augmented by one constant scalar theta along the caller's direction d of the 16 fields: step forcing pi_k = Gamma_k d
//          through the transpose of the epilogue's chain rule (tangent_coefficients, beside jac_columns: eight wave-uniform
//          coefficients), formed by every group from its own tangent
//          columns when the records are staged -- a butterfly over the 16 lanes of the group --, 7 doubles per step in LDS.
//          The value function gains the column p (7 doubles in LDS); per step, beside the phases above:
//   A      lanes 49..55 also: a = P pi + p, a second chain inside the loop that forms P g
//   B      every lane: hf = B' a, column pj of a' Phi -- three more chains in the loop that forms S -- and f = S^-1 hf by the
//          same closed forms as G; lane 0 stores f_k (f_t on the last step); lanes 49..55 store p <- Phi' a - G' S f
//   C      lane q < 9: E_q += (Lambda g) f_k + (Lambda gamma) f_t and the seven navigation columns += (Lambda g) K_k +
//          (Lambda gamma) k_t, eight more accumulators per row
//   epilogue   parameter column c -= E_q w_c (w: the knowledge row), jac_nav = -[navigation columns | E_q].
//          pi0 (the scalar of the value function) is not carried: no output depends on it.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>

#include "ascent.h"
#include "ascent_device.hpp"
#include "ascent_flight.hpp"
#include "ascent_flight_dev.hpp"
#include "ascent_guide.hpp"
#include "ascent_tangent_dev.hpp"
#include "ascent_trim.hpp"

namespace ascent {
namespace {

constexpr int GW = 64;                     // the sweeping wavefront
constexpr int W_QE3 = 0, W_RU = 3, W_RT = 4, W_SMAX = 5;      // rows of weights [6][batch]

// orders the LDS traffic of the phases of one wavefront (the hardware executes a wavefront's LDS instructions in order)
ASC_DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int NNAV = ASCENT_NAV_ROWS;

// FF = false: g_gains, and no trace of the feed-forward arguments (all null) in the code
template <int FORM, bool FF>
ASC_DEV void gains_body(const ascent_params *__restrict__ P, long batch, int K, int substeps,
                        const double *__restrict__ blob, const double *__restrict__ traj,
                        const double *__restrict__ weights, double *__restrict__ gain_u,
                        double *__restrict__ gain_t, double *__restrict__ summary,
                        double *__restrict__ jac, double *__restrict__ jac_u, const double *__restrict__ ff_dir,
                        const double *__restrict__ ff_know, double *__restrict__ ff_u, double *__restrict__ ff_t,
                        double *__restrict__ jac_nav) {
  __shared__ double rec[CH * REC];
  __shared__ double Ps[49], Ms[49], Ws[14], Gs[14], Ls[JROWS * 7], As[JROWS * NACC];
  __shared__ double pis[FF ? CH * 7 : 1], pv[FF ? 7 : 1], av[FF ? 7 : 1], Ns[FF ? JROWS * NNAV : 1];      // pi_k, p, a, nav accumulators
  __shared__ int frozen_s;
  const long p = blockIdx.x;
  const size_t B = (size_t)batch;
  const int t = threadIdx.x, g = t >> 4, col = t & (NCOL - 1);
  const int nt = K + 1;
  const double *b = blob + p, *tr = traj + p;
  const ascent_params prm = P[p];
  const Der d = derive(prm);
  const double tf = b[(size_t)(21 * K + S_TH) * B];
  const double dt = (tf * d.T) / K;
  const int m = flight_substeps(dt, substeps);
  const double hs = dt / m;
  const double ru = weights[(size_t)W_RU * B + p], rt = weights[(size_t)W_RT * B + p], smax = weights[(size_t)W_SMAX * B + p];
  const int pi = t < 49 ? t / 7 : 0, pj = t % 7;      // lane (pi, pj) of P; every lane: column pj of a gain row

  // pi_k = R[:, C_DT .. C_MRATE] . coef: the epilogue's chain rule transposed onto the direction; this lane's coefficient
  double cf = 0.0;
  bool dok = true;
  if constexpr (FF) {
    double dd[16], coef[NACC];
    ASC_UNROLL
    for (int i = 0; i < 16; i++) { dd[i] = ff_dir[(size_t)i * B + p]; dok = dok && finite1(dd[i]); }
    if (ff_know) {
      ASC_UNROLL
      for (int i = 0; i < 16; i++) dok = dok && finite1(ff_know[(size_t)i * B + p]);
    }
    tangent_coefficients<FORM>(prm, d, tf, K, dd, coef);
    ASC_UNROLL
    for (int a = 0; a < NACC; a++) cf = col == C_DT + a ? coef[a] : cf;
  }

  ApsisDirect dir = {0.0, 0.0, 0.0, 0.0};
  double nf = 0.0, gmax = 0.0, tmax = 0.0, fmax_u = 0.0, fmax_t = 0.0;
  if (t < GW) {
    double zK[7], q[3];
    load_node(tr, B, nt, K, zK);
    ASC_UNROLL
    for (int i = 0; i < 3; i++) q[i] = weights[(size_t)(W_QE3 + i) * B + p];
    const bool wok = q[0] >= 0.0 && q[1] >= 0.0 && q[2] >= 0.0 && ru > 0.0 && rt > 0.0 && smax >= 0.0 && finite1(q[0]) &&
                     finite1(q[1]) && finite1(q[2]) && finite1(ru) && finite1(rt) && finite1(smax);
    if (t == 0) frozen_s = wok && dok ? 0 : 1;
    // P_K = sum_i q_i c_i c_i'
    const Terminal tm = terminal_eval(d, zK);
    const double cg[3][7] = {{tm.e3g[0], tm.e3g[1], tm.e3g[2], tm.e3g[3], 0.0, 0.0, 0.0},
                             {tm.g1g[0], tm.g1g[1], 0.0, 0.0, 0.0, 0.0, 0.0},
                             {0.0, 0.0, tm.g2g[0], tm.g2g[1], 0.0, 0.0, 0.0}};
    if (t < 49) {
      double a = 0.0;
      ASC_UNROLL
      for (int i = 0; i < 3; i++) {
        double ci = 0.0, cj = 0.0;
        ASC_UNROLL
        for (int l = 0; l < 7; l++) { ci = l == pi ? cg[i][l] : ci; cj = l == pj ? cg[i][l] : cj; }
        a += q[i] * (ci * cj);
      }
      Ps[t] = a;
    }
    if constexpr (FF) {
      if (t < 7) pv[t] = 0.0;
    }
    // Lambda_K = I / grad apsides, as j_jac
    if (jac) {
      double L[7];
      ASC_UNROLL
      for (int i = 0; i < 7; i++) L[i] = t == i ? 1.0 : 0.0;
      lambda_apsis_rows(prm, zK, t, L, dir);
      if (t < JROWS) {
        ASC_UNROLL
        for (int i = 0; i < 7; i++) Ls[t * 7 + i] = L[i];
        ASC_UNROLL
        for (int a = 0; a < NACC; a++) As[t * NACC + a] = 0.0;
        if constexpr (FF) {
          ASC_UNROLL
          for (int a = 0; a < NNAV; a++) Ns[t * NNAV + a] = 0.0;
        }
      }
    }
    for (int k = t; k < K; k += GW) nf += fabs(b[(size_t)(7 * K + k) * B]) < 0.999 ? 1.0 : 0.0;
    nf = wave_sum(nf);
  }
  __syncthreads();

  const int nch = (K + CH - 1) / CH;
  for (int c = nch - 1; c >= 0; c--) {
    if (frozen_s) break;                      // uniform: read between two barriers
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
      if constexpr (FF) {                     // pi of this step: the group's parameter columns times their coefficients, summed over the group
        ASC_UNROLL
        for (int i = 0; i < 7; i++) {
          double v = col >= C_DT ? dz[i] * cf : 0.0;
          ASC_UNROLL
          for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off);
          if (col == 0) pis[g * 7 + i] = v;
        }
      }
    }
    __syncthreads();
    if (t < GW) {
      const int top = K - c * CH < CH ? K - c * CH : CH;
      bool ok = true;
      for (int s = top - 1; s >= 0 && ok; s--) {
        const double *R = rec + s * REC;
        const int kk = c * CH + s;            // step kk + 1
        const double uk = b[(size_t)(7 * K + kk) * B];
        const bool f1 = fabs(uk) < 0.999, f2 = kk + 1 == K && smax > 0.0;
        // A
        if (t < 49) {
          double a = 0.0;
          ASC_UNROLL
          for (int l = 0; l < 7; l++) a += Ps[pi * 7 + l] * R[l * NCOL + pj];
          Ms[t] = a;
        } else if (t < 63) {
          const int cc = t < 56 ? C_U : C_DT;
          const double sc = t < 56 ? 1.0 : dt;
          double a = 0.0, e = 0.0;
          if constexpr (FF) e = pv[pj];
          ASC_UNROLL
          for (int l = 0; l < 7; l++) {
            a += Ps[pj * 7 + l] * (sc * R[l * NCOL + cc]);
            if constexpr (FF) e += Ps[pj * 7 + l] * pis[s * 7 + l];      // a second chain beside the first, in all 14 lanes: no branch of its own
          }
          Ws[t - 49] = a;
          if constexpr (FF) {
            if (t < 56) av[pj] = e;
          }
        }
        wave_sync();
        // B
        double s11 = ru, s12 = 0.0, s22 = rt, h1 = 0.0, h2 = 0.0;
        ASC_UNROLL
        for (int l = 0; l < 7; l++) {
          const double gl = R[l * NCOL + C_U], tl = dt * R[l * NCOL + C_DT];
          s11 += gl * Ws[l];
          s12 += gl * Ws[7 + l];
          s22 += tl * Ws[7 + l];
          h1 += Ws[l] * R[l * NCOL + pj];
          h2 += Ws[7 + l] * R[l * NCOL + pj];
        }
        double e1 = 0.0, e2 = 0.0, ep = 0.0;  // B' a, and column pj of a' Phi
        if constexpr (FF) {
          ASC_UNROLL
          for (int l = 0; l < 7; l++) {
            e1 += R[l * NCOL + C_U] * av[l];
            e2 += (dt * R[l * NCOL + C_DT]) * av[l];
            ep += R[l * NCOL + pj] * av[l];
          }
        }
        double g1 = 0.0, g2 = 0.0, fu = 0.0, ft = 0.0;
        if (f1 && f2) {
          const double det = s11 * s22 - s12 * s12;
          ok = finite1(s11) && finite1(s12) && finite1(s22) && s11 > 0.0 && s22 > 0.0 && det > 0.0;
          g1 = (s22 * h1 - s12 * h2) / det;
          g2 = (s11 * h2 - s12 * h1) / det;
          if constexpr (FF) {
            fu = (s22 * e1 - s12 * e2) / det;
            ft = (s11 * e2 - s12 * e1) / det;
          }
        } else if (f1) {
          ok = finite1(s11) && s11 > 0.0;
          g1 = h1 / s11;
          if constexpr (FF) fu = e1 / s11;
          s12 = 0.0; s22 = 0.0;
        } else if (f2) {
          ok = finite1(s22) && s22 > 0.0;
          g2 = h2 / s22;
          if constexpr (FF) ft = e2 / s22;
          s11 = 0.0; s12 = 0.0;
        } else {
          s11 = 0.0; s12 = 0.0; s22 = 0.0;
        }
        if (!ok) break;                       // uniform: every lane computed the same S
        if constexpr (FF) {
          if (t == 0) {
            ff_u[(size_t)kk * B + p] = fu;
            if (kk + 1 == K) ff_t[p] = ft;
          }
          fmax_u = max_nan(fmax_u, fabs(fu));
          fmax_t = max_nan(fmax_t, fabs(ft));
          // p <- Phi' a - G' S f: every lane holds column pj of G and of a' Phi; lanes 49..55 store theirs (p is read in A only)
          if (t >= 49 && t < 56) pv[pj] = ep - (g1 * (s11 * fu + s12 * ft) + g2 * (s12 * fu + s22 * ft));
        }
        if (t < 7) {
          Gs[t] = g1;
          Gs[7 + t] = g2;
          gain_u[((size_t)t * K + kk) * B + p] = g1;
          if (kk + 1 == K) gain_t[(size_t)t * B + p] = g2;
          gmax = max_nan(gmax, fabs(g1));
          tmax = max_nan(tmax, fabs(g2));
        }
        wave_sync();
        // C
        if (t < 49) {
          double nij = 0.0, nji = 0.0;
          ASC_UNROLL
          for (int l = 0; l < 7; l++) {
            nij += R[l * NCOL + pi] * Ms[l * 7 + pj];
            nji += R[l * NCOL + pj] * Ms[l * 7 + pi];
          }
          const double ui = Gs[pi], uj = Gs[pj], ti = Gs[7 + pi], tj = Gs[7 + pj];
          nij -= ui * (s11 * uj + s12 * tj) + ti * (s12 * uj + s22 * tj);
          nji -= uj * (s11 * ui + s12 * ti) + tj * (s12 * ui + s22 * ti);
          Ps[t] = 0.5 * (nij + nji);
        }
        if (jac && t < JROWS) {
          double L[7], o[NCOL];
          ASC_UNROLL
          for (int i = 0; i < 7; i++) L[i] = Ls[t * 7 + i];
          ASC_UNROLL
          for (int cc = 0; cc < NCOL; cc++) {
            double a = 0.0;
            ASC_UNROLL
            for (int i = 0; i < 7; i++) a += L[i] * R[i * NCOL + cc];
            o[cc] = a;
          }
          if (jac_u) jac_u[((size_t)t * K + kk) * B + p] = o[C_U];
          ASC_UNROLL
          for (int a = 0; a < NACC; a++) As[t * NACC + a] += o[C_DT + a];
          const double ot = dt * o[C_DT];
          if constexpr (FF) {
            double *N = Ns + t * NNAV;
            ASC_UNROLL
            for (int i = 0; i < 7; i++) {
              double v = N[i];
              if (f1) v += o[C_U] * Gs[i];
              if (f2) v += ot * Gs[7 + i];
              N[i] = v;
            }
            double v = N[7];
            if (f1) v += o[C_U] * fu;
            if (f2) v += ot * ft;
            N[7] = v;
          }
          ASC_UNROLL
          for (int i = 0; i < 7; i++) {
            double v = o[i];
            if (f1) v -= o[C_U] * Gs[i];
            if (f2) v -= ot * Gs[7 + i];
            Ls[t * 7 + i] = v;
          }
        }
        wave_sync();
      }
      if (!ok && t == 0) frozen_s = 1;
    }
    __syncthreads();
  }
  __syncthreads();
  const bool frozen = frozen_s != 0;

  if (t < GW) {
    gmax = t < 7 ? gmax : 0.0;
    tmax = t < 7 ? tmax : 0.0;
    ASC_UNROLL
    for (int off = 4; off >= 1; off >>= 1) { gmax = max_nan(gmax, __shfl_xor(gmax, off)); tmax = max_nan(tmax, __shfl_xor(tmax, off)); }
    if (t == 0) {
      summary[(size_t)0 * B + p] = frozen ? 2.0 : 0.0;
      summary[(size_t)1 * B + p] = nf;
      summary[(size_t)2 * B + p] = frozen ? NAN : gmax;
      summary[(size_t)3 * B + p] = frozen ? NAN : tmax;
      summary[(size_t)4 * B + p] = (double)m;
      if constexpr (FF) {                     // wave-uniform: every lane formed the same f
        summary[(size_t)5 * B + p] = frozen ? NAN : fmax_u;
        summary[(size_t)6 * B + p] = frozen ? NAN : fmax_t;
      }
    }
  }
  if (frozen) {                               // NaN gains and Jacobian; after the sweeping wavefront's own stores have landed
    __threadfence();
    __syncthreads();
    for (int e = t; e < 7 * K; e += JB) gain_u[(size_t)e * B + p] = NAN;
    if (t < 7) gain_t[(size_t)t * B + p] = NAN;
    if (jac)
      for (int e = t; e < JROWS * JCOLS; e += JB) jac[(size_t)e * B + p] = NAN;
    if (jac_u)
      for (int e = t; e < JROWS * K; e += JB) jac_u[(size_t)e * B + p] = NAN;
    if constexpr (FF) {
      for (int e = t; e < K; e += JB) ff_u[(size_t)e * B + p] = NAN;
      if (t == 0) ff_t[p] = NAN;
      if (jac_nav)
        for (int e = t; e < JROWS * NNAV; e += JB) jac_nav[(size_t)e * B + p] = NAN;
    }
    return;
  }

  if (jac && t < JROWS) {
    double o[JCOLS];
    jac_columns<FORM>(prm, d, tf, K, Ls + t * 7, As + t * NACC, dir, o);
    if constexpr (FF) {                                               // theta-hat = w . dp steers against E_q
      const double *N = Ns + t * NNAV;
      const double eq = N[7];
      ASC_UNROLL
      for (int cc = 0; cc < 16; cc++) o[7 + cc] -= eq * ff_know[(size_t)cc * B + p];
      if (jac_nav) {
        ASC_UNROLL
        for (int a = 0; a < NNAV; a++) jac_nav[((size_t)t * NNAV + a) * B + p] = -N[a];
      }
    }
    ASC_UNROLL
    for (int cc = 0; cc < JCOLS; cc++) jac[((size_t)t * JCOLS + cc) * B + p] = o[cc];
  }
}

template <int FORM>
__global__ __launch_bounds__(JB) void g_gains(const ascent_params *__restrict__ P, long batch, int K, int substeps,
                                              const double *__restrict__ blob, const double *__restrict__ traj,
                                              const double *__restrict__ weights, double *__restrict__ gain_u,
                                              double *__restrict__ gain_t, double *__restrict__ summary,
                                              double *__restrict__ jac, double *__restrict__ jac_u) {
  gains_body<FORM, false>(P, batch, K, substeps, blob, traj, weights, gain_u, gain_t, summary, jac, jac_u, nullptr, nullptr, nullptr,
                          nullptr, nullptr);
}

template <int FORM>
__global__ __launch_bounds__(JB) void g_gains_ff(const ascent_params *__restrict__ P, long batch, int K, int substeps,
                                                 const double *__restrict__ blob, const double *__restrict__ traj,
                                                 const double *__restrict__ weights, double *__restrict__ gain_u,
                                                 double *__restrict__ gain_t, double *__restrict__ summary,
                                                 double *__restrict__ jac, double *__restrict__ jac_u,
                                                 const double *__restrict__ ff_dir, const double *__restrict__ ff_know,
                                                 double *__restrict__ ff_u, double *__restrict__ ff_t, double *__restrict__ jac_nav) {
  gains_body<FORM, true>(P, batch, K, substeps, blob, traj, weights, gain_u, gain_t, summary, jac, jac_u, ff_dir, ff_know, ff_u, ff_t,
                         jac_nav);
}

}  // namespace

size_t gains_ws_bytes(int K, long batch) { return jac_ws_bytes(K, batch); }

template <int FORM>
static void gains_launch(const Call &c, int substeps, const GainsIO &io, const double *traj) {
  const dim3 grid((unsigned)c.batch), block(JB);
  if (io.ff_dir)
    hipLaunchKernelGGL((g_gains_ff<FORM>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, io.blob, traj, io.weights, io.gain_u,
                       io.gain_t, io.summary, io.jac, io.jac_u, io.ff_dir, io.ff_know, io.ff_u, io.ff_t, io.jac_nav);
  else
    hipLaunchKernelGGL((g_gains<FORM>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, io.blob, traj, io.weights, io.gain_u,
                       io.gain_t, io.summary, io.jac, io.jac_u);
}

int gains_run(const Call &c, int substeps, const GainsIO &io, double *ws) {
  const FlightWs w = flight_ws(ws, c.K, c.batch);
  if (const int rc = flight_fly_only(c, substeps, io.blob, w.traj, w.fsum)) return rc;
  if (c.form == 1) gains_launch<1>(c, substeps, io, w.traj);
  else gains_launch<0>(c, substeps, io, w.traj);
  ASC_CHK(c.err, c.errlen, hipGetLastError());
  return ASCENT_OK;
}

}  // namespace ascent
