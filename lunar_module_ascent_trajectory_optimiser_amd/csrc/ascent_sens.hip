// Post-optimal sensitivity of the optimal objective to the problem parameters (include/ascent.h: ascent_param_sensitivity).
//
// Envelope theorem: at a KKT point (v*, lambda*, z*) of the scaled NLP the gradient of the optimal objective is the partial
// derivative of the Lagrangian with respect to the parameter, the iterate held fixed.  In the blob's sign convention
//     L = J + lambda'c + nu3 e3 + nu1 (g1 - s1) + nu2 (g2 - s2) - zL'(v - lb) - zU'(ub - v)
// so  dJ*/dp = dJ/dp + lambda' dc/dp + nu' d(terminal)/dp + zL' d lb/dp - zU' d ub/dp.  The kernels see the parameters only
// through struct Der (ascent_device.hpp: derive_t), so the per-step work differentiates the defects and terminal conditions
// with respect to the Der constants; an epilogue applies the chain rule d Der / d p back to the 16 fields of ascent_params.
//
// Defect of step k (za = z_{k-1}, zb = z_k, dt = h T tf, control held over the step):  c = zb - za - Phi(za, zb, u, dt; Der)
//   scheme 0  Phi = dt f(zb)
//   scheme 1  Phi = dt/2 (f(za) + f(zb))
//   scheme 2  Phi = dt/6 (f(za) + 4 f(zm) + f(zb)),  zm = (za + zb)/2 + dt/8 (f(za) - f(zb))
// For scheme 2, with mu = f_z(zm)' lambda:
//   lambda' dPhi/dDer = dt/6 [(lambda + dt/2 mu)' f_Der(za) + 4 lambda' f_Der(zm) + (lambda - dt/2 mu)' f_Der(zb)]
//   lambda' dPhi/d dt = 1/6 lambda'(f(za) + 4 f(zm) + f(zb)) + dt/12 mu'(f(za) - f(zb))
// and d dt / d T_scale = h tf (T is a parameter of every defect).  Formulation 1's algebraic angle row
// angle_k - (angle_ub/2)(u_k + 1) contributes -lambda_angle (u_k + 1)/2 to d/d angle_ub.
//
// Mapping: a workgroup of SB threads covers PB consecutive problems (PB a power of two: 64 for large batches, down to 16 so
// that the grid has some hundreds of workgroups, down to 1 for a single NLP); thread t takes problem t % PB and the t / PB-th
// contiguous segment of the steps.  Problem-fastest rows make every load of a group of PB lanes one contiguous run of 8*PB
// bytes.  Each thread accumulates d L / d Der over its segment (the next step's rows are loaded before the current one is
// evaluated); lanes of one problem are summed with cross-lane shuffles, the waves of the workgroup in LDS, in a fixed order
// (results depend on the batch size only through PB, never on timing).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>

#include "ascent.h"
#include "ascent_device.hpp"
#include "ascent_sens.hpp"

namespace ascent {
namespace {

constexpr int SB = 256;                    // threads per workgroup
constexpr int NWV = SB / 64;               // waves per workgroup
// d L / d Der accumulators (D_PEN: sum_k |u_k - u_{k-1}|, the objective's derivative with respect to its weight)
enum { D_RHO0, D_RHOF, D_VP2, D_GAM, D_THR, D_ALPHA, D_MRATE, D_MS, D_M0, D_T, D_AUB, D_TLB, D_TUB, D_HT, D_ET, D_PEN, NACC };

// acc += s * w' (d f / d Der) at (z, u)
template <int FORM>
ASC_DEV void add_fder(const Der &d, const double *z, double u, const double *w, double s, double *acc) {
  double dax[ACC_NDER], day[ACC_NDER];
  accel_dder(d, z[IX], z[IY], z[IA], z[IM], dax, day);
  const double wx = s * w[IVX], wy = s * w[IVY];
  acc[D_RHO0] += wx * dax[ACC_RHO0] + wy * day[ACC_RHO0];
  acc[D_GAM] += wx * dax[ACC_GAM] + wy * day[ACC_GAM];
  acc[D_THR] += wx * dax[ACC_THR] + wy * day[ACC_THR];
  acc[D_M0] += wx * dax[ACC_M0] + wy * day[ACC_M0];
  acc[D_MS] += wx * dax[ACC_MS] + wy * day[ACC_MS];
  if (FORM == 0) acc[D_ALPHA] += s * w[IW] * u;
  acc[D_MRATE] += s * w[IM];
}

template <int FORM>
ASC_DEV void fval(const Der &d, const double *z, double u, double *F) {
  double ax, ay;
  accel<0>(d, z[IX], z[IY], z[IA], z[IM], 0.0, 0.0, ax, ay, nullptr, nullptr);
  rhs_f<FORM>(d, z, u, ax, ay, F);
}

ASC_DEV double dot7(const double *a, const double *b) {
  double s = 0.0;
  ASC_UNROLL
  for (int i = 0; i < 7; i++) s += a[i] * b[i];
  return s;
}

// the rows of one step that the kernel reads: z_k, u_k, lambda_k, zU_angle of node k
struct StepRows { double z[7], u, l[7], zu; };
ASC_DEV void load_step(const double *__restrict__ b, size_t B, int K, int k, StepRows &s) {
  ASC_UNROLL
  for (int i = 0; i < 7; i++) s.z[i] = b[(size_t)(7 * k + i) * B];
  s.u = b[(size_t)(7 * K + k) * B];
  ASC_UNROLL
  for (int i = 0; i < 7; i++) s.l[i] = b[(size_t)(8 * K + 7 * k + i) * B];
  s.zu = b[(size_t)(15 * K + 6 * k + 1) * B];
}

// d L / d Der of one step's defect: acc gets -lambda' dPhi/dDer, acc[D_T] -h tf lambda' dPhi/d dt
template <int SCHEME, int FORM>
ASC_DEV void step_terms(const Der &d, double dt, double htf, const double *za, const StepRows &s, double *acc) {
  double fa[7], fb[7];
  fval<FORM>(d, s.z, s.u, fb);
  if constexpr (SCHEME == 0) {
    add_fder<FORM>(d, s.z, s.u, s.l, -dt, acc);
    acc[D_T] -= htf * dot7(s.l, fb);
  } else if constexpr (SCHEME == 1) {
    fval<FORM>(d, za, s.u, fa);
    add_fder<FORM>(d, za, s.u, s.l, -0.5 * dt, acc);
    add_fder<FORM>(d, s.z, s.u, s.l, -0.5 * dt, acc);
    double fs[7];
    ASC_UNROLL
    for (int i = 0; i < 7; i++) fs[i] = fa[i] + fb[i];
    acc[D_T] -= htf * 0.5 * dot7(s.l, fs);
  } else {
    fval<FORM>(d, za, s.u, fa);
    const double e8 = 0.125 * dt;
    double zm[7], fm[7], Gm[8], ax, ay;
    ASC_UNROLL
    for (int i = 0; i < 7; i++) zm[i] = 0.5 * (za[i] + s.z[i]) + e8 * (fa[i] - fb[i]);
    accel<1>(d, zm[IX], zm[IY], zm[IA], zm[IM], 0.0, 0.0, ax, ay, Gm, nullptr);
    rhs_f<FORM>(d, zm, s.u, ax, ay, fm);
    double mu[7], wa[7], wb[7], fs[7], fdf[7];
    fzt_lambda<FORM>(Gm, s.l, mu);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) {
      wa[i] = s.l[i] + 0.5 * dt * mu[i];
      wb[i] = s.l[i] - 0.5 * dt * mu[i];
      fs[i] = fa[i] + 4.0 * fm[i] + fb[i];
      fdf[i] = fa[i] - fb[i];
    }
    const double c6 = -dt * (1.0 / 6.0);
    add_fder<FORM>(d, za, s.u, wa, c6, acc);
    add_fder<FORM>(d, zm, s.u, s.l, 4.0 * c6, acc);
    add_fder<FORM>(d, s.z, s.u, wb, c6, acc);
    acc[D_T] -= htf * ((1.0 / 6.0) * dot7(s.l, fs) + dt * (1.0 / 12.0) * dot7(mu, fdf));
  }
  if (FORM == 1) acc[D_AUB] -= 0.5 * s.l[IA] * (s.u + 1.0);
}

// chain rule d Der / d p: grad[16] (ascent_params field order) from the reduced accumulators
ASC_DEV void chain_rule(const ascent_params &p, const double *D, int terminal, int form, int mp, double *g) {
  const double S = p.r_peri, GM = p.G * p.M, R0 = p.R0;
  const double gam = GM / (S * S * S), thr = p.Ft / S, mrate = p.mdot / p.fuel_mass;
  double gGM = D[D_GAM] / (S * S * S);
  double gR0 = (D[D_RHO0] + D[D_RHOF]) / S;
  double gS = -(D[D_RHO0] + D[D_RHOF]) * R0 / (S * S) - 3.0 * D[D_GAM] * gam / S - D[D_THR] * thr / S;
  double gRa = 0.0;
  const double rp = R0 + S, ra = R0 + p.r_apo;
  if (terminal == 0) {          // vp2 = GM / ((R0 + (S + r_apo)/2) S^2)
    const double Q = R0 + 0.5 * (S + p.r_apo), vp2 = GM / (Q * S * S);
    gGM += D[D_VP2] / (Q * S * S);
    gR0 -= D[D_VP2] * vp2 / Q;
    gRa -= D[D_VP2] * 0.5 * vp2 / Q;
    gS -= D[D_VP2] * (0.5 * vp2 / Q + 2.0 * vp2 / S);
  } else if (terminal == 1) {   // vp2 = GM (2/rp - 2/(rp + ra)) / S^2
    const double V = 2.0 / rp - 2.0 / (rp + ra), S2 = S * S;
    const double dVrp = -2.0 / (rp * rp) + 2.0 / ((rp + ra) * (rp + ra)), dVra = 2.0 / ((rp + ra) * (rp + ra));
    gGM += D[D_VP2] * V / S2;
    gR0 += D[D_VP2] * GM / S2 * (dVrp + dVra);
    gRa += D[D_VP2] * GM / S2 * dVra;
    gS += D[D_VP2] * (GM / S2 * dVrp - 2.0 * GM * V / (S2 * S));
  } else {                      // ht = sqrt(2 GM rp ra / (rp + ra)) / S^2,  Et = -GM / (S^2 (rp + ra))
    const double ht = sqrt(2.0 * GM * rp * ra / (rp + ra)) / (S * S), Et = -GM / (S * S * (rp + ra));
    const double hrp = 0.5 * ht * (1.0 / rp - 1.0 / (rp + ra)), hra = 0.5 * ht * (1.0 / ra - 1.0 / (rp + ra));
    const double erp = -Et / (rp + ra);
    gGM += D[D_HT] * ht / (2.0 * GM) + D[D_ET] * Et / GM;
    gR0 += D[D_HT] * (hrp + hra) + D[D_ET] * 2.0 * erp;
    gRa += D[D_HT] * hra + D[D_ET] * erp;
    gS += D[D_HT] * (hrp - 2.0 * ht / S) + D[D_ET] * (erp - 2.0 * Et / S);
  }
  const double pen = mp ? D[D_PEN] : 0.0;
  g[0] = p.M * gGM;                                  // G
  g[1] = p.G * gGM;                                  // M
  g[2] = gR0;                                        // R0
  g[3] = D[D_THR] / S;                               // Ft
  g[4] = D[D_M0];                                    // M0
  g[5] = D[D_MRATE] / p.fuel_mass;                   // mdot
  g[6] = -D[D_MRATE] * mrate / p.fuel_mass;          // fuel_mass
  g[7] = D[D_MS];                                    // mass_scalar
  g[8] = D[D_ALPHA] / 3.0;                           // ang_acc_max
  g[9] = gS;                                         // r_peri
  g[10] = gRa;                                       // r_apo
  g[11] = D[D_T];                                    // T_scale
  g[12] = D[D_AUB] + (form == 1 ? 0.5 * p.dcost * pen : 0.0);   // angle_ub (formulation 1: the penalty weight dcost angle_ub/2)
  g[13] = D[D_TLB];                                  // tf_lb
  g[14] = D[D_TUB];                                  // tf_ub
  g[15] = (form == 1 ? 0.5 * p.angle_ub : 1.0) * pen;   // dcost
}

template <int SCHEME, int FORM>
__global__ __launch_bounds__(SB) void s_sens(const ascent_params *__restrict__ P, long batch, int K, int pb, int terminal, int mp,
                                             const double *__restrict__ blob, double *__restrict__ grad) {
  __shared__ double red[NACC][NWV][64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int seg = t / pb, nseg = SB / pb;
  const long p = (long)blockIdx.x * pb + (t & (pb - 1));
  const bool on = p < batch;
  double acc[NACC];
  ASC_UNROLL
  for (int a = 0; a < NACC; a++) acc[a] = 0.0;
  if (on) {
    const size_t B = (size_t)batch;
    const double *b = blob + p;
    const Der d = derive_t(P[p], terminal);
    const double tf = b[(size_t)(21 * K + S_TH) * B];
    const double htf = tf / K, dt = htf * d.T;
    const int k0 = (int)((long)seg * K / nseg), k1 = (int)((long)(seg + 1) * K / nseg);
    double za[7], uprev = FORM == 1 ? -1.0 : 0.0;        // node 0: the initial conditions, all zero; u_{-1}: the MV's initial value
    ASC_UNROLL
    for (int i = 0; i < 7; i++) za[i] = k0 ? b[(size_t)(7 * (k0 - 1) + i) * B] : 0.0;
    if (k0) uprev = b[(size_t)(7 * K + k0 - 1) * B];
    if (k0 < k1) {
      StepRows cur, nxt;
      load_step(b, B, K, k0, cur);
      for (int k = k0; k < k1; k++) {
        load_step(b, B, K, k + 1 < k1 ? k + 1 : k, nxt);
        step_terms<SCHEME, FORM>(d, dt, htf, za, cur, acc);
        acc[D_AUB] -= cur.zu;
        acc[D_PEN] += fabs(cur.u - uprev);
        ASC_UNROLL
        for (int i = 0; i < 7; i++) za[i] = cur.z[i];
        uprev = cur.u;
        cur = nxt;
      }
      if (k1 == K) {      // terminal conditions at z_K (= za now)
        const double nu3 = b[(size_t)(21 * K + S_NU3) * B], nu1 = b[(size_t)(21 * K + S_NU1) * B], nu2 = b[(size_t)(21 * K + S_NU2) * B];
        const double et = za[IY] + d.rho0, r2 = za[IX] * za[IX] + et * et, rho = sqrt(r2);
        if (terminal == 2) {      // g1 = x ydot - (y+rho0) xdot - ht,  g2 = Et - |v|^2/2 + gam/rho
          acc[D_RHO0] += -nu1 * za[IVX] - nu2 * d.gam * et / (r2 * rho);
          acc[D_HT] -= nu1;
          acc[D_ET] += nu2;
          acc[D_GAM] += nu2 / rho;
        } else {                  // e3 = (y+rho0) ydot + x xdot,  g1 = rho - rhof,  g2 = |v|^2 - vp2
          acc[D_RHO0] += nu3 * za[IVY] + nu1 * et / rho;
          acc[D_RHOF] -= nu1;
          acc[D_VP2] -= nu2;
        }
      }
    }
    if (seg == 0) {       // tf bounds
      acc[D_TLB] += b[(size_t)(21 * K + S_ZLT) * B];
      acc[D_TUB] -= b[(size_t)(21 * K + S_ZUT) * B];
    }
  }
  // the lanes of one problem in a wave (lane = j + PB * i), then the waves, in a fixed order
  ASC_UNROLL
  for (int a = 0; a < NACC; a++)
    for (int off = 32; off >= pb; off >>= 1) acc[a] += __shfl_xor(acc[a], off);
  if (lane < pb) {
    ASC_UNROLL
    for (int a = 0; a < NACC; a++) red[a][wv][lane] = acc[a];
  }
  __syncthreads();
  if (t < pb && on) {
    double D[NACC], g[16];
    ASC_UNROLL
    for (int a = 0; a < NACC; a++) {
      double s = red[a][0][t];
      for (int w = 1; w < NWV; w++) s += red[a][w][t];
      D[a] = s;
    }
    chain_rule(P[p], D, terminal, FORM, mp, g);
    ASC_UNROLL
    for (int i = 0; i < 16; i++) grad[(size_t)i * batch + p] = g[i];
  }
}

}  // namespace

int sens_problems_per_group(long batch) {
  int pb = 64;
  while (pb > 16 && (batch + pb - 1) / pb < 512) pb >>= 1;
  while (pb > 1 && pb / 2 >= batch) pb >>= 1;
  return pb;
}

int sens_run(const Call &c, int terminal, const double *dblob, double *dgrad) {
  const ascent_params *dp = c.dp;
  const long batch = c.batch;
  const int K = c.K, scheme = c.scheme, formulation = c.form, move_penalty = c.mp;
  hipStream_t stream = c.stream;
  const int pb = sens_problems_per_group(batch);
  const dim3 grid((unsigned)((batch + pb - 1) / pb)), block(SB);
  if (scheme == 0 && formulation == 1)
    hipLaunchKernelGGL((s_sens<0, 1>), grid, block, 0, stream, dp, batch, K, pb, terminal, move_penalty, dblob, dgrad);
  else if (scheme == 0)
    hipLaunchKernelGGL((s_sens<0, 0>), grid, block, 0, stream, dp, batch, K, pb, terminal, move_penalty, dblob, dgrad);
  else if (scheme == 1)
    hipLaunchKernelGGL((s_sens<1, 0>), grid, block, 0, stream, dp, batch, K, pb, terminal, move_penalty, dblob, dgrad);
  else
    hipLaunchKernelGGL((s_sens<2, 0>), grid, block, 0, stream, dp, batch, K, pb, terminal, move_penalty, dblob, dgrad);
  ASC_CHK(c.err, c.errlen, hipGetLastError());
  return ASCENT_OK;
}

}  // namespace ascent
