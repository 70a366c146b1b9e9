// Fused one-lane-per-NLP kernels of the batched ascent NLP solver (gfx950), behind the host interface of
// ascent_fused.hpp: one lane = one NLP for the whole interior-point loop, HBM tiles of step records.
// (The C ABI in ascent_solver.hip routes a solve here only under an environment override)
//
// Kernel structure (one lane = one NLP, one 64-lane wavefront = one workgroup = one "tile" of 64 NLPs):
//   k_solve       the whole interior-point loop; per iteration
//                   pass B   evaluate defects/Jacobian/Hessian blocks of every collocation step and
//                            factorise the bordered block-tridiagonal KKT system backwards in time
//                   pass F   forward substitution: primal step, fraction-to-boundary, merit slope
//                   pass A   adjoint substitution: multiplier step, bound-multiplier steps
//                   pass T   merit function at trial points (backtracking line search)
//                   pass UE  accept the step and evaluate the KKT error of the new iterate (fused)
//   k_eval_nodes  per-(step, problem) defects + Jacobian + Hessian blocks (parity surface)
//   k_kkt_step    one Newton step at a caller-supplied iterate (parity surface)
//
// Workspace layout in HBM: [tile][step k][field][64 lanes] doubles.  A pass streams the step
// records of its tile in time order (forwards or backwards); every access of a wavefront is one
// contiguous 512-byte row whose address is a wave-uniform base plus the lane, so loads use scalar
// base registers.  Each pass is written as  prefetch(next step) / compute(current step) / store,  so
// the HBM latency of step k-1 is hidden behind the arithmetic of step k (there is one wavefront per
// SIMD at these register counts, so there is no other wavefront to switch to).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "ascent.h"
#include "ascent_device.hpp"
#include "ascent_tile.hpp"
#include "ascent_fused.hpp"

using namespace ascent;

namespace {

// rows of one step record
constexpr int R_Z = 0, R_U = 7, R_L = 8, R_ZB = 15;          // iterate: z[7] u lambda[7] zb[6]
constexpr int R_DZ = 21, R_DU = 28, R_DL = 29, R_DZB = 36;   // step:    same order
constexpr int R_G = 42, R_E = 50, R_H = 54, R_F = 64, R_C = 71, R_KA = 78, R_K0 = 85, R_ID = 88;
constexpr int R_STAGE = 94;

__host__ __device__ inline size_t tile_doubles(int K) { return (size_t)K * R_STAGE * WAVE; }

struct W {  // one lane's view of its tile
  gdbl *tile;  // wave-uniform base of this wavefront's tile
  int K;
  double h;
  Der d;
};
using Tile = TileT<R_STAGE>;

// ---------------------------------------------------------------------------------------------
// pass UE: (optionally) accept the step  it += alpha*step  and evaluate the KKT error pieces of the
// resulting iterate, backwards in time.  `s` holds the already-updated scalars.
// ---------------------------------------------------------------------------------------------
struct InUE {
  double zp[7], dzp[7], l[7], dl[7], zb[6], dzb[6], u, du;
};
template <bool UPDATE>
ASC_DEV void loadUE(const Tile &t_, int k, InUE &in) {
  const gdbl *sp = t_.st(k);
  ldn<7>(t_, sp, R_L, in.l);
  ldn<6>(t_, sp, R_ZB, in.zb);
  in.u = ROW(sp, R_U);
  if (UPDATE) {
    ldn<7>(t_, sp, R_DL, in.dl);
    ldn<6>(t_, sp, R_DZB, in.dzb);
    in.du = ROW(sp, R_DU);
  }
  if (k > 0) {
    const gdbl *spp = t_.st(k - 1);
    ldn<7>(t_, spp, R_Z, in.zp);
    if (UPDATE) ldn<7>(t_, spp, R_DZ, in.dzp);
  } else {
    ASC_UNROLL
    for (int i = 0; i < 7; i++) { in.zp[i] = 0.0; in.dzp[i] = 0.0; }
  }
}

template <bool UPDATE>
ASC_PASS ErrParts pass_update_error(const W &w, const Scal &s, double alpha, double adu, double mu) {
  const Der &d = w.d;
  const Tile t_(w.tile);
  const int K = uniform(w.K);
  const double hT = w.h * d.T, dt = hT * s.th;
  double rd = 0.0, cinf = 0.0, pmin = 1e300, pmax = -1e300, l1 = 0.0, zsum = 0.0, rth = 1.0;
  double z[7], ln[7];
  {
    gdbl *sp = t_.st(K - 1);
    ldn<7>(t_, sp, R_Z, z);
    if (UPDATE) {
      double dz[7];
      ldn<7>(t_, sp, R_DZ, dz);
      ASC_UNROLL
      for (int i = 0; i < 7; i++) z[i] += alpha * dz[i];
      stn<7>(t_, sp, R_Z, z);
    }
  }
  ASC_UNROLL
  for (int i = 0; i < 7; i++) ln[i] = 0.0;
  const double mlo = mu * 1e-10, mhi = mu * 1e10;
  auto body = [&](InUE &cur, int k) __attribute__((always_inline)) {
    gdbl *sp = t_.st(k);
    if (UPDATE) {
      ASC_UNROLL
      for (int i = 0; i < 7; i++) { cur.zp[i] += alpha * cur.dzp[i]; cur.l[i] += alpha * cur.dl[i]; }
      cur.u += alpha * cur.du;
      const double dist[6] = {z[IA], d.aub - z[IA], z[IM], 1.0 - z[IM], cur.u + 1.0, 1.0 - cur.u};
      ASC_UNROLL
      for (int b = 0; b < 6; b++) {   // keep z within [mu/(k d), k mu/d], k = 1e10
        const double id = rcp(dist[b]);
        cur.zb[b] = fmin(fmax(cur.zb[b] + adu * cur.dzb[b], mlo * id), mhi * id);
      }
      if (k > 0) stn<7>(t_, t_.st(k - 1), R_Z, cur.zp);
      stn<7>(t_, sp, R_L, cur.l);
      stn<6>(t_, sp, R_ZB, cur.zb);
      ROW(sp, R_U) = cur.u;
    }
    double G[8], F[7], fl[7], r[7], ax, ay;
    accel<1>(d, z[IX], z[IY], z[IA], z[IM], 0.0, 0.0, ax, ay, G, nullptr);
    rhs_f(d, z, cur.u, ax, ay, F);
    fzt_lambda(G, cur.l, fl);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) {
      r[i] = cur.l[i] - dt * fl[i] - ln[i];
      rth -= hT * F[i] * cur.l[i];
      l1 += fabs(cur.l[i]);
      cinf = fmax(cinf, fabs(z[i] - cur.zp[i] - dt * F[i]));
    }
    r[IA] += cur.zb[1] - cur.zb[0];
    r[IM] += cur.zb[3] - cur.zb[2];
    if (k == K - 1) {
      const Terminal t = terminal_eval(d, z);
      r[IX] += s.nu3 * t.e3g[0] + s.nu1 * t.g1g[0];
      r[IY] += s.nu3 * t.e3g[1] + s.nu1 * t.g1g[1];
      r[IVX] += s.nu3 * t.e3g[2] + s.nu2 * t.g2g[0];
      r[IVY] += s.nu3 * t.e3g[3] + s.nu2 * t.g2g[1];
      cinf = fmax(cinf, fmax(fabs(t.e3), fmax(fabs(t.g1 - s.s1), fabs(t.g2 - s.s2))));
    }
    ASC_UNROLL
    for (int i = 0; i < 7; i++) rd = fmax(rd, fabs(r[i]));
    rd = fmax(rd, fabs(-dt * d.alpha * cur.l[IW] - cur.zb[4] + cur.zb[5]));
    const double lo[3] = {z[IA], z[IM], cur.u + 1.0}, up[3] = {d.aub - z[IA], 1.0 - z[IM], 1.0 - cur.u};
    ASC_UNROLL
    for (int b = 0; b < 3; b++) {
      const double p1 = lo[b] * cur.zb[2 * b], p2 = up[b] * cur.zb[2 * b + 1];
      pmin = fmin(pmin, fmin(p1, p2));
      pmax = fmax(pmax, fmax(p1, p2));
      zsum += cur.zb[2 * b] + cur.zb[2 * b + 1];
    }
    cpy<7>(ln, cur.l);
    cpy<7>(z, cur.zp);
  };
#define LD_(k_, buf_) loadUE<UPDATE>(t_, k_, buf_)
  ASC_SWEEP_BACKWARD(InUE, LD_, body)
#undef LD_
  rd = fmax(rd, fabs(rth - s.zlt + s.zut));
  rd = fmax(rd, fmax(fabs(-s.nu1 - s.zs1), fabs(-s.nu2 - s.zs2)));
  const double pr[4] = {(s.th - d.tlb) * s.zlt, (d.tub - s.th) * s.zut, s.s1 * s.zs1, s.s2 * s.zs2};
  ASC_UNROLL
  for (int j = 0; j < 4; j++) { pmin = fmin(pmin, pr[j]); pmax = fmax(pmax, pr[j]); }
  l1 += fabs(s.nu3) + fabs(s.nu1) + fabs(s.nu2);
  zsum += s.zlt + s.zut + s.zs1 + s.zs2;
  ErrParts e;
  e.rd = rd; e.cinf = cinf; e.pmin = pmin; e.pmax = pmax;
  e.sd = fmax(100.0, (l1 + zsum) / (double)(13 * K + 7)) * 0.01;
  return e;
}

// ---------------------------------------------------------------------------------------------
// pass B: evaluate + backward factorisation.  Returns 0, or 1 when the inertia is wrong.
// ---------------------------------------------------------------------------------------------
struct BorderOut {
  double dth, dnu3, c1, sig1, sig2, rs1, rs2;
};
struct InB {
  double zp[7], l[7], zb[6], u;
};
ASC_DEV void loadB(const Tile &t_, int k, InB &in) {
  const gdbl *sp = t_.st(k);
  ldn<7>(t_, sp, R_L, in.l);
  ldn<6>(t_, sp, R_ZB, in.zb);
  in.u = ROW(sp, R_U);
  if (k > 0) {
    ldn<7>(t_, t_.st(k - 1), R_Z, in.zp);
  } else {
    ASC_UNROLL
    for (int i = 0; i < 7; i++) in.zp[i] = 0.0;
  }
}

ASC_PASS int pass_backward(const W &w, const Scal &s, double mu, double dw, BorderOut &out) {
  const Der &d = w.d;
  const Tile t_(w.tile);
  const int K = uniform(w.K);
  const double hT = w.h * d.T, dt = hT * s.th, be = dt * d.alpha;
  double P[28], p0[7], p1[7], p2[7];
  ASC_UNROLL
  for (int i = 0; i < 28; i++) P[i] = 0.0;
  ASC_UNROLL
  for (int i = 0; i < 7; i++) { p0[i] = p1[i] = p2[i] = 0.0; }
  double S10 = 0.0, S11 = 0.0, S12 = 0.0, S20 = 0.0, S22 = 0.0, rth = 1.0;
  double z[7], ln[7];
  ldn<7>(t_, t_.st(K - 1), R_Z, z);
  ASC_UNROLL
  for (int i = 0; i < 7; i++) ln[i] = 0.0;
  const Terminal tm = terminal_eval(d, z);
  const double is1 = rcp(s.s1), is2 = rcp(s.s2);
  const double sig1 = s.zs1 * is1 + dw, sig2 = s.zs2 * is2 + dw;
  const double rs1 = -mu * is1 - s.nu1, rs2 = -mu * is2 - s.nu2;
  const double cg1 = tm.g1 - s.s1, cg2 = tm.g2 - s.s2;
  double c1 = fabs(tm.e3) + fabs(cg1) + fabs(cg2);
  int bad = 0;
  auto body = [&](InB &cur, int k) __attribute__((always_inline)) {
    gdbl *sp = t_.st(k);
    double G[8], E[4], H[10], F[7], fl[7], ax, ay;
    accel<2>(d, z[IX], z[IY], z[IA], z[IM], -dt * cur.l[IVX], -dt * cur.l[IVY], ax, ay, G, H);
    rhs_f(d, z, cur.u, ax, ay, F);
    implicit_block(G, dt, E);
    fzt_lambda(G, cur.l, fl);
    double rz[7], gt[7], cc[7];
    ASC_UNROLL
    for (int i = 0; i < 7; i++) {
      rz[i] = cur.l[i] - dt * fl[i] - ln[i];
      gt[i] = -hT * fl[i];
      cc[i] = z[i] - cur.zp[i] - dt * F[i];
      c1 += fabs(cc[i]);
      rth -= hT * F[i] * cur.l[i];
    }
    // reciprocal distances to the bounds of angle, mass, u (reused by passes F and A)
    const double a = z[IA], m = z[IM], u = cur.u;
    const double id[6] = {rcp(a), rcp(d.aub - a), rcp(m), rcp(1.0 - m), rcp(u + 1.0), rcp(1.0 - u)};
    stn<6>(t_, sp, R_ID, id);
    rz[IA] += mu * (id[1] - id[0]);
    rz[IM] += mu * (id[3] - id[2]);
    const double ru = -be * cur.l[IW] + mu * (id[5] - id[4]);
    const double gu = -hT * d.alpha * cur.l[IW];
    const double R = cur.zb[4] * id[4] + cur.zb[5] * id[5] + dw;
    const double qa = cur.zb[0] * id[0] + cur.zb[1] * id[1], qm = cur.zb[2] * id[2] + cur.zb[3] * id[3];
    // N = Q_k + P_{k+1}, built in place in P
    P[sid(IX, IX)] += H[0]; P[sid(IX, IY)] += H[1]; P[sid(IX, IA)] += H[2]; P[sid(IX, IM)] += H[3];
    P[sid(IY, IY)] += H[4]; P[sid(IY, IA)] += H[5]; P[sid(IY, IM)] += H[6];
    P[sid(IA, IA)] += H[7] + qa; P[sid(IA, IM)] += H[8]; P[sid(IM, IM)] += H[9] + qm;
    ASC_UNROLL
    for (int i = 0; i < 7; i++) P[sid(i, i)] += dw;
    if (k == K - 1) {
      terminal_hessian(P, tm, s.nu3, s.nu1, s.nu2, sig1, sig2);
      const double w1 = s.nu1 + sig1 * cg1 + rs1, w2 = s.nu2 + sig2 * cg2 + rs2;
      rz[IX] += s.nu3 * tm.e3g[0] + w1 * tm.g1g[0];
      rz[IY] += s.nu3 * tm.e3g[1] + w1 * tm.g1g[1];
      rz[IVX] += s.nu3 * tm.e3g[2] + w2 * tm.g2g[0];
      rz[IVY] += s.nu3 * tm.e3g[3] + w2 * tm.g2g[1];
    }
    stn<8>(t_, sp, R_G, G);
    stn<4>(t_, sp, R_E, E);
    stn<10>(t_, sp, R_H, H);
    stn<7>(t_, sp, R_F, F);
    stn<7>(t_, sp, R_C, cc);
    // M = A^-T N A^-1 (in place), pivot, gain, P_k
    congruence(P, G, E, dt);
    const double D = R + be * be * P[sid(IW, IW)];
    if (!(D > 0.0)) bad = 1;
    const double iD = rcp(D);
    double mw[7], kap[7];
    ASC_UNROLL
    for (int i = 0; i < 7; i++) { mw[i] = be * P[sid(i, IW)]; kap[i] = mw[i] * iD; }
    ASC_UNROLL
    for (int i = 0; i < 7; i++) {
      ASC_UNROLL
      for (int j = i; j < 7; j++) P[sid(i, j)] -= mw[i] * kap[j];
    }
    stn<7>(t_, sp, R_KA, kap);
    // three right-hand sides (0: residual, 1: -B_theta, 2: -B_nu3)
    double n[7], nt[7], q0[7], q1[7], rc1[7], Prc[7], k00, k01, k02;
    ASC_UNROLL
    for (int i = 0; i < 7; i++) n[i] = -rz[i] + p0[i];
    solveAT(G, E, dt, n, nt);
    k00 = (be * nt[IW] - ru) * iD;
    ASC_UNROLL
    for (int i = 0; i < 7; i++) { q0[i] = nt[i] - mw[i] * k00; n[i] = -cc[i]; }
    symv(P, n, Prc);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) p0[i] = q0[i] - Prc[i];
    ASC_UNROLL
    for (int i = 0; i < 7; i++) n[i] = -gt[i] + p1[i];
    solveAT(G, E, dt, n, nt);
    k01 = (be * nt[IW] - gu) * iD;
    ASC_UNROLL
    for (int i = 0; i < 7; i++) { q1[i] = nt[i] - mw[i] * k01; rc1[i] = hT * F[i]; }
    symv(P, rc1, Prc);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) p1[i] = q1[i] - Prc[i];
    cpy<7>(n, p2);
    if (k == K - 1) { n[IX] -= tm.e3g[0]; n[IY] -= tm.e3g[1]; n[IVX] -= tm.e3g[2]; n[IVY] -= tm.e3g[3]; }
    solveAT(G, E, dt, n, nt);
    k02 = be * nt[IW] * iD;
    ASC_UNROLL
    for (int i = 0; i < 7; i++) p2[i] = nt[i] - mw[i] * k02;   // q2 = p2 (no defect part)
    ROW(sp, R_K0) = k00; ROW(sp, R_K0 + 1) = k01; ROW(sp, R_K0 + 2) = k02;
    // Schur-complement entries S_ij = rho_i' K0^-1 rho_j accumulated step by step
    double a10 = D * k01 * k00, a11 = D * k01 * k01, a12 = D * k01 * k02, a20 = D * k02 * k00;
    ASC_UNROLL
    for (int i = 0; i < 7; i++) {
      a10 += 0.5 * (rc1[i] * (q0[i] + p0[i]) - cc[i] * (q1[i] + p1[i]));
      a11 += rc1[i] * (q1[i] + p1[i]);
      a12 += rc1[i] * p2[i];
      a20 -= cc[i] * p2[i];
    }
    S10 += a10; S11 += a11; S12 += a12; S20 += a20; S22 += D * k02 * k02;
    cpy<7>(ln, cur.l);
    cpy<7>(z, cur.zp);
  };
#define LD_(k_, buf_) loadB(t_, k_, buf_)
  ASC_SWEEP_BACKWARD(InB, LD_, body)
#undef LD_
  if (bad) return 1;
  const double itl = rcp(s.th - d.tlb), itu = rcp(d.tub - s.th);
  rth += mu * (itu - itl);
  const double sth = s.zlt * itl + s.zut * itu + dw;
  const double a11 = sth - S11, a12 = -S12, a22 = -S22;
  const double b1 = -rth + S10, b2 = -tm.e3 + S20;
  const double det = a11 * a22 - a12 * a12;
  if (!(det < 0.0)) return 1;
  const double idet = 1.0 / det;
  out.dth = (b1 * a22 - a12 * b2) * idet;
  out.dnu3 = (a11 * b2 - a12 * b1) * idet;
  out.c1 = c1; out.sig1 = sig1; out.sig2 = sig2; out.rs1 = rs1; out.rs2 = rs2;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// pass F: forward substitution (primal step), primal fraction-to-boundary, barrier slope and the
// barrier sum at the current iterate
// ---------------------------------------------------------------------------------------------
struct InF {
  double G[8], E[4], cc[7], F[7], ka[7], k0[3], id[6], a, m, u;
};
ASC_DEV void loadF(const Tile &t_, int k, InF &in) {
  const gdbl *sp = t_.st(k);
  ldn<8>(t_, sp, R_G, in.G);
  ldn<4>(t_, sp, R_E, in.E);
  ldn<7>(t_, sp, R_C, in.cc);
  ldn<7>(t_, sp, R_F, in.F);
  ldn<7>(t_, sp, R_KA, in.ka);
  ldn<3>(t_, sp, R_K0, in.k0);
  ldn<6>(t_, sp, R_ID, in.id);
  in.a = ROW(sp, R_Z + IA);
  in.m = ROW(sp, R_Z + IM);
  in.u = ROW(sp, R_U);
}

ASC_PASS void pass_forward(const W &w, const Scal &s, double mu, double tau, double dth, double dnu3,
                           double &apr, double &gd, double &slog, double *dzK) {
  const Der &d = w.d;
  const Tile t_(w.tile);
  const int K = uniform(w.K);
  const double hT = w.h * d.T, dt = hT * s.th, be = dt * d.alpha;
  double dzp[7];
  ASC_UNROLL
  for (int i = 0; i < 7; i++) dzp[i] = 0.0;
  double rmax = 0.0, gsum = 0.0, lsum = 0.0;   // max of -dx/dist over all bounds; barrier slope / mu; sum of logs
  auto body = [&](InF &cur, int k) __attribute__((always_inline)) {
    gdbl *sp = t_.st(k);
    double xi[7], dz[7];
    double du = cur.k0[0] + cur.k0[1] * dth + cur.k0[2] * dnu3;
    ASC_UNROLL
    for (int i = 0; i < 7; i++) {
      xi[i] = dzp[i] - cur.cc[i] + hT * cur.F[i] * dth;
      du -= cur.ka[i] * xi[i];
    }
    xi[IW] += be * du;
    solveA(cur.G, cur.E, dt, xi, dz);
    stn<7>(t_, sp, R_DZ, dz);
    ROW(sp, R_DU) = du;
    cpy<7>(dzp, dz);
    const double *id = cur.id;
    ASC_FTBR(rmax, id[0], dz[IA]); ASC_FTBR(rmax, id[1], -dz[IA]);
    ASC_FTBR(rmax, id[2], dz[IM]); ASC_FTBR(rmax, id[3], -dz[IM]);
    ASC_FTBR(rmax, id[4], du); ASC_FTBR(rmax, id[5], -du);
    gsum += dz[IA] * (id[1] - id[0]) + dz[IM] * (id[3] - id[2]) + du * (id[5] - id[4]);
    const double a = cur.a, m = cur.m, u = cur.u;
    lsum += log((a * (d.aub - a)) * (m * (1.0 - m)) * ((u + 1.0) * (1.0 - u)));
  };
#define LD_(k_, buf_) loadF(t_, k_, buf_)
  ASC_SWEEP_FORWARD(InF, LD_, body)
#undef LD_
  if (rmax * apr > tau) apr = tau / rmax;
  gd += mu * gsum;
  slog += lsum;
  cpy<7>(dzK, dzp);
}

// ---------------------------------------------------------------------------------------------
// pass A: adjoint substitution (multiplier step), bound-multiplier steps, dual fraction-to-boundary,
// and c'(lambda + dlambda) for the curvature estimate
// ---------------------------------------------------------------------------------------------
struct InA {
  double G[8], E[4], H[10], dz[7], l[7], zb[6], cc[7], id[6], du;
};
ASC_DEV void loadA(const Tile &t_, int k, InA &in) {
  const gdbl *sp = t_.st(k);
  ldn<8>(t_, sp, R_G, in.G);
  ldn<4>(t_, sp, R_E, in.E);
  ldn<10>(t_, sp, R_H, in.H);
  ldn<7>(t_, sp, R_DZ, in.dz);
  ldn<7>(t_, sp, R_L, in.l);
  ldn<6>(t_, sp, R_ZB, in.zb);
  ldn<7>(t_, sp, R_C, in.cc);
  ldn<6>(t_, sp, R_ID, in.id);
  in.du = ROW(sp, R_DU);
}

ASC_PASS void pass_adjoint(const W &w, const Scal &s, double mu, double dw, double tau, double dth,
                           double dnu3, double sig1, double sig2, double rs1, double rs2, double &adu,
                           double &cl) {
  const Der &d = w.d;
  const Tile t_(w.tile);
  const int K = uniform(w.K);
  const double hT = w.h * d.T, dt = hT * s.th;
  double dln[7], ln[7];
  ASC_UNROLL
  for (int i = 0; i < 7; i++) { dln[i] = 0.0; ln[i] = 0.0; }
  auto body = [&](InA &cur, int k) __attribute__((always_inline)) {
    gdbl *sp = t_.st(k);
    const double *H = cur.H, *dz = cur.dz, *id = cur.id;
    const double du = cur.du;
    const double qa = cur.zb[0] * id[0] + cur.zb[1] * id[1], qm = cur.zb[2] * id[2] + cur.zb[3] * id[3];
    double fl[7], r[7], dl[7];
    fzt_lambda(cur.G, cur.l, fl);
    // r = -(rz + gt*dtheta) + dlambda_{k+1} - Q dz, with rz = l - dt*fl - l_{k+1} + barrier gradient
    ASC_UNROLL
    for (int i = 0; i < 7; i++)
      r[i] = -(cur.l[i] - dt * fl[i] - ln[i]) + hT * fl[i] * dth + dln[i] - dw * dz[i];
    r[IA] -= mu * (id[1] - id[0]);
    r[IM] -= mu * (id[3] - id[2]);
    r[IX] -= H[0] * dz[IX] + H[1] * dz[IY] + H[2] * dz[IA] + H[3] * dz[IM];
    r[IY] -= H[1] * dz[IX] + H[4] * dz[IY] + H[5] * dz[IA] + H[6] * dz[IM];
    r[IA] -= H[2] * dz[IX] + H[5] * dz[IY] + (H[7] + qa) * dz[IA] + H[8] * dz[IM];
    r[IM] -= H[3] * dz[IX] + H[6] * dz[IY] + H[8] * dz[IA] + (H[9] + qm) * dz[IM];
    if (k == K - 1) {
      double zK[7], QT[28], qd[7];
      ldn<7>(t_, sp, R_Z, zK);
      const Terminal tm = terminal_eval(d, zK);
      ASC_UNROLL
      for (int i = 0; i < 28; i++) QT[i] = 0.0;
      terminal_hessian(QT, tm, s.nu3, s.nu1, s.nu2, sig1, sig2);
      symv(QT, dz, qd);
      ASC_UNROLL
      for (int i = 0; i < 7; i++) r[i] -= qd[i];
      const double w1 = s.nu1 + sig1 * (tm.g1 - s.s1) + rs1, w2 = s.nu2 + sig2 * (tm.g2 - s.s2) + rs2;
      r[IX] -= s.nu3 * tm.e3g[0] + w1 * tm.g1g[0] + tm.e3g[0] * dnu3;
      r[IY] -= s.nu3 * tm.e3g[1] + w1 * tm.g1g[1] + tm.e3g[1] * dnu3;
      r[IVX] -= s.nu3 * tm.e3g[2] + w2 * tm.g2g[0] + tm.e3g[2] * dnu3;
      r[IVY] -= s.nu3 * tm.e3g[3] + w2 * tm.g2g[1] + tm.e3g[3] * dnu3;
    }
    solveAT(cur.G, cur.E, dt, r, dl);
    stn<7>(t_, sp, R_DL, dl);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) cl += cur.cc[i] * (cur.l[i] + dl[i]);
    // bound multipliers: dz_L = mu/d - z_L - z_L/d*dx,  dz_U = mu/d - z_U + z_U/d*dx
    const double dx[3] = {dz[IA], dz[IM], du};
    double dzb[6];
    ASC_UNROLL
    for (int b = 0; b < 3; b++) {
      const double zl = cur.zb[2 * b], zu = cur.zb[2 * b + 1];
      dzb[2 * b] = id[2 * b] * (mu - zl * dx[b]) - zl;
      dzb[2 * b + 1] = id[2 * b + 1] * (mu + zu * dx[b]) - zu;
      ASC_FTB(adu, zl, dzb[2 * b]);
      ASC_FTB(adu, zu, dzb[2 * b + 1]);
    }
    stn<6>(t_, sp, R_DZB, dzb);
    cpy<7>(dln, dl);
    cpy<7>(ln, cur.l);
  };
#define LD_(k_, buf_) loadA(t_, k_, buf_)
  ASC_SWEEP_BACKWARD(InA, LD_, body)
#undef LD_
}

// ---------------------------------------------------------------------------------------------
// pass T: l1 merit function at the trial point iterate + alpha*step
// ---------------------------------------------------------------------------------------------
struct InT {
  double z[7], dz[7], u, du;
};
ASC_DEV void loadT(const Tile &t_, int k, InT &in) {
  const gdbl *sp = t_.st(k);
  ldn<7>(t_, sp, R_Z, in.z);
  ldn<7>(t_, sp, R_DZ, in.dz);
  in.u = ROW(sp, R_U);
  in.du = ROW(sp, R_DU);
}

ASC_PASS double pass_trial(const W &w, const Scal &s, const Scal &ds, double alpha, double mu, double nu_pen) {
  const Der &d = w.d;
  const Tile t_(w.tile);
  const int K = uniform(w.K);
  const double th = s.th + alpha * ds.th, s1 = s.s1 + alpha * ds.s1, s2 = s.s2 + alpha * ds.s2;
  const double dt = w.h * d.T * th;
  double sl = log(((th - d.tlb) * (d.tub - th)) * (s1 * s2));
  double c1 = 0.0, zp[7], z[7];
  ASC_UNROLL
  for (int i = 0; i < 7; i++) { zp[i] = 0.0; z[i] = 0.0; }
  auto body = [&](InT &cur, int k) __attribute__((always_inline)) {
    (void)k;
    double F[7], ax, ay;
    ASC_UNROLL
    for (int i = 0; i < 7; i++) z[i] = cur.z[i] + alpha * cur.dz[i];
    const double u = cur.u + alpha * cur.du;
    accel<0>(d, z[IX], z[IY], z[IA], z[IM], 0.0, 0.0, ax, ay, nullptr, nullptr);
    rhs_f(d, z, u, ax, ay, F);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) { c1 += fabs(z[i] - zp[i] - dt * F[i]); zp[i] = z[i]; }
    // a negative factor (trial point outside a bound) gives NaN or a wrong sign pair; the fraction-to-
    // boundary rule keeps every factor positive, and a NaN merit value is rejected by the line search
    const double pa = z[IA] * (d.aub - z[IA]), pm = z[IM] * (1.0 - z[IM]), pu = (u + 1.0) * (1.0 - u);
    sl += (pa > 0.0 && pm > 0.0 && pu > 0.0) ? log(pa * pm * pu) : NAN;
  };
#define LD_(k_, buf_) loadT(t_, k_, buf_)
  ASC_SWEEP_FORWARD(InT, LD_, body)
#undef LD_
  const Terminal tm = terminal_eval(d, z);
  c1 += fabs(tm.e3) + fabs(tm.g1 - s1) + fabs(tm.g2 - s2);
  return th - mu * sl + nu_pen * c1;
}

// ---------------------------------------------------------------------------------------------
// initial point
// ---------------------------------------------------------------------------------------------
// cold start: straight-line states toward a tangential insertion point, u = 0
ASC_DEV void cold_guess(const W &w, Scal &s) {
  const Der &d = w.d;
  const Tile t_(w.tile);
  const int K = uniform(w.K);
  const double tf0 = 0.9, dr = 0.166, aend = 0.5, vp = sqrt(d.vp2), dt = w.h * d.T * tf0;
  const double sdr = sin(dr), cdr = cos(dr);
  const double xf = -d.rhof * sdr, yf = d.rhof * cdr - d.rho0;
  for (int k = 0; k < K; k++) {
    const double fr = (double)(k + 1) / K;
    gdbl *sp = t_.st(k);
    const double z[7] = {fr * xf, fr * yf, -fr * vp * cdr, -fr * vp * sdr, fr * aend, aend / (K * dt),
                         d.mrate * dt * (k + 1)};
    stn<7>(t_, sp, R_Z, z);
    ROW(sp, R_U) = 0.0;
  }
  s.th = tf0;
}

// interior point + multipliers. mode 0/1: primal only (multipliers reset); 2: keep multipliers
ASC_DEV void init_point(const W &w, Scal &s, int mode) {
  const Der &d = w.d;
  const Tile t_(w.tile);
  const int K = uniform(w.K);
  for (int k = 0; k < K; k++) {
    gdbl *sp = t_.st(k);
    ROW(sp, R_Z + IA) = push_in(ROW(sp, R_Z + IA), 0.0, d.aub);
    ROW(sp, R_Z + IM) = push_in(ROW(sp, R_Z + IM), 0.0, 1.0);
    ROW(sp, R_U) = push_in(ROW(sp, R_U), -1.0, 1.0);
    if (mode != 2) {
      ASC_UNROLL
      for (int b = 0; b < 6; b++) ROW(sp, R_ZB + b) = 1.0;
      ASC_UNROLL
      for (int i = 0; i < 7; i++) ROW(sp, R_L + i) = 0.0;
    } else {
      ASC_UNROLL
      for (int b = 0; b < 6; b++) ROW(sp, R_ZB + b) = fmax(ROW(sp, R_ZB + b), 1e-12);
    }
  }
  s.th = push_in(s.th, d.tlb, d.tub);
  double zK[7];
  ldn<7>(t_, t_.st(K - 1), R_Z, zK);
  const Terminal tm = terminal_eval(d, zK);
  if (mode != 2) {
    s.s1 = fmax(tm.g1, 1e-2); s.s2 = fmax(tm.g2, 1e-2);
    s.zlt = s.zut = s.zs1 = s.zs2 = 1.0;
    s.nu3 = s.nu1 = s.nu2 = 0.0;
  } else {
    s.s1 = fmax(s.s1, 1e-10); s.s2 = fmax(s.s2, 1e-10);
    s.zlt = fmax(s.zlt, 1e-12); s.zut = fmax(s.zut, 1e-12);
    s.zs1 = fmax(s.zs1, 1e-12); s.zs2 = fmax(s.zs2, 1e-12);
  }
}

// Newton step at the current iterate: passes B, F, A.  Returns 0 / 1 (wrong inertia).
struct StepInfo { double apr, adu, gd, cl, c1, slog; };

ASC_DEV int newton_step(const W &w, const Scal &s, double mu, double dw, Scal &ds, StepInfo &si) {
  BorderOut bo;
  if (pass_backward(w, s, mu, dw, bo)) return 1;
  const Der &d = w.d;
  const double tau = fmax(0.99, 1.0 - mu);
  double apr = 1.0, adu = 1.0, gd = 0.0, cl = 0.0, slog = 0.0, dzK[7];
  pass_forward(w, s, mu, tau, bo.dth, bo.dnu3, apr, gd, slog, dzK);
  pass_adjoint(w, s, mu, dw, tau, bo.dth, bo.dnu3, bo.sig1, bo.sig2, bo.rs1, bo.rs2, adu, cl);
  double zK[7];
  const Tile t_(w.tile);
  ldn<7>(t_, t_.st(w.K - 1), R_Z, zK);
  const Terminal tm = terminal_eval(d, zK);
  ds.th = bo.dth; ds.nu3 = bo.dnu3;
  ds.s1 = (tm.g1 - s.s1) + tm.g1g[0] * dzK[IX] + tm.g1g[1] * dzK[IY];
  ds.s2 = (tm.g2 - s.s2) + tm.g2g[0] * dzK[IVX] + tm.g2g[1] * dzK[IVY];
  ds.nu1 = bo.sig1 * ds.s1 + bo.rs1;
  ds.nu2 = bo.sig2 * ds.s2 + bo.rs2;
  ds.zs1 = mu / s.s1 - s.zs1 - s.zs1 / s.s1 * ds.s1;
  ds.zs2 = mu / s.s2 - s.zs2 - s.zs2 / s.s2 * ds.s2;
  const double dl = s.th - d.tlb, dU = d.tub - s.th;
  ds.zlt = mu / dl - s.zlt - s.zlt / dl * ds.th;
  ds.zut = mu / dU - s.zut + s.zut / dU * ds.th;
  ASC_FTB(apr, dl, ds.th); ASC_FTB(apr, dU, -ds.th);
  ASC_FTB(apr, s.s1, ds.s1); ASC_FTB(apr, s.s2, ds.s2);
  ASC_FTB(adu, s.zlt, ds.zlt); ASC_FTB(adu, s.zut, ds.zut);
  ASC_FTB(adu, s.zs1, ds.zs1); ASC_FTB(adu, s.zs2, ds.zs2);
  gd += ds.th * (1.0 - mu / dl + mu / dU) - mu * ds.s1 / s.s1 - mu * ds.s2 / s.s2;
  cl += tm.e3 * (s.nu3 + ds.nu3) + (tm.g1 - s.s1) * (s.nu1 + ds.nu1) + (tm.g2 - s.s2) * (s.nu2 + ds.nu2);
  slog += log((dl * dU) * (s.s1 * s.s2));
  si.apr = apr; si.adu = adu; si.gd = gd; si.cl = cl; si.c1 = bo.c1; si.slog = slog;
  return 0;
}

ASC_DEV W make_w(double *ws, int K, const ascent_params &prm) {
  W w;
  w.tile = (gdbl *)ws + (size_t)blockIdx.x * tile_doubles(K);
  w.K = K;
  w.h = 1.0 / K;
  w.d = derive(prm);
  return w;
}

// external blob rows ([row][batch], include/ascent.h) <-> step records
ASC_DEV void blob_to_tile(const W &w, const double *blob, long batch, long p, int r_z, int r_u, int r_l,
                          int r_zb, Scal &s) {
  const Tile t_(w.tile);
  const int K = uniform(w.K);
  for (int k = 0; k < K; k++) {
    gdbl *sp = t_.st(k);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) {
      ROW(sp, r_z + i) = blob[(7L * k + i) * batch + p];
      ROW(sp, r_l + i) = blob[(8L * K + 7L * k + i) * batch + p];
    }
    ROW(sp, r_u) = blob[(7L * K + k) * batch + p];
    ASC_UNROLL
    for (int b = 0; b < 6; b++) ROW(sp, r_zb + b) = blob[(15L * K + 6L * k + b) * batch + p];
  }
  const double *sc = blob + (21L * K) * batch + p;
  s.th = sc[S_TH * batch]; s.zlt = sc[S_ZLT * batch]; s.zut = sc[S_ZUT * batch];
  s.s1 = sc[S_S1 * batch]; s.s2 = sc[S_S2 * batch]; s.zs1 = sc[S_ZS1 * batch]; s.zs2 = sc[S_ZS2 * batch];
  s.nu3 = sc[S_NU3 * batch]; s.nu1 = sc[S_NU1 * batch]; s.nu2 = sc[S_NU2 * batch];
}

ASC_DEV void tile_to_blob(const W &w, double *blob, long batch, long p, int r_z, int r_u, int r_l, int r_zb,
                          const Scal &s) {
  const Tile t_(w.tile);
  const int K = uniform(w.K);
  for (int k = 0; k < K; k++) {
    const gdbl *sp = t_.st(k);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) {
      blob[(7L * k + i) * batch + p] = ROW(sp, r_z + i);
      blob[(8L * K + 7L * k + i) * batch + p] = ROW(sp, r_l + i);
    }
    blob[(7L * K + k) * batch + p] = ROW(sp, r_u);
    ASC_UNROLL
    for (int b = 0; b < 6; b++) blob[(15L * K + 6L * k + b) * batch + p] = ROW(sp, r_zb + b);
  }
  double *sc = blob + (21L * K) * batch + p;
  sc[S_TH * batch] = s.th; sc[S_ZLT * batch] = s.zlt; sc[S_ZUT * batch] = s.zut;
  sc[S_S1 * batch] = s.s1; sc[S_S2 * batch] = s.s2; sc[S_ZS1 * batch] = s.zs1; sc[S_ZS2 * batch] = s.zs2;
  sc[S_NU3 * batch] = s.nu3; sc[S_NU1 * batch] = s.nu1; sc[S_NU2 * batch] = s.nu2;
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
#ifdef ASCENT_PROFILE   // diagnostic build only (scripts/pass_profile.py): shader cycles per pass
__device__ unsigned long long g_prof[8];
#define PROF_T0 long long t0_ = clock64();
#define PROF_ADD(i) do { long long t1_ = clock64(); prof[i] += t1_ - t0_; t0_ = t1_; } while (0)
#else
#define PROF_T0
#define PROF_ADD(i) do { } while (0)
#endif

__global__ __launch_bounds__(WAVE) void k_solve(const ascent_params *params, long batch, int K, double *ws,
                                                const double *guess, int warm, int max_iter, double tol,
                                                double mu_init, double *traj, double *tf_out, int *status_out,
                                                int *iters_out, double *blob_out) {
  const long p = (long)blockIdx.x * WAVE + threadIdx.x;
  if (p >= batch) return;
  const W w = make_w(ws, K, params[p]);
  Scal s;
  // a guess whose theta is not positive means "no guess for this problem" (nested iteration: the coarse solve failed)
  const int asked_warm = warm;
  if (warm && !(guess[(21L * K + S_TH) * batch + p] > 0.0)) warm = 0;
  if (warm) {
    blob_to_tile(w, guess, batch, p, R_Z, R_U, R_L, R_ZB, s);
  } else {
    cold_guess(w, s);
  }
  init_point(w, s, warm);
  double mu = (asked_warm && !warm) ? 0.1 : mu_init, nu_pen = 1.0, dw_last = 0.0;
  int status = ASCENT_MAX_ITER, iters = 0;
#ifdef ASCENT_PROFILE
  long long prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  PROF_T0
  ErrParts e = pass_update_error<false>(w, s, 0.0, 0.0, mu);
  PROF_ADD(0);
  for (int iter = 0; iter < max_iter; iter++) {
    if (e.err(0.0) <= tol) { status = ASCENT_CONVERGED; break; }
    while (mu > tol * 0.1 && e.err(mu) <= 10.0 * mu) {
      mu = fmax(tol * 0.1, fmin(0.2 * mu, mu * sqrt(mu)));
      nu_pen = 1.0;
    }
    double dw = 0.0;
    Scal ds;
    StepInfo si;
    bool fail = false;
    while (newton_step(w, s, mu, dw, ds, si)) {
      dw = next_delta_w(dw, dw_last);
      if (dw > 1e10) { fail = true; break; }
    }
    if (fail) { status = ASCENT_REGULARISATION_FAILED; break; }
    dw_last = dw;
    PROF_ADD(1);
    const double curv = -si.gd + si.cl;
    if (si.c1 > 0.0) {
      const double need = (si.gd + 0.5 * fmax(curv, 0.0)) / (0.9 * si.c1);
      if (nu_pen < need) nu_pen = need + 1.0;
    }
    const double Dm = si.gd - nu_pen * si.c1;
    const double phi0 = s.th - mu * si.slog + nu_pen * si.c1;
    double alpha = si.apr;
    bool ok = false;
    for (int ls = 0; ls < 40; ls++) {
      const double phit = pass_trial(w, s, ds, alpha, mu, nu_pen);
      if (isfinite(phit) && phit <= phi0 + 1e-8 * alpha * Dm + 2.220446049250313e-15 * fabs(phi0)) { ok = true; break; }
      alpha *= 0.5;
    }
    if (!ok) { status = ASCENT_LINESEARCH_FAILED; break; }
    PROF_ADD(3);
    s.th += alpha * ds.th; s.s1 += alpha * ds.s1; s.s2 += alpha * ds.s2;
    s.nu3 += alpha * ds.nu3; s.nu1 += alpha * ds.nu1; s.nu2 += alpha * ds.nu2;
    s.zlt = clipz(s.zlt + si.adu * ds.zlt, s.th - w.d.tlb, mu);
    s.zut = clipz(s.zut + si.adu * ds.zut, w.d.tub - s.th, mu);
    s.zs1 = clipz(s.zs1 + si.adu * ds.zs1, s.s1, mu);
    s.zs2 = clipz(s.zs2 + si.adu * ds.zs2, s.s2, mu);
    e = pass_update_error<true>(w, s, alpha, si.adu, mu);
    iters = iter + 1;
    PROF_ADD(4);
  }
  if (status == ASCENT_MAX_ITER && e.err(0.0) <= tol) status = ASCENT_CONVERGED;
#ifdef ASCENT_PROFILE
  if (threadIdx.x == 0)
    for (int i = 0; i < 8; i++) atomicAdd(&g_prof[i], (unsigned long long)prof[i]);
#endif
  tf_out[p] = s.th;
  status_out[p] = status;
  iters_out[p] = iters;
  if (blob_out) tile_to_blob(w, blob_out, batch, p, R_Z, R_U, R_L, R_ZB, s);
  if (traj) {
    const Tile t_(w.tile);
    const int nt = K + 1;
    for (int k = 0; k < nt; k++) {
      double z[7], u = 0.0, ax, ay;
      if (k) {
        ldn<7>(t_, t_.st(k - 1), R_Z, z);
        u = ROW(t_.st(k - 1), R_U);
      } else {
        ASC_UNROLL
        for (int i = 0; i < 7; i++) z[i] = 0.0;
      }
      accel<0>(w.d, z[IX], z[IY], z[IA], z[IM], 0.0, 0.0, ax, ay, nullptr, nullptr);
      const double v[10] = {z[IX], z[IY], z[IVX], z[IVY], ax, ay, z[IA], z[IW], u, z[IM]};
      ASC_UNROLL
      for (int f = 0; f < 10; f++) traj[((long)f * nt + k) * batch + p] = v[f];
    }
  }
}

// thread = (problem, step): defects, Jacobian and Hessian blocks of one collocation step
__global__ __launch_bounds__(256) void k_eval_nodes(const ascent_params *params, long batch, int K,
                                                    const double *it, double *defects, double *jac,
                                                    double *hess) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  if (p >= batch) return;
  const Der d = derive(params[p]);
  const double th = it[(21L * K + S_TH) * batch + p];
  const double dt = (1.0 / K) * d.T * th;
  double z[7], zp[7], G[8], H[10], F[7], ax, ay;
  ASC_UNROLL
  for (int i = 0; i < 7; i++) {
    z[i] = it[(7L * k + i) * batch + p];
    zp[i] = k ? it[(7L * (k - 1) + i) * batch + p] : 0.0;
  }
  const double u = it[(7L * K + k) * batch + p];
  const double lvx = it[(8L * K + 7L * k + IVX) * batch + p], lvy = it[(8L * K + 7L * k + IVY) * batch + p];
  accel<2>(d, z[IX], z[IY], z[IA], z[IM], -dt * lvx, -dt * lvy, ax, ay, G, H);
  rhs_f(d, z, u, ax, ay, F);
  ASC_UNROLL
  for (int i = 0; i < 7; i++) defects[(7L * k + i) * batch + p] = z[i] - zp[i] - dt * F[i];
  ASC_UNROLL
  for (int i = 0; i < 8; i++) jac[(8L * k + i) * batch + p] = G[i];
  ASC_UNROLL
  for (int i = 0; i < 10; i++) hess[(10L * k + i) * batch + p] = H[i];
}

__global__ __launch_bounds__(WAVE) void k_kkt_step(const ascent_params *params, long batch, int K, double *ws,
                                                   const double *it, const double *mu, const double *dw,
                                                   double *step, int *inertia) {
  const long p = (long)blockIdx.x * WAVE + threadIdx.x;
  if (p >= batch) return;
  const W w = make_w(ws, K, params[p]);
  Scal s, ds;
  blob_to_tile(w, it, batch, p, R_Z, R_U, R_L, R_ZB, s);
  StepInfo si;
  const int rc = newton_step(w, s, mu[p], dw[p], ds, si);
  inertia[p] = rc;
  if (rc == 0) tile_to_blob(w, step, batch, p, R_DZ, R_DU, R_DL, R_DZB, ds);
}

}  // namespace

namespace ascent {

static int launched(const Call &c) {      // ASCENT_OK, or ASCENT_E_HIP when the launch just made was refused
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return ASCENT_OK;
  snprintf(c.err, c.errlen, "fused kernel launch: %s", hipGetErrorString(e));
  return ASCENT_E_HIP;
}

size_t fused_ws_bytes(int K, long batch) { return (size_t)((batch + WAVE - 1) / WAVE) * tile_doubles(K) * sizeof(double); }

int fused_run(const Call &c, double *ws, const SolveIO &io) {
  hipLaunchKernelGGL(k_solve, dim3((unsigned)((c.batch + WAVE - 1) / WAVE)), dim3(WAVE), 0, c.stream, c.dp, c.batch, c.K, ws, io.guess, io.warm,
                     io.max_iter, io.tol, io.mu0, io.traj, io.tf, io.status, io.iters, io.blob);
  return launched(c);
}

int fused_probe(const Call &c, double *ws, const ProbeIO &io) {
  hipLaunchKernelGGL(k_kkt_step, dim3((unsigned)((c.batch + WAVE - 1) / WAVE)), dim3(WAVE), 0, c.stream, c.dp, c.batch, c.K, ws, io.iterate, io.mu,
                     io.dw, io.step, io.inertia);
  return launched(c);
}

int fused_eval_nodes(const Call &c, const ProbeIO &io) {
  hipLaunchKernelGGL(k_eval_nodes, dim3((unsigned)((c.batch + 255) / 256), c.K), dim3(256), 0, c.stream, c.dp, c.batch, c.K, io.iterate, io.defects,
                     io.jac, io.hess);
  return launched(c);
}

}  // namespace ascent

#ifdef ASCENT_PROFILE
extern "C" int ascent_debug_profile(unsigned long long *out8, int reset) {
  unsigned long long z[8] = {0};
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_prof), sizeof z) != hipSuccess) return -1;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof z) != hipSuccess) return -1;
  return 0;
}
#endif
