// Monte Carlo dispersion of flown solutions (include/ascent.h: ascent_disperse_batch): one solution blob shared by many
// perturbed flights, reduced on the device to the moments and extrema of the nine end quantities of the flight Jacobian.
//
// The flight of a sample is f_fly's (ascent_flight.hip): K collocation steps of m classical RK4 substeps, the control held over
// a step, with a perturbed initial state, perturbed ascent_params fields (derive per sample), a perturbed t_f and perturbed
// controls.  m is the nominal flight's (flight_substeps at the blob's t_f and the nominal T_scale), held for every sample as
// the Jacobian holds it.  The nominal flight itself is f_fly, unchanged, into the workspace trajectory: its last node and
// its summary rows 2 / 3 are the nominal rows and the centre of the moments.
//
// f_disperse        one lane per (problem, sample); a workgroup of DB = 256 threads is 256 consecutive samples of one problem
//          (workgroup g of the linear grid: problem g / nwg, chunk g % nwg, nwg = ceil(samples / 256); below 193 samples the
//          workgroup is only the one to three wavefronts that hold samples).  The lanes of a
//          wavefront share the problem, so the blob's u_k, sigma and the parameters are wave-uniform loads, and xi[24 + k][s]
//          is one contiguous 512-byte run per wave and step, loaded for the next step before the current one is integrated.
//          Latency-bound like f_fly: 4 m K dependent right-hand sides per lane.  The 73 values of a record (count, 9 sums and 45
//          products of the differences from the centre, 9 minima, 9 maxima) are reduced one at a time -- butterfly over the
//          wave, wave 0..3 through LDS in that order -- into one partial record per workgroup.
// f_disperse_stats  one lane per problem, problem-fastest: the partial records added in ascending chunk order, then the 82 rows.
// f_disperse_guided f_disperse under state feedback (ascent_disperse_guided_batch): same mapping, same record, same reduction.
// f_disperse_navigated  f_disperse_guided with the feed-forward f_k theta-hat and the navigation errors of
//          ascent_disperse_navigated_batch: one body with f_disperse_guided (guided_body<FORM, NAV>).
// f_disperse<FORM, true> / f_history_guided  f_disperse / f_disperse_navigated with the per-node history of
//          ascent_disperse_history_batch (HIST, an `if constexpr` in the two step loops): at a history node every lane holds its ten
//          quantities, and the 42 values of the node's record are reduced like the end record -- one barrier per history node.
// f_history_drifting    f_history_guided with the eight knowledge errors as first-order Gauss-Markov sequences
//          (ascent_disperse_drifting_batch; guided_body<FORM, 2, true>): per step eight more draws, loaded with the next step's gains.
// f_history_stats   one lane per (problem, node): the node's partial records added in ascending chunk order, then the 52 rows.
// The kernels share their head (sample_lane, perturbed_sample) and their tail (end_rows, reduce_partial); only the step loops
// differ.  One host function, disperse_run, launches whichever kernel the call's kind names.
// The order of every addition is fixed by `samples` alone: a problem gives the same bits alone as inside any batch.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>

#include "ascent.h"
#include "ascent_device.hpp"
#include "ascent_disperse.hpp"
#include "ascent_flight.hpp"
#include "ascent_flight_dev.hpp"

namespace ascent {
namespace {

constexpr int DB = 256;                    // f_disperse: threads per workgroup = samples per partial record
constexpr int DNW = DB / 64;
constexpr int SW = 64;                     // f_disperse_stats: threads per workgroup
constexpr int NQ = ASCENT_DISPERSE_ROWS, NC = ASCENT_DISPERSE_COLS;
// a partial record: rows of [nwg][NREC][batch]
constexpr int R_N = 0, R_SUM = 1, R_PROD = R_SUM + NQ, R_MIN = R_PROD + NQ * (NQ + 1) / 2, R_MAX = R_MIN + NQ, NREC = R_MAX + NQ;
// stats_out rows
constexpr int O_N = 0, O_NOM = 1, O_MEAN = O_NOM + NQ, O_COV = O_MEAN + NQ, O_MIN = O_COV + NQ * (NQ + 1) / 2, O_MAX = O_MIN + NQ;
static_assert(O_MAX + NQ == ASCENT_DISPERSE_STAT_ROWS, "stats_out layout");
constexpr long MAX_GRID = 1L << 22;        // workgroups per launch: 2^30 threads
// the history (ascent_disperse_history_batch): a partial record per workgroup and history node, rows of [nwg][NJ][HREC][batch]
constexpr int HQ = ASCENT_HISTORY_QUANTITIES;
constexpr int H_N = 0, H_SUM = 1, H_SQ = H_SUM + HQ, H_MIN = H_SQ + HQ, H_MAX = H_MIN + HQ, H_CLIP = H_MAX + HQ, HREC = H_CLIP + 1;
// hist_out rows
constexpr int HO_N = 0, HO_NOM = 1, HO_MEAN = HO_NOM + HQ, HO_VAR = HO_MEAN + HQ, HO_MIN = HO_VAR + HQ, HO_MAX = HO_MIN + HQ, HO_CLIP = HO_MAX + HQ;
static_assert(HO_CLIP + 1 == ASCENT_HISTORY_ROWS, "hist_out layout");

// butterflies: every lane ends with the same bits (no lane contributes a NaN: invalid samples enter as +-inf)
ASC_DEV double wave_min(double v) {
  ASC_UNROLL
  for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  return v;
}
ASC_DEV double wave_max(double v) {
  ASC_UNROLL
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

// the nominal flight's nine rows from f_fly's trajectory and summary
ASC_DEV void nominal_rows(const double *__restrict__ traj, const double *__restrict__ fsum, size_t B, long p, int K, double *r) {
  load_node(traj + p, B, K + 1, K, r);
  r[7] = fsum[(size_t)2 * B + p];
  r[8] = fsum[(size_t)3 * B + p];
}

// the record of one wavefront into red[]: rows r of a sample, its validity, the centre
ASC_DEV void wave_record(const double *r, bool valid, const double *cen, int lane, double *red) {
#pragma clang fp contract(off)      // a product fused into the first addition of its butterfly would differ between the lanes
  double dq[NQ];
  ASC_UNROLL
  for (int q = 0; q < NQ; q++) dq[q] = valid ? r[q] - cen[q] : 0.0;
  double v = wave_sum(valid ? 1.0 : 0.0);
  if (lane == 0) red[R_N] = v;
  ASC_UNROLL
  for (int q = 0; q < NQ; q++) {
    v = wave_sum(dq[q]);
    if (lane == 0) red[R_SUM + q] = v;
  }
  int idx = R_PROD;
  ASC_UNROLL
  for (int i = 0; i < NQ; i++) {
    ASC_UNROLL
    for (int j = i; j < NQ; j++, idx++) {
      const double pr = dq[i] * dq[j];
      v = wave_sum(pr);
      if (lane == 0) red[idx] = v;
    }
  }
  ASC_UNROLL
  for (int q = 0; q < NQ; q++) {
    v = wave_min(valid ? r[q] : INFINITY);
    if (lane == 0) red[R_MIN + q] = v;
    v = wave_max(valid ? r[q] : -INFINITY);
    if (lane == 0) red[R_MAX + q] = v;
  }
}

// Where a lane of the dispersion kernels stands: its problem p, chunk c, sample s, and what every sample of the problem shares --
// the blob column b, the 16 fields pf in declaration order, the blob's t_f and the nominal flight's substeps m, held.
struct Lane {
  long p;
  int c, t, s, m;
  size_t B, NS;
  const double *b, *pf;
  double tf0;
};

// the head of a dispersion kernel, every lane: indexing, the centre of the moments, and the rows of a lane without a sample
ASC_DEV void sample_lane(const ascent_params *__restrict__ P, long batch, int K, int substeps, int samples, int nwg, long g0,
                         const double *__restrict__ blob, const double *__restrict__ traj, const double *__restrict__ fsum,
                         Lane &l, double *cen, double *r) {
  const long g = g0 + blockIdx.x;
  l.p = g / nwg;
  l.c = (int)(g - l.p * nwg);
  l.t = threadIdx.x;
  l.s = l.c * DB + l.t;
  l.B = (size_t)batch; l.NS = (size_t)samples;
  l.b = blob + l.p;
  l.pf = reinterpret_cast<const double *>(P + l.p);      // the 16 fields in declaration order
  l.tf0 = l.b[(size_t)(21 * K + S_TH) * l.B];
  l.m = flight_substeps((l.tf0 * l.pf[11]) / K, substeps);      // the nominal flight's, held
  nominal_rows(traj, fsum, l.B, l.p, K, cen);
  ASC_UNROLL
  for (int q = 0; q < NQ; q++) cen[q] = finite1(cen[q]) ? cen[q] : 0.0;
  ASC_UNROLL
  for (int q = 0; q < NQ; q++) r[q] = NAN;
}

// the head of a lane that has a sample: the 24 sigmas (wave-uniform) and draws, loaded together -- a draw counts only where its
// sigma is not zero --, the perturbed initial state, parameters (derive per sample) and t_f, the step dt and the substep hs
ASC_DEV void perturbed_sample(const Lane &l, int K, const double *__restrict__ xi, const double *__restrict__ sigma, double *sg,
                              double *xv, double *z, ascent_params &prm, Der &d, double &dt, double &hs) {
  const double *x = xi + l.s;
  ASC_UNROLL
  for (int i = 0; i < NC; i++) sg[i] = sigma[(size_t)i * l.B + l.p];
  ASC_UNROLL
  for (int i = 0; i < NC; i++) xv[i] = x[(size_t)i * l.NS];
  double f[16];
  ASC_UNROLL
  for (int i = 0; i < 7; i++) z[i] = sg[i] != 0.0 ? sg[i] * xv[i] : 0.0;
  ASC_UNROLL
  for (int i = 0; i < 16; i++) f[i] = sg[7 + i] != 0.0 ? l.pf[i] + sg[7 + i] * xv[7 + i] : l.pf[i];
  const double tf = sg[23] != 0.0 ? l.tf0 + sg[23] * xv[23] : l.tf0;
  prm = {f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9], f[10], f[11], f[12], f[13], f[14], f[15]};
  d = derive(prm);
  dt = (tf * d.T) / K;
  hs = dt / l.m;
}

// the tail of a lane that has a sample: the nine end rows from the flown state, and the caller's copy of them
ASC_DEV void end_rows(const Lane &l, const ascent_params &prm, const double *z, double *r, double *__restrict__ samples_out) {
  ASC_UNROLL
  for (int i = 0; i < 7; i++) r[i] = z[i];
  apsides_of(prm, z[IX], z[IY], z[IVX], z[IVY], r[7], r[8]);
  if (samples_out) {
    ASC_UNROLL
    for (int q = 0; q < NQ; q++) samples_out[((size_t)q * l.NS + l.s) * l.B + l.p] = r[q];
  }
}

// the tail of a dispersion kernel, every lane: validity, the wavefront's record, and the waves that exist (4, or fewer where
// samples <= 192) reduced in wave order into the workgroup's partial record
ASC_DEV void reduce_partial(const Lane &l, const double *r, const double *cen, double (*red)[NREC], double *__restrict__ partial) {
  bool valid = true;
  ASC_UNROLL
  for (int q = 0; q < NQ; q++) valid = valid && finite1(r[q]);
  wave_record(r, valid, cen, l.t & 63, red[l.t >> 6]);
  __syncthreads();
  const int nw = (int)blockDim.x >> 6;
  for (int i = l.t; i < NREC; i += (int)blockDim.x) {
    double a = red[0][i];
    for (int w = 1; w < nw; w++) {
      const double o = red[w][i];
      a = i < R_MIN ? a + o : i < R_MAX ? fmin(a, o) : fmax(a, o);
    }
    partial[((size_t)l.c * NREC + i) * l.B + l.p] = a;
  }
}

// What a history kernel is given beyond its plain sibling: every stride-th node and the last one, nj of them; the partial
// records and the caller's per-sample rows (or null)
struct HistArgs {
  int stride, nj;
  double *partial, *samples;
};

// altitude above R0 (m) of a scaled position, fields as apsides_of takes them.  Not contracted: f_history_stats and the flights
// compute the nominal one each for itself and must agree in every bit
// The position is taken through an empty asm: apsides_of forms the same products on the last node, and a product the compiler
// found shared with this function would no longer be fused into its addition there -- the end rows would lose the bits of the
// call without the history.
ASC_DEV double altitude_of(double x, double y, double r_peri, double R0) {
#pragma clang fp contract(off)
  asm volatile("" : "+v"(x), "+v"(y));
  const double X = x * r_peri, Y = y * r_peri + R0;
  return sqrt(X * X + Y * Y) - R0;
}

// the nominal flight's ten quantities at node j (1 .. K): f_fly's trajectory with the nominal fields, the blob's u_j, no correction
ASC_DEV void history_nominal(const double *__restrict__ tr, const double *__restrict__ b, const double *__restrict__ pf, size_t B,
                             int K, int j, double *nom) {
  load_node(tr, B, K + 1, j, nom);
  nom[7] = altitude_of(nom[IX], nom[IY], pf[9], pf[2]);
  nom[8] = b[(size_t)(7 * K + j - 1) * B];
  nom[9] = 0.0;
}

// One history node, every lane of the workgroup (a lane without a sample: has = false): the ten quantities h of the lane's
// sample at node j and whether the command of step j was clipped.  The 42 values of the node's record are reduced exactly as
// wave_record and reduce_partial reduce the end rows -- a butterfly per value, then the wavefronts in order -- so that the last
// node's count, sums, squares and extrema of the state are the end statistics' bits.  One barrier per history node: the two
// halves of hred alternate, and the barrier of node i + 1 stands between the reads of node i and the writes of node i + 2.
ASC_DEV void history_node(const Lane &l, bool has, int K, int j, const HistArgs &H, const double *__restrict__ traj, const double *h,
                          bool clip) {
#pragma clang fp contract(off)      // as wave_record: a square fused into the first addition of its butterfly would differ between the lanes
  __shared__ double hred[2][DNW][HREC];
  const int i = (j + H.stride - 1) / H.stride - 1, lane = l.t & 63;
  double cen[HQ];
  history_nominal(traj + l.p, l.b, l.pf, l.B, K, j, cen);
  bool valid = has;
  ASC_UNROLL
  for (int q = 0; q < HQ; q++) {
    cen[q] = finite1(cen[q]) ? cen[q] : 0.0;
    valid = valid && finite1(h[q]);
  }
  if (H.samples && has) {
    ASC_UNROLL
    for (int q = 0; q < HQ; q++) H.samples[(((size_t)q * H.nj + i) * l.NS + l.s) * l.B + l.p] = h[q];
  }
  double *red = hred[i & 1][l.t >> 6];
  double v = wave_sum(valid ? 1.0 : 0.0);
  if (lane == 0) red[H_N] = v;
  ASC_UNROLL
  for (int q = 0; q < HQ; q++) {
    const double dq = valid ? h[q] - cen[q] : 0.0;
    v = wave_sum(dq);
    if (lane == 0) red[H_SUM + q] = v;
    const double sq = dq * dq;
    v = wave_sum(sq);
    if (lane == 0) red[H_SQ + q] = v;
    v = wave_min(valid ? h[q] : INFINITY);
    if (lane == 0) red[H_MIN + q] = v;
    v = wave_max(valid ? h[q] : -INFINITY);
    if (lane == 0) red[H_MAX + q] = v;
  }
  v = wave_sum(valid && clip ? 1.0 : 0.0);
  if (lane == 0) red[H_CLIP] = v;
  __syncthreads();
  if (l.t < HREC) {
    const int nw = (int)blockDim.x >> 6;
    double a = hred[i & 1][0][l.t];
    for (int w = 1; w < nw; w++) {
      const double o = hred[i & 1][w][l.t];
      a = l.t < H_MIN || l.t == H_CLIP ? a + o : l.t < H_MAX ? fmin(a, o) : fmax(a, o);
    }
    H.partial[(((size_t)l.c * H.nj + i) * HREC + l.t) * l.B + l.p] = a;
  }
}

// HIST (include/ascent.h: ascent_disperse_history_batch): after the steps that end at a history node the ten quantities of the
// node are reduced over the workgroup (history_node).  Its barrier needs every wavefront, so a lane without a sample flies the
// last sample again and is left out of every record and output.  samples_out has the twelve rows of the guided calls, the last
// three zero.  HIST = false: no trace of the history in the code (the kernel is a kernel, not a wrapper of a shared body as the
// guided ones are, because the wrapping alone changes the code the compiler emits for it).
template <int FORM, bool HIST>
__global__ __launch_bounds__(DB) void f_disperse(const ascent_params *__restrict__ P, long batch, int K, int substeps, int samples,
                                                 int nwg, long g0, const double *__restrict__ blob,
                                                 const double *__restrict__ traj, const double *__restrict__ fsum,
                                                 const double *__restrict__ xi, const double *__restrict__ sigma,
                                                 const double *__restrict__ sigma_u, double *__restrict__ partial,
                                                 double *__restrict__ samples_out, HistArgs H) {
  __shared__ double red[DNW][NREC];
  Lane l;
  double cen[NQ], r[NQ];
  sample_lane(P, batch, K, substeps, samples, nwg, g0, blob, traj, fsum, l, cen, r);
  const bool has = l.s < samples;
  if constexpr (HIST) {
    if (!has) { l.s = samples - 1; samples_out = nullptr; }
  }
  if (HIST || has) {
    const size_t B = l.B, NS = l.NS;
    const int m = l.m;
    double sg[NC], xv[NC], z[7], dt, hs;
    ascent_params prm;
    Der d;
    perturbed_sample(l, K, xi, sigma, sg, xv, z, prm, d, dt, hs);
    const double *ub = l.b + (size_t)(7 * K) * B, *su = sigma_u ? sigma_u + l.p : nullptr, *xu = xi + l.s + (size_t)NC * NS;
    double u = ub[0];
    if (su) {
      const double s0 = su[0];
      if (s0 != 0.0) u += s0 * xu[0];
    }
    for (int k = 0; k < K; k++) {
      const int kn = k + 1 < K ? k + 1 : k;
      const double un = ub[(size_t)kn * B], sgn = su ? su[(size_t)kn * B] : 0.0, xn = su ? xu[(size_t)kn * NS] : 0.0;
      fly_step<FORM>(d, z, u, hs, m);
      if constexpr (HIST) {
        if ((k + 1) % H.stride == 0 || k + 1 == K) {
          const double h[HQ] = {z[0], z[1], z[2], z[3], z[4], z[5], z[6], altitude_of(z[IX], z[IY], prm.r_peri, prm.R0), u, 0.0};
          history_node(l, has, K, k + 1, H, traj, h, false);
        }
      }
      u = sgn != 0.0 ? un + sgn * xn : un;
    }
    end_rows(l, prm, z, r, samples_out);
    if constexpr (HIST) {
      if (samples_out) {
        ASC_UNROLL
        for (int q = NQ; q < ASCENT_GUIDED_SAMPLE_ROWS; q++) samples_out[((size_t)q * NS + l.s) * B + l.p] = 0.0;
      }
      if (!has) {
        ASC_UNROLL
        for (int q = 0; q < NQ; q++) r[q] = NAN;
      }
    }
  }
  reduce_partial(l, r, cen, red, partial);
}

// f_disperse with the feedback of include/ascent.h: ascent_disperse_guided_batch.  Per step 7 nominal-state and 7 gain doubles
// more, wave-uniform, loaded for the next step with its u before the current one is integrated.  The command of a step whose
// gain row is all zero is u_k itself, and without a stretch hs is f_disperse's: such a flight has f_disperse's bits.  A
// non-finite K.dz makes the command NaN, so the sample is invalid (a clip would hide it).
// NAV (f_disperse_navigated; include/ascent.h: ascent_disperse_navigated_batch): per step one more wave-uniform double, f_k, loaded
// with the next step's gains, and per sample eight more draws loaded once: the navigation bias nu added to dz where its sigma is
// not zero, and theta-hat, what the sample believes its parameter deviation is.  Each addition is skipped where its factor is
// zero, so with nothing new given, or all of it zero, a flight has f_disperse_guided's bits.  NAV = false: f_disperse_guided, the
// new arguments all null and no trace of them in the code.
// HIST (f_history_guided): as in f_disperse; quantity 9 is the correction `dot` of the step, exactly 0 where the step has neither
// gain nor feed-forward, and the clipped flag of the step is the comparison behind nclip.
// NAV = 2 (f_history_drifting; include/ascent.h: ascent_disperse_drifting_batch): the eight knowledge errors are first-order
// Gauss-Markov sequences, n_k = phi n_{k-1} + q omega_{k-1}, n_0 the navigated call's draw; step k steers on n_k.  phi and q are
// wave-uniform and held for the flight; the draws of the next step are loaded with its gains, one 512-byte run per wave and row,
// and only for rows whose q is not zero.  A channel with phi = 1 and q = 0 is frozen: never updated, its draws never read, its
// arithmetic the navigated call's.  A phi outside [0, 1] or a q that is negative or not finite makes every sample of the problem NaN.
struct DriftArgs { const double *phi, *q, *xi; };

template <int FORM, int NAV, bool HIST>
ASC_DEV void guided_body(const ascent_params *__restrict__ P, long batch, int K, int substeps, int samples,
                         int nwg, long g0, const double *__restrict__ blob,
                         const double *__restrict__ traj, const double *__restrict__ fsum,
                         const double *__restrict__ xi, const double *__restrict__ sigma,
                         const double *__restrict__ sigma_u, const double *__restrict__ gain_u,
                         const double *__restrict__ gain_t, const double *__restrict__ stretch_max,
                         const double *__restrict__ ff_u, const double *__restrict__ ff_t, const double *__restrict__ ff_know,
                         const double *__restrict__ xi_nav, const double *__restrict__ sigma_nav,
                         double *__restrict__ partial, double *__restrict__ samples_out, const HistArgs &H,
                         const DriftArgs &G = DriftArgs{}) {
  __shared__ double red[DNW][NREC];
  Lane l;
  double cen[NQ], r[NQ];
  sample_lane(P, batch, K, substeps, samples, nwg, g0, blob, traj, fsum, l, cen, r);
  const bool has = l.s < samples;
  if constexpr (HIST) {
    if (!has) { l.s = samples - 1; samples_out = nullptr; }
  }
  if (HIST || has) {
    const size_t B = l.B, NS = l.NS;
    const long p = l.p;
    const int s = l.s, m = l.m, nt = K + 1;
    double sg[NC], xv[NC], z[7], dt, hs;
    ascent_params prm;
    Der d;
    perturbed_sample(l, K, xi, sigma, sg, xv, z, prm, d, dt, hs);
    const double smax = gain_t && stretch_max ? stretch_max[p] : 0.0;
    const double *ub = l.b + (size_t)(7 * K) * B, *su = sigma_u ? sigma_u + p : nullptr, *xu = xi + s + (size_t)NC * NS;
    const double *tr = traj + p, *gu = gain_u + p;
    double un = ub[0], sgn = su ? su[0] : 0.0, xn = su ? xu[0] : 0.0, zn[7], kn[7];
    load_node(tr, B, nt, 0, zn);
    ASC_UNROLL
    for (int i = 0; i < 7; i++) kn[i] = gu[(size_t)i * K * B];
    // the navigation bias (applied where its sigma is not zero) and theta-hat = w . (applied field deviations) + the knowledge error
    double nu[7], th = 0.0, fn = 0.0;
    [[maybe_unused]] double thw = 0.0;      // NAV = 2: theta-hat without the knowledge error
    bool nav[7];
    if constexpr (NAV) {
      ASC_UNROLL
      for (int i = 0; i < 7; i++) {
        const double sn = sigma_nav ? sigma_nav[(size_t)i * B + p] : 0.0;
        nav[i] = sn != 0.0;
        nu[i] = nav[i] ? sn * xi_nav[(size_t)i * NS + s] : 0.0;
      }
      if (ff_know) {
        // (w sigma) xi, not w (sigma xi): a product sigma xi shared with the field's own perturbation above would keep that one
        // from being fused into its addition, and the sample's parameters would lose f_disperse_guided's bits
        ASC_UNROLL
        for (int i = 0; i < 16; i++) {
          const double ws = ff_know[(size_t)i * B + p] * sg[7 + i];
          th += sg[7 + i] != 0.0 ? ws * xv[7 + i] : 0.0;
        }
      }
      const double s7 = sigma_nav ? sigma_nav[(size_t)7 * B + p] : 0.0;
      if constexpr (NAV == 2) thw = th;
      if (s7 != 0.0) th += s7 * xi_nav[(size_t)7 * NS + s];
      fn = ff_u ? ff_u[p] : 0.0;
    }
    // the drifting channels: nu[0..6] and n7 are the errors the coming step steers on (n_1 before the first step), on[a] the draw
    // behind the step after it.  A frozen channel keeps the values and the theta-hat computed above.
    [[maybe_unused]] double ph[8], qd[8], on[8], n7 = 0.0;
    [[maybe_unused]] bool upd[8];
    [[maybe_unused]] const double *xd = nullptr;
    if constexpr (NAV == 2) {
      bool bad = false;
      xd = G.xi + s;
      ASC_UNROLL
      for (int a = 0; a < 8; a++) {
        ph[a] = G.phi ? G.phi[(size_t)a * B + p] : 1.0;
        qd[a] = G.q ? G.q[(size_t)a * B + p] : 0.0;
        bad = bad || !(ph[a] >= 0.0 && ph[a] <= 1.0) || !(qd[a] >= 0.0 && qd[a] <= 1.7976931348623157e308);
        upd[a] = !(ph[a] == 1.0 && qd[a] == 0.0);
        on[a] = qd[a] != 0.0 ? xd[(size_t)a * K * NS] : 0.0;
      }
      if (upd[7]) {
        // the draw of channel 7 once more, through an empty asm: a product shared with theta-hat's above would keep that one
        // from being fused into its addition, and a frozen channel would lose the navigated call's bits
        const double s7 = sigma_nav ? sigma_nav[(size_t)7 * B + p] : 0.0;
        double x7 = s7 != 0.0 ? xi_nav[(size_t)7 * NS + s] : 0.0;
        asm volatile("" : "+v"(x7));
        n7 = s7 * x7;
      }
      ASC_UNROLL
      for (int a = 0; a < 7; a++) {
        if (upd[a]) nu[a] = qd[a] != 0.0 ? ph[a] * nu[a] + qd[a] * on[a] : ph[a] * nu[a];
        nav[a] = nav[a] || qd[a] != 0.0;
      }
      if (upd[7]) {
        n7 = qd[7] != 0.0 ? ph[7] * n7 + qd[7] * on[7] : ph[7] * n7;
        th = thw + n7;
      }
      if (bad) {
        ASC_UNROLL
        for (int i = 0; i < 7; i++) z[i] = NAN;
      }
    }
    double nclip = 0.0, dmax = 0.0, stretch = 0.0;
    for (int k = 0; k < K; k++) {
      // the command of this step from the state it starts at
      double dz[7], dot = 0.0;
      bool zero = true;
      ASC_UNROLL
      for (int i = 0; i < 7; i++) {
        dz[i] = z[i] - zn[i];
        if constexpr (NAV) dz[i] = nav[i] ? dz[i] + nu[i] : dz[i];
        dot += kn[i] * dz[i];
        zero = zero && kn[i] == 0.0;
      }
      double uc = un;
      [[maybe_unused]] bool clip = false;
      if constexpr (NAV) zero = zero && fn == 0.0;
      if (!zero) {
        double w = un - dot;
        if constexpr (NAV) {
          if (fn != 0.0) {
            const double ft = fn * th;
            w -= ft;
            dot += ft;                        // the whole correction K.dz + f theta-hat
          }
        }
        uc = finite1(dot) ? fmin(1.0, fmax(-1.0, w)) : NAN;
        nclip += uc != w ? 1.0 : 0.0;
        if constexpr (HIST) clip = uc != w;
        dmax = (dot != dot || dmax != dmax) ? NAN : fmax(dmax, fabs(dot));
      }
      const double u = sgn != 0.0 ? uc + sgn * xn : uc;
      double h = hs;
      if (k == K - 1 && smax > 0.0) {
        double dtau = 0.0;
        ASC_UNROLL
        for (int i = 0; i < 7; i++) dtau -= gain_t[(size_t)i * B + p] * dz[i];
        if constexpr (NAV) {
          const double f2 = ff_t ? ff_t[p] : 0.0;
          if (f2 != 0.0) dtau -= f2 * th;
        }
        stretch = finite1(dtau) ? fmin(smax, fmax(-smax, dtau)) : NAN;
        h = (dt * (1.0 + stretch)) / m;
      }
      const int kq = k + 1 < K ? k + 1 : k;
      un = ub[(size_t)kq * B]; sgn = su ? su[(size_t)kq * B] : 0.0; xn = su ? xu[(size_t)kq * NS] : 0.0;
      load_node(tr, B, nt, kq, zn);
      ASC_UNROLL
      for (int i = 0; i < 7; i++) kn[i] = gu[((size_t)i * K + kq) * B];
      if constexpr (NAV) fn = ff_u ? ff_u[(size_t)kq * B + p] : 0.0;
      if constexpr (NAV == 2) {
        ASC_UNROLL
        for (int a = 0; a < 8; a++) on[a] = qd[a] != 0.0 ? xd[((size_t)a * K + kq) * NS] : 0.0;
      }
      fly_step<FORM>(d, z, u, h, m);
      if constexpr (NAV == 2) {      // n_{k+2} for the next step (after the last step: not used)
        ASC_UNROLL
        for (int a = 0; a < 7; a++) {
          if (upd[a]) nu[a] = qd[a] != 0.0 ? ph[a] * nu[a] + qd[a] * on[a] : ph[a] * nu[a];
        }
        if (upd[7]) {
          n7 = qd[7] != 0.0 ? ph[7] * n7 + qd[7] * on[7] : ph[7] * n7;
          th = thw + n7;
        }
      }
      if constexpr (HIST) {
        if ((k + 1) % H.stride == 0 || k + 1 == K) {
          const double hq[HQ] = {z[0], z[1], z[2], z[3], z[4], z[5], z[6], altitude_of(z[IX], z[IY], prm.r_peri, prm.R0), u,
                                 zero ? 0.0 : dot};
          history_node(l, has, K, k + 1, H, traj, hq, clip);
        }
      }
    }
    if constexpr (HIST) {
      ASC_UNROLL
      for (int i = 0; i < 7; i++) asm volatile("" : "+v"(z[i]));
    }
    end_rows(l, prm, z, r, samples_out);
    if (samples_out) {
      samples_out[((size_t)(NQ + 0) * NS + s) * B + p] = nclip;
      samples_out[((size_t)(NQ + 1) * NS + s) * B + p] = dmax;
      samples_out[((size_t)(NQ + 2) * NS + s) * B + p] = stretch;
    }
    if constexpr (HIST) {
      if (!has) {
        ASC_UNROLL
        for (int q = 0; q < NQ; q++) r[q] = NAN;
      }
    }
  }
  reduce_partial(l, r, cen, red, partial);
}

template <int FORM>
__global__ __launch_bounds__(DB) void f_disperse_guided(const ascent_params *__restrict__ P, long batch, int K, int substeps, int samples,
                                                        int nwg, long g0, const double *__restrict__ blob,
                                                        const double *__restrict__ traj, const double *__restrict__ fsum,
                                                        const double *__restrict__ xi, const double *__restrict__ sigma,
                                                        const double *__restrict__ sigma_u, const double *__restrict__ gain_u,
                                                        const double *__restrict__ gain_t, const double *__restrict__ stretch_max,
                                                        double *__restrict__ partial, double *__restrict__ samples_out) {
  guided_body<FORM, false, false>(P, batch, K, substeps, samples, nwg, g0, blob, traj, fsum, xi, sigma, sigma_u, gain_u, gain_t, stretch_max,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, partial, samples_out, HistArgs{});
}

struct NavArgs { const double *ff_u, *ff_t, *ff_know, *xi_nav, *sigma_nav; };

template <int FORM>
__global__ __launch_bounds__(DB) void f_disperse_navigated(const ascent_params *__restrict__ P, long batch, int K, int substeps, int samples,
                                                           int nwg, long g0, const double *__restrict__ blob,
                                                           const double *__restrict__ traj, const double *__restrict__ fsum,
                                                           const double *__restrict__ xi, const double *__restrict__ sigma,
                                                           const double *__restrict__ sigma_u, const double *__restrict__ gain_u,
                                                           const double *__restrict__ gain_t, const double *__restrict__ stretch_max,
                                                           NavArgs nav, double *__restrict__ partial, double *__restrict__ samples_out) {
  guided_body<FORM, true, false>(P, batch, K, substeps, samples, nwg, g0, blob, traj, fsum, xi, sigma, sigma_u, gain_u, gain_t, stretch_max,
                                 nav.ff_u, nav.ff_t, nav.ff_know, nav.xi_nav, nav.sigma_nav, partial, samples_out, HistArgs{});
}

template <int FORM>
__global__ __launch_bounds__(DB) void f_history_guided(const ascent_params *__restrict__ P, long batch, int K, int substeps, int samples,
                                                       int nwg, long g0, const double *__restrict__ blob,
                                                       const double *__restrict__ traj, const double *__restrict__ fsum,
                                                       const double *__restrict__ xi, const double *__restrict__ sigma,
                                                       const double *__restrict__ sigma_u, const double *__restrict__ gain_u,
                                                       const double *__restrict__ gain_t, const double *__restrict__ stretch_max,
                                                       NavArgs nav, double *__restrict__ partial, double *__restrict__ samples_out,
                                                       HistArgs hist) {
  guided_body<FORM, true, true>(P, batch, K, substeps, samples, nwg, g0, blob, traj, fsum, xi, sigma, sigma_u, gain_u, gain_t, stretch_max,
                                nav.ff_u, nav.ff_t, nav.ff_know, nav.xi_nav, nav.sigma_nav, partial, samples_out, hist);
}

template <int FORM>
__global__ __launch_bounds__(DB) void f_history_drifting(const ascent_params *__restrict__ P, long batch, int K, int substeps, int samples,
                                                         int nwg, long g0, const double *__restrict__ blob,
                                                         const double *__restrict__ traj, const double *__restrict__ fsum,
                                                         const double *__restrict__ xi, const double *__restrict__ sigma,
                                                         const double *__restrict__ sigma_u, const double *__restrict__ gain_u,
                                                         const double *__restrict__ gain_t, const double *__restrict__ stretch_max,
                                                         NavArgs nav, DriftArgs drift, double *__restrict__ partial,
                                                         double *__restrict__ samples_out, HistArgs hist) {
  guided_body<FORM, 2, true>(P, batch, K, substeps, samples, nwg, g0, blob, traj, fsum, xi, sigma, sigma_u, gain_u, gain_t, stretch_max,
                             nav.ff_u, nav.ff_t, nav.ff_know, nav.xi_nav, nav.sigma_nav, partial, samples_out, hist, drift);
}

__global__ __launch_bounds__(SW) void f_disperse_stats(long batch, int K, int nwg, const double *__restrict__ traj,
                                                       const double *__restrict__ fsum, const double *__restrict__ partial,
                                                       double *__restrict__ stats) {
  const long p = (long)blockIdx.x * SW + threadIdx.x;
  if (p >= batch) return;
  const size_t B = (size_t)batch;
  const double *pr = partial + p;
  double *out = stats + p;
  double nom[NQ], S[NQ];
  nominal_rows(traj, fsum, B, p, K, nom);
  double n = 0.0;
  for (int c = 0; c < nwg; c++) n += pr[((size_t)c * NREC + R_N) * B];
  out[(size_t)O_N * B] = n;
  ASC_UNROLL
  for (int q = 0; q < NQ; q++) {
    double a = 0.0, lo = INFINITY, hi = -INFINITY;
    for (int c = 0; c < nwg; c++) {
      a += pr[((size_t)c * NREC + R_SUM + q) * B];
      lo = fmin(lo, pr[((size_t)c * NREC + R_MIN + q) * B]);
      hi = fmax(hi, pr[((size_t)c * NREC + R_MAX + q) * B]);
    }
    S[q] = a;
    out[(size_t)(O_NOM + q) * B] = nom[q];
    // n = 0: NaN; n = 1: the sample itself (centre + (sample - centre) may round)
    out[(size_t)(O_MEAN + q) * B] = n == 1.0 ? lo : (finite1(nom[q]) ? nom[q] : 0.0) + a / n;
    out[(size_t)(O_MIN + q) * B] = n > 0.0 ? lo : NAN;
    out[(size_t)(O_MAX + q) * B] = n > 0.0 ? hi : NAN;
  }
  int idx = 0;
  ASC_UNROLL
  for (int i = 0; i < NQ; i++) {
    ASC_UNROLL
    for (int j = i; j < NQ; j++, idx++) {
      double a = 0.0;
      for (int c = 0; c < nwg; c++) a += pr[((size_t)c * NREC + R_PROD + idx) * B];
      out[(size_t)(O_COV + idx) * B] = n >= 2.0 ? (a - S[i] * S[j] / n) / (n - 1.0) : NAN;
    }
  }
}

// The 52 rows of hist_out from the partial records of the history nodes: one lane per (problem, node), problem fastest, lane
// e0 + ... of B * NJ; the chunks added in ascending order, the expressions of f_disperse_stats
__global__ __launch_bounds__(SW) void f_history_stats(const ascent_params *__restrict__ P, long batch, int K, int nwg, int stride, int nj,
                                                      long e0, const double *__restrict__ blob, const double *__restrict__ traj,
                                                      const double *__restrict__ partial, double *__restrict__ hist) {
  const long e = e0 + (long)blockIdx.x * SW + threadIdx.x;
  if (e >= batch * nj) return;
  const int i = (int)(e / batch);
  const long p = e - (long)i * batch;
  const size_t B = (size_t)batch;
  const int j = (i + 1) * stride < K ? (i + 1) * stride : K;
  const double *pr = partial + ((size_t)i * HREC) * B + p;      // chunk c: + c * nj * HREC * B
  const size_t cs = (size_t)nj * HREC * B;
  double *out = hist + (size_t)i * B + p;                       // row r: + r * nj * B
  const size_t rs = (size_t)nj * B;
  double nom[HQ];
  history_nominal(traj + p, blob + p, reinterpret_cast<const double *>(P + p), B, K, j, nom);
  double n = 0.0, nc = 0.0;
  for (int c = 0; c < nwg; c++) {
    n += pr[c * cs + (size_t)H_N * B];
    nc += pr[c * cs + (size_t)H_CLIP * B];
  }
  out[HO_N * rs] = n;
  out[HO_CLIP * rs] = nc;
  ASC_UNROLL
  for (int q = 0; q < HQ; q++) {
    double a = 0.0, sq = 0.0, lo = INFINITY, hi = -INFINITY;
    for (int c = 0; c < nwg; c++) {
      a += pr[c * cs + (size_t)(H_SUM + q) * B];
      sq += pr[c * cs + (size_t)(H_SQ + q) * B];
      lo = fmin(lo, pr[c * cs + (size_t)(H_MIN + q) * B]);
      hi = fmax(hi, pr[c * cs + (size_t)(H_MAX + q) * B]);
    }
    out[(HO_NOM + q) * rs] = nom[q];
    out[(HO_MEAN + q) * rs] = n == 1.0 ? lo : (finite1(nom[q]) ? nom[q] : 0.0) + a / n;
    out[(HO_VAR + q) * rs] = n >= 2.0 ? (sq - a * a / n) / (n - 1.0) : NAN;
    out[(HO_MIN + q) * rs] = n > 0.0 ? lo : NAN;
    out[(HO_MAX + q) * rs] = n > 0.0 ? hi : NAN;
  }
}

int groups_per_problem(int samples) { return (samples + DB - 1) / DB; }
// below 193 samples a workgroup holds only the wavefronts that fly: whole wavefronts, so the butterflies see 64 lanes
int threads_per_group(int samples) { return samples >= DB ? DB : (samples + 63) / 64 * 64; }

}  // namespace

int history_nodes(int K, int node_stride) { return K / node_stride + (K % node_stride != 0); }

size_t disperse_ws_bytes(int K, long batch, int samples, int node_stride) {
  const size_t nj = node_stride > 0 ? (size_t)history_nodes(K, node_stride) : 0;
  return flight_ws_bytes(K, batch) + (size_t)groups_per_problem(samples) * (NREC + nj * HREC) * (size_t)batch * sizeof(double);
}

template <int FORM>
static void disperse_launch(const Call &c, DisperseKind kind, dim3 grid, dim3 block, int substeps, int samples, int nwg, long g0,
                            const DisperseIO &io, const FlightWs &w) {
  double *partial = w.rest;
  if (io.hist) {      // the history: the partial records of the nodes follow the end records
    const HistArgs h{io.node_stride, history_nodes(c.K, io.node_stride), partial + (size_t)nwg * NREC * c.batch, io.hist_samples};
    if (io.nav_phi)
      hipLaunchKernelGGL((f_history_drifting<FORM>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, samples, nwg, g0, io.blob,
                         w.traj, w.fsum, io.xi, io.sigma, io.sigma_u, io.gain_u, io.gain_t, io.stretch_max,
                         NavArgs{io.ff_u, io.ff_t, io.ff_know, io.xi_nav, io.sigma_nav}, DriftArgs{io.nav_phi, io.nav_q, io.xi_drift}, partial,
                         io.samples_out, h);
    else if (kind == DISPERSE_OPEN)
      hipLaunchKernelGGL((f_disperse<FORM, true>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, samples, nwg, g0, io.blob,
                         w.traj, w.fsum, io.xi, io.sigma, io.sigma_u, partial, io.samples_out, h);
    else
      hipLaunchKernelGGL((f_history_guided<FORM>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, samples, nwg, g0, io.blob,
                         w.traj, w.fsum, io.xi, io.sigma, io.sigma_u, io.gain_u, io.gain_t, io.stretch_max,
                         NavArgs{io.ff_u, io.ff_t, io.ff_know, io.xi_nav, io.sigma_nav}, partial, io.samples_out, h);
  } else if (kind == DISPERSE_OPEN)
    hipLaunchKernelGGL((f_disperse<FORM, false>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, samples, nwg, g0, io.blob, w.traj,
                       w.fsum, io.xi, io.sigma, io.sigma_u, partial, io.samples_out, HistArgs{});
  else if (kind == DISPERSE_GUIDED)
    hipLaunchKernelGGL((f_disperse_guided<FORM>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, samples, nwg, g0, io.blob,
                       w.traj, w.fsum, io.xi, io.sigma, io.sigma_u, io.gain_u, io.gain_t, io.stretch_max, partial, io.samples_out);
  else
    hipLaunchKernelGGL((f_disperse_navigated<FORM>), grid, block, 0, c.stream, c.dp, c.batch, c.K, substeps, samples, nwg, g0, io.blob,
                       w.traj, w.fsum, io.xi, io.sigma, io.sigma_u, io.gain_u, io.gain_t, io.stretch_max,
                       NavArgs{io.ff_u, io.ff_t, io.ff_know, io.xi_nav, io.sigma_nav}, partial, io.samples_out);
}

int disperse_run(const Call &c, DisperseKind kind, int substeps, int samples, const DisperseIO &io, double *ws) {
  const FlightWs w = flight_ws(ws, c.K, c.batch);      // rest: the partial records
  if (const int rc = flight_fly_only(c, substeps, io.blob, w.traj, w.fsum)) return rc;
  const int nwg = groups_per_problem(samples);
  const long total = c.batch * nwg;
  for (long g0 = 0; g0 < total; g0 += MAX_GRID) {
    const dim3 grid((unsigned)(total - g0 < MAX_GRID ? total - g0 : MAX_GRID)), block(threads_per_group(samples));
    if (c.form == 1) disperse_launch<1>(c, kind, grid, block, substeps, samples, nwg, g0, io, w);
    else disperse_launch<0>(c, kind, grid, block, substeps, samples, nwg, g0, io, w);
    ASC_CHK(c.err, c.errlen, hipGetLastError());
  }
  const dim3 gst((unsigned)((c.batch + SW - 1) / SW)), bst(SW);
  hipLaunchKernelGGL(f_disperse_stats, gst, bst, 0, c.stream, c.batch, c.K, nwg, w.traj, w.fsum, w.rest, io.stats);
  ASC_CHK(c.err, c.errlen, hipGetLastError());
  if (io.hist) {
    const int nj = history_nodes(c.K, io.node_stride);
    const long lanes = c.batch * nj, per = MAX_GRID * SW;
    for (long e0 = 0; e0 < lanes; e0 += per) {
      const long left = lanes - e0 < per ? lanes - e0 : per;
      hipLaunchKernelGGL(f_history_stats, dim3((unsigned)((left + SW - 1) / SW)), bst, 0, c.stream, c.dp, c.batch, c.K, nwg,
                         io.node_stride, nj, e0, io.blob, w.traj, w.rest + (size_t)nwg * NREC * c.batch, io.hist);
      ASC_CHK(c.err, c.errlen, hipGetLastError());
    }
  }
  return ASCENT_OK;
}

}  // namespace ascent
