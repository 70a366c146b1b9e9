// Device-side pieces shared by the persistent kernels (ascent_persist.hip: backward Euler / trapezoid / v1, p_solve; ascent_hs.hip:
// Hermite-Simpson, h_solve): the workspace layout of an NLP, the per-NLP scalar record, 16-lane reductions and broadcasts, what a node
// evaluation loads, the partial sums of the merit function and the KKT error.  Included inside each translation unit's anonymous
// namespace (everything here has internal linkage).
#pragma once
#include <hip/hip_runtime.h>

#include "ascent.h"
#include "ascent_device.hpp"
#include "ascent_tile.hpp"

namespace {
using namespace ascent;

constexpr int NPW = 4, CH = 16;                 // NLPs per wavefront, nodes per chunk
constexpr int O_Z = 0, O_U = 7, O_L = 8, O_ZB = 15;
constexpr int O_LU = 21, O_PP = 22, O_PN = 23, O_ZP = 24, O_ZN = 25;      // move penalty only: lambda_u, p, n, z_p, z_n
// Rows of an NLP's node arrays: two iterate buffers, the step, the feedback gains of the factorisation.  MP = 1: with the l1 move
// penalty (ascent_opts.move_penalty, the reference's angledoubledot.DCOST, Launch_Optimiser.py:99) the control is the eighth
// state of a stage and an iterate carries five more rows per node.
// A row has Kp >= K + 1 columns; the columns k >= K of the iterate and step rows are zero halos: p_init / p_transfer write +0.0 there
// and every store of p_solve into a node row stands under k < K, so they stay +0.0 for the life of a level (see load_node below).
template <int MP>
struct Lay {
  static constexpr int NS = 7 + MP, NIT = 21 + 5 * MP;
  static constexpr int R_IT = 0, R_ST = 2 * NIT, R_KA = 3 * NIT, R_K0 = R_KA + NS, NROWS = R_K0 + 3;
  // LDS stage rows (one chunk): blocks of the factorisation; the forward / adjoint phases reuse the area
  // (MP: the mass row of hT F is a constant of the NLP and the barrier gradients are folded into rz, so that the stage stays within
  //  56 rows -- with 12 output rows and the small arrays 40 672 bytes per wavefront: four wavefronts per CU, as without the penalty)
  static constexpr int S_G = 0, S_E = 8, S_H = 12, S_F = 22, S_C = S_F + 7 - MP, S_RZ = S_C + NS, S_GT = S_RZ + NS, S_SC = S_GT + NS;
  static constexpr int S_ROWS = MP ? 56 : 55;        // (MP: S_SC + 3 = 55 in the factor phase; the forward phase's 7 lanes x 8 rows)
  static constexpr int OUT_ROWS = 11 + MP;
  static_assert(S_SC + (MP ? 3 : 5) <= S_ROWS, "stage rows");
};
constexpr int R_IT = 0;
constexpr int LDW = 65;                         // row stride in doubles: odd, so that the 16 rows a sweep step gathers hit 16 banks
enum {
  X_STATE, X_ITERS, X_STATUS, X_CUR, X_FIRST, X_LS, X_MU, X_NUP, X_DW, X_DWL, X_ALPHA, X_ADU, X_PHI0, X_DM, X_C1, X_SL,
  X_RTH, X_DTH, X_DNU3, X_SIG1, X_SIG2, X_RS1, X_RS2, X_CG1, X_CG2,
  X_ITB,                     // iterations spent on the coarser grids of the nested iteration
  X_PROBE, X_PDW,            // parity probe: one round at the caller's iterate, mu and delta_w, then stop (1: Newton step; 2: the node rows of the factor phase)
  X_TEVAL,                   // the trial point of the next round has been evaluated already (by the adjoint phase)
  X_P,                       // 10 reduced partials of that trial point: rd cinf pmin pmax l1 zsum rth c1 sl mv
  X_PEND = X_P + 9,
  X_MV,                      // move penalty: sum of the slack pairs of the iterate (its part of the objective, without the weight)
  X_S,                       // 10 scalars of the iterate
  X_D = X_S + 10,            // 10 step scalars
  NSCAL = X_D + 10
};
constexpr int NSCAL_PAD = 64;
static_assert(NSCAL <= NSCAL_PAD, "scalar record");
enum { ST_TRIAL = 0, ST_FACTOR = 1, ST_FACTORED = 2, ST_DONE = 3 };

struct PGeo {
  int K, Kp, nch, form, mp, term, wide;      // wide: one NLP per wavefront, 64-node chunks; term: ascent_opts.terminal 2 (burnout anywhere on the ellipse) or 0
  __host__ __device__ int nit() const { return mp ? Lay<1>::NIT : Lay<0>::NIT; }
  __host__ __device__ int r_st() const { return 2 * nit(); }
  __host__ __device__ int nrows() const { return mp ? Lay<1>::NROWS : Lay<0>::NROWS; }
  // (the scalar record padded to 64 doubles: with Kp a multiple of 16 every NLP then starts on a 128-byte line, and so does every row of it --
  //  a chunk row of an NLP is ONE line instead of straddling two)
  __host__ __device__ size_t nlp_doubles() const { return (size_t)nrows() * Kp + NSCAL_PAD; }
};

template <int SRC>
ASC_DEV double bcast16(double v) {
  const long x = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(long, v), 0x150 + SRC, 0xf, 0xf, false);
  return __builtin_bit_cast(double, x);
}
template <int N>
struct OneHot {
  double m[N];
  ASC_DEV explicit OneHot(int role) {
    ASC_UNROLL
    for (int i = 0; i < N; i++) m[i] = (role == i || (i == 0 && role >= N)) ? 1.0 : 0.0;
  }
  ASC_DEV double pick(const double *v) const {
    double r = m[0] * v[0];
    ASC_UNROLL
    for (int i = 1; i < N; i++) r += m[i] * v[i];
    return r;
  }
};
// A phase's own copy of a lane constant (role, grp, ...).  p_solve derives LDS addresses, row selections and masks from the lane's index;
// derived from the kernel's copy they are invariants of the round loop: the compiler computes them once, parks them in AGPRs or scratch
// for the whole kernel and fetches them back inside every serial step.  The empty asm makes the copy opaque, so that what a phase derives
// from it is computed at the top of that phase and lives in VGPRs for that phase alone.  The value is unchanged.  DESIGN.md 4a-live.
ASC_DEV int phase_local(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
ASC_DEV void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// reductions over the 16 lanes of an NLP (xor strides stay inside the row of 16): the butterfly written with shuffles -- every stage an
// LDS round trip (two ds_bpermute_b32 and a wait) on a chain of four.  Kept for p_solve without the move penalty (see gsumW below) and as
// the reference of the reduce probe (ascent_reduce_probe).
ASC_DEV double gsum16_shfl(double v) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8); return v; }
ASC_DEV double gmax16_shfl(double v) { v = fmax(v, __shfl_xor(v, 1)); v = fmax(v, __shfl_xor(v, 2)); v = fmax(v, __shfl_xor(v, 4)); return fmax(v, __shfl_xor(v, 8)); }
ASC_DEV double gmin16_shfl(double v) { v = fmin(v, __shfl_xor(v, 1)); v = fmin(v, __shfl_xor(v, 2)); v = fmin(v, __shfl_xor(v, 4)); return fmin(v, __shfl_xor(v, 8)); }
// The same butterfly on DPP moves (v_mov_b32_dpp pairs: no LDS operation, no wait).  Stages 1 and 2 are the xor-1 and xor-2 exchanges
// (quad_perm [1,0,3,2], [2,3,0,1]); after them the four lanes of a quad hold the same bits, so the mirrored partner of stage 3 (the
// other quad of the half, row_half_mirror) and of stage 4 (the other half of the row, row_mirror) delivers the operand the xor-4 / xor-8
// partner would: the results equal the shuffle versions' bit for bit (tests/test_gpu_reduce_probe.py).
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_ROW_SHR = 0x110, DPP_ROW_MIRROR = 0x140, DPP_HALF_MIRROR = 0x141;
template <int CTRL>
ASC_DEV double dpp16(double v) {
  const long x = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(long, v), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, x);
}
ASC_DEV double gsum16(double v) { v += dpp16<DPP_XOR1>(v); v += dpp16<DPP_XOR2>(v); v += dpp16<DPP_HALF_MIRROR>(v); v += dpp16<DPP_ROW_MIRROR>(v); return v; }
ASC_DEV double gmax16(double v) { v = fmax(v, dpp16<DPP_XOR1>(v)); v = fmax(v, dpp16<DPP_XOR2>(v)); v = fmax(v, dpp16<DPP_HALF_MIRROR>(v)); return fmax(v, dpp16<DPP_ROW_MIRROR>(v)); }
ASC_DEV double gmin16(double v) { v = fmin(v, dpp16<DPP_XOR1>(v)); v = fmin(v, dpp16<DPP_XOR2>(v)); v = fmin(v, dpp16<DPP_HALF_MIRROR>(v)); return fmin(v, dpp16<DPP_ROW_MIRROR>(v)); }
// inclusive prefix sum over the 16 lanes of an NLP (nl: the lane's index in its row): row_shr with the lane's own value as the old
// operand, so that the lanes nl < sft, which have no source, keep theirs -- what __shfl_up with width 16 hands them
template <int SFT>
ASC_DEV double shr16(double v) {
  const long x = __builtin_bit_cast(long, v);
  const int lo = (int)x, hi = (int)(x >> 32);
  const unsigned rlo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, DPP_ROW_SHR + SFT, 0xf, 0xf, false);
  const unsigned rhi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, DPP_ROW_SHR + SFT, 0xf, 0xf, false);
  return __builtin_bit_cast(double, (long)(((unsigned long)rhi << 32) | rlo));
}
ASC_DEV double scan16(double v, int nl) {
  double t;
  t = shr16<1>(v); if (nl >= 1) v += t;
  t = shr16<2>(v); if (nl >= 2) v += t;
  t = shr16<4>(v); if (nl >= 4) v += t;
  t = shr16<8>(v); if (nl >= 8) v += t;
  return v;
}
template <int W>      // (W = 16: the reference of the probe; W = 64: the scan of the one-NLP-per-wavefront form)
ASC_DEV double scan_shfl(double v, int nl) {
  ASC_UNROLL
  for (int sft = 1; sft < W; sft *= 2) {
    const double t = __shfl_up(v, sft, W);
    if (nl >= sft) v += t;
  }
  return v;
}
template <int WIDE, int DPP = 1> ASC_DEV double scanW(double v, int nl) { if constexpr (WIDE) return scan_shfl<64>(v, nl); else if constexpr (DPP) return scan16(v, nl); else return scan_shfl<16>(v, nl); }
// ... or over the whole wavefront (WIDE: one NLP per wavefront)
// (DPP = 0: the shuffle versions.  p_solve without the move penalty keeps them: with the DPP forms its register allocation moves -- 52 more
//  AGPR copies in the adjoint chunk loop, +0.9 % on the unpenalised sweep -- while the penalised kernels and h_solve gain)
template <int WIDE, int DPP = 1> ASC_DEV double gsumW(double v) { v = DPP ? gsum16(v) : gsum16_shfl(v); if constexpr (WIDE) { v += __shfl_xor(v, 16); v += __shfl_xor(v, 32); } return v; }
template <int WIDE, int DPP = 1> ASC_DEV double gmaxW(double v) { v = DPP ? gmax16(v) : gmax16_shfl(v); if constexpr (WIDE) { v = fmax(v, __shfl_xor(v, 16)); v = fmax(v, __shfl_xor(v, 32)); } return v; }
template <int WIDE, int DPP = 1> ASC_DEV double gminW(double v) { v = DPP ? gmin16(v) : gmin16_shfl(v); if constexpr (WIDE) { v = fmin(v, __shfl_xor(v, 16)); v = fmin(v, __shfl_xor(v, 32)); } return v; }

template <typename PT>      // (a generic or an LDS pointer)
ASC_DEV Scal lds_scal(PT sc, int r0) {
  Scal s;
  s.th = sc[r0 + S_TH]; s.zlt = sc[r0 + S_ZLT]; s.zut = sc[r0 + S_ZUT]; s.s1 = sc[r0 + S_S1]; s.s2 = sc[r0 + S_S2];
  s.zs1 = sc[r0 + S_ZS1]; s.zs2 = sc[r0 + S_ZS2]; s.nu3 = sc[r0 + S_NU3]; s.nu1 = sc[r0 + S_NU1]; s.nu2 = sc[r0 + S_NU2];
  return s;
}
ASC_DEV void put_scal(double *sc, int r0, const Scal &s) {
  sc[r0 + S_TH] = s.th; sc[r0 + S_ZLT] = s.zlt; sc[r0 + S_ZUT] = s.zut; sc[r0 + S_S1] = s.s1; sc[r0 + S_S2] = s.s2;
  sc[r0 + S_ZS1] = s.zs1; sc[r0 + S_ZS2] = s.zs2; sc[r0 + S_NU3] = s.nu3; sc[r0 + S_NU1] = s.nu1; sc[r0 + S_NU2] = s.nu2;
}
ASC_DEV Scal trial_scal(const Der &d, const Scal &s, const Scal &ds, double alpha, double adu, double mu, bool first) {
  Scal t = s;
  if (first) return t;
  t.th += alpha * ds.th; t.s1 += alpha * ds.s1; t.s2 += alpha * ds.s2;
  t.nu3 += alpha * ds.nu3; t.nu1 += alpha * ds.nu1; t.nu2 += alpha * ds.nu2;
  t.zlt = clipz(s.zlt + adu * ds.zlt, t.th - d.tlb, mu);
  t.zut = clipz(s.zut + adu * ds.zut, d.tub - t.th, mu);
  t.zs1 = clipz(s.zs1 + adu * ds.zs1, t.s1, mu);
  t.zs2 = clipz(s.zs2 + adu * ds.zs2, t.s2, mu);
  return t;
}

struct NodeIn {      // what a node evaluation reads: node k of the iterate, the state of node k-1, the multipliers of node k+1
  double z[7], zp[7], l[7], ln[7], zb[6], u;
  double up, lu, lun, pp, pn, zpp, zpn;      // move penalty only: u_{k-1}, lambda_u of nodes k and k+1, the slack pair and its multipliers
};
// Zero halo columns.  Kp >= K + 1 (geo_of), and in every node row of the two iterate buffers and of the step (rows R_IT .. R_KA - 1)
// the columns k >= K hold +0.0 for the whole life of a level: p_init and p_transfer write them, and every store of p_solve into
// these rows stands under k < K (trial_primal, trial_dual, the step stores of the forward and adjoint phases, the probe rows).
// The neighbour of the first node is then the last pad column of the row in front, the neighbour of the last node the row's own
// column K: node k-1 / k+1 of a row is loaded without a test and the grid ends read the +0.0 a select would produce.  Two loads
// keep their select: row O_Z + 0 of an iterate at k = 0 (in front of buffer 0 lies the scalar record of the NLP before, or nothing),
// and the control "before node 0" of the v1 formulation's movement equations, which is -1 (the angle starts at 0), not 0.
// (load_step below: the rows are the step's -- the row in front of its O_Z + 0 is the second iterate buffer's last, the control before node 0 is 0.)
// (Kp is taken as a 64-bit stride here: a row address is then one v_lshl_add_u64 instead of add, sign extension and shift-add.  Here
//  only -- in trial_* or all of p_solve it costs scratch or time)
template <int MP = 0, int FORM = 0>
ASC_DEV void load_node(const double *it, long Kp, int k, NodeIn &n) {
  ASC_UNROLL
  for (int i = 0; i < 7; i++) {
    n.z[i] = it[(O_Z + i) * Kp + k];
    n.l[i] = it[(O_L + i) * Kp + k];
    n.zp[i] = (i > 0 || k > 0) ? it[(O_Z + i) * Kp + k - 1] : 0.0;
    n.ln[i] = it[(O_L + i) * Kp + k + 1];
  }
  n.u = it[O_U * Kp + k];
  ASC_UNROLL
  for (int b = 0; b < 6; b++) n.zb[b] = it[(O_ZB + b) * Kp + k];
  if constexpr (MP) {
    n.up = (FORM != 1 || k > 0) ? it[O_U * Kp + k - 1] : -1.0;
    n.lu = it[O_LU * Kp + k];
    n.lun = it[O_LU * Kp + k + 1];
    n.pp = it[O_PP * Kp + k]; n.pn = it[O_PN * Kp + k]; n.zpp = it[O_ZP * Kp + k]; n.zpn = it[O_ZN * Kp + k];
  }
}
// The rows of the step that p_solve stores: dz, du, dl and (MP) d lambda_u with their neighbours (no select: see above).
// The bound-multiplier rows and the slack pair's are not stored: the caller computes them from the iterate (step_locals, ascent_persist.hip).
template <int MP = 0>
ASC_DEV void load_step(const double *stp, long Kp, int k, NodeIn &n) {
  ASC_UNROLL
  for (int i = 0; i < 7; i++) {
    n.z[i] = stp[(O_Z + i) * Kp + k];
    n.l[i] = stp[(O_L + i) * Kp + k];
    n.zp[i] = stp[(O_Z + i) * Kp + k - 1];
    n.ln[i] = stp[(O_L + i) * Kp + k + 1];
  }
  n.u = stp[O_U * Kp + k];
  if constexpr (MP) {
    n.up = stp[O_U * Kp + k - 1];
    n.lu = stp[O_LU * Kp + k];
    n.lun = stp[O_LU * Kp + k + 1];
  }
}

// Partial sums of the merit function and the KKT error over the nodes a lane evaluates
struct Part {
  double rd, cinf, pmin, pmax, l1, zsum, rth, c1, sl, mv;
  ASC_DEV void clear() { rd = 0.0; cinf = 0.0; pmin = 1e300; pmax = -1e300; l1 = 0.0; zsum = 0.0; rth = 0.0; c1 = 0.0; sl = 0.0; mv = 0.0; }
  template <int MP = 0>
  ASC_DEV void reduce16() {
    rd = gmax16(rd); cinf = gmax16(cinf); pmin = gmin16(pmin); pmax = gmax16(pmax);
    l1 = gsum16(l1); zsum = gsum16(zsum); rth = gsum16(rth); c1 = gsum16(c1); sl = gsum16(sl);
    if constexpr (MP) mv = gsum16(mv);
  }
  template <int MP, int WIDE, int DPP = 1>
  ASC_DEV void reduceW() {
    rd = gmaxW<WIDE, DPP>(rd); cinf = gmaxW<WIDE, DPP>(cinf); pmin = gminW<WIDE, DPP>(pmin); pmax = gmaxW<WIDE, DPP>(pmax);
    l1 = gsumW<WIDE, DPP>(l1); zsum = gsumW<WIDE, DPP>(zsum); rth = gsumW<WIDE, DPP>(rth); c1 = gsumW<WIDE, DPP>(c1); sl = gsumW<WIDE, DPP>(sl);
    if constexpr (MP) mv = gsumW<WIDE, DPP>(mv);
  }
};
struct TrialCtx {       // what the trial point of an NLP needs besides the node data
  double alpha, adu, mlo, mhi, dt, be, hT, dcw;
  bool first;
  Scal stt;
};

#ifdef PERSIST_PROFILE      // diagnostic build (scripts/persist_profile.py): shader cycles per phase, wavefront 0
#define PROF_DECL long long prof_[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; long long pt_ = clock64();
#define PROF(i_) do { const long long t1_ = clock64(); prof_[i_] += t1_ - pt_; pt_ = t1_; } while (0)
#define PROF_END do { if (blockIdx.x == 0 && threadIdx.x == 0) printf("[persist profile] cycles: A %lld | B eval %lld serial %lld flush %lld | F eval %lld serial %lld post %lld | Adj eval %lld serial %lld | rest %lld\n", prof_[0], prof_[1], prof_[2], prof_[3], prof_[4], prof_[5], prof_[6], prof_[7], prof_[8], prof_[9]); } while (0)
#else
#define PROF_DECL
#define PROF(i_) do { } while (0)
#define PROF_END do { } while (0)
#endif

}  // namespace
