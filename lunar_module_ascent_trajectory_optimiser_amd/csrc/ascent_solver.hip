// libascent: batched primal-dual interior-point solver for the lunar-ascent collocation NLP of
// /root/reference/Launch_Optimiser.py, hand-written for MI355X (gfx950).  Replaces the
// m.solve() call at Launch_Optimiser.py:177 (GEKKO -> APMonitor -> IPOPT/MUMPS).
//
// This file is the C ABI (include/ascent.h): argument checks, workspaces, staging of host pointers, the nested
// iteration over grid levels, and route(), which picks the kernel family of a call.  Every entry point refuses argument errors
// first, then looks at the device, then takes the device's lock; it describes the call to the families in one Call
// (ascent_host.hpp), and the entry points that allocate per call stage host pointers through one Staging.  The families sit
// behind their own host interfaces:
//   persistent p_solve / h_solve    ascent_persist.hpp (ascent_persist.hip, ascent_hs.hip)
//   dense blocks d_* / pc_*         ascent_dense.hpp (ascent_dense.hip, ascent_blocktri.hip)
//   split pipeline q_*              ascent_pipeline.hpp (ascent_pipeline.hip)
//   fused k_solve                   ascent_fused.hpp (ascent_fused.hip)
// The calls on a solution blob after the solve share one host path, BlobCall below (checks, device lock, the analysis workspace
// of the device, staging, the Call and the staged blob); each states only its own checks, its buffers and its run function:
//   post-optimal sensitivity s_sens                       ascent_sens.hpp (ascent_sens.hip)
//   flight verification f_fly / f_local                   ascent_flight.hpp (ascent_flight.hip)
//   flight Jacobian and trim j_jac / t_update / t_final   ascent_trim.hpp (ascent_trim.hip)
//   guidance gains g_gains / g_gains_ff                   ascent_guide.hpp (ascent_guide.hip), one GainsIO for both calls
//   dispersion f_disperse / _guided / _navigated          ascent_disperse.hpp (ascent_disperse.hip), one DisperseIO for all three
//   linear covariance corridor l_lincov                   ascent_lincov.hpp (ascent_lincov.hip)
//   navigation filter n_filter / l_lincov_filtered        ascent_navfilter.hpp (ascent_navfilter.hip)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>
#include <cmath>

#include "ascent.h"
#include "ascent_host.hpp"
#include "ascent_device.hpp"
#include "ascent_tile.hpp"
#include "ascent_pipeline.hpp"
#include "ascent_dense.hpp"
#include "ascent_blocktri.hpp"
#include "ascent_persist.hpp"
#include "ascent_fused.hpp"
#include "ascent_sens.hpp"
#include "ascent_flight.hpp"
#include "ascent_trim.hpp"
#include "ascent_disperse.hpp"
#include "ascent_guide.hpp"
#include "ascent_lincov.hpp"
#include "ascent_navfilter.hpp"
#include "ascent_quantile.hpp"

using namespace ascent;

namespace {

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
thread_local char g_err[512] = "";

#define HIPCHK(call) ASC_CHK(g_err, sizeof g_err, call)

// ---------------------------------------------------------------------------------------------
// Nested iteration (mesh continuation).  A cold start on a grid of >= 40 nodes first solves the same NLP on a
// grid of three tenths of the nodes (recursively: 201 -> 60 -> 17), prolongs that primal-dual solution to the next
// grid and warm-starts the solve there: with mu0 = 1e-6 from the coarsest (cold-started) grid, with mu0 = max(1e-9,
// tol/100) from a grid that was itself warm-started (ASCENT_NESTED_MU=first,next overrides the pair for experiments:
// scripts/nested_mu_scan.py; DESIGN.md has the scan -- tol/10 and 0.4 tol are 2 % and 7 % faster on the config-3 batch and
// 30 % at N = 2000, but leave the convergence test on a knife edge often enough that iteration counts differ between kernel
// families, and with 0.4 tol t_f depends on the start by 40 mu = 1.7e-8).  On the config-3 sweep 9.7 + 4 + 7.7 iterations on 17 / 59 / 200
// intervals instead of 24 on 200, and hardly any straggler tail (scripts/nested_levels.py compares the policies).  (The CPU
// restatement under the test tree follows the same rule, constants and arithmetic, so that iteration counts can be
// compared one to one.)
// ---------------------------------------------------------------------------------------------
constexpr int NESTED_MIN_NODES = 40;
constexpr double NESTED_MU_FIRST = 1e-6;     // warm start from the cold-started coarsest grid
inline double nested_mu_next(double tol) { return fmax(1e-9, 1e-2 * tol); }      // warm start from a grid that was warm-started itself (tol: of the finest grid)
// ... with the move penalty: the slack pairs of the movement equations are re-centred on every grid, and where the control's movement
// changes sign a pair swaps roles through the kink of |.| -- at mu = 1e-9 up to seven fraction-to-boundary-limited iterations; started
// at 1e-5 / 1e-8 the config-3 sweep's 200-node level takes 9-13 iterations instead of 9-16 (the kernel waits for its slowest NLP)
constexpr double NESTED_MU_FIRST_MP = 1e-5;
inline double nested_mu_next_mp(double tol) { return fmax(1e-8, 10.0 * tol); }
constexpr double NESTED_COARSE_TOL = 1e-3;   // coarse levels: the reference's own OTOL/RTOL (their discretisation error is 1e-2)
// (three tenths of the nodes; a grid that would spill one to three intervals into another 16-interval chunk of the
//  persistent kernel gives them up: 18 nodes -> 17)
inline int coarse_of(int nt) {
  int c = (3 * nt + 5) / 10;
  if (c < 14) c = 14;
  const int over = (c - 1) % 16;
  if (c > 17 && over >= 1 && over <= 3) c -= over;
  return c;
}

// Prolongation of external blobs ([row][batch]): linear in tau; node 0 is the fixed initial state (zero, except the
// algebraic angle of the v1 formulation) for the states and the first node for everything else; bound multipliers
// scale with the step; scalars are copied.  A problem whose coarse solve did not converge gets theta = -1, which
// the solvers read as "no guess".  acc_iters collects the iterations spent on the coarser levels.
__global__ __launch_bounds__(WAVE) void k_prolong(const double *bc, const int *status_c, const int *iters_c, int Kc,
                                                  double *bf, int Kf, long batch, int form, int *acc_iters,
                                                  int first_level) {
  const long p = (long)blockIdx.x * WAVE + threadIdx.x;
  if (p >= batch) return;
  const int k = blockIdx.y;
  const double x = (double)(k + 1) / (double)Kf * (double)Kc;
  int j = (int)x;
  if (j > Kc - 1) j = Kc - 1;
  const double wt = x - (double)j;
  const long ja = j ? j - 1 : 0;
  const double zsc = (double)Kc / (double)Kf;
#define BC(r) bc[(long)(r) * batch + p]
#define BF(r) bf[(long)(r) * batch + p]
  for (int i = 0; i < 7; i++) {
    const double a = j ? BC(7 * ja + i) : ((form == 1 && i == IA) ? BC(i) : 0.0), b = BC(7L * j + i);
    BF(7L * k + i) = fma(wt, b - a, a);
    const double la = BC(8L * Kc + 7 * ja + i), lb = BC(8L * Kc + 7L * j + i);
    BF(8L * Kf + 7L * k + i) = fma(wt, lb - la, la);
  }
  {
    const double a = BC(7L * Kc + ja), b = BC(7L * Kc + j);
    BF(7L * Kf + k) = fma(wt, b - a, a);
  }
  for (int b6 = 0; b6 < 6; b6++) {
    const double a = BC(15L * Kc + 6 * ja + b6), b = BC(15L * Kc + 6L * j + b6);
    BF(15L * Kf + 6L * k + b6) = fma(wt, b - a, a) * zsc;
  }
  if (k == 0) {
    const bool ok = status_c[p] == ASCENT_CONVERGED;
    for (int r = 0; r < NSC; r++) BF(21L * Kf + r) = (r == S_TH && !ok) ? -1.0 : BC(21L * Kc + r);
    acc_iters[p] = (first_level ? 0 : acc_iters[p]) + iters_c[p];
  }
#undef BC
#undef BF
}

__global__ __launch_bounds__(WAVE) void k_add_iters(int *iters, const int *acc, long batch) {
  const long p = (long)blockIdx.x * WAVE + threadIdx.x;
  if (p < batch) iters[p] += acc[p];
}

// ascent_opts.terminal = 1: the terminal speed becomes the vis-viva speed at the periapsis of the (r_peri, r_apo) ellipse.
// Every kernel derives its constants from the parameter struct (derive(): circular speed of the mean radius, LO:72-78), so
// the solvers run on a copy whose r_apo is replaced by the apoapsis r' for which that mean-radius formula gives the wanted
// speed:  GM / (R0 + (r_peri + r')/2) = GM (2/rp - 2/(rp + ra)).
__global__ __launch_bounds__(WAVE) void k_terminal_params(const ascent_params *in, ascent_params *out, long batch) {
  const long p = (long)blockIdx.x * WAVE + threadIdx.x;
  if (p >= batch) return;
  ascent_params q = in[p];
  const double rp = q.R0 + q.r_peri, ra = q.R0 + q.r_apo;
  q.r_apo = 2.0 * (1.0 / (2.0 / rp - 2.0 / (rp + ra)) - q.R0) - q.r_peri;
  out[p] = q;
}

// ---------------------------------------------------------------------------------------------
// Routing: which kernel family runs a call, and in which form (DESIGN.md section 4 has the measurements behind every
// threshold).  route() is the only reader of the routing overrides, on every call:
//   ASCENT_PIPELINE=persist|split|fused|dense   a family by name
//   ASCENT_FACTOR=wide|lane                     the split pipeline with its 16-lane / one-lane sweeps
//   ASCENT_SMALL_BATCH=off                      no dense blocks for a handful of NLPs on a long grid
//   ASCENT_DENSE_NEWTON=pcr|riccati             the dense path's Newton solver
//   ASCENT_PERSIST_WIDE=1|0                     the persistent kernels with one / four NLPs per wavefront
// ---------------------------------------------------------------------------------------------
struct Route {
  int path;       // enum ascent_path, never ASCENT_PATH_AUTO
  bool pcr;       // ASCENT_PATH_DENSE: Newton systems by cyclic reduction over the nodes (else the serial Riccati recursion)
  bool wide;      // ASCENT_PATH_PERSIST: one NLP per wavefront (else four)
};

// What a kernel family does not carry (beyond the option checks of check_options): nullptr, or the reason for refusing the call.
const char *unsupported(int path, const ascent_opts *o) {
  switch (path) {
    case ASCENT_PATH_PERSIST:      // backward Euler (both formulations), the trapezoid, Hermite-Simpson without the move penalty
      return o->scheme != 0 && o->formulation != 0 ? "the persistent kernels have formulation 1 with scheme 0 only"
           : o->scheme == 2 && o->move_penalty ? "the persistent Hermite-Simpson kernel has no move penalty (the dense-block path has)"
           : nullptr;
    case ASCENT_PATH_DENSE:
      return o->formulation != 0 ? "the dense-block path has formulation 0 only" : nullptr;
    case ASCENT_PATH_FUSED:
      if (o->scheme != 0 || o->formulation != 0) return "the fused path has scheme 0, formulation 0 only";
      break;
    default:      // the split pipeline
      if (o->scheme == 2) return "scheme 2 exists in the persistent Hermite-Simpson kernel and in the dense-block path only";
  }
  if (o->move_penalty || o->terminal == 2)
    return "move_penalty = 1 and terminal 2 exist in the persistent kernel and in the dense-block path only (ASCENT_PIPELINE / ASCENT_FACTOR name another family)";
  return nullptr;
}

static bool env_is(const char *e, const char *v) { return e && !strcmp(e, v); }

// The path of ascent_solve_batch; the first rule that applies wins.
static int auto_path(const ascent_opts *o, int64_t batch, const char *pipe, const char *factor, bool small_off) {
  if (o->solver_path == ASCENT_PATH_DENSE) return ASCENT_PATH_DENSE;
  // The move penalty, terminal 2 and Hermite-Simpson exist in the persistent kernels and in the dense-block path: an override
  // that names any other family (ASCENT_FACTOR names the split pipeline) means the dense one.  So does Hermite-Simpson with
  // the move penalty.
  const bool other = (pipe && strcmp(pipe, "persist")) || factor;
  if (o->scheme == 2 && (o->move_penalty || o->formulation != 0 || other)) return ASCENT_PATH_DENSE;
  if ((o->move_penalty || o->terminal == 2) && o->formulation == 0 && other) return ASCENT_PATH_DENSE;
  if (pipe) {
    if (env_is(pipe, "dense") && o->formulation == 0) return ASCENT_PATH_DENSE;
  } else if (!small_off && o->formulation == 0 && !factor && o->terminal != 2) {
    // A handful of NLPs cannot fill the one-wavefront-per-NLP kernels; the dense-block path with cyclic reduction over the
    // nodes spreads one NLP over hundreds of wavefronts: on grids of >= 400 intervals while batch <= min(6, intervals/300)
    // (section 4d, scripts/small_batch_paths.py).  Not for terminal 2, which has no cyclic-reduction variant (see pcr below).
    const int64_t K = (int64_t)o->n_nodes - 1;
    const int64_t lim = K < 400 ? 0 : (K / 300 < 6 ? K / 300 : 6);
    if (batch <= lim) return ASCENT_PATH_DENSE;
  }
  // the persistent kernels are ahead of the other families at every batch size (section 4a-wide, scripts/batch_sweep2.py)
  if (o->scheme <= 2 && !unsupported(ASCENT_PATH_PERSIST, o) && (pipe ? env_is(pipe, "persist") : !factor)) return ASCENT_PATH_PERSIST;
  // the split pipeline while the batch alone cannot fill the chip, the fused kernel above (section 4b, scripts/batch_sweep.py)
  const bool split = o->scheme == 1 || o->formulation == 1 || env_is(pipe, "split") || (!env_is(pipe, "fused") && batch <= 24576);
  if (!split) return ASCENT_PATH_FUSED;
  // the 16-lanes-per-NLP sweeps pay while the chip has idle SIMDs (one wavefront per SIMD), the one-lane sweeps above
  const bool wide = factor ? factor[0] == 'w' : batch <= 4096;
  return wide ? ASCENT_PATH_SPLIT_WIDE : ASCENT_PATH_SPLIT_LANE;
}

// requested: ASCENT_PATH_AUTO (the path of ascent_solve_batch) or the explicit path of a parity surface.  probe: a parity
// surface's call rather than a solve (an explicit ASCENT_DENSE_NEWTON then holds for terminal 2 as well).
Route route(const ascent_opts *o, int64_t batch, int requested, bool probe) {
  const char *pipe = getenv("ASCENT_PIPELINE"), *factor = getenv("ASCENT_FACTOR"), *small = getenv("ASCENT_SMALL_BATCH");
  const char *newton = getenv("ASCENT_DENSE_NEWTON"), *pwide = getenv("ASCENT_PERSIST_WIDE");
  const int path = requested != ASCENT_PATH_AUTO ? requested : auto_path(o, batch, pipe, factor, env_is(small, "off"));
  Route r{path, false, false};
  // Cyclic reduction wins while batch x nodes leaves SIMDs idle (section 4d).  Never in a solve with terminal 2: its
  // curvature test sees no inertia and picks regularisations that stall on the nearly dependent terminal conditions.
  if (path == ASCENT_PATH_DENSE && (o->terminal != 2 || (probe && newton))) {
    if (env_is(newton, "pcr")) r.pcr = true;
    else if (env_is(newton, "riccati")) r.pcr = false;
    else r.pcr = batch <= (o->move_penalty ? 32 : 64);      // (16x16 node blocks with the move penalty)
  }
  // one NLP per wavefront while four per wavefront cannot give every SIMD a wavefront (section 4a-wide)
  if (path == ASCENT_PATH_PERSIST) r.wide = pwide ? pwide[0] == '1' : batch <= 1024;
  return r;
}

struct DeviceWs {
  double *ws = nullptr;
  size_t bytes = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool launched = false;
  // nested iteration: solution blob of the coarser level, guess blob of the finer one, per-level status / iterations
  double *sol = nullptr, *gss = nullptr, *tfc = nullptr;
  size_t sol_n = 0, gss_n = 0, int_n = 0;
  int *st_c = nullptr, *it_c = nullptr, *acc = nullptr;
  // staging buffers of host-pointer calls, kept between calls (the GEKKO-style front end solves one NLP per call)
  ascent_params *h_p = nullptr, *t_p = nullptr;
  size_t t_p_n = 0;
  double *h_guess = nullptr, *h_traj = nullptr, *h_tf = nullptr, *h_blob = nullptr;
  int *h_status = nullptr, *h_iters = nullptr;
  size_t h_p_n = 0, h_guess_n = 0, h_traj_n = 0, h_tf_n = 0, h_blob_n = 0, h_status_n = 0, h_iters_n = 0;
};
constexpr int MAX_DEV = 64;
// Workspaces per device: slot 0 serves the default stream, the parity surfaces and every stream that finds no free slot;
// up to WS_SLOTS - 1 further caller streams get a workspace of their own, so that solves enqueued on different streams
// overlap on the device (the wavefronts of one fill the SIMDs the stragglers of the other leave idle).
constexpr int WS_SLOTS = 4;
DeviceWs g_wss[MAX_DEV][WS_SLOTS];
hipStream_t g_ws_stream[MAX_DEV][WS_SLOTS];
int g_ws_last[MAX_DEV];
std::mutex g_mu[MAX_DEV];
#define g_ws_slot0(dev_) g_wss[dev_][0]

static int slot_for(int dev, hipStream_t s) {       // (under g_mu[dev])
  if (!s) return 0;
  for (int i = 1; i < WS_SLOTS; i++)
    if (g_ws_stream[dev][i] == s) return i;
  for (int i = 1; i < WS_SLOTS; i++)
    if (!g_ws_stream[dev][i]) { g_ws_stream[dev][i] = s; return i; }
  for (int i = 1; i < WS_SLOTS; i++) {      // table full: a slot whose last solve has finished goes to the new stream (its old one may be gone)
    DeviceWs &w = g_wss[dev][i];
    if (!w.launched || hipEventQuery(w.ev1) == hipSuccess) { g_ws_stream[dev][i] = s; return i; }
  }
  return 0;
}

// The parity surfaces and ascent_kkt_solve run on the null stream in workspace 0, which is also the fallback of caller streams
// that found no slot of their own: before they touch it they wait for whatever solve was last enqueued there (a non-blocking
// stream does not synchronise with the null stream by itself), and they become the device's "last solve" for ascent_last_kernel_ms.
static int claim_slot0(int dev) {                   // (under g_mu[dev])
  DeviceWs &w = g_wss[dev][0];
  if (w.launched) HIPCHK(hipEventSynchronize(w.ev1));
  g_ws_last[dev] = 0;
  return 0;
}

int ensure_ws(DeviceWs &w, size_t bytes) {
  if (!w.ev0) {
    HIPCHK(hipEventCreate(&w.ev0));
    HIPCHK(hipEventCreate(&w.ev1));
  }
  if (w.bytes >= bytes) return 0;
  if (w.ws) HIPCHK(hipFree(w.ws));
  w.ws = nullptr;
  w.bytes = 0;
  hipError_t e = hipMalloc(&w.ws, bytes);
  if (e != hipSuccess) {
    snprintf(g_err, sizeof g_err, "workspace hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    return ASCENT_E_NOMEM;
  }
  w.bytes = bytes;
  return 0;
}

template <typename T>
int grow(T *&ptr, size_t &have, size_t need) {
  if (have >= need) return 0;
  if (ptr) HIPCHK(hipFree(ptr));
  ptr = nullptr; have = 0;
  const hipError_t e = hipMalloc(&ptr, need * sizeof(T));
  if (e != hipSuccess) { snprintf(g_err, sizeof g_err, "scratch hipMalloc(%zu bytes): %s", need * sizeof(T), hipGetErrorString(e)); return ASCENT_E_NOMEM; }
  have = need;
  return 0;
}

int check_device(int device_id) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { snprintf(g_err, sizeof g_err, "no HIP device available"); return ASCENT_E_NODEVICE; }
  if (device_id < 0 || device_id >= n || device_id >= MAX_DEV) { snprintf(g_err, sizeof g_err, "device %d of %d", device_id, n); return ASCENT_E_NODEVICE; }
  return 0;
}

int check_options(const ascent_params *p, int64_t batch, const ascent_opts *o) {
  if (!p || !o || batch <= 0) { snprintf(g_err, sizeof g_err, "null params/opts or batch <= 0"); return ASCENT_E_ARG; }
  if (o->n_nodes < 3 || o->n_nodes > 65536) { snprintf(g_err, sizeof g_err, "n_nodes out of range (3 .. 65536)"); return ASCENT_E_ARG; }
  if (o->formulation != 0 && o->formulation != 1) { snprintf(g_err, sizeof g_err, "formulation %d not supported (0 = current script, 1 = v1 script)", o->formulation); return ASCENT_E_ARG; }
  if (o->formulation == 1 && o->scheme != 0 && o->scheme != 2) { snprintf(g_err, sizeof g_err, "formulation 1 is available with scheme 0 only"); return ASCENT_E_ARG; }
  if (o->coarse_nodes != -1 && o->coarse_nodes != 0 && (o->coarse_nodes < 3 || o->coarse_nodes >= o->n_nodes)) { snprintf(g_err, sizeof g_err, "coarse_nodes must be -1 (off), 0 (automatic) or in [3, n_nodes)"); return ASCENT_E_ARG; }
  if (o->scheme < 0 || o->scheme > 2) { snprintf(g_err, sizeof g_err, "scheme %d not supported (0 = backward Euler, the reference's NODES=2; 1 = trapezoid; 2 = Hermite-Simpson)", o->scheme); return ASCENT_E_ARG; }
  if (o->terminal < 0 || o->terminal > 2) { snprintf(g_err, sizeof g_err, "terminal %d not supported (0 = reference, 1 = periapsis of the ellipse, 2 = anywhere on the ellipse)", o->terminal); return ASCENT_E_ARG; }
  if (o->terminal == 2 && o->formulation != 0) { snprintf(g_err, sizeof g_err, "terminal 2 has formulation 0 only"); return ASCENT_E_ARG; }
  if (o->solver_path != ASCENT_PATH_AUTO && o->solver_path != ASCENT_PATH_DENSE) { snprintf(g_err, sizeof g_err, "solver_path must be 0 (automatic) or ASCENT_PATH_DENSE"); return ASCENT_E_ARG; }
  if ((o->scheme == 2 || o->solver_path == ASCENT_PATH_DENSE) && o->formulation != 0) { snprintf(g_err, sizeof g_err, "the dense-block path (scheme 2 / ASCENT_PATH_DENSE) has formulation 0 only"); return ASCENT_E_ARG; }
  if (o->move_penalty && o->formulation != 0 && (o->scheme != 0 || o->solver_path == ASCENT_PATH_DENSE)) { snprintf(g_err, sizeof g_err, "move_penalty = 1 with formulation 1: scheme 0, persistent kernel only"); return ASCENT_E_ARG; }
  if (o->move_penalty != 0 && o->move_penalty != 1) { snprintf(g_err, sizeof g_err, "move_penalty must be 0 or 1"); return ASCENT_E_ARG; }
  return 0;
}
// move_penalty = 1 on host-resident parameter sets: every weight must be positive
int check_dcost(const ascent_params *p, int64_t batch) {
  for (int64_t i = 0; i < batch; i++)
    if (!(p[i].dcost > 0.0)) { snprintf(g_err, sizeof g_err, "move_penalty = 1 needs ascent_params.dcost > 0 (problem %lld has %g)", (long long)i, p[i].dcost); return ASCENT_E_ARG; }
  return 0;
}

// workspace of one grid level of K intervals on the routed family
size_t ws_bytes(const Route &r, int K, int64_t batch, int mp) {
  switch (r.path) {
    case ASCENT_PATH_PERSIST: return persist_ws_bytes(K, (long)batch, mp);
    case ASCENT_PATH_DENSE: return r.pcr ? dense_pcr_ws_bytes(K, (long)batch) : dense_ws_bytes(K, (long)batch);
    case ASCENT_PATH_FUSED: return fused_ws_bytes(K, (long)batch);
    default: return pipeline_ws_bytes(K, (long)batch);
  }
}

// What ascent_solve_batch can solve for this batch, for every entry point that takes a solve's options: the route of the
// solve, what its family does not carry, and (host-resident parameter sets only) the weights of the move penalty.
int check_solvable(const ascent_params *p, int64_t batch, const ascent_opts *o, int ptr_is_device, Route *route_out = nullptr) {
  const Route r = route(o, batch, ASCENT_PATH_AUTO, false);
  if (const char *why = unsupported(r.path, o)) { snprintf(g_err, sizeof g_err, "%s", why); return ASCENT_E_ARG; }
  // (device-resident parameter sets are not read here: p_init / d_init refuse a bad weight per problem, ASCENT_INVALID_PROBLEM)
  if (o->move_penalty && !ptr_is_device) if (const int rc = check_dcost(p, batch)) return rc;
  if (route_out) *route_out = r;
  return 0;
}

Call call_of(const ascent_params *dp, int64_t batch, const ascent_opts *o, hipStream_t stream) {
  return ascent::call_of(dp, (long)batch, o, stream, g_err, sizeof g_err);
}

// Device copies of the arrays of a host-pointer call, freed when the call returns.  With device pointers every member hands
// its argument back.  The first failure is kept: ask failed() before launching on what in / out / scratch returned.
class Staging {
 public:
  Staging(hipStream_t stream, int ptr_is_device) : stream_(stream), device_(ptr_is_device != 0) {}
  ~Staging() { for (void *d : owned_) (void)hipFree(d); }
  Staging(const Staging &) = delete;
  Staging &operator=(const Staging &) = delete;
  template <typename T>
  T *scratch(size_t n) {      // device memory of this call, neither copied in nor out
    void *d = nullptr;
    if (rc_ || note(hipMalloc(&d, n * sizeof(T)), "staging hipMalloc")) return nullptr;
    owned_.push_back(d);
    return (T *)d;
  }
  template <typename T>
  const T *in(const T *p, size_t n) {      // the copy is enqueued on the stream
    if (device_ || !p) return p;
    T *d = scratch<T>(n);
    if (d) note(hipMemcpyAsync(d, p, n * sizeof(T), hipMemcpyHostToDevice, stream_), "staging hipMemcpyAsync");
    return d;
  }
  template <typename T>
  T *out(T *p, size_t n) {      // null stays null: an optional output the caller did not ask for
    if (device_ || !p) return p;
    T *d = scratch<T>(n);
    if (d) outs_.push_back({p, d, n * sizeof(T)});
    return d;
  }
  int failed() const { return rc_; }
  // Host pointers: the outputs back in the order they were registered, then wait for the stream.  Device pointers: the call
  // stays asynchronous on a caller's stream; the null stream is waited for.
  int finish() {
    if (rc_) return rc_;
    for (const Out &o : outs_) HIPCHK(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, stream_));
    if (!device_ || !stream_) HIPCHK(hipStreamSynchronize(stream_));
    return ASCENT_OK;
  }

 private:
  struct Out { void *host, *dev; size_t bytes; };
  int note(hipError_t e, const char *what) {
    if (e != hipSuccess) { snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e)); rc_ = ASCENT_E_HIP; }
    return rc_;
  }
  hipStream_t stream_;
  bool device_;
  int rc_ = 0;
  std::vector<void *> owned_;
  std::vector<Out> outs_;
};

}  // namespace

// grid levels of the nested iteration, finest first (levels[0] = n_nodes); one level = a plain solve
static int nested_levels(const ascent_opts *o, int *levels) {
  int nlev = 1;
  levels[0] = o->n_nodes;
  if (o->warm_start == 0 && o->coarse_nodes != -1) {
    if (o->coarse_nodes > 0) {
      levels[nlev++] = o->coarse_nodes;
    } else {
      for (int n = o->n_nodes; n >= NESTED_MIN_NODES && nlev < 8;) {
        const int c = coarse_of(n);
        if (c >= n) break;
        levels[nlev++] = c;
        n = c;
      }
    }
  }
  return nlev;
}

extern "C" {

#ifdef ASCENT_PROFILE
int ascent_debug_profile(unsigned long long *out8, int reset) {
  unsigned long long z[8] = {0};
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_prof), sizeof z) != hipSuccess) return -1;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof z) != hipSuccess) return -1;
  return 0;
}
#endif

int ascent_version(void) { return 300; }

int ascent_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *ascent_strerror(int code) {
  switch (code) {
    case ASCENT_OK: return "ok";
    case ASCENT_E_ARG: case ASCENT_E_HIP: case ASCENT_E_NODEVICE: case ASCENT_E_NOMEM: case ASCENT_E_NOTERM:
      return g_err[0] ? g_err : "error";
    default: return "unknown error code";
  }
}

double ascent_last_kernel_ms(int device_id) {
  if (device_id < 0 || device_id >= MAX_DEV) return -1.0;
  std::lock_guard<std::mutex> lock(g_mu[device_id]);
  DeviceWs &w = g_wss[device_id][g_ws_last[device_id]];
  if (!w.launched) return -1.0;
  if (hipSetDevice(device_id) != hipSuccess) return -1.0;
  if (hipEventSynchronize(w.ev1) != hipSuccess) return -1.0;
  float ms = -1.f;
  if (hipEventElapsedTime(&ms, w.ev0, w.ev1) != hipSuccess) return -1.0;
  return ms;
}

int ascent_solve_batch(const ascent_params *p, int64_t batch, const ascent_opts *o,
                       const double *guess, double *traj_out, double *tf_out, int32_t *status_out,
                       int32_t *iters_out, double *sol_blob_out, int device_id, void *stream_,
                       int ptr_is_device) {
  int rc = check_options(p, batch, o);
  if (rc) return rc;
  if (!tf_out || !status_out || !iters_out) { snprintf(g_err, sizeof g_err, "null output pointer"); return ASCENT_E_ARG; }
  if (o->warm_start < 0 || o->warm_start > 2 || (o->warm_start && !guess)) { snprintf(g_err, sizeof g_err, "warm_start needs a guess blob"); return ASCENT_E_ARG; }
  if (!(o->tol > 0) || o->max_iter < 0) { snprintf(g_err, sizeof g_err, "tol must be > 0, max_iter >= 0"); return ASCENT_E_ARG; }
  Route r{};
  if ((rc = check_solvable(p, batch, o, ptr_is_device, &r))) return rc;
  if ((rc = check_device(device_id))) return rc;
  std::lock_guard<std::mutex> lock(g_mu[device_id]);
  HIPCHK(hipSetDevice(device_id));
  hipStream_t stream = (hipStream_t)stream_;
  const int K = o->n_nodes - 1, nt = o->n_nodes;
  const size_t rows = 21 * (size_t)K + NSC;
  const bool persist = r.path == ASCENT_PATH_PERSIST;
  int levels[8];
  const int nlev = nested_levels(o, levels);
  const int slot = slot_for(device_id, stream);
  DeviceWs &w = g_wss[device_id][slot];
  g_ws_last[device_id] = slot;
  rc = ensure_ws(w, persist ? persist_ws_bytes_nested(levels, nlev, (long)batch, (int)o->move_penalty) : ws_bytes(r, K, batch, (int)o->move_penalty));
  if (rc) return rc;
  const double mu0 = o->mu_init > 0 ? o->mu_init : (o->warm_start ? 1e-4 : 0.1);

  const ascent_params *dp = p;
  const double *dguess = guess;
  double *dtraj = traj_out, *dtf = tf_out, *dblob = sol_blob_out;
  int *dstatus = status_out, *diters = iters_out;
  // a predecessor on this device may still be executing on another stream: it owns the workspace until its last kernel
  if (w.launched) HIPCHK(hipStreamWaitEvent(stream, w.ev1, 0));
  if (!ptr_is_device) {
    if ((rc = grow(w.h_p, w.h_p_n, (size_t)batch))) return rc;
    HIPCHK(hipMemcpyAsync(w.h_p, p, batch * sizeof(ascent_params), hipMemcpyHostToDevice, stream));
    dp = w.h_p;
    if (o->warm_start) {
      if ((rc = grow(w.h_guess, w.h_guess_n, rows * batch))) return rc;
      HIPCHK(hipMemcpyAsync(w.h_guess, guess, rows * batch * sizeof(double), hipMemcpyHostToDevice, stream));
      dguess = w.h_guess;
    }
    if (traj_out) { if ((rc = grow(w.h_traj, w.h_traj_n, (size_t)10 * nt * batch))) return rc; dtraj = w.h_traj; }
    if (sol_blob_out) { if ((rc = grow(w.h_blob, w.h_blob_n, rows * batch))) return rc; dblob = w.h_blob; }
    if ((rc = grow(w.h_tf, w.h_tf_n, (size_t)batch))) return rc;
    dtf = w.h_tf;
    if ((rc = grow(w.h_status, w.h_status_n, (size_t)batch))) return rc;
    dstatus = w.h_status;
    if ((rc = grow(w.h_iters, w.h_iters_n, (size_t)batch))) return rc;
    diters = w.h_iters;
  }
  if (o->terminal == 1) {
    if ((rc = grow(w.t_p, w.t_p_n, (size_t)batch))) return rc;
    hipLaunchKernelGGL(k_terminal_params, dim3((unsigned)((batch + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, dp, w.t_p, (long)batch);
    HIPCHK(hipGetLastError());
    dp = w.t_p;
  }
  if (nlev > 1 && !persist) {
    size_t n3 = w.int_n, n3b = w.int_n, n3c = w.int_n, ntf = w.int_n;
    rc = grow(w.sol, w.sol_n, (21 * (size_t)(levels[1] - 1) + NSC) * batch);
    if (!rc) rc = grow(w.gss, w.gss_n, rows * batch);
    if (!rc) rc = grow(w.st_c, n3, (size_t)batch);
    if (!rc) rc = grow(w.it_c, n3b, (size_t)batch);
    if (!rc) rc = grow(w.acc, n3c, (size_t)batch);
    if (!rc) rc = grow(w.tfc, ntf, (size_t)batch);
    if (rc) return rc;
    w.int_n = n3;
  }
  HIPCHK(hipEventRecord(w.ev0, stream));
  double mu_first = o->move_penalty ? NESTED_MU_FIRST_MP : NESTED_MU_FIRST, mu_next = o->move_penalty ? nested_mu_next_mp(o->tol) : nested_mu_next(o->tol);
  if (const char *e = getenv("ASCENT_NESTED_MU")) sscanf(e, "%lf,%lf", &mu_first, &mu_next);      // experiments only ("first,next")
  const Call c = call_of(dp, batch, o, stream);
  const double tol_coarse = fmax(o->tol, NESTED_COARSE_TOL);
  if (persist) {      // all levels inside the kernel's own layout
    const SolveIO io{dguess, (int)o->warm_start, (int)o->max_iter, o->tol, mu0, dtraj, dtf, dstatus, diters, dblob};
    if ((rc = persist_run_nested(c, r.wide, levels, nlev, w.ws, io, tol_coarse, mu_first, mu_next))) return rc;
  }
  for (int l = nlev - 1; l >= 0 && !persist; l--) {
    const bool fin = l == 0, first = l == nlev - 1;
    Call cl = c;
    cl.K = levels[l] - 1;
    const SolveIO io{first ? dguess : w.gss, first ? (int)o->warm_start : 2, (int)o->max_iter, fin ? o->tol : tol_coarse,
                     first ? mu0 : (l == nlev - 2 ? mu_first : mu_next), fin ? dtraj : nullptr, fin ? dtf : w.tfc,
                     fin ? dstatus : w.st_c, fin ? diters : w.it_c, fin ? dblob : w.sol};
    switch (r.path) {
      case ASCENT_PATH_DENSE: rc = dense_run(cl, w.ws, io, r.pcr); break;
      case ASCENT_PATH_FUSED: rc = fused_run(cl, w.ws, io); break;
      default: rc = pipeline_run(cl, w.ws, io, r.path == ASCENT_PATH_SPLIT_WIDE, nullptr);
    }
    if (rc) return rc;
    if (!fin) {
      const int Kf = levels[l - 1] - 1;
      hipLaunchKernelGGL(k_prolong, dim3((unsigned)((batch + WAVE - 1) / WAVE), (unsigned)Kf), dim3(WAVE), 0, stream, w.sol,
                         w.st_c, w.it_c, cl.K, w.gss, Kf, (long)batch, (int)o->formulation, w.acc, first ? 1 : 0);
      HIPCHK(hipGetLastError());
    }
  }
  if (nlev > 1 && !persist) {
    hipLaunchKernelGGL(k_add_iters, dim3((unsigned)((batch + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, diters, w.acc, (long)batch);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(w.ev1, stream));
  w.launched = true;
  if (!ptr_is_device) {
    if (traj_out) HIPCHK(hipMemcpyAsync(traj_out, dtraj, (size_t)10 * nt * batch * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (sol_blob_out) HIPCHK(hipMemcpyAsync(sol_blob_out, dblob, rows * batch * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(tf_out, dtf, batch * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(status_out, dstatus, batch * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(iters_out, diters, batch * sizeof(int), hipMemcpyDeviceToHost, stream));
  }
  if (!ptr_is_device || !stream) HIPCHK(hipStreamSynchronize(stream));
  return ASCENT_OK;
}

int ascent_workspace_layout(int64_t batch, const ascent_opts *o, int64_t *out4) {
  if (!o || !out4 || batch <= 0 || o->n_nodes < 3) return ASCENT_E_ARG;
  int levels[8];
  const int nlev = nested_levels(o, levels), mp = (int)o->move_penalty;
  out4[0] = (int64_t)persist_ws_bytes_nested(levels, nlev, (long)batch, mp);
  out4[1] = (int64_t)persist_level_bytes_used(levels[0] - 1, (long)batch, mp);
  out4[2] = nlev > 1 ? (int64_t)persist_region1_offset(levels, (long)batch, mp) : 0;
  out4[3] = nlev > 1 ? (int64_t)persist_level_bytes_used(levels[1] - 1, (long)batch, mp) : 0;
  return nlev;
}

int ascent_default_path(int64_t batch, const ascent_opts *o) {
  if (!o || batch <= 0) return ASCENT_E_ARG;
  return route(o, batch, ASCENT_PATH_AUTO, false).path;
}

int ascent_eval_nodes_path(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *iterate,
                           double *defects, double *jac_blocks, double *hess_blocks, int device_id, int path) {
  int rc = check_options(p, batch, o);
  if (rc) return rc;
  if (o->move_penalty) { snprintf(g_err, sizeof g_err, "the parity surfaces take the unpenalised NLP only (move_penalty = 1 is an option of ascent_solve_batch)"); return ASCENT_E_ARG; }
  if (!iterate || !defects || !jac_blocks || !hess_blocks) { snprintf(g_err, sizeof g_err, "null pointer"); return ASCENT_E_ARG; }
  if (path < ASCENT_PATH_AUTO || path > ASCENT_PATH_PERSIST) { snprintf(g_err, sizeof g_err, "unknown path %d", path); return ASCENT_E_ARG; }
  const Route r = route(o, batch, path, true);
  if (r.path == ASCENT_PATH_DENSE) { snprintf(g_err, sizeof g_err, "the dense-block path exposes its node evaluation through ascent_dense_records"); return ASCENT_E_ARG; }
  if (o->scheme == 2) { snprintf(g_err, sizeof g_err, "the node evaluation of scheme 2 is exposed through ascent_dense_records"); return ASCENT_E_ARG; }
  ascent_opts rows_o = *o;
  rows_o.terminal = 0;      // (the node rows do not see the terminal condition)
  if (const char *why = unsupported(r.path, &rows_o)) { snprintf(g_err, sizeof g_err, "%s", why); return ASCENT_E_ARG; }
  if ((rc = check_device(device_id))) return rc;
  std::lock_guard<std::mutex> lock(g_mu[device_id]);
  HIPCHK(hipSetDevice(device_id));
  if ((rc = claim_slot0(device_id))) return rc;
  const int K = o->n_nodes - 1;
  Staging st(nullptr, 0);
  const Call c = call_of(st.in(p, (size_t)batch), batch, &rows_o, nullptr);
  ProbeIO io{};
  io.iterate = st.in(iterate, (21 * (size_t)K + NSC) * batch);
  io.defects = st.out(defects, (size_t)7 * K * batch);
  io.jac = st.out(jac_blocks, (size_t)8 * K * batch);
  io.hess = st.out(hess_blocks, (size_t)10 * K * batch);
  double *ws = nullptr;
  if (r.path != ASCENT_PATH_FUSED) {      // (k_eval_nodes needs no workspace)
    if ((rc = ensure_ws(g_ws_slot0(device_id), ws_bytes(r, K, batch, 0)))) return rc;
    ws = g_ws_slot0(device_id).ws;
    double *zero = st.scratch<double>((size_t)batch);      // mu, delta_w: not used by the node evaluation
    if (zero) HIPCHK(hipMemset(zero, 0, batch * sizeof(double)));
    io.mu = io.dw = zero;
  }
  if ((rc = st.failed())) return rc;
  switch (r.path) {
    case ASCENT_PATH_FUSED: rc = fused_eval_nodes(c, io); break;
    case ASCENT_PATH_PERSIST: rc = persist_probe_rows(c, r.wide, ws, io); break;
    default: rc = pipeline_probe(c, ws, io, r.path == ASCENT_PATH_SPLIT_WIDE);
  }
  return rc ? rc : st.finish();
}

int ascent_eval_nodes(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *iterate,
                      double *defects, double *jac_blocks, double *hess_blocks, int device_id) {
  return ascent_eval_nodes_path(p, batch, o, iterate, defects, jac_blocks, hess_blocks, device_id, ASCENT_PATH_AUTO);
}

// ascent_opts.terminal = 1 on a parity surface: in place on the call's private copy of the parameters
static int terminal_params_in_place(const ascent_opts *o, const ascent_params *dp, int64_t batch) {
  if (o->terminal != 1) return 0;
  hipLaunchKernelGGL(k_terminal_params, dim3((unsigned)((batch + WAVE - 1) / WAVE)), dim3(WAVE), 0, 0, dp, const_cast<ascent_params *>(dp), (long)batch);
  HIPCHK(hipGetLastError());
  return 0;
}

int ascent_kkt_step_path(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *iterate,
                         const double *mu, const double *delta_w, double *step, int32_t *inertia_out, int device_id,
                         int path) {
  int rc = check_options(p, batch, o);
  if (rc) return rc;
  if (!iterate || !mu || !delta_w || !step || !inertia_out) { snprintf(g_err, sizeof g_err, "null pointer"); return ASCENT_E_ARG; }
  if (path < ASCENT_PATH_AUTO || path > ASCENT_PATH_PERSIST) { snprintf(g_err, sizeof g_err, "unknown path %d", path); return ASCENT_E_ARG; }
  const Route r = route(o, batch, path, true);
  if (const char *why = unsupported(r.path, o)) { snprintf(g_err, sizeof g_err, "%s", why); return ASCENT_E_ARG; }
  if (o->move_penalty && (rc = check_dcost(p, batch))) return rc;
  if ((rc = check_device(device_id))) return rc;
  std::lock_guard<std::mutex> lock(g_mu[device_id]);
  HIPCHK(hipSetDevice(device_id));
  if ((rc = claim_slot0(device_id))) return rc;
  const int K = o->n_nodes - 1;
  const size_t rows = 21 * (size_t)K + NSC;
  if ((rc = ensure_ws(g_ws_slot0(device_id), ws_bytes(r, K, batch, (int)o->move_penalty)))) return rc;
  double *ws = g_ws_slot0(device_id).ws;
  Staging st(nullptr, 0);
  const Call c = call_of(st.in(p, (size_t)batch), batch, o, nullptr);
  ProbeIO io{};
  io.iterate = st.in(iterate, rows * batch);
  io.mu = st.in(mu, (size_t)batch);
  io.dw = st.in(delta_w, (size_t)batch);
  io.step = st.out(step, rows * batch);
  io.inertia = st.out(inertia_out, (size_t)batch);
  if ((rc = st.failed())) return rc;
  HIPCHK(hipMemset(io.step, 0, rows * batch * sizeof(double)));
  if ((rc = terminal_params_in_place(o, c.dp, batch))) return rc;
  switch (r.path) {
    case ASCENT_PATH_DENSE: rc = dense_probe(c, ws, io, r.pcr); break;
    case ASCENT_PATH_PERSIST: rc = persist_probe(c, r.wide, ws, io); break;
    case ASCENT_PATH_FUSED: rc = fused_probe(c, ws, io); break;
    default: rc = pipeline_probe(c, ws, io, r.path == ASCENT_PATH_SPLIT_WIDE);
  }
  if (rc || (rc = st.finish())) return rc;
  for (int64_t q = 0; q < batch; q++) inertia_out[q] = inertia_out[q] != 0;     // (the dense path reports a status code)
  return ASCENT_OK;
}

int ascent_dense_records(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *iterate,
                         double *records, int device_id) {
  int rc = check_options(p, batch, o);
  if (rc) return rc;
  if (o->move_penalty) { snprintf(g_err, sizeof g_err, "the parity surfaces take the unpenalised NLP only (move_penalty = 1 is an option of ascent_solve_batch)"); return ASCENT_E_ARG; }
  if (!iterate || !records) { snprintf(g_err, sizeof g_err, "null pointer"); return ASCENT_E_ARG; }
  if (const char *why = unsupported(ASCENT_PATH_DENSE, o)) { snprintf(g_err, sizeof g_err, "%s", why); return ASCENT_E_ARG; }
  if ((rc = check_device(device_id))) return rc;
  std::lock_guard<std::mutex> lock(g_mu[device_id]);
  HIPCHK(hipSetDevice(device_id));
  if ((rc = claim_slot0(device_id))) return rc;
  const int K = o->n_nodes - 1;
  if ((rc = ensure_ws(g_ws_slot0(device_id), dense_ws_bytes(K, (long)batch)))) return rc;
  Staging st(nullptr, 0);
  Call c = call_of(st.in(p, (size_t)batch), batch, o, nullptr);
  c.term = 0;      // (the stage records do not see the terminal condition)
  ProbeIO io{};
  io.iterate = st.in(iterate, (21 * (size_t)K + NSC) * batch);
  io.records = st.out(records, (size_t)batch * K * 6 * 64);
  double *zero = st.scratch<double>((size_t)batch);      // mu, delta_w: not used by the records
  if ((rc = st.failed())) return rc;
  HIPCHK(hipMemset(zero, 0, batch * sizeof(double)));
  io.mu = io.dw = zero;
  if ((rc = terminal_params_in_place(o, c.dp, batch))) return rc;
  if ((rc = dense_probe(c, g_ws_slot0(device_id).ws, io, false))) return rc;
  return st.finish();
}

int ascent_coast_batch(const ascent_params *p, int64_t batch, const double *final_state, int32_t coast_nodes,
                       double *coast_traj, double *coast_tf, double *apsides, int device_id, void *stream_,
                       int ptr_is_device) {
  if (!p || batch <= 0 || !final_state || !coast_traj || !coast_tf || !apsides) { snprintf(g_err, sizeof g_err, "null pointer or batch <= 0"); return ASCENT_E_ARG; }
  if (coast_nodes < 1 || coast_nodes > 65535) { snprintf(g_err, sizeof g_err, "coast_nodes out of range (1 .. 65535)"); return ASCENT_E_ARG; }
  int rc = check_device(device_id);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(g_mu[device_id]);
  HIPCHK(hipSetDevice(device_id));
  hipStream_t stream = (hipStream_t)stream_;
  Staging st(stream, ptr_is_device);
  const Call c = call_of(st.in(p, (size_t)batch), batch, nullptr, stream);
  const double *ds = st.in(final_state, (size_t)4 * batch);
  double *dc = st.out(coast_traj, (size_t)4 * (coast_nodes + 1) * batch), *dt = st.out(coast_tf, (size_t)batch), *da = st.out(apsides, (size_t)2 * batch);
  if ((rc = st.failed()) || (rc = coast_run(c, ds, coast_nodes, dc, dt, da))) return rc;
  return st.finish();
}

// ---------------------------------------------------------------------------------------------
// The calls on a solution blob after the solve: sensitivity, flight, flight Jacobian, trim, dispersion, guidance gains.
//
// All but the first two work in the analysis workspace of the device: one buffer per device, apart from the solver's.  A call on
// another stream than its predecessor waits for the predecessor's last kernel (an event) before it reuses the buffer; growing it
// frees the old one, which waits for the device.
// ---------------------------------------------------------------------------------------------
namespace {
struct AnalysisWs { double *ws = nullptr; size_t bytes = 0; hipEvent_t ev = nullptr; bool used = false; };
AnalysisWs g_analysis_ws[MAX_DEV];

int analysis_ws_claim(int dev, size_t bytes, hipStream_t stream, double **out) {      // (under g_mu[dev])
  AnalysisWs &w = g_analysis_ws[dev];
  if (!w.ev) HIPCHK(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
  if (w.bytes < bytes) {
    if (w.ws) HIPCHK(hipFree(w.ws));
    w.ws = nullptr; w.bytes = 0;
    const hipError_t e = hipMalloc(&w.ws, bytes);
    if (e != hipSuccess) { snprintf(g_err, sizeof g_err, "workspace hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); return ASCENT_E_NOMEM; }
    w.bytes = bytes;
  } else if (w.used) {
    HIPCHK(hipStreamWaitEvent(stream, w.ev, 0));
  }
  *out = w.ws;
  return 0;
}
int analysis_ws_release(int dev, hipStream_t stream) {
  AnalysisWs &w = g_analysis_ws[dev];
  HIPCHK(hipEventRecord(w.ev, stream));
  w.used = true;
  return 0;
}

int check_substeps(int32_t substeps) {
  if (substeps < 0 || substeps > ASCENT_FLIGHT_MAX_SUBSTEPS) { snprintf(g_err, sizeof g_err, "substeps out of range (0 = automatic, 1 .. %d)", ASCENT_FLIGHT_MAX_SUBSTEPS); return ASCENT_E_ARG; }
  return 0;
}
int check_samples(int32_t samples) {
  if (samples < 1 || samples > ASCENT_DISPERSE_MAX_SAMPLES) { snprintf(g_err, sizeof g_err, "samples out of range (1 .. %d)", ASCENT_DISPERSE_MAX_SAMPLES); return ASCENT_E_ARG; }
  return 0;
}

// What the ten entry points below share, in the order their defects have always been reported.  An entry point puts its own
// null and range checks between the steps, then names its buffers (st.in / st.out) and its run function:
//   options()               check_options
//   solvable()              check_solvable
//   flight_like(substeps)   both, and between them: the blob, the substep range, terminal 2 refused
//   open(device_id, bytes)  the device, its lock, the analysis workspace (bytes > 0), the Call and the staged blob
//   close()                 after the run function: the workspace released and the staging finished
class BlobCall {
 public:
  BlobCall(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, void *stream, int ptr_is_device)
      : p_(p), batch_(batch), o_(o), blob_(sol_blob), device_(ptr_is_device), stream_((hipStream_t)stream), st(stream_, ptr_is_device) {}
  int options() { return check_options(p_, batch_, o_); }
  int solvable() { return check_solvable(p_, batch_, o_, device_); }
  int flight_like(int32_t substeps) {      // what ascent_fly_batch refuses, plus terminal = 2
    int rc = options();
    if (rc) return rc;
    if (!blob_) { snprintf(g_err, sizeof g_err, "null solution blob"); return ASCENT_E_ARG; }
    if ((rc = check_substeps(substeps))) return rc;
    if (o_->terminal == 2) { snprintf(g_err, sizeof g_err, "terminal 2 is not supported by the flight Jacobian and the trim (its two conditions are nearly dependent where burnout sits at an apsis)"); return ASCENT_E_ARG; }
    return solvable();
  }
  int open(int device_id, size_t ws_bytes) {
    int rc = check_device(device_id);
    if (rc) return rc;
    dev_ = device_id;
    lock_ = std::unique_lock<std::mutex>(g_mu[dev_]);
    HIPCHK(hipSetDevice(dev_));
    K = o_->n_nodes - 1;
    if (ws_bytes && (rc = analysis_ws_claim(dev_, ws_bytes, stream_, &ws))) return rc;
    c = call_of(st.in(p_, (size_t)batch_), batch_, o_, stream_);
    blob = st.in(blob_, (21 * (size_t)K + NSC) * batch_);
    return 0;
  }
  int close() {
    if (ws)
      if (const int rc = analysis_ws_release(dev_, stream_)) return rc;
    return st.finish();
  }

 private:
  const ascent_params *p_;
  int64_t batch_;
  const ascent_opts *o_;
  const double *blob_;
  int device_, dev_ = -1;
  hipStream_t stream_;
  std::unique_lock<std::mutex> lock_;      // declared before st: the staging frees its copies while the device is still locked

 public:
  Staging st;
  Call c{};
  int K = 0;
  const double *blob = nullptr;      // the staged solution blob
  double *ws = nullptr;              // the analysis workspace, where the call claimed one
};

// The refusals ascent_disperse_history_batch and ascent_covariance_history_batch share beyond BlobCall's, each with its one text:
// the knowledge row without a feed-forward, and the history nodes with what needs gain_u (guided: any such argument was given)
int check_ff_know(const double *ff_know, const double *ff_u) {
  if (ff_know && !ff_u) { snprintf(g_err, sizeof g_err, "ff_know needs ff_u"); return ASCENT_E_ARG; }
  return 0;
}
int check_history_nodes(const ascent_opts *o, int32_t node_stride, const double *gain_u, bool guided) {
  if (node_stride < 1 || node_stride > o->n_nodes - 1) { snprintf(g_err, sizeof g_err, "node_stride out of range (1 .. K = %d)", o->n_nodes - 1); return ASCENT_E_ARG; }
  if (!gain_u && guided) {
    snprintf(g_err, sizeof g_err, "gain_t, stretch_max, ff_u, ff_t, ff_know, xi_nav and sigma_nav need gain_u");
    return ASCENT_E_ARG;
  }
  return 0;
}

// The refusals ascent_disperse_drifting_batch and ascent_covariance_drifting_batch add to their parents': phi and q together and
// with gain_u, the draws (monte_carlo) with q, and with host pointers every phi in [0, 1] and every q >= 0 and finite
int check_drift(const double *nav_phi, const double *nav_q, const double *xi_drift, bool monte_carlo, const double *gain_u, int64_t batch,
                int ptr_is_device) {
  if ((nav_phi != nullptr) != (nav_q != nullptr)) { snprintf(g_err, sizeof g_err, "nav_phi and nav_q come together"); return ASCENT_E_ARG; }
  if (nav_phi && !gain_u) { snprintf(g_err, sizeof g_err, "nav_phi and nav_q need gain_u"); return ASCENT_E_ARG; }
  if (monte_carlo && nav_q && !xi_drift) { snprintf(g_err, sizeof g_err, "nav_q needs xi_drift"); return ASCENT_E_ARG; }
  if (nav_phi && !ptr_is_device) {
    for (int64_t i = 0; i < ASCENT_NAV_ROWS * batch; i++) {
      if (!(nav_phi[i] >= 0.0 && nav_phi[i] <= 1.0)) { snprintf(g_err, sizeof g_err, "nav_phi outside [0, 1] (channel %d, problem %lld)", (int)(i / batch), (long long)(i % batch)); return ASCENT_E_ARG; }
      if (!(nav_q[i] >= 0.0 && std::isfinite(nav_q[i]))) { snprintf(g_err, sizeof g_err, "nav_q negative or not finite (channel %d, problem %lld)", (int)(i / batch), (long long)(i % batch)); return ASCENT_E_ARG; }
    }
  }
  return 0;
}

// What ascent_sample_quantiles and ascent_disperse_quantiles_batch refuse of the arguments they share
int check_probs(const double *probs, int32_t n_probs) {
  if (!probs) { snprintf(g_err, sizeof g_err, "null probs"); return ASCENT_E_ARG; }
  if (n_probs < 1 || n_probs > QUANTILE_MAX_PROBS) { snprintf(g_err, sizeof g_err, "n_probs out of range (1 .. %d)", QUANTILE_MAX_PROBS); return ASCENT_E_ARG; }
  for (int j = 0; j < n_probs; j++)
    if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) { snprintf(g_err, sizeof g_err, "probability %d outside [0, 1] or not finite", j); return ASCENT_E_ARG; }
  return 0;
}
int check_limits(const double *limits, const double *below, int32_t n_limits, const char *lname, const char *bname) {
  if ((limits != nullptr) != (below != nullptr)) { snprintf(g_err, sizeof g_err, "%s and %s come together", lname, bname); return ASCENT_E_ARG; }
  if (limits && (n_limits < 1 || n_limits > QUANTILE_MAX_LIMITS)) { snprintf(g_err, sizeof g_err, "n_limits out of range (1 .. %d)", QUANTILE_MAX_LIMITS); return ASCENT_E_ARG; }
  return 0;
}

// The sample rows of ascent_disperse_quantiles_batch in the analysis workspace, behind what the flight needs: the twelve end
// rows, then the ten quantities at the NJ history nodes
size_t quantile_scratch_bytes(int K, int64_t batch, int32_t samples, int32_t node_stride) {
  const size_t nj = node_stride > 0 ? (size_t)history_nodes(K, node_stride) : 0;
  return (ASCENT_GUIDED_SAMPLE_ROWS + ASCENT_HISTORY_QUANTITIES * nj) * (size_t)samples * (size_t)batch * sizeof(double);
}

// The selection of ascent_disperse_quantiles_batch: the caller's pointers, staged by quantiles_behind
struct QuantileRequest {
  const double *probs;
  int n_probs;
  const double *limits, *hist_limits;
  int n_limits;
  double *quant, *below, *hist_quant, *hist_below;
};

// disperse_call's last step with a QuantileRequest: the flight's kernels with the sample rows directed to the workspace, then the
// selection over them (the counts are stats_out's and hist_out's rows 0 and are not written again; nothing is allocated, so with
// device pointers the call only enqueues).  The open-loop flight without history writes nine rows; the other three are zeroed here.
int quantiles_behind(BlobCall &b, DisperseKind kind, int substeps, int samples, DisperseIO io, bool history, size_t flight_bytes,
                     const QuantileRequest &qr) {
  Staging &st = b.st;
  const size_t B = (size_t)b.c.batch, S = (size_t)samples, NJ = history ? (size_t)history_nodes(b.K, io.node_stride) : 0;
  const size_t end = ASCENT_GUIDED_SAMPLE_ROWS * S * B;
  double *rows = b.ws + flight_bytes / sizeof(double);
  io.samples_out = rows;
  io.hist_samples = history && qr.hist_quant ? rows + end : nullptr;
  QuantileIO e{}, h{};
  e.values = rows; e.Q = ASCENT_GUIDED_SAMPLE_ROWS; e.G = 1; e.V = ASCENT_DISPERSE_ROWS; e.samples = samples; e.batch = b.c.batch;
  e.n_probs = qr.n_probs;
  for (int j = 0; j < qr.n_probs; j++) e.probs[j] = qr.probs[j];
  h = e;
  e.limits = st.in(qr.limits, (size_t)qr.n_limits * e.Q * B); e.n_limits = qr.n_limits;
  e.quant = st.out(qr.quant, (size_t)qr.n_probs * e.Q * B);
  e.below = st.out(qr.below, (size_t)qr.n_limits * e.Q * B);
  if (io.hist_samples) {
    h.values = io.hist_samples; h.Q = ASCENT_HISTORY_QUANTITIES; h.G = (int)NJ; h.V = ASCENT_HISTORY_QUANTITIES;
    h.limits = st.in(qr.hist_limits, (size_t)qr.n_limits * h.Q * B); h.n_limits = qr.n_limits;
    h.quant = st.out(qr.hist_quant, (size_t)qr.n_probs * h.Q * NJ * B);
    h.below = st.out(qr.hist_below, (size_t)qr.n_limits * h.Q * NJ * B);
  }
  int rc = st.failed();
  if (rc) return rc;
  if (kind == DISPERSE_OPEN && !history)
    HIPCHK(hipMemsetAsync(rows + ASCENT_DISPERSE_ROWS * S * B, 0, (ASCENT_GUIDED_SAMPLE_ROWS - ASCENT_DISPERSE_ROWS) * S * B * sizeof(double), b.c.stream));
  if ((rc = disperse_run(b.c, kind, substeps, samples, io, b.ws)) || (rc = quantile_run(e, b.c.stream, g_err, sizeof g_err))) return rc;
  if (io.hist_samples && (rc = quantile_run(h, b.c.stream, g_err, sizeof g_err))) return rc;
  return b.close();
}

// ascent_disperse_batch, ascent_disperse_guided_batch and ascent_disperse_navigated_batch: io holds the caller's pointers.
// history: ascent_disperse_history_batch, the kind picked from gain_u by the entry point; its own refusals stand after the
// refusals the three share, each of which keeps its place and its text.
int disperse_call(const ascent_params *p, int64_t batch, const ascent_opts *o, int32_t substeps, int32_t samples, DisperseKind kind,
                  DisperseIO io, int device_id, void *stream_, int ptr_is_device, bool history = false, bool drifting = false,
                  const QuantileRequest *qr = nullptr) {
  BlobCall b(p, batch, o, io.blob, stream_, ptr_is_device);
  int rc = b.options();
  if (rc) return rc;
  if (kind == DISPERSE_OPEN) {
    if (!io.blob || !io.xi || !io.sigma || !io.stats) { snprintf(g_err, sizeof g_err, "null solution blob, xi, sigma or stats_out"); return ASCENT_E_ARG; }
  } else if (!io.blob || !io.xi || !io.sigma || !io.gain_u || !io.stats) { snprintf(g_err, sizeof g_err, "null solution blob, xi, sigma, gain_u or stats_out"); return ASCENT_E_ARG; }
  if ((rc = check_samples(samples))) return rc;
  if ((io.xi_nav != nullptr) != (io.sigma_nav != nullptr)) { snprintf(g_err, sizeof g_err, "xi_nav and sigma_nav come together"); return ASCENT_E_ARG; }
  if ((rc = check_ff_know(io.ff_know, io.ff_u)) || (rc = check_substeps(substeps))) return rc;
  if (history) {
    if (!io.hist) { snprintf(g_err, sizeof g_err, "null hist_out"); return ASCENT_E_ARG; }
    if ((rc = check_history_nodes(o, io.node_stride, io.gain_u, io.gain_t || io.stretch_max || io.ff_u || io.ff_t || io.ff_know || io.xi_nav || io.sigma_nav))) return rc;
  }
  if ((rc = b.solvable())) return rc;
  if (drifting && (rc = check_drift(io.nav_phi, io.nav_q, io.xi_drift, true, io.gain_u, batch, ptr_is_device))) return rc;
  const size_t flight_bytes = disperse_ws_bytes(o->n_nodes - 1, (long)batch, samples, history ? io.node_stride : 0);
  if ((rc = b.open(device_id, flight_bytes + (qr ? quantile_scratch_bytes(o->n_nodes - 1, batch, samples, history ? io.node_stride : 0) : 0)))) return rc;
  Staging &st = b.st;
  const size_t K = (size_t)b.K, B = (size_t)batch, S = (size_t)samples;
  io.blob = b.blob;
  io.xi = st.in(io.xi, (ASCENT_DISPERSE_COLS + (io.sigma_u ? K : 0)) * S);
  io.sigma = st.in(io.sigma, ASCENT_DISPERSE_COLS * B);
  io.sigma_u = st.in(io.sigma_u, K * B);
  io.gain_u = st.in(io.gain_u, 7 * K * B);
  io.gain_t = st.in(io.gain_t, 7 * B);
  io.stretch_max = st.in(io.stretch_max, B);
  io.ff_u = st.in(io.ff_u, K * B);
  io.ff_t = st.in(io.ff_t, B);
  io.ff_know = st.in(io.ff_know, 16 * B);
  io.xi_nav = st.in(io.xi_nav, ASCENT_NAV_ROWS * S);
  io.sigma_nav = st.in(io.sigma_nav, ASCENT_NAV_ROWS * B);
  io.nav_phi = st.in(io.nav_phi, ASCENT_NAV_ROWS * B);
  io.nav_q = st.in(io.nav_q, ASCENT_NAV_ROWS * B);
  io.xi_drift = st.in(io.nav_q ? io.xi_drift : nullptr, ASCENT_NAV_ROWS * K * S);
  io.stats = st.out(io.stats, ASCENT_DISPERSE_STAT_ROWS * B);
  io.samples_out = st.out(io.samples_out, (kind == DISPERSE_OPEN && !history ? ASCENT_DISPERSE_ROWS : ASCENT_GUIDED_SAMPLE_ROWS) * S * B);
  if (history) {
    const size_t NJ = (size_t)history_nodes(b.K, io.node_stride);
    io.hist = st.out(io.hist, ASCENT_HISTORY_ROWS * NJ * B);
    io.hist_samples = st.out(io.hist_samples, ASCENT_HISTORY_QUANTITIES * NJ * S * B);
  }
  if (qr) return quantiles_behind(b, kind, substeps, samples, io, history, flight_bytes, *qr);
  if ((rc = b.st.failed()) || (rc = disperse_run(b.c, kind, substeps, samples, io, b.ws))) return rc;
  return b.close();
}

// ascent_covariance_history_batch: io holds the caller's pointers.  The order of the refusals is disperse_call's.
int lincov_call(const ascent_params *p, int64_t batch, const ascent_opts *o, int32_t substeps, LincovIO io, int device_id, void *stream_,
                int ptr_is_device, bool drifting = false) {
  BlobCall b(p, batch, o, io.blob, stream_, ptr_is_device);
  int rc = b.options();
  if (rc) return rc;
  if (!io.blob || !io.sigma || !io.nominal || !io.cov) { snprintf(g_err, sizeof g_err, "null solution blob, sigma, nominal_out or cov_out"); return ASCENT_E_ARG; }
  if ((rc = check_ff_know(io.ff_know, io.ff_u)) || (rc = check_substeps(substeps))) return rc;
  if ((rc = check_history_nodes(o, io.node_stride, io.gain_u, io.gain_t || io.stretch_max || io.ff_u || io.ff_t || io.ff_know || io.sigma_nav))) return rc;
  if ((rc = b.solvable())) return rc;
  if (drifting && (rc = check_drift(io.nav_phi, io.nav_q, nullptr, false, io.gain_u, batch, ptr_is_device))) return rc;
  if ((rc = b.open(device_id, lincov_ws_bytes(o->n_nodes - 1, (long)batch)))) return rc;
  Staging &st = b.st;
  const size_t K = (size_t)b.K, B = (size_t)batch, NJ = (size_t)history_nodes(b.K, io.node_stride);
  io.blob = b.blob;
  io.sigma = st.in(io.sigma, ASCENT_DISPERSE_COLS * B);
  io.sigma_u = st.in(io.sigma_u, K * B);
  io.gain_u = st.in(io.gain_u, 7 * K * B);
  io.gain_t = st.in(io.gain_t, 7 * B);
  io.stretch_max = st.in(io.stretch_max, B);
  io.ff_u = st.in(io.ff_u, K * B);
  io.ff_t = st.in(io.ff_t, B);
  io.ff_know = st.in(io.ff_know, 16 * B);
  io.sigma_nav = st.in(io.sigma_nav, ASCENT_NAV_ROWS * B);
  io.nav_phi = st.in(io.nav_phi, ASCENT_NAV_ROWS * B);
  io.nav_q = st.in(io.nav_q, ASCENT_NAV_ROWS * B);
  io.nominal = st.out(io.nominal, ASCENT_HISTORY_QUANTITIES * NJ * B);
  io.cov = st.out(io.cov, ASCENT_LINCOV_COV_ROWS * NJ * B);
  io.jac = st.out(io.jac, (size_t)ASCENT_HISTORY_QUANTITIES * ASCENT_LINCOV_COLS * NJ * B);
  if ((rc = b.st.failed()) || (rc = lincov_run(b.c, substeps, io, b.ws))) return rc;
  return b.close();
}

// What ascent_navigation_filter and ascent_covariance_filtered_batch refuse of the measurements and the initial knowledge: the
// counts, the null pointers and, with host pointers, the values
int check_measurements(const double *sigma_nav, const double *filter_q, const double *meas_h, const double *meas_sigma, int32_t n_meas,
                       int32_t meas_stride, int64_t batch, int ptr_is_device) {
  if (n_meas < 1 || n_meas > ASCENT_NAVFILTER_MAX_MEAS) { snprintf(g_err, sizeof g_err, "n_meas out of range (1 .. %d)", ASCENT_NAVFILTER_MAX_MEAS); return ASCENT_E_ARG; }
  if (meas_stride < 1) { snprintf(g_err, sizeof g_err, "meas_stride must be at least 1"); return ASCENT_E_ARG; }
  if (!sigma_nav || !meas_h || !meas_sigma) { snprintf(g_err, sizeof g_err, "null sigma_nav, meas_h or meas_sigma"); return ASCENT_E_ARG; }
  if (ptr_is_device) return 0;
  for (int64_t i = 0; i < n_meas * batch; i++)
    if (!(meas_sigma[i] > 0.0 && std::isfinite(meas_sigma[i]))) { snprintf(g_err, sizeof g_err, "meas_sigma not positive or not finite (measurement %d, problem %lld)", (int)(i / batch), (long long)(i % batch)); return ASCENT_E_ARG; }
  for (int64_t i = 0; i < 7 * n_meas * batch; i++)
    if (!std::isfinite(meas_h[i])) { snprintf(g_err, sizeof g_err, "meas_h not finite (measurement %d, problem %lld)", (int)(i / (7 * batch)), (long long)(i % batch)); return ASCENT_E_ARG; }
  for (int64_t i = 0; i < 7 * batch; i++) {
    if (!std::isfinite(sigma_nav[i])) { snprintf(g_err, sizeof g_err, "sigma_nav not finite (row %d, problem %lld)", (int)(i / batch), (long long)(i % batch)); return ASCENT_E_ARG; }
    if (filter_q && !std::isfinite(filter_q[i])) { snprintf(g_err, sizeof g_err, "filter_q not finite (row %d, problem %lld)", (int)(i / batch), (long long)(i % batch)); return ASCENT_E_ARG; }
  }
  return 0;
}

// ascent_navigation_filter: io holds the caller's pointers
int navfilter_call(const ascent_params *p, int64_t batch, const ascent_opts *o, int32_t substeps, NavFilterIO io, int device_id,
                   void *stream_, int ptr_is_device) {
  BlobCall b(p, batch, o, io.blob, stream_, ptr_is_device);
  int rc = b.options();
  if (rc) return rc;
  if (!io.blob || !io.gain_l || !io.summary) { snprintf(g_err, sizeof g_err, "null solution blob, gain_l_out or summary_out"); return ASCENT_E_ARG; }
  if ((rc = check_substeps(substeps))) return rc;
  if ((rc = check_measurements(io.sigma_nav, io.filter_q, io.meas_h, io.meas_sigma, io.n_meas, io.meas_stride, batch, ptr_is_device))) return rc;
  if ((rc = b.solvable())) return rc;
  if ((rc = b.open(device_id, lincov_ws_bytes(o->n_nodes - 1, (long)batch)))) return rc;
  Staging &st = b.st;
  const size_t K = (size_t)b.K, B = (size_t)batch, M = (size_t)io.n_meas;
  io.blob = b.blob;
  io.sigma_nav = st.in(io.sigma_nav, 7 * B);
  io.sigma_u = st.in(io.sigma_u, K * B);
  io.filter_q = st.in(io.filter_q, 7 * B);
  io.meas_h = st.in(io.meas_h, M * 7 * B);
  io.meas_sigma = st.in(io.meas_sigma, M * B);
  io.gain_l = st.out(io.gain_l, M * 7 * K * B);
  io.pfilt = st.out(io.pfilt, ASCENT_NAV_COV_ROWS * K * B);
  io.summary = st.out(io.summary, ASCENT_NAVFILTER_ROWS * B);
  if ((rc = b.st.failed()) || (rc = navfilter_run(b.c, substeps, io, b.ws))) return rc;
  return b.close();
}

// ascent_covariance_filtered_batch: io holds the caller's pointers.  The order of the shared refusals is lincov_call's.
int filtered_call(const ascent_params *p, int64_t batch, const ascent_opts *o, int32_t substeps, FilteredIO io, int device_id,
                  void *stream_, int ptr_is_device) {
  BlobCall b(p, batch, o, io.blob, stream_, ptr_is_device);
  int rc = b.options();
  if (rc) return rc;
  if (!io.blob || !io.sigma || !io.nominal || !io.cov) { snprintf(g_err, sizeof g_err, "null solution blob, sigma, nominal_out or cov_out"); return ASCENT_E_ARG; }
  if (!io.nav_cov || !io.gain_l) { snprintf(g_err, sizeof g_err, "null nav_cov_out or gain_l"); return ASCENT_E_ARG; }
  if ((rc = check_substeps(substeps))) return rc;
  if (io.node_stride < 1 || io.node_stride > o->n_nodes - 1) { snprintf(g_err, sizeof g_err, "node_stride out of range (1 .. K = %d)", o->n_nodes - 1); return ASCENT_E_ARG; }
  if (!io.gain_u && (io.gain_t || io.stretch_max)) { snprintf(g_err, sizeof g_err, "gain_t and stretch_max need gain_u"); return ASCENT_E_ARG; }
  if ((rc = check_measurements(io.sigma_nav, nullptr, io.meas_h, io.meas_sigma, io.n_meas, io.meas_stride, batch, ptr_is_device))) return rc;
  if ((rc = b.solvable())) return rc;
  if ((rc = b.open(device_id, lincov_ws_bytes(o->n_nodes - 1, (long)batch)))) return rc;
  Staging &st = b.st;
  const size_t K = (size_t)b.K, B = (size_t)batch, M = (size_t)io.n_meas, NJ = (size_t)history_nodes(b.K, io.node_stride);
  io.blob = b.blob;
  io.sigma = st.in(io.sigma, ASCENT_DISPERSE_COLS * B);
  io.sigma_u = st.in(io.sigma_u, K * B);
  io.gain_u = st.in(io.gain_u, 7 * K * B);
  io.gain_t = st.in(io.gain_t, 7 * B);
  io.stretch_max = st.in(io.stretch_max, B);
  io.sigma_nav = st.in(io.sigma_nav, 7 * B);
  io.gain_l = st.in(io.gain_l, M * 7 * K * B);
  io.meas_h = st.in(io.meas_h, M * 7 * B);
  io.meas_sigma = st.in(io.meas_sigma, M * B);
  io.nominal = st.out(io.nominal, ASCENT_HISTORY_QUANTITIES * NJ * B);
  io.cov = st.out(io.cov, ASCENT_LINCOV_COV_ROWS * NJ * B);
  io.nav_cov = st.out(io.nav_cov, ASCENT_NAV_COV_ROWS * NJ * B);
  io.jac = st.out(io.jac, (size_t)ASCENT_HISTORY_QUANTITIES * ASCENT_LINCOV_COLS * NJ * B);
  io.nav_jac = st.out(io.nav_jac, (size_t)7 * ASCENT_LINCOV_COLS * NJ * B);
  if ((rc = b.st.failed()) || (rc = lincov_filtered_run(b.c, substeps, io, b.ws))) return rc;
  return b.close();
}

// ascent_guidance_gains and ascent_guidance_feedforward (ff): io holds the caller's pointers
int gains_call(const ascent_params *p, int64_t batch, const ascent_opts *o, int32_t substeps, bool ff, GainsIO io, int device_id,
               void *stream_, int ptr_is_device) {
  BlobCall b(p, batch, o, io.blob, stream_, ptr_is_device);
  int rc = b.flight_like(substeps);
  if (rc) return rc;
  if (!io.weights || !io.gain_u || !io.gain_t || !io.summary) { snprintf(g_err, sizeof g_err, "null weights, gain_u_out, gain_t_out or summary_out"); return ASCENT_E_ARG; }
  if (ff && (!io.ff_dir || !io.ff_u || !io.ff_t)) { snprintf(g_err, sizeof g_err, "null ff_dir, ff_u_out or ff_t_out"); return ASCENT_E_ARG; }
  if (io.jac_u && !io.jac) { snprintf(g_err, sizeof g_err, "jac_u_cl_out needs jac_cl_out"); return ASCENT_E_ARG; }
  if (io.jac_nav && !io.jac) { snprintf(g_err, sizeof g_err, "jac_nav_out needs jac_cl_out"); return ASCENT_E_ARG; }
  if (ff && io.jac && !io.ff_know) { snprintf(g_err, sizeof g_err, "jac_cl_out needs ff_know"); return ASCENT_E_ARG; }
  if ((rc = b.open(device_id, gains_ws_bytes(o->n_nodes - 1, (long)batch)))) return rc;
  Staging &st = b.st;
  const size_t K = (size_t)b.K, B = (size_t)batch;
  io.blob = b.blob;
  io.weights = st.in(io.weights, 6 * B);
  io.ff_dir = st.in(io.ff_dir, 16 * B);
  io.ff_know = st.in(io.ff_know, 16 * B);
  io.gain_u = st.out(io.gain_u, 7 * K * B);
  io.gain_t = st.out(io.gain_t, 7 * B);
  io.ff_u = st.out(io.ff_u, K * B);
  io.ff_t = st.out(io.ff_t, B);
  io.summary = st.out(io.summary, (ff ? ASCENT_GUIDE_FF_ROWS : ASCENT_GUIDE_ROWS) * B);
  io.jac = st.out(io.jac, 9 * 24 * B);
  io.jac_u = st.out(io.jac_u, 9 * K * B);
  io.jac_nav = st.out(io.jac_nav, 9 * ASCENT_NAV_ROWS * B);
  if ((rc = b.st.failed()) || (rc = gains_run(b.c, substeps, io, b.ws))) return rc;
  return b.close();
}
}  // namespace

int ascent_param_sensitivity(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                             double *grad_out, int device_id, void *stream_, int ptr_is_device) {
  BlobCall b(p, batch, o, sol_blob, stream_, ptr_is_device);
  int rc = b.options();
  if (rc) return rc;
  if (!sol_blob || !grad_out) { snprintf(g_err, sizeof g_err, "null solution blob or output pointer"); return ASCENT_E_ARG; }
  if ((rc = b.solvable()) || (rc = b.open(device_id, 0))) return rc;
  double *dg = b.st.out(grad_out, (size_t)16 * batch);
  if ((rc = b.st.failed()) || (rc = sens_run(b.c, o->terminal, b.blob, dg))) return rc;
  return b.close();
}

int ascent_fly_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                     double *flown_traj, double *local_err, double *summary, int device_id, void *stream_, int ptr_is_device) {
  BlobCall b(p, batch, o, sol_blob, stream_, ptr_is_device);
  int rc = b.options();
  if (rc) return rc;
  if (!sol_blob || !summary) { snprintf(g_err, sizeof g_err, "null solution blob or summary pointer"); return ASCENT_E_ARG; }
  if ((rc = check_substeps(substeps)) || (rc = b.solvable()) || (rc = b.open(device_id, 0))) return rc;
  double *dt = b.st.out(flown_traj, (size_t)ASCENT_TRAJ_FIELDS * o->n_nodes * batch), *dl = b.st.out(local_err, (size_t)7 * b.K * batch);
  double *ds = b.st.out(summary, (size_t)ASCENT_FLIGHT_ROWS * batch);
  if ((rc = b.st.failed()) || (rc = flight_run(b.c, substeps, b.blob, dt, dl, ds))) return rc;
  return b.close();
}

int ascent_flight_jacobian(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                           double *jac_out, double *jac_u_out, int device_id, void *stream_, int ptr_is_device) {
  BlobCall b(p, batch, o, sol_blob, stream_, ptr_is_device);
  int rc = b.flight_like(substeps);
  if (rc) return rc;
  if (!jac_out) { snprintf(g_err, sizeof g_err, "null jac_out"); return ASCENT_E_ARG; }
  if ((rc = b.open(device_id, jac_ws_bytes(o->n_nodes - 1, (long)batch)))) return rc;
  double *dj = b.st.out(jac_out, (size_t)9 * 24 * batch), *du = b.st.out(jac_u_out, (size_t)9 * b.K * batch);
  if ((rc = b.st.failed()) || (rc = jac_run(b.c, substeps, b.blob, dj, du, b.ws))) return rc;
  return b.close();
}

int ascent_trim_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                      int32_t rounds, double tol, double *trim_blob_out, double *summary_out, int device_id, void *stream_,
                      int ptr_is_device) {
  BlobCall b(p, batch, o, sol_blob, stream_, ptr_is_device);
  int rc = b.flight_like(substeps);
  if (rc) return rc;
  if (!trim_blob_out || !summary_out) { snprintf(g_err, sizeof g_err, "null trim_blob_out or summary_out"); return ASCENT_E_ARG; }
  if (rounds < 0 || rounds > 32) { snprintf(g_err, sizeof g_err, "rounds out of range (1 .. 32, 0 = 6)"); return ASCENT_E_ARG; }
  if ((rc = b.open(device_id, trim_ws_bytes(o->n_nodes - 1, (long)batch)))) return rc;
  if (rounds == 0) rounds = 6;
  if (!(tol > 0.0)) tol = 1e-10;
  double *dout = b.st.out(trim_blob_out, (21 * (size_t)b.K + NSC) * batch), *ds = b.st.out(summary_out, (size_t)ASCENT_TRIM_ROWS * batch);
  if ((rc = b.st.failed()) || (rc = trim_run(b.c, o->terminal, substeps, rounds, tol, b.blob, dout, ds, b.ws))) return rc;
  return b.close();
}

int ascent_disperse_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                          int32_t samples, const double *xi, const double *sigma, const double *sigma_u, double *stats_out,
                          double *samples_out, int device_id, void *stream_, int ptr_is_device) {
  DisperseIO io{};
  io.blob = sol_blob; io.xi = xi; io.sigma = sigma; io.sigma_u = sigma_u;
  io.stats = stats_out; io.samples_out = samples_out;
  return disperse_call(p, batch, o, substeps, samples, DISPERSE_OPEN, io, device_id, stream_, ptr_is_device);
}

int ascent_guidance_gains(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                          const double *weights, double *gain_u_out, double *gain_t_out, double *summary_out, double *jac_cl_out,
                          double *jac_u_cl_out, int device_id, void *stream_, int ptr_is_device) {
  GainsIO io{};
  io.blob = sol_blob; io.weights = weights;
  io.gain_u = gain_u_out; io.gain_t = gain_t_out; io.summary = summary_out; io.jac = jac_cl_out; io.jac_u = jac_u_cl_out;
  return gains_call(p, batch, o, substeps, false, io, device_id, stream_, ptr_is_device);
}

int ascent_disperse_guided_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                                 int32_t samples, const double *xi, const double *sigma, const double *sigma_u, const double *gain_u,
                                 const double *gain_t, const double *stretch_max, double *stats_out, double *samples_out,
                                 int device_id, void *stream_, int ptr_is_device) {
  DisperseIO io{};
  io.blob = sol_blob; io.xi = xi; io.sigma = sigma; io.sigma_u = sigma_u;
  io.gain_u = gain_u; io.gain_t = gain_t; io.stretch_max = stretch_max;
  io.stats = stats_out; io.samples_out = samples_out;
  return disperse_call(p, batch, o, substeps, samples, DISPERSE_GUIDED, io, device_id, stream_, ptr_is_device);
}

int ascent_guidance_feedforward(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                                const double *weights, const double *ff_dir, const double *ff_know, double *gain_u_out,
                                double *gain_t_out, double *ff_u_out, double *ff_t_out, double *summary_out, double *jac_cl_out,
                                double *jac_u_cl_out, double *jac_nav_out, int device_id, void *stream_, int ptr_is_device) {
  GainsIO io{};
  io.blob = sol_blob; io.weights = weights; io.ff_dir = ff_dir; io.ff_know = ff_know;
  io.gain_u = gain_u_out; io.gain_t = gain_t_out; io.ff_u = ff_u_out; io.ff_t = ff_t_out; io.summary = summary_out;
  io.jac = jac_cl_out; io.jac_u = jac_u_cl_out; io.jac_nav = jac_nav_out;
  return gains_call(p, batch, o, substeps, true, io, device_id, stream_, ptr_is_device);
}

int ascent_disperse_navigated_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                                    int32_t samples, const double *xi, const double *sigma, const double *sigma_u, const double *gain_u,
                                    const double *gain_t, const double *stretch_max, const double *ff_u, const double *ff_t,
                                    const double *ff_know, const double *xi_nav, const double *sigma_nav, double *stats_out,
                                    double *samples_out, int device_id, void *stream_, int ptr_is_device) {
  DisperseIO io{};
  io.blob = sol_blob; io.xi = xi; io.sigma = sigma; io.sigma_u = sigma_u;
  io.gain_u = gain_u; io.gain_t = gain_t; io.stretch_max = stretch_max;
  io.ff_u = ff_u; io.ff_t = ff_t; io.ff_know = ff_know; io.xi_nav = xi_nav; io.sigma_nav = sigma_nav;
  io.stats = stats_out; io.samples_out = samples_out;
  return disperse_call(p, batch, o, substeps, samples, DISPERSE_NAVIGATED, io, device_id, stream_, ptr_is_device);
}

int ascent_disperse_history_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                                  int32_t samples, const double *xi, const double *sigma, const double *sigma_u, const double *gain_u,
                                  const double *gain_t, const double *stretch_max, const double *ff_u, const double *ff_t,
                                  const double *ff_know, const double *xi_nav, const double *sigma_nav, int32_t node_stride,
                                  double *stats_out, double *samples_out, double *hist_out, double *hist_samples_out, int device_id,
                                  void *stream_, int ptr_is_device) {
  DisperseIO io{};
  io.blob = sol_blob; io.xi = xi; io.sigma = sigma; io.sigma_u = sigma_u;
  io.gain_u = gain_u; io.gain_t = gain_t; io.stretch_max = stretch_max;
  io.ff_u = ff_u; io.ff_t = ff_t; io.ff_know = ff_know; io.xi_nav = xi_nav; io.sigma_nav = sigma_nav;
  io.stats = stats_out; io.samples_out = samples_out;
  io.node_stride = node_stride; io.hist = hist_out; io.hist_samples = hist_samples_out;
  return disperse_call(p, batch, o, substeps, samples, gain_u ? DISPERSE_NAVIGATED : DISPERSE_OPEN, io, device_id, stream_, ptr_is_device, true);
}

int ascent_covariance_history_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                                    const double *sigma, const double *sigma_u, const double *gain_u, const double *gain_t,
                                    const double *stretch_max, const double *ff_u, const double *ff_t, const double *ff_know,
                                    const double *sigma_nav, int32_t node_stride, double *nominal_out, double *cov_out,
                                    double *jac_hist_out, int device_id, void *stream_, int ptr_is_device) {
  LincovIO io{};
  io.blob = sol_blob; io.sigma = sigma; io.sigma_u = sigma_u;
  io.gain_u = gain_u; io.gain_t = gain_t; io.stretch_max = stretch_max;
  io.ff_u = ff_u; io.ff_t = ff_t; io.ff_know = ff_know; io.sigma_nav = sigma_nav;
  io.node_stride = node_stride; io.nominal = nominal_out; io.cov = cov_out; io.jac = jac_hist_out;
  return lincov_call(p, batch, o, substeps, io, device_id, stream_, ptr_is_device);
}

int ascent_disperse_drifting_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                                   int32_t samples, const double *xi, const double *sigma, const double *sigma_u, const double *gain_u,
                                   const double *gain_t, const double *stretch_max, const double *ff_u, const double *ff_t,
                                   const double *ff_know, const double *xi_nav, const double *sigma_nav, const double *nav_phi,
                                   const double *nav_q, const double *xi_drift, int32_t node_stride, double *stats_out,
                                   double *samples_out, double *hist_out, double *hist_samples_out, int device_id, void *stream_,
                                   int ptr_is_device) {
  DisperseIO io{};
  io.blob = sol_blob; io.xi = xi; io.sigma = sigma; io.sigma_u = sigma_u;
  io.gain_u = gain_u; io.gain_t = gain_t; io.stretch_max = stretch_max;
  io.ff_u = ff_u; io.ff_t = ff_t; io.ff_know = ff_know; io.xi_nav = xi_nav; io.sigma_nav = sigma_nav;
  io.nav_phi = nav_phi; io.nav_q = nav_q; io.xi_drift = xi_drift;
  io.stats = stats_out; io.samples_out = samples_out;
  io.node_stride = node_stride; io.hist = hist_out; io.hist_samples = hist_samples_out;
  return disperse_call(p, batch, o, substeps, samples, gain_u ? DISPERSE_NAVIGATED : DISPERSE_OPEN, io, device_id, stream_, ptr_is_device, true,
                       true);
}

int ascent_covariance_drifting_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                                     const double *sigma, const double *sigma_u, const double *gain_u, const double *gain_t,
                                     const double *stretch_max, const double *ff_u, const double *ff_t, const double *ff_know,
                                     const double *sigma_nav, const double *nav_phi, const double *nav_q, int32_t node_stride,
                                     double *nominal_out, double *cov_out, double *jac_hist_out, int device_id, void *stream_,
                                     int ptr_is_device) {
  LincovIO io{};
  io.blob = sol_blob; io.sigma = sigma; io.sigma_u = sigma_u;
  io.gain_u = gain_u; io.gain_t = gain_t; io.stretch_max = stretch_max;
  io.ff_u = ff_u; io.ff_t = ff_t; io.ff_know = ff_know; io.sigma_nav = sigma_nav;
  io.nav_phi = nav_phi; io.nav_q = nav_q;
  io.node_stride = node_stride; io.nominal = nominal_out; io.cov = cov_out; io.jac = jac_hist_out;
  return lincov_call(p, batch, o, substeps, io, device_id, stream_, ptr_is_device, true);
}

int ascent_navigation_filter(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                             const double *sigma_nav, const double *sigma_u, const double *filter_q, const double *meas_h,
                             const double *meas_sigma, int32_t n_meas, int32_t meas_stride, double *gain_l_out, double *pfilt_out,
                             double *summary_out, int device_id, void *stream_, int ptr_is_device) {
  NavFilterIO io{};
  io.blob = sol_blob; io.sigma_nav = sigma_nav; io.sigma_u = sigma_u; io.filter_q = filter_q;
  io.meas_h = meas_h; io.meas_sigma = meas_sigma; io.n_meas = n_meas; io.meas_stride = meas_stride;
  io.gain_l = gain_l_out; io.pfilt = pfilt_out; io.summary = summary_out;
  return navfilter_call(p, batch, o, substeps, io, device_id, stream_, ptr_is_device);
}

int ascent_covariance_filtered_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                                     const double *sigma, const double *sigma_u, const double *gain_u, const double *gain_t,
                                     const double *stretch_max, const double *sigma_nav, const double *gain_l, const double *meas_h,
                                     const double *meas_sigma, int32_t n_meas, int32_t meas_stride, int32_t node_stride,
                                     double *nominal_out, double *cov_out, double *nav_cov_out, double *jac_hist_out,
                                     double *nav_jac_out, int device_id, void *stream_, int ptr_is_device) {
  FilteredIO io{};
  io.blob = sol_blob; io.sigma = sigma; io.sigma_u = sigma_u;
  io.gain_u = gain_u; io.gain_t = gain_t; io.stretch_max = stretch_max;
  io.sigma_nav = sigma_nav; io.gain_l = gain_l; io.meas_h = meas_h; io.meas_sigma = meas_sigma;
  io.n_meas = n_meas; io.meas_stride = meas_stride; io.node_stride = node_stride;
  io.nominal = nominal_out; io.cov = cov_out; io.nav_cov = nav_cov_out; io.jac = jac_hist_out; io.nav_jac = nav_jac_out;
  return filtered_call(p, batch, o, substeps, io, device_id, stream_, ptr_is_device);
}

int ascent_sample_quantiles(const double *values, int32_t quantities, int32_t groups, int32_t valid_quantities, int32_t samples,
                            int64_t batch, const double *probs, int32_t n_probs, const double *limits_or_null, int32_t n_limits,
                            double *count_out, double *quant_out, double *below_out_or_null, int device_id, void *stream_,
                            int ptr_is_device) {
  if (!values || !count_out || !quant_out) { snprintf(g_err, sizeof g_err, "null values, count_out or quant_out"); return ASCENT_E_ARG; }
  if (quantities < 1 || groups < 1 || batch < 1) { snprintf(g_err, sizeof g_err, "quantities, groups and batch must be at least 1"); return ASCENT_E_ARG; }
  if (valid_quantities < 0 || valid_quantities > quantities) { snprintf(g_err, sizeof g_err, "valid_quantities out of range (0 .. quantities = %d)", quantities); return ASCENT_E_ARG; }
  int rc = check_samples(samples);
  if (rc || (rc = check_probs(probs, n_probs)) || (rc = check_limits(limits_or_null, below_out_or_null, n_limits, "limits", "below_out"))) return rc;
  if ((rc = check_device(device_id))) return rc;
  std::lock_guard<std::mutex> lock(g_mu[device_id]);
  HIPCHK(hipSetDevice(device_id));
  hipStream_t stream = (hipStream_t)stream_;
  Staging st(stream, ptr_is_device);
  const size_t Q = (size_t)quantities, G = (size_t)groups, B = (size_t)batch, NL = limits_or_null ? (size_t)n_limits : 0;
  QuantileIO io{};
  io.values = st.in(values, Q * G * (size_t)samples * B);
  io.Q = quantities; io.G = groups; io.V = valid_quantities; io.samples = samples; io.batch = (long)batch;
  io.n_probs = n_probs;
  for (int j = 0; j < n_probs; j++) io.probs[j] = probs[j];
  io.limits = st.in(limits_or_null, NL * Q * B); io.n_limits = (int)NL;
  io.count = st.out(count_out, G * B);
  io.quant = st.out(quant_out, (size_t)n_probs * Q * G * B);
  io.below = st.out(below_out_or_null, NL * Q * G * B);
  if ((rc = st.failed()) || (rc = quantile_run(io, stream, g_err, sizeof g_err))) return rc;
  return st.finish();
}

int64_t ascent_disperse_quantiles_bytes(int64_t batch, int32_t n_nodes, int32_t samples, int32_t node_stride) {
  if (batch < 1 || n_nodes < 3 || n_nodes > 65536 || samples < 1 || samples > ASCENT_DISPERSE_MAX_SAMPLES || node_stride < 0 ||
      node_stride > n_nodes - 1)
    return ASCENT_E_ARG;
  return (int64_t)(disperse_ws_bytes(n_nodes - 1, (long)batch, samples, node_stride) + quantile_scratch_bytes(n_nodes - 1, batch, samples, node_stride));
}

int ascent_disperse_quantiles_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                                    int32_t samples, const double *xi, const double *sigma, const double *sigma_u, const double *gain_u,
                                    const double *gain_t, const double *stretch_max, const double *ff_u, const double *ff_t,
                                    const double *ff_know, const double *xi_nav, const double *sigma_nav, const double *nav_phi,
                                    const double *nav_q, const double *xi_drift, int32_t node_stride, double *stats_out,
                                    double *hist_out_or_null, const double *probs, int32_t n_probs, const double *limits_or_null,
                                    const double *hist_limits_or_null, int32_t n_limits, double *quant_out, double *below_out_or_null,
                                    double *hist_quant_out_or_null, double *hist_below_out_or_null, int device_id, void *stream_,
                                    int ptr_is_device) {
  int rc = check_probs(probs, n_probs);
  if (rc) return rc;
  if (!quant_out) { snprintf(g_err, sizeof g_err, "null quant_out"); return ASCENT_E_ARG; }
  if ((rc = check_limits(limits_or_null, below_out_or_null, n_limits, "limits", "below_out")) ||
      (rc = check_limits(hist_limits_or_null, hist_below_out_or_null, n_limits, "hist_limits", "hist_below_out")))
    return rc;
  if (node_stride == 0 && (hist_out_or_null || hist_limits_or_null || hist_quant_out_or_null || hist_below_out_or_null)) {
    snprintf(g_err, sizeof g_err, "hist_out, hist_limits, hist_quant_out and hist_below_out need node_stride > 0");
    return ASCENT_E_ARG;
  }
  if (hist_below_out_or_null && !hist_quant_out_or_null) { snprintf(g_err, sizeof g_err, "hist_below_out needs hist_quant_out"); return ASCENT_E_ARG; }
  const bool drifting = nav_phi || nav_q || xi_drift, history = node_stride != 0 || drifting;      // (node_stride 0 with them: refused as the drifting call refuses it)
  const bool nav = ff_u || ff_t || ff_know || xi_nav || sigma_nav;
  DisperseIO io{};
  io.blob = sol_blob; io.xi = xi; io.sigma = sigma; io.sigma_u = sigma_u;
  io.gain_u = gain_u; io.gain_t = gain_t; io.stretch_max = stretch_max;
  io.ff_u = ff_u; io.ff_t = ff_t; io.ff_know = ff_know; io.xi_nav = xi_nav; io.sigma_nav = sigma_nav;
  io.nav_phi = nav_phi; io.nav_q = nav_q; io.xi_drift = xi_drift;
  io.stats = stats_out;
  io.node_stride = node_stride; io.hist = hist_out_or_null;
  const QuantileRequest qr{probs, n_probs, limits_or_null, hist_limits_or_null, n_limits, quant_out, below_out_or_null, hist_quant_out_or_null,
                           hist_below_out_or_null};
  DisperseKind kind = DISPERSE_OPEN;
  if (history) kind = gain_u ? DISPERSE_NAVIGATED : DISPERSE_OPEN;
  else if (gain_u) kind = nav ? DISPERSE_NAVIGATED : DISPERSE_GUIDED;
  else if (gain_t || stretch_max || nav) { snprintf(g_err, sizeof g_err, "gain_t, stretch_max, ff_u, ff_t, ff_know, xi_nav and sigma_nav need gain_u"); return ASCENT_E_ARG; }
  return disperse_call(p, batch, o, substeps, samples, kind, io, device_id, stream_, ptr_is_device, history, drifting, &qr);
}

int ascent_kkt_step(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *iterate,
                    const double *mu, const double *delta_w, double *step, int32_t *inertia_out, int device_id) {
  return ascent_kkt_step_path(p, batch, o, iterate, mu, delta_w, step, inertia_out, device_id, ASCENT_PATH_AUTO);
}

int ascent_reduce_probe(const double *in, int64_t n, double *out, int device_id) {
  if (!in || !out || n <= 0 || n > 65535) { snprintf(g_err, sizeof g_err, "ascent_reduce_probe: null pointer or n outside 1 .. 65535"); return ASCENT_E_ARG; }
  int rc = check_device(device_id);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(g_mu[device_id]);
  HIPCHK(hipSetDevice(device_id));
  Staging st(nullptr, 0);
  const double *din = st.in(in, (size_t)n * WAVE);
  double *dout = st.out(out, (size_t)n * ASCENT_REDUCE_PROBE_ROWS * WAVE);
  if ((rc = st.failed())) return rc;
  if ((rc = reduce_probe_run(din, (long)n, dout, nullptr, g_err, sizeof g_err))) return rc;
  return st.finish();
}

int ascent_kkt_solve(int64_t batch, int32_t n, int32_t bs, int32_t nb, const double *diag, const double *lower,
                     const double *upper, const double *border, const double *border_diag, const double *rhs,
                     double *sol, int device_id, int algo) {
  if (batch <= 0 || n < 1 || n > 65535 || bs < 1 || bs > 16 || nb < 0 || nb > 15 || (algo != 0 && algo != 1)) {
    snprintf(g_err, sizeof g_err, "ascent_kkt_solve: need batch > 0, 1 <= n_nodes <= 65535, 1 <= bs <= 16, 0 <= nb <= 15, algo 0 | 1");
    return ASCENT_E_ARG;
  }
  if (!diag || !lower || !upper || !rhs || !sol || (nb && (!border || !border_diag))) { snprintf(g_err, sizeof g_err, "null pointer"); return ASCENT_E_ARG; }
  int rc = check_device(device_id);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(g_mu[device_id]);
  HIPCHK(hipSetDevice(device_id));
  if ((rc = claim_slot0(device_id))) return rc;
  if ((rc = ensure_ws(g_ws_slot0(device_id), blocktri_ws_bytes(n, (long)batch, algo)))) return rc;
  DeviceWs &w = g_ws_slot0(device_id);
  const size_t nblk = (size_t)batch * n * bs * bs, nbor = (size_t)batch * n * bs * (nb ? nb : 1), nrow = (size_t)n * bs + nb;
  const size_t ny = (size_t)batch * n * bs * (1 + nb);
  std::vector<double> Y(ny);
  Staging st(nullptr, 0);
  const double *dd = st.in(diag, nblk), *dl = st.in(lower, nblk), *du = st.in(upper, nblk);
  const double *db = nb ? st.in(border, nbor) : st.scratch<double>(nbor);
  const double *dr = st.in(rhs, batch * nrow);
  double *dy = st.out(Y.data(), ny);
  if ((rc = st.failed())) return rc;
  int singular = 0;
  rc = blocktri_run((long)batch, n, bs, nb, dd, dl, du, db, dr, w.ws, dy, algo, &singular, 0, w.ev0, w.ev1, g_err, sizeof g_err);
  if (rc) return rc;
  w.launched = true;
  if (singular) { snprintf(g_err, sizeof g_err, "ascent_kkt_solve: singular pivot inside a block (no pivoting)"); return ASCENT_E_ARG; }
  if ((rc = st.finish())) return rc;
  // close the border on the host: S = d - B'Y_B,  y = S^-1 (s - B'Y_r),  x = Y_r - Y_B y
  const int nc = 1 + nb;
  std::vector<double> S((size_t)nb * nb), t(nb), yv(nb);
  for (int64_t q = 0; q < batch; q++) {
    const double *Yq = Y.data() + (size_t)q * n * bs * nc;
    const double *Bq = nb ? border + (size_t)q * n * bs * nb : nullptr;
    const double *rq = rhs + (size_t)q * nrow;
    double *xq = sol + (size_t)q * nrow;
    for (int a = 0; a < nb; a++) {
      t[a] = rq[(size_t)n * bs + a];
      for (int b = 0; b < nb; b++) S[(size_t)a * nb + b] = border_diag[((size_t)q * nb + a) * nb + b];
      for (size_t r = 0; r < (size_t)n * bs; r++) {
        const double ba = Bq[r * nb + a];
        t[a] -= ba * Yq[r * nc];
        for (int b = 0; b < nb; b++) S[(size_t)a * nb + b] -= ba * Yq[r * nc + 1 + b];
      }
    }
    for (int a = 0; a < nb; a++) {            // Gaussian elimination with partial pivoting on [S | t]
      int pv = a;
      for (int r = a + 1; r < nb; r++) if (std::fabs(S[(size_t)r * nb + a]) > std::fabs(S[(size_t)pv * nb + a])) pv = r;
      if (S[(size_t)pv * nb + a] == 0.0) { snprintf(g_err, sizeof g_err, "ascent_kkt_solve: singular border Schur complement"); return ASCENT_E_ARG; }
      if (pv != a) { for (int b = 0; b < nb; b++) std::swap(S[(size_t)a * nb + b], S[(size_t)pv * nb + b]); std::swap(t[a], t[pv]); }
      for (int r = a + 1; r < nb; r++) {
        const double f = S[(size_t)r * nb + a] / S[(size_t)a * nb + a];
        for (int b = a; b < nb; b++) S[(size_t)r * nb + b] -= f * S[(size_t)a * nb + b];
        t[r] -= f * t[a];
      }
    }
    for (int a = nb - 1; a >= 0; a--) {
      double v = t[a];
      for (int b = a + 1; b < nb; b++) v -= S[(size_t)a * nb + b] * yv[b];
      yv[a] = v / S[(size_t)a * nb + a];
    }
    for (size_t r = 0; r < (size_t)n * bs; r++) {
      double v = Yq[r * nc];
      for (int b = 0; b < nb; b++) v -= Yq[r * nc + 1 + b] * yv[b];
      xq[r] = v;
    }
    for (int a = 0; a < nb; a++) xq[(size_t)n * bs + a] = yv[a];
  }
  return ASCENT_OK;
}

}  // extern "C"
