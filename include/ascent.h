/* libascent -- C ABI of the MI355X-native batched lunar-ascent NLP solver.
 *
 * Drop-in boundary.  The reference has no FFI of its own: its hot path is
 * the single call  m.solve(disp=True)  at /root/reference/Launch_Optimiser.py:177, which ships the
 * model declared at Launch_Optimiser.py:19-176 to GEKKO -> APMonitor -> IPOPT.  These entry points
 * are what a GEKKO-compatible front end binds instead of that call (see INTEGRATION.md for the
 * ctypes stub); lunar_module_ascent_trajectory_optimiser_amd/gekko_shim.py is such a front end.
 *
 * Conventions
 *   - every entry point returns 0 on success or a negative ascent_status code (usage / HIP error,
 *     text via ascent_strerror); per-problem solver outcomes go to status_out, never the return code
 *   - plain pointers and sizes only; the caller owns every buffer; the library allocates only its
 *     private per-device workspace
 *   - all arrays are double precision, structure-of-arrays with the PROBLEM index fastest:
 *       element (row r, problem p) of an array with `batch` problems lives at  a[r*batch + p]
 *   - scaled units exactly as the reference's GEKKO variables (Launch_Optimiser.py:83-109):
 *       lengths / Scalar (= r_peri), mass = burnt fraction of fuel_mass, angle = physical/3,
 *       u = angular acceleration / ang_acc_max, tf = final time / T_scale
 */
#ifndef ASCENT_H
#define ASCENT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One NLP's physical parameters, SI units.  Mirrors Launch_Optimiser.py:38-75,107-109. */
typedef struct ascent_params {
  double G;            /* :50  gravitational constant                                   */
  double M;            /* :51  mass of the Moon, kg                                     */
  double R0;           /* :52  lunar radius, m                                          */
  double Ft;           /* :61  thrust, N                                                */
  double M0;           /* :62  wet mass, kg                                             */
  double mdot;         /* :63,65 propellant mass flow, kg/s (mflow = mdot/fuel_mass)    */
  double fuel_mass;    /* :64  kg                                                       */
  double mass_scalar;  /* :108 mass scale in (M0 - mass_scalar*mass); = fuel_mass in the
                               current script, 2576 in the v1 script (PDF p26)          */
  double ang_acc_max;  /* :66  angular-acceleration cap, rad/s^2                         */
  double r_peri;       /* :70  target periapsis altitude, m (= Rfmin = Scalar, :73,107) */
  double r_apo;        /* :71  target apoapsis altitude, m                              */
  double T_scale;      /* :38  final_time = 470 s (time scale; tf in [tf_lb, tf_ub])    */
  double angle_ub;     /* :94  upper bound of angle (= physical/3), pi/3                */
  double tf_lb;        /* :39                                                            */
  double tf_ub;        /* :39                                                            */
  double dcost;        /* :99  MV movement penalty (applied with ascent_opts.move_penalty = 1) */
} ascent_params;

typedef struct ascent_opts {
  int32_t n_nodes;     /* :20  nt, number of grid points (tau_k = k/(nt-1), :21), 3 .. 65536 */
  int32_t scheme;      /* 0 = NODES=2 two-point collocation = backward Euler (:25);
                          1 = trapezoid, control held over the step (not a reference scheme);
                          2 = Hermite-Simpson (compressed form, control held over the step; the method
                              source the reference's report cites, PDF p3/p25) -- a persistent kernel of its
                              own (h_solve); with move_penalty = 1 the dense-block solver path             */
  int32_t max_iter;    /* :28  interior-point iteration cap                              */
  int32_t warm_start;  /* 0 = built-in cold-start guess, 1 = primal part of `guess`,
                          2 = full primal-dual `guess` (multipliers kept)                */
  double tol;          /* KKT error tolerance (the reference's OTOL/RTOL, :31-32)        */
  double mu_init;      /* initial barrier parameter (<=0: 0.1 cold, 1e-4 warm)           */
  int32_t formulation; /* 0 = current script: u = angledoubledot is the MV (:96-100);
                          1 = v1 script (PDF p26-28): the angle itself is the MV -- carried in
                              the same arrays: angle = (angle_ub/2)(u+1), angledot = 0, and the
                              `angledoubledot` field holds that normalised control u            */
  int32_t coarse_nodes; /* nested iteration for cold starts (warm_start == 0): the NLP is first solved on a coarse
                           grid, that primal-dual solution is prolonged to the n_nodes grid and warm-starts it.
                           0 = automatic (grids of >= 40 nodes; coarse grid = max(14, (3 n_nodes + 5)/10) nodes,
                           recursively: 201 -> 60 -> 17 -- a grid one to three intervals beyond a multiple of 16 gives them up; coarse levels are solved to max(tol, 1e-3); a level
                           warm-started from the cold-started coarsest grid begins at mu = 1e-6, one warm-started
                           from a warm-started grid at mu = max(1e-9, tol/100); with move_penalty = 1: 1e-5 and
                           max(1e-8, 10 tol)), -1 = off (single grid),
                           > 0 = that many coarse nodes (two levels).
                           iters_out counts the iterations of all levels.                              */
  int32_t terminal;     /* 0 = the reference's terminal speed (:72-78: circular speed of the MEAN radius, imposed at
                               r_peri with r.v = 0, :158-173);
                           1 = the (r_peri, r_apo) ellipse proper (README.md:7): same three constraints with the vis-viva
                               speed at the periapsis of that ellipse, so that the burnout orbit is the target ellipse and
                               ascent_coast_batch's coast arc ends at its apoapsis;
                           2 = burnout ANYWHERE on that ellipse -- the burn--coast problem of BASELINE config 5 with the coast
                               arc eliminated exactly (two-body motion): two conditions, angular momentum >= and specific energy
                               <= those of the ellipse (an orbit nested in the target annulus; both active at the optimum), no
                               r.v = 0; ascent_coast_batch continues from whatever true anomaly the burn ends at.
                               Persistent kernels (every scheme) and dense-block path, formulation 0           */
  int32_t solver_path;  /* 0 = automatic (the persistent kernels: p_solve for schemes 0/1, h_solve for scheme 2; a handful of NLPs on a long
                               grid and scheme 2 with the move penalty: the dense-block path; ascent_default_path tells);
                           ASCENT_PATH_DENSE = the dense-block path for any scheme (formulation 0 only)       */
  int32_t move_penalty; /* 0 = ascent_params.dcost is ignored (a sweep's parameter sets may carry none);
                           1 = :99 angledoubledot.DCOST applied -- the model the reference declares: the objective is
                               tf + dcost * sum_k |u_k - u_{k-1}| (u_{-1} = 0, the MV's initial value; an l1 term with a slack pair
                               per step, as APMonitor documents DCOST).  Schemes 0 / 1: inside the persistent kernel (the control
                               becomes the eighth state of a stage, the pair reduces to one pivot); scheme 2: dense-block path.
                               With formulation 1 (the v1 script's angle.DCOST, PDF p26; scheme 0): the penalty is on the angle,
                               i.e. weight dcost * angle_ub / 2 on the normalised control, which starts from -1 (angle 0).
                               Needs dcost > 0 for every problem.  Host-resident parameters (ptr_is_device = 0): a dcost that is
                               not positive (zero, negative, NaN) is refused for the whole call, ASCENT_E_ARG.  Device-resident
                               parameters are not read by the host: the kernels that set the starting point check the weight, and
                               such a problem is not iterated -- status ASCENT_INVALID_PROBLEM, 0 iterations, and tf, traj and blob
                               hold its starting point (all finite); the other problems of the batch are solved as without it */
  int32_t reserved;     /* 0 */
} ascent_opts;

enum ascent_status {           /* function return codes */
  ASCENT_OK = 0,
  ASCENT_E_ARG = -1,           /* null pointer / bad size / unsupported option           */
  ASCENT_E_HIP = -2,           /* a HIP runtime call failed (see ascent_strerror)        */
  ASCENT_E_NODEVICE = -3,      /* no such device                                         */
  ASCENT_E_NOMEM = -4,         /* workspace allocation failed                            */
  ASCENT_E_NOTERM = -5         /* the host-steered pipeline exceeded its round budget (a solver
                                  condition that the per-problem statuses could not express)   */
};
/* Every entry point refuses argument errors (ASCENT_E_ARG) before it looks at the device, so a bad argument is reported
   as such on a machine without a GPU as well, not as ASCENT_E_NODEVICE. */

enum ascent_problem_status {   /* values written to status_out[] */
  ASCENT_CONVERGED = 0,
  ASCENT_MAX_ITER = 1,
  ASCENT_LINESEARCH_FAILED = 2,
  ASCENT_REGULARISATION_FAILED = 3,  /* numerical breakdown: inertia could not be corrected */
  ASCENT_INVALID_PROBLEM = 4         /* move_penalty = 1 with a dcost that is not positive (device-resident parameters): not iterated */
};

/* Row counts of the SoA arrays, K = n_nodes-1 (node 0 is fixed by the initial conditions,
 * Launch_Optimiser.py:145-151):
 *   iterate / step / guess "blob":  21*K + 10 rows
 *       rows [0,7K)     z_k  : node k=1..K, fields x y xdot ydot angle angledot mass  (row 7(k-1)+f)
 *       rows [7K,8K)    u_k  : angledoubledot
 *       rows [8K,15K)   lambda_k : multipliers of the 7 collocation defects of step k
 *       rows [15K,21K)  bound multipliers zL_angle zU_angle zL_mass zU_mass zL_u zU_u per node
 *       rows 21K..21K+9 tf, zL_tf, zU_tf, s1, s2, z_s1, z_s2, nu3, nu1, nu2
 *                       (s_i: slacks of the two terminal inequalities :161,:169; nu: multipliers of
 *                        the terminal r.v = 0 (:173) and of the two slack equations)
 *   traj_out: 10*n_nodes rows, row f*n_nodes + k, fields in the order of the reference's .value
 *       lists: x y xdot ydot xdoubledot ydoubledot angle angledot angledoubledot mass  (:187-202)
 */
#define ASCENT_BLOB_ROWS(n_nodes) (21 * ((n_nodes) - 1) + 10)
#define ASCENT_TRAJ_FIELDS 10

int ascent_version(void);
int ascent_device_count(void);
const char *ascent_strerror(int code);

/* Solve `batch` independent ascent NLPs (replaces m.solve, Launch_Optimiser.py:177).
 * p: AoS [batch] parameter structs (host or device per ptr_is_device, like every other pointer).
 * guess_or_null: blob [21K+10][batch] when o->warm_start != 0.
 * traj_out [10*n_nodes][batch], tf_out/status_out/iters_out [batch]; sol_blob_out_or_null
 * [21K+10][batch] receives the full primal-dual solution (usable as a warm start).
 * stream: hipStream_t or NULL.  With host pointers the call returns after the results are in the
 * caller's buffers.  With ptr_is_device != 0 and a stream, the persistent kernels (schemes 0 and 1, both
 * formulations, with or without the move penalty; scheme 2 without it; every terminal mode: the default at every batch size,
 * ascent_default_path) are only enqueued -- a handful of launches per grid level, no host involvement (with the NULL stream the
 * call waits for the solve); the split pipeline (ASCENT_PIPELINE=split) and the dense-block path (scheme 2 with the move
 * penalty, a few NLPs on long grids) synchronise the stream once per burst of interior-point rounds, because the host steers the
 * rounds, and return with the last kernels enqueued.
 * Concurrency: host-side, calls on one device are serialised by a mutex.  Device-side, the library keeps a workspace per
 * caller stream (up to three non-default streams per device; the default stream, the parity surfaces and any further
 * stream share workspace 0): solves enqueued on different streams with device pointers overlap on the device -- the
 * wavefronts of one fill the SIMDs the stragglers of the other leave idle (bench.py: pipelined_two_streams) -- while
 * a call whose predecessor in the SAME workspace is still executing makes its stream wait for that predecessor's last
 * kernel first (hipStreamWaitEvent), so two solves never share a workspace in flight.  ascent_last_kernel_ms reports
 * the most recently enqueued solve of the device. */
int ascent_solve_batch(const ascent_params *p, int64_t batch, const ascent_opts *o,
                       const double *guess_or_null, double *traj_out, double *tf_out,
                       int32_t *status_out, int32_t *iters_out, double *sol_blob_out_or_null,
                       int device_id, void *hip_stream_or_null, int ptr_is_device);

/* Per-node pieces of the path, exposed for parity testing (Launch_Optimiser.py:114-136):
 * iterate: blob [21K+10][batch] (z, u, lambda, tf are read).
 * defects [7K][batch]: z_k - z_{k-1} - h*T*tf*f(z_k,u_k), row 7(k-1)+f.
 * jac_blocks [8K][batch]: d(xdoubledot)/d(x,y,angle,mass), d(ydoubledot)/d(x,y,angle,mass).
 * hess_blocks [10K][batch]: upper triangle (xx xy xa xm yy ya ym aa am mm) of the Hessian of
 *   -h*T*tf*(lambda_xdot*xdoubledot + lambda_ydot*ydoubledot), the node's Lagrangian block.
 * Host pointers. */
int ascent_eval_nodes(const ascent_params *p, int64_t batch, const ascent_opts *o,
                      const double *iterate, double *defects, double *jac_blocks,
                      double *hess_blocks, int device_id);

/* One Newton step of the barrier problem: factorises and solves the bordered block-tridiagonal
 * KKT system at `iterate` with barrier parameter mu[p] and primal regularisation delta_w[p].
 * step [21K+10][batch]; inertia_out[p] = 0 if the KKT matrix had the correct inertia, 1 if not
 * (step then undefined).  Host pointers. */
int ascent_kkt_step(const ascent_params *p, int64_t batch, const ascent_opts *o,
                    const double *iterate, const double *mu, const double *delta_w, double *step,
                    int32_t *inertia_out, int device_id);

/* The same two parity surfaces through a chosen solver path.  ascent_eval_nodes / ascent_kkt_step above take the path
 * ascent_solve_batch would take for that batch (the same routing decision, environment overrides included; see
 * ascent_default_path); these run one round of exactly the kernels of the named path at the given iterate:
 *   ASCENT_PATH_FUSED       k_eval_nodes / the passes of k_solve (scheme 0, formulation 0 only)
 *   ASCENT_PATH_SPLIT_LANE  q_trial_eval -> q_decide_factor -> q_forward -> q_local -> q_adjoint
 *   ASCENT_PATH_SPLIT_WIDE  q_trial_eval -> q_factor_wide -> q_forward_wide -> q_local -> q_adjoint_wide
 *   ASCENT_PATH_PERSIST     p_solve / h_solve (the default of ascent_solve_batch): see the enum below
 *   ASCENT_PATH_DENSE       d_eval -> d_newton (ascent_kkt_step_path; with move_penalty = 1 as well, like ASCENT_PATH_PERSIST)
 * The split paths take schemes 0/1 and formulations 0/1.  For scheme 1 (trapezoid) `defects` is the trapezoid
 * defect and the Hessian block of node k is weighted by -(h*T*tf/2)*(lambda_k + lambda_{k+1}). */
enum ascent_path { ASCENT_PATH_AUTO = 0, ASCENT_PATH_FUSED = 1, ASCENT_PATH_SPLIT_LANE = 2, ASCENT_PATH_SPLIT_WIDE = 3,
                   ASCENT_PATH_DENSE = 4, /* d_eval -> d_newton, one wavefront per NLP on dense 8x8 blocks: schemes 0/1/2 */
                   ASCENT_PATH_PERSIST = 5 /* one round of the persistent kernel -- p_solve (schemes 0 / 1, formulation 1 with scheme 0) or
                                              h_solve (scheme 2, Hermite-Simpson, without the move penalty): ascent_kkt_step_path returns its
                                              Newton step; ascent_eval_nodes_path (schemes 0 / 1) the node rows it stages in LDS for the
                                              factorisation sweep, copied out before the sweep would read them */ };
/* Which kernels ascent_solve_batch runs for a batch of this size with these options (and the environment overrides
 * ASCENT_PIPELINE, ASCENT_FACTOR, ASCENT_SMALL_BATCH, ASCENT_DENSE_NEWTON, read on every call): an ascent_path value, never
 * ASCENT_PATH_AUTO -- the decision the solve itself makes, not a second copy of it.  No device work.  (A path that cannot
 * carry the options -- ASCENT_PIPELINE=split with the move penalty, say -- is reported as it is; the solve then refuses.) */
int ascent_default_path(int64_t batch, const ascent_opts *o);
/* Diagnostic (no device work): the persistent kernel's device workspace for a solve of `batch` NLPs with these options.
 * Returns the number of grid levels of the nested iteration (>= 1) or a negative code; out4[0] = bytes allocated,
 * out4[1] = bytes the finest level's kernels use from offset 0, out4[2] = offset of the second region (the two regions
 * alternate between the levels; 0 with one level), out4[3] = bytes the largest level living in the second region uses. */
int ascent_workspace_layout(int64_t batch, const ascent_opts *o, int64_t *out4);
int ascent_eval_nodes_path(const ascent_params *p, int64_t batch, const ascent_opts *o,
                           const double *iterate, double *defects, double *jac_blocks,
                           double *hess_blocks, int device_id, int path);
int ascent_kkt_step_path(const ascent_params *p, int64_t batch, const ascent_opts *o,
                         const double *iterate, const double *mu, const double *delta_w, double *step,
                         int32_t *inertia_out, int device_id, int path);

/* Dense stage records as the dense-block path's node kernel (d_eval) leaves them at `iterate` (parity surface for the
 * Hermite-Simpson derivatives): records[batch][K][6][64] doubles, six row-major 8x8 grids per step (7 states + one
 * padding slot): 0 = d c_k/d z_{k-1}, 1 = d c_k/d z_k, 2/3/4 = the (z_{k-1},z_{k-1}) / (z_{k-1},z_k) / (z_k,z_k) blocks of the
 * Hessian of lambda_k'c_k, 5 = vectors by row: c_k, d c_k/du_k, d c_k/d tf, and the (z_{k-1},tf), (z_k,tf) Hessian
 * columns.  Host pointers. */
int ascent_dense_records(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *iterate,
                         double *records, int device_id);

/* The coast arc after the burn (second phase of BASELINE config 5; the reference's v1 script propagated it with
 * explicit Euler, PDF p28-29): Kepler-exact two-body propagation of every problem's final state to the next
 * apoapsis of its orbit, sampled uniformly in time.
 * final_state [4][batch]: scaled x, y, xdot, ydot of the last node (rows 0..3 of traj_out at node n_nodes-1);
 * coast_traj [4][coast_nodes+1][batch] (same scaled units), coast_nodes 1 .. 65535; node j is the state after
 *   j * coast_tf * T_scale / coast_nodes seconds.  Node 0 is the input state, bit for bit: the arc is propagated from the
 *   burnout state itself (Kepler's equation in the difference of the eccentric anomaly, Lagrange's f and g coefficients), with
 *   e cos E0 = 1 - r/a and e sin E0 = r.v / sqrt(GM a) used as they are -- nothing is divided by the eccentricity, so the arc is
 *   continuous through e -> 0 and there is no near-circular switch;
 * coast_tf [batch]: coast duration / T_scale = (pi - M0) / n with M0 = E0 - e sin E0, E0 = atan2(e sin E0, e cos E0) in
 *   (-pi, pi]: 0 <= duration < one period.  Near the circle E0, and with it the duration, is as ill-determined as the place of
 *   the apsides themselves (an input rounding moves it by about eps / e); where e sin E0 and e cos E0 are both exactly 0 the
 *   duration is half a period;
 * apsides [2][batch]: periapsis and apoapsis altitude above R0, m: the one definition of the library (also rows 2..5 of
 *   ascent_fly_batch): e = |eccentricity vector|, periapsis h^2 / (GM (1 + e)) - R0, apoapsis a (1 + e) - R0 with the semi-major
 *   axis from the vis-viva equation.
 * Specific energy >= 0 (parabolic or faster) is not an error: the call returns ASCENT_OK, that problem's coast_traj and coast_tf
 *   are NaN, its periapsis is the same expression and its apoapsis +inf; the other problems of the batch are not affected.
 * Host or device pointers (ptr_is_device), optional stream (device pointers and a stream: one kernel is enqueued). */
int ascent_coast_batch(const ascent_params *p, int64_t batch, const double *final_state, int32_t coast_nodes,
                       double *coast_traj, double *coast_tf, double *apsides, int device_id,
                       void *hip_stream_or_null, int ptr_is_device);

/* Post-optimal sensitivity (envelope theorem) of the optimal objective to every ascent_params field, from a
 * solution blob written by ascent_solve_batch with the same options.  grad_out [16][batch]: row i is d J* / d(field i of
 * ascent_params, in declaration order), in units of the scaled objective per SI unit of that field, where J is the
 * objective of the scaled NLP as solved: tf (= final time / T_scale), plus dcost * sum_k |u_k - u_{k-1}| with
 * move_penalty = 1 (formulation 1: weight dcost * angle_ub / 2, u_{-1} = -1).  The value is the partial derivative of
 * the Lagrangian at the blob,  dJ/dp + lambda' dc/dp + nu' d(terminal)/dp + zL' d lb/dp - zU' d ub/dp  (defects of the
 * scheme, formulation 1's angle row, the terminal conditions of o->terminal, the angle_ub and tf bounds, and the penalty
 * sum taken from the blob's controls): one read of the blob, no KKT solve.  It is the derivative of the optimum only at
 * a converged solution: for problems whose status was not ASCENT_CONVERGED the rows are defined (computed at whatever
 * the blob holds) but meaningless.  d(final time)/dp in seconds = T_scale * row, plus tf for the T_scale row.
 * Options: refuses (ASCENT_E_ARG) exactly what ascent_solve_batch refuses for these options and this batch; the fields
 * that only steer the iteration (max_iter, tol, mu_init, warm_start) are not read.  Host or device pointers
 * (ptr_is_device); with device pointers and a stream the call only enqueues one kernel. */
int ascent_param_sensitivity(const ascent_params *p, int64_t batch, const ascent_opts *o,
                             const double *sol_blob, double *grad_out,
                             int device_id, void *hip_stream_or_null, int ptr_is_device);

/* Flight verification: what a solution's control reaches when it is flown.  The solver returns the minimiser of the
 * discretised problem; this integrates the model's ODEs (Launch_Optimiser.py:114-136, scaled as everywhere here) under the
 * control of a solution blob written by ascent_solve_batch with the same options, with a fixed-step classical RK4 on the
 * device, and reports the distance between the flown trajectory and the NLP's.
 * Model: node 0 is the zero initial state; step k (node k-1 -> k, duration dt = tf * T_scale / K seconds) flies with the
 * blob's u_k held constant, for every scheme; formulation 1: the angle is held at (angle_ub/2)(u_k + 1) over step k and
 * angledot stays 0.  move_penalty and terminal do not change the ODEs.
 * substeps: RK4 steps per collocation step, 1 .. ASCENT_FLIGHT_MAX_SUBSTEPS for every problem, or 0 = automatic: per problem
 * m = clamp(ceil(dt / 0.5 s), 1, ASCENT_FLIGHT_MAX_SUBSTEPS), m = 1 if dt is not finite (the RK4 error of a whole ascent is
 * then below 1e-4 m; DESIGN.md has the measurement).
 * flown_traj_out_or_null [10*n_nodes][batch]: the flown trajectory in the layout and field order of traj_out (accelerations
 *   evaluated at the flown state; the control row as ascent_solve_batch writes it for this blob).
 * local_err_out_or_null [7K][batch], row 7(k-1)+f: eta_k = (the NLP's z_{k-1} flown over step k) - z_k, the local
 *   discretisation error of every collocation step, scaled units; steps are independent of each other.
 * summary_out [ASCENT_FLIGHT_ROWS][batch], SI units:
 *   0 position miss |flown - NLP| at the last node (m)        1 velocity miss (m/s)
 *   2 / 3 periapsis / apoapsis altitude above R0 of the flown burnout orbit (m)    4 / 5 the same for the NLP's last node
 *         (the same function as ascent_coast_batch's apsides, bit for bit; specific energy >= 0 gives apoapsis +inf)
 *   6 max over steps of the local position error |eta_k(x, y)| (m)      7 of the local velocity error (m/s)
 *   8 the step k (1-based) where row 6 is attained         9 the m used
 * Options: refuses (ASCENT_E_ARG) exactly what ascent_solve_batch refuses for these options and this batch; max_iter, tol,
 * mu_init, warm_start are not read.  For problems whose status was not ASCENT_CONVERGED the rows are defined (computed from
 * whatever the blob holds, NaN allowed) but meaningless; the work per problem is bounded by 4 * K * ASCENT_FLIGHT_MAX_SUBSTEPS
 * right-hand sides whatever the blob holds -- a bound, not a small one: a garbage t_f on a grid of tens of thousands of nodes
 * keeps one lane busy for minutes, so callers with long grids should not pass blobs of unconverged problems as they are (set
 * their t_f row to 0 or NaN: m = 1).  Host or device pointers (ptr_is_device); with device pointers and a stream the
 * call only enqueues two kernels (no host read, no synchronisation). */
#define ASCENT_FLIGHT_ROWS 10
#define ASCENT_FLIGHT_MAX_SUBSTEPS 4096
int ascent_fly_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                     int32_t substeps, double *flown_traj_out_or_null, double *local_err_out_or_null,
                     double *summary_out, int device_id, void *hip_stream_or_null, int ptr_is_device);

/* Flight Jacobian: the exact derivative of the discrete RK4 flight that ascent_fly_batch computes -- the open-loop
 * counterpart of ascent_param_sensitivity (which gives d t_f* / dp under re-optimisation): what a dispersed vehicle does under
 * the nominal control.  The map is F(z_0, p, t_f, u_1..u_K) -> the flown state at the last node: RK4 with m substeps per
 * collocation step, m as ascent_fly_batch picks it at the blob (substeps = 0) and then held fixed; formulation 1 resets the
 * angle at the start of every step.  It is the derivative of the arithmetic itself (the tangent of every RK4 stage), so it
 * agrees with finite differences of ascent_fly_batch to their truncation error.
 * Rows q (9): 0..6 the flown z_K in scaled units (x y xdot ydot angle angledot mass); 7 / 8 the flown periapsis / apoapsis
 *   altitude in metres (summary rows 2 / 3 of ascent_fly_batch); row 8 is NaN where the flown specific energy is >= 0.
 *   The eccentricity and its derivative come from the eccentricity vector (relative error about eps / e).  On an exactly
 *   circular flown orbit (e = 0) the apsides have a kink and no derivative: rows 7 and 8 are then both the gradient of a - R0
 *   (the mean of the one-sided derivatives; finite); row 7 + row 8 is the gradient of 2 a - 2 R0 at every e.
 * jac_out [9][24][batch], element (q, c, problem) at jac_out[(q*24 + c)*batch + problem]: columns 0..6 the initial state z_0
 *   (zero in every blob; scaled units), 7..22 the 16 ascent_params fields in declaration order, per SI unit of the field with
 *   the blob held fixed in scaled units, 23 the scaled t_f.  Fields the flight does not read give exact zeros: r_apo, tf_lb,
 *   tf_ub, dcost, angle_ub in formulation 0, ang_acc_max in formulation 1.
 * jac_u_out_or_null [9][K][batch]: entry (q, k-1) is d/d u_k.
 * Options: refuses (ASCENT_E_ARG) exactly what ascent_fly_batch refuses, plus terminal = 2.  Garbage blobs: the work is
 * bounded as in ascent_fly_batch (K / 16 chunks of at most 4 * ASCENT_FLIGHT_MAX_SUBSTEPS serial right-hand sides after the
 * fly-out itself); NaN rows are allowed.  A problem gives the same bits alone as inside any batch.  Host or device pointers
 * (ptr_is_device); with device pointers and a stream the call only enqueues two kernels (the library's workspace for these
 * two entry points is allocated on the first call of that size). */
int ascent_flight_jacobian(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                           int32_t substeps, double *jac_out, double *jac_u_out_or_null, int device_id,
                           void *hip_stream_or_null, int ptr_is_device);

/* Trim: a least-norm Newton correction of (t_f, u) that drives the FLOWN terminal conditions to zero, so that the control,
 * flown by ascent_fly_batch, reaches the orbit the NLP asked for.  Conditions c(z): e3, g1, g2 of the terminal constraints
 * (r.v = 0, radius, speed^2 with the target speed of o->terminal = 0 or 1), as equalities, at the flown last node, scaled units.
 * One round, per problem: fly; stop and freeze if |c|_inf <= tol; A = grad c [J_tf | J_u] (3 x (K+1), from rows 0..6 of the
 * flight Jacobian); weights W: t_f 1, u_k 1 where |u_k| < 0.999 and 0 otherwise (saturated controls stay where they are);
 * delta = -W A' (A W A')^-1 c;  t_f += delta_0,  u <- clip(u + delta, -1, 1).  `rounds` rounds are enqueued (1 .. 32, 0 = 6);
 * converged problems freeze themselves on the device, there is no host round trip.  tol <= 0: 1e-10.  With substeps = 0 every
 * round picks m from its current t_f.  A non-finite condition or a pivot of the 3 x 3 normal matrix below 1e-300 freezes the
 * problem with status 2: no fault, bounded work.
 * trim_blob_out [21K+10][batch]: the input blob with the u rows and the t_f row replaced and the state rows replaced by the
 *   flown states of the trimmed control (ascent_fly_batch on it reports zero local error).  The multipliers are copied
 *   unchanged and are STALE: the trimmed point is not a KKT point of the NLP.
 * summary_out [ASCENT_TRIM_ROWS][batch]:
 *   0 status: 0 converged, 1 rounds exhausted, 2 frozen as non-finite or singular       1 rounds used (updates applied)
 *   2 final |c|_inf        3 |c|_inf before the first round        4 delta t_f in seconds        5 max_k |u_k - u_k(input)|
 *   6 number of free controls (|u_k| < 0.999) at the last round that looked at the problem
 *   7 / 8 flown periapsis / apoapsis altitude after the trim, m (as ascent_fly_batch rows 2 / 3)
 *   9 the largest violation of 0 <= angle <= angle_ub along the trimmed flight (scaled angle; 0 = none)
 * Options, pointers and stream as ascent_flight_jacobian; with device pointers and a stream the call only enqueues (one copy,
 * one memset, three kernels per round and two more). */
#define ASCENT_TRIM_ROWS 10
int ascent_trim_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                      int32_t rounds, double tol, double *trim_blob_out, double *summary_out, int device_id,
                      void *hip_stream_or_null, int ptr_is_device);

/* Monte Carlo dispersion: what a dispersed vehicle does under the nominal control, beyond the linear answer of
 * ascent_flight_jacobian.  Every problem's blob is flown `samples` times with perturbed inputs and the nine end quantities of
 * the flight Jacobian (rows q: the flown z_K in scaled units, the flown periapsis / apoapsis altitude in metres) are reduced on
 * the device to their count, mean, covariance and extrema; the blob is shared by the samples, never tiled.
 * Perturbations: sample s of problem b flies the blob's control exactly as ascent_fly_batch does, with
 *   z_0[i] = sigma[i][b] * xi[i][s] (scaled units; i = 0..6),
 *   field i of ascent_params (SI, declaration order) + sigma[7+i][b] * xi[7+i][s], the derived constants recomputed per sample,
 *   the scaled t_f + sigma[23][b] * xi[23][s],
 *   u_k + sigma_u[k-1][b] * xi[24+k-1][s], not clipped (a control execution error is physical).
 *   The blob stays fixed in scaled units -- the convention of the flight Jacobian, so J (sigma o xi_s) is the first-order
 *   prediction of sample s.  xi is the caller's table, normally unit normals, shared by every problem of the batch (common
 *   random numbers: the problems of a sweep see the same draws).  A perturbation is applied only where its sigma is non-zero:
 *   with sigma = 0 the quantity is the nominal one bit for bit, whatever xi holds.
 * substeps: as ascent_fly_batch; the m picked at the nominal blob and the nominal T_scale is held for every sample, as the
 *   Jacobian holds it: the work per sample is bounded by 4 * K * m right-hand sides whatever xi holds.
 * A sample is valid if all nine rows are finite (an escaping sample has apoapsis +inf and is invalid); invalid samples are left
 *   out of every statistic and are counted by their absence from row 0.
 * xi [24 + K][samples], sample index fastest ([24][samples] suffices when sigma_u is null); sigma [24][batch];
 *   sigma_u_or_null [K][batch].
 * stats_out [ASCENT_DISPERSE_STAT_ROWS][batch]:
 *   0        the number of valid samples n
 *   1..9     the nominal flight's nine rows (rows 8 / 9 are summary rows 2 / 3 of ascent_fly_batch on the same blob, bit for bit)
 *   10..18   mean                         19..63  upper triangle, row-major, of the unbiased sample covariance (NaN where n < 2)
 *   64..72 / 73..81   minimum / maximum over the valid samples (NaN where n = 0)
 *   Moments are accumulated on the differences from the nominal rows (centre 0 for a nominal row that is not finite), so that a
 *   standard deviation of 1e-8 of the mean keeps its digits; with n = 1 the mean is that sample itself.  The order of the additions is fixed -- a butterfly inside a
 *   wavefront, the four wavefronts of a workgroup (256 consecutive samples) in order, the workgroups in ascending order --: the
 *   result depends on `samples`, not on the batch size, the problem's place in the batch, host or device pointers, or timing.
 * samples_out_or_null [9][samples][batch], element (q, s, problem) at ((q*samples + s)*batch + problem): every sample's nine rows,
 *   invalid ones as they came out.
 * Options: refuses (ASCENT_E_ARG) exactly what ascent_fly_batch refuses (terminal = 2 is accepted: the terminal mode does not
 * enter the flight), samples outside 1 .. ASCENT_DISPERSE_MAX_SAMPLES, and a null xi, sigma or stats_out.  Garbage blobs: bounded
 * work as stated; a blob with a non-finite t_f gives n = 0 and NaN statistics.  Host or device pointers (ptr_is_device); with
 * device pointers and a stream the call only enqueues (f_fly, f_disperse, f_disperse_stats; no host read, no synchronisation).
 * The device workspace -- the nominal trajectory and ceil(samples / 256) partial records of 73 doubles per problem -- is the one
 * of ascent_flight_jacobian / ascent_trim_batch. */
#define ASCENT_DISPERSE_COLS 24     /* columns of ascent_flight_jacobian's jac_out: z_0 (7), the 16 ascent_params fields, scaled t_f */
#define ASCENT_DISPERSE_ROWS 9      /* rows q of ascent_flight_jacobian: flown z_K (scaled), flown periapsis / apoapsis altitude (m) */
#define ASCENT_DISPERSE_STAT_ROWS 82
#define ASCENT_DISPERSE_MAX_SAMPLES 65536
int ascent_disperse_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                          int32_t substeps, int32_t samples, const double *xi, const double *sigma,
                          const double *sigma_u_or_null, double *stats_out, double *samples_out_or_null, int device_id,
                          void *hip_stream_or_null, int ptr_is_device);

/* Guidance gains: the neighbouring-optimal linear feedback about a flown solution -- what a dispersed vehicle needs to steer
 * back to the nominal flight and to cut off on its state, where ascent_disperse_batch flies it open loop.
 * Linearisation: that of ascent_flight_jacobian, about the flight ascent_fly_batch computes at the blob.  Deviations (scaled
 * units) obey dz_k = Phi_k dz_{k-1} + g_k du_k + [k = K] gamma_K tau: Phi_k = dz_k/dz_{k-1}, g_k = dz_k/du_k, gamma_K = dt *
 * dz_K/d dt, tau the relative stretch of the last step's duration (the cutoff channel).
 * Cost: 1/2 sum_i q_i (c_i' dz_K)^2 + 1/2 r_u sum_k du_k^2 + 1/2 r_t tau^2, c_i the gradients of the trim's three conditions
 *   (e3, g1, g2) at the nominal flown z_K.  The target is the nominal flown end conditions, not c = 0: pass a trimmed blob
 *   (ascent_trim_batch) to aim at the orbit.
 * weights [6][batch]: q_e3, q_g1, q_g2 >= 0, r_u > 0, r_t > 0, stretch_max >= 0 (the bound of |tau|; 0: no cutoff channel).
 * Recursion, plain form, k = K .. 1 from P_K = sum_i q_i c_i c_i': B holds the column g_k if |u_k| < 0.999 (the trim's rule: a
 *   saturated control has no authority and its gain row is exactly 0) and the column gamma_K if k = K and stretch_max > 0;
 *   S = R + B' P_k B, G = S^-1 B' P_k Phi_k, P_{k-1} = Phi_k' P_k Phi_k - G' S G, symmetrised by averaging; without a column
 *   P_{k-1} = Phi_k' P_k Phi_k.  In double precision the recursion loses digits as q grows (relative to an 80-bit run of itself:
 *   about 1e-12 at q = 1e6, 5e-8 at 1e9, 3e-5 at 1e12 on the nominal problem).
 * gain_u_out [7][K][batch], element (state i, step k-1, problem) at ((i*K + k-1)*batch + problem): K_k, so that the commanded
 *   control of step k is u_k - K_k . (z - z_{k-1}^nominal).   gain_t_out [7][batch]: k_t, tau = -k_t . (z - z_{K-1}^nominal); zero
 *   where stretch_max = 0.
 * summary_out [ASCENT_GUIDE_ROWS][batch]: 0 status (0 ok, 2 frozen)   1 number of free controls (|u_k| < 0.999)
 *   2 max_k |K_k|_inf   3 |k_t|_inf   4 the substeps m used.
 * A non-finite S, a pivot or a determinant of S <= 0, or a weights column outside the ranges above freezes the problem: status
 *   2, NaN gains, NaN rows 2 / 3 and a NaN closed-loop Jacobian; no fault, bounded work.
 * jac_cl_out_or_null [9][24][batch], jac_u_cl_out_or_null [9][K][batch] (the latter only with the former): the flight Jacobian
 *   of the closed loop under these gains, clips ignored, rows / columns / layout of ascent_flight_jacobian; the column of u_k now
 *   means the execution error of step k.  Where every gain is zero (q = 0) it is ascent_flight_jacobian's.
 * Options, substeps, refusals (terminal = 2 included), garbage blobs, pointers and stream as ascent_flight_jacobian; a problem
 * gives the same bits alone as inside any batch; with device pointers and a stream the call only enqueues two kernels. */
#define ASCENT_GUIDE_ROWS 5
int ascent_guidance_gains(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                          const double *weights, double *gain_u_out, double *gain_t_out, double *summary_out,
                          double *jac_cl_out_or_null, double *jac_u_cl_out_or_null, int device_id, void *hip_stream_or_null,
                          int ptr_is_device);

/* Guided Monte Carlo dispersion: ascent_disperse_batch with every sample steering by a linear state feedback.  The gains are the
 * caller's (ascent_guidance_gains' or any other), layouts as above.  Sample s at step k, from its state z at node k-1 (perfect
 * state knowledge; blob and nominal flight fixed in scaled units):
 *   dz = z - z_{k-1}^nominal (the flight of ascent_fly_batch at the blob);
 *   commanded control clip(u_k - K_k . dz, -1, 1); where the gain row of the step is all zero, u_k itself, bit for bit;
 *   executed control: the command + sigma_u[k-1][b] * xi[24+k-1][s], not clipped;
 *   on the last step, with gain_t and stretch_max both given and stretch_max[b] > 0: the sample's dt times
 *   1 + clip(-k_t . dz, -stretch_max[b], +stretch_max[b]).
 *   A K_k . dz or k_t . dz that is not finite (NaN or inf gains) makes the command NaN: the sample is invalid.
 * m is held as in ascent_disperse_batch: 4 * K * m right-hand sides per sample whatever the gains hold.
 * stats_out exactly as ascent_disperse_batch: same reduction, same fixed order, same validity rule.  With all-zero gains and no
 * stretch the call gives the bits of ascent_disperse_batch.
 * samples_out_or_null [ASCENT_GUIDED_SAMPLE_ROWS][samples][batch]: the nine rows, then the number of steps whose command was
 *   clipped, max_k |K_k . dz|, and the stretch applied.
 * Refuses what ascent_disperse_batch refuses, and a null gain_u. */
#define ASCENT_GUIDED_SAMPLE_ROWS 12
int ascent_disperse_guided_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                                 int32_t substeps, int32_t samples, const double *xi, const double *sigma,
                                 const double *sigma_u_or_null, const double *gain_u, const double *gain_t_or_null,
                                 const double *stretch_max_or_null, double *stats_out, double *samples_out_or_null,
                                 int device_id, void *hip_stream_or_null, int ptr_is_device);

/* Guidance gains with a parameter feed-forward: ascent_guidance_gains for a vehicle that knows (an estimate of) one of its own
 * parameter deviations -- its thrust, from an accelerometer -- and plans the rest of the burn with it.
 * ff_dir [16][batch]: a direction d in the space of the 16 ascent_params fields (SI, declaration order), per problem.  The
 *   parameter deviation is theta * d with a constant scalar theta in the units d implies (d = e_Ft: newtons of thrust).
 * Dynamics: dz_k = Phi_k dz_{k-1} + g_k du_k + pi_k theta + [k = K] gamma_K tau, pi_k = Gamma_k d: the step's derivative with
 *   respect to the fields (blob fixed in scaled units, as ascent_flight_jacobian) along d.  The "direct" dependence of the
 *   apsides on G, M, R0 and r_peri is not part of pi_k.  Cost, weights, columns and the 0.999 / stretch_max rules: unchanged.  The
 *   target stays the nominal flown end conditions linearised in z; a direction that moves the conditions themselves (G, M, R0,
 *   r_peri, r_apo) is accepted and treated the same way, and is then not the neighbouring optimum of the orbit target.
 * Recursion: the value function 1/2 [dz; theta]' [[P, p], [p', pi0]] [dz; theta], p_K = 0.  P, S and G are ascent_guidance_gains'
 *   (certainty equivalence).  Per step, a = P_k pi_k + p_k: f = S^-1 B' a, p_{k-1} = Phi_k' a - G' S f; without a column f = 0 and
 *   p_{k-1} = Phi_k' a.  pi0 is not computed.
 * Law: du_k = -K_k . dz - f_k theta-hat, tau = -k_t . dz - f_t theta-hat, theta-hat what the vehicle believes theta is.
 * gain_u_out, gain_t_out and summary rows 0..4 are the bits of ascent_guidance_gains for the same inputs, whatever ff_dir holds.
 * ff_u_out [K][batch]: f_k (exactly 0 for a saturated control);  ff_t_out [batch]: f_t (0 where stretch_max = 0).
 * summary_out [ASCENT_GUIDE_FF_ROWS][batch]: rows 0..4 as ascent_guidance_gains, 5 max_k |f_k|, 6 |f_t|.
 * ff_know_or_null [16][batch]: a row w with theta-hat = w . dp, dp the vehicle's 16 SI parameter deviations (for d = e_Ft and a
 *   thrust known exactly, w = e_Ft).  Needed by the closed-loop Jacobian only.
 * jac_cl_out_or_null, jac_u_cl_out_or_null: as ascent_guidance_gains, of the closed loop under the law above with theta-hat =
 *   w . dp: every parameter column c is ascent_guidance_gains' minus E w_c, E = sum_k (Lambda_k g_k) f_k + (Lambda_K gamma_K) f_t.
 * jac_nav_out_or_null [9][ASCENT_NAV_ROWS][batch] (only with jac_cl_out): the derivative of the nine rows with respect to
 *   columns 0..6, a bias nu of the vehicle's state knowledge (it steers on dz + nu; scaled units):
 *   -sum_k (Lambda_k g_k) K_k' - (Lambda_K gamma_K) k_t';  column 7, an error of theta-hat: -E.
 *   Row 8 is NaN where the flown energy is >= 0, as everywhere.
 * With ff_dir = 0: ff_u, ff_t and column 7 of jac_nav are zero and jac_cl, jac_u_cl are ascent_guidance_gains' bits.
 * A non-finite entry of ff_dir or ff_know freezes the problem like a bad weight: status 2, NaN gains, feed-forward and Jacobians.
 * Refuses what ascent_guidance_gains refuses, a null ff_dir, ff_u_out or ff_t_out, jac_nav_out without jac_cl_out, and jac_cl_out
 * without ff_know.  Everything else as ascent_guidance_gains; with device pointers and a stream the call only enqueues two
 * kernels (f_fly, g_gains_ff). */
#define ASCENT_NAV_ROWS 8            /* 7 state-knowledge biases (scaled units), 1 error of theta-hat */
#define ASCENT_GUIDE_FF_ROWS 7       /* ASCENT_GUIDE_ROWS, then 5 max_k |f_k|, 6 |f_t| */
int ascent_guidance_feedforward(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                                int32_t substeps, const double *weights, const double *ff_dir, const double *ff_know_or_null,
                                double *gain_u_out, double *gain_t_out, double *ff_u_out, double *ff_t_out, double *summary_out,
                                double *jac_cl_out_or_null, double *jac_u_cl_out_or_null, double *jac_nav_out_or_null,
                                int device_id, void *hip_stream_or_null, int ptr_is_device);

/* Guided Monte Carlo dispersion with a feed-forward and navigation errors: ascent_disperse_guided_batch where no sample knows
 * its state perfectly and every sample has a belief theta-hat about its parameter deviation.  Sample s of problem b:
 *   nu_i = sigma_nav[i][b] * xi_nav[i][s] where that sigma is non-zero, else 0 (i = 0..6; scaled units);
 *   theta-hat = sum_i ff_know[i][b] * (the applied deviation of field i: sigma[7+i][b] * xi[7+i][s] where that sigma is non-zero,
 *   else 0; formed as (ff_know * sigma) * xi) + sigma_nav[7][b] * xi_nav[7][s] where that sigma is non-zero; 0 where ff_know is
 *   null and sigma_nav[7][b] = 0.
 * At step k: dz_i = z_i - z_i^nominal as ascent_disperse_guided_batch, then dz_i += nu_i only where nu_i is applied.  Where the
 *   gain row of the step is all zero and f_k = 0 the command is u_k itself, bit for bit; otherwise w = u_k - K_k . dz, then
 *   w -= f_k * theta-hat only where f_k != 0, and the command is clip(w, -1, 1), NaN where K_k . dz + f_k theta-hat is not finite.
 *   Execution error and stretch as ascent_disperse_guided_batch with dtau = -k_t . dz, then - f_t * theta-hat where f_t != 0.
 * samples_out row 10 is max_k |K_k . dz + f_k theta-hat|.  The 12 sample rows, the held m, the validity rule, the 82-row
 *   reduction and its fixed order: ascent_disperse_guided_batch's.
 * ff_u_or_null [K][batch], ff_t_or_null [batch], ff_know_or_null [16][batch] (only with ff_u), xi_nav_or_null
 *   [ASCENT_NAV_ROWS][samples], sample fastest, and sigma_nav_or_null [ASCENT_NAV_ROWS][batch] (both or neither).
 * With the five all null, or all given and zero, the call gives ascent_disperse_guided_batch's bits.
 * Refuses what ascent_disperse_guided_batch refuses, xi_nav without sigma_nav or the reverse, and ff_know without ff_u. */
int ascent_disperse_navigated_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                                    int32_t substeps, int32_t samples, const double *xi, const double *sigma,
                                    const double *sigma_u_or_null, const double *gain_u, const double *gain_t_or_null,
                                    const double *stretch_max_or_null, const double *ff_u_or_null, const double *ff_t_or_null,
                                    const double *ff_know_or_null, const double *xi_nav_or_null, const double *sigma_nav_or_null,
                                    double *stats_out, double *samples_out_or_null, int device_id, void *hip_stream_or_null,
                                    int ptr_is_device);

/* Monte Carlo history: the dispersion corridor of a flight.  One of the three dispersion calls above, with the samples reduced
 * not only at the end of the burn but at the nodes on the way: how wide the corridor is, whether a sample comes back to the
 * surface, whether the guided vehicle leaves its angle bounds, where the feedback clips.
 * Which flight: gain_u null -- ascent_disperse_batch's (gain_t, stretch_max, ff_*, xi_nav and sigma_nav must then be null);
 *   gain_u given -- ascent_disperse_navigated_batch's, which with everything after stretch_max null is
 *   ascent_disperse_guided_batch's bit for bit.  stats_out [82][batch] and the rows of samples_out_or_null are the bits of that
 *   call on the same inputs; samples_out is always [ASCENT_GUIDED_SAMPLE_ROWS][samples][batch], rows 9..11 exactly 0 in the
 *   open-loop flight.  The history changes nothing those calls compute.
 * History nodes: node_stride in 1 .. K; NJ = K / node_stride + (K % node_stride != 0) nodes j_i = min((i + 1) * node_stride, K),
 *   i = 0 .. NJ-1: every node_stride-th node and always the last one.  Node 0 (the perturbation of z_0 itself) is not reported.
 * The ASCENT_HISTORY_QUANTITIES quantities q of sample s at node j:
 *   0..6  the flown state z at node j, scaled units (on the last node after the cutoff stretch)
 *   7     altitude (m): sqrt(X*X + Y*Y) - R0, X = x * r_peri, Y = y * r_peri + R0, with the sample's own perturbed fields
 *   8     the executed control of step j, the step that ends at node j: the command + sigma_u * xi, what the flight was given (in
 *         formulation 1 the normalised angle command)
 *   9     the correction of step j, K_j . dz + f_j * theta-hat; exactly 0 where the step's gain row and f_j are all zero, and in
 *         the open-loop flight.
 * A sample is valid at node j if its ten quantities there are all finite (a NaN stays: the count does not rise with j).  This
 *   is not the rule of stats_out, which also asks for a finite apoapsis: an escaping sample is valid in the history.
 * hist_out [ASCENT_HISTORY_ROWS][NJ][batch], element (row r, node i, problem) at ((r*NJ + i)*batch + problem):
 *   0        n, the number of samples valid at the node
 *   1..10    the nominal flight's ten quantities: state and altitude from the trajectory of ascent_fly_batch on the blob with the
 *            nominal fields, the blob's u_j, correction 0
 *   11..20   mean              21..30   unbiased variance (NaN where n < 2)
 *   31..40 / 41..50   minimum / maximum over the valid samples (NaN where n = 0)
 *   51       the number of valid samples whose command of step j was clipped (the rule behind samples_out row 9; counted only where
 *            the step has a gain or a feed-forward; 0 in the open-loop flight)
 *   Moments on the differences from the nominal rows (centre 0 where a nominal row is not finite), the expressions of stats_out:
 *   mean = centre + sum / n (n = 1: the sample itself), variance = (sum of squares - sum * sum / n) / (n - 1).  The order of the
 *   additions is that of stats_out: a butterfly inside a wavefront, the wavefronts of a workgroup in order, the workgroups in
 *   ascending order.  Where every sample is valid under both rules, rows 0, 11..17, 21..27, 31..37 and 41..47 of the last node are,
 *   bit for bit, rows 0, 10..16, the seven diagonal covariance entries of the state (19, 28, 36, 43, 49, 54, 58), 64..70 and
 *   73..79 of stats_out.  A node's rows do not depend on node_stride, the batch size, the problem's place in the batch, host or
 *   device pointers, or whether the optional outputs were asked for.
 * hist_samples_out_or_null [ASCENT_HISTORY_QUANTITIES][NJ][samples][batch], element (q, i, s, problem) at
 *   (((q*NJ + i)*samples + s)*batch + problem): every sample's ten quantities, invalid ones as they came out.  The only thing of
 *   size samples * K, and only when asked for.
 * Refuses (ASCENT_E_ARG, before the device is looked at, no array touched) what ascent_disperse_navigated_batch refuses, a null
 *   hist_out, node_stride outside 1 .. K, and any of gain_t, stretch_max, ff_*, xi_nav, sigma_nav without gain_u.  terminal = 2 is
 *   accepted.  Garbage blobs: bounded work as ascent_disperse_batch; a non-finite t_f gives n = 0 and NaN rows at every node.
 * Host or device pointers; with device pointers and a stream the call only enqueues (f_fly, f_disperse with the history or f_history_guided,
 *   f_disperse_stats, f_history_stats; no host read, no synchronisation).  Device workspace: that of ascent_disperse_batch plus
 *   ceil(samples / 256) * NJ * 42 * batch doubles of partial records. */
#define ASCENT_HISTORY_QUANTITIES 10
#define ASCENT_HISTORY_ROWS 52
int ascent_disperse_history_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                                  int32_t substeps, int32_t samples, const double *xi, const double *sigma,
                                  const double *sigma_u_or_null, const double *gain_u_or_null, const double *gain_t_or_null,
                                  const double *stretch_max_or_null, const double *ff_u_or_null, const double *ff_t_or_null,
                                  const double *ff_know_or_null, const double *xi_nav_or_null, const double *sigma_nav_or_null,
                                  int32_t node_stride, double *stats_out, double *samples_out_or_null, double *hist_out,
                                  double *hist_samples_out_or_null, int device_id, void *hip_stream_or_null, int ptr_is_device);

/* Linear covariance corridor: what ascent_disperse_history_batch samples, to first order and without sampling -- the covariance
 * of the ten history quantities at every history node from one deterministic forward sweep per problem, and their derivative.
 * Model: the derivative of the arithmetic of ascent_disperse_history_batch's flight about the nominal flight of ascent_fly_batch at
 *   the blob; clips ignored, the substeps m held, the blob fixed in scaled units.  Which flight: gain_u null -- the open loop;
 *   gain_u given -- the navigated one (with everything after stretch_max null, the guided one), the arguments and their "both or
 *   neither" rules as in that call.
 * Constants c, ASCENT_LINCOV_COLS = ASCENT_DISPERSE_COLS + ASCENT_NAV_ROWS columns: 0..6 dz_0 (scaled), 7..22 the 16 fields (SI),
 *   23 the scaled t_f, 24..30 the knowledge bias nu (scaled), 31 the error e of theta-hat = w . dp + e (w = ff_know, 0 where null).
 *   sigma [24][batch] and sigma_nav_or_null [8][batch] (null: zero) are their standard deviations; sigma_u_or_null [K][batch] that
 *   of the white execution error eps_k of step k, independent per step.
 * Step k: corr_k = K_k . (dz_{k-1} + nu) + f_k theta-hat, du_k = -corr_k + eps_k, dz_k = Phi_k dz_{k-1} + g_k du_k + Gamma_k dp +
 *   (dz_k/dt_f) dt_f, and on step K, with gain_t and stretch_max > 0, + gamma_K tau, tau = -k_t . (dz_{K-1} + nu) - f_t theta-hat;
 *   Phi_k, g_k, Gamma_k, gamma_K as ascent_guidance_gains / ascent_guidance_feedforward state them.
 * The ten quantities y_j: the rows of ascent_disperse_history_batch -- 0..6 dz_j, 7 the altitude (its gradient at the nominal
 *   node times dz_j, plus its direct dependence on R0 and r_peri), 8 du_j, 9 corr_j.
 * History nodes: node_stride, NJ and j_i as ascent_disperse_history_batch; node 0 is not reported.
 * nominal_out [10][NJ][batch]: rows 1..10 of hist_out of ascent_disperse_history_batch on the same blob, bit for bit.
 * jac_hist_out_or_null [10][ASCENT_LINCOV_COLS][NJ][batch], element (q, c, i, problem) at (((q*32 + c)*NJ + i)*batch + problem):
 *   S_j = d y_j / d c.  At node K rows 0..6 are those of ascent_flight_jacobian (open loop) or of jac_cl | jac_nav of
 *   ascent_guidance_feedforward, computed forward instead of by the adjoint sweep.
 * cov_out [ASCENT_LINCOV_COV_ROWS][NJ][batch]: the upper triangle of cov_j, row by row ((0,0), (0,1), .., (0,9), (1,1), ..):
 *   cov_j = S_j diag(sigma_c^2) S_j' + N_j, summed over the columns in ascending order, a column whose sigma is 0 contributing
 *   exactly 0, the noise part added last: N_j = Y_j Q_{j-1} Y_j' + sigma_u,j^2 y_j y_j', Q_0 = 0, Q_k = A_k Q_{k-1} A_k' + sigma_u,k^2
 *   g_k g_k', A_k = Phi_k - g_k K_k' (- gamma_K k_t' on a stretched last step), Y_j = d y_j / d dz_{j-1}, y_j = d y_j / d eps_j.
 * All-zero gains without stretch give the bits of gain_u null.  The order of every addition is fixed: a node's rows do not
 *   depend on node_stride, the batch size, the problem's place in the batch, host or device pointers, or whether jac_hist_out was
 *   asked for.
 * Refuses (ASCENT_E_ARG, before the device is looked at, no array touched) what ascent_disperse_history_batch refuses of these
 *   arguments -- ff_know without ff_u, substeps or node_stride out of range, any of gain_t, stretch_max, ff_*, sigma_nav without
 *   gain_u -- and a null sigma, nominal_out or cov_out.  terminal = 2 is accepted.  Garbage blobs: the work is bounded as in
 *   ascent_flight_jacobian (K m tangent steps per problem whatever the blob holds); a non-finite t_f gives NaN rows at every node,
 *   NaN or inf gains give NaN rows from the node where they enter.
 * Host or device pointers; with device pointers and a stream the call only enqueues two kernels (f_fly, l_lincov; no host read,
 *   no synchronisation).  Device workspace: that of ascent_flight_jacobian; the sweep's state lives in LDS. */
#define ASCENT_LINCOV_COLS 32
#define ASCENT_LINCOV_COV_ROWS 55
int ascent_covariance_history_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                                    int32_t substeps, const double *sigma, const double *sigma_u_or_null,
                                    const double *gain_u_or_null, const double *gain_t_or_null, const double *stretch_max_or_null,
                                    const double *ff_u_or_null, const double *ff_t_or_null, const double *ff_know_or_null,
                                    const double *sigma_nav_or_null, int32_t node_stride, double *nominal_out, double *cov_out,
                                    double *jac_hist_out_or_null, int device_id, void *hip_stream_or_null, int ptr_is_device);

/* Time-varying navigation error: ascent_disperse_history_batch and ascent_covariance_history_batch with the eight knowledge
 * channels a (0..6 the state-knowledge error in scaled units, 7 the error of theta-hat) as first-order Gauss-Markov sequences per
 * sample instead of one bias per flight:
 *   n_a,0 = sigma_nav[a] * xi_nav[a][s]                       (the navigated call's draw; applied where sigma_nav[a] != 0)
 *   n_a,k = phi_a * n_a,k-1 + q_a * omega[a][k-1][s]          k = 1 .. K
 * Step k (node k-1 -> k) steers on dz_{k-1} + nu_k, nu_k = n_{0..6,k}, with theta-hat_k = w . dp + n_{7,k}; the cutoff stretch of
 *   step K uses the same nu_K and theta-hat_K.  The command law, the clip, the execution error, the validity rules and the
 *   reductions are ascent_disperse_navigated_batch's.  q_a = sigma * sqrt(1 - phi_a^2) keeps a variance sigma^2 stationary; q_a = 0
 *   with phi_a < 1 is an estimate that converges geometrically.
 * nav_phi_or_null and nav_q_or_null [ASCENT_NAV_ROWS][batch], both or neither, only with gain_u; phi in [0, 1], q >= 0.
 * A channel is frozen where phi_a == 1 and q_a == 0, or where the two arrays are null: it is never updated, its row of the draws
 *   is never read, and it is computed exactly as in the parent call.  With all eight frozen both calls return the parent's bits
 *   (with the arrays null they are the parent calls).  A channel that is not frozen is applied where sigma_nav[a] != 0 or
 *   q_a != 0: with sigma_nav[a] == 0 and q_a != 0 it starts at 0.
 *
 * ascent_disperse_drifting_batch: the arguments of ascent_disperse_history_batch, and after sigma_nav_or_null the two arrays and
 *   xi_drift_or_null [ASCENT_NAV_ROWS][K][samples], sample fastest, element (a, k, s) at ((a*K + k)*samples + s): omega[a][k][s],
 *   the draw behind step k + 1; required with nav_q, read only in rows whose q_a != 0.  stats_out, samples_out_or_null, hist_out
 *   and hist_samples_out_or_null exactly as ascent_disperse_history_batch defines them; hist_out is required (node_stride = K for
 *   the end statistics alone).
 * ascent_covariance_drifting_batch: the arguments of ascent_covariance_history_batch and the two arrays; outputs and layouts the same.
 *   Columns 24..31 stay the derivative with respect to n_a,0: their forcing at step k is scaled by phi_a^k, the running product
 *   multiplied once per step in ascending order.  The omega are independent unit white noise like eps_k, and the noise part is
 *     N_j = sum_k sigma_u,k^2 m_jk m_jk' + sum_a sum_{k<=j} q_a^2 r_jak r_jak',
 *   m_jk and r_jak the responses of y_j to a unit eps_k and a unit omega_a,k.  The kernel carries it as a recursion, with
 *   kappa_k = (K_k, f_k), B_k = -g_k kappa_k' (- gamma_K (k_t, f_t)' on a stretched last step) and Phi_n = diag(phi):
 *     D_k = Phi_n D_{k-1} Phi_n + diag(q^2)                    (8, diagonal; D_0 = 0)
 *     C_k = A_k C_{k-1} Phi_n + B_k D_k                         (7 x 8, the covariance of dz_k and n_k; C_0 = 0)
 *     Q_k = A_k Q_{k-1} A_k' + A_k C_{k-1} Phi_n B_k' + (its transpose) + B_k D_k B_k' + sigma_u,k^2 g_k g_k'
 *   and rows 7 (altitude), 8 (du_j) and 9 (corr_j = K_j . dz_{j-1} + kappa_j . n_j) pick up the cross terms through
 *   C_{j-1} Phi_n and D_j.  Q stays exactly symmetric.
 * Refuse (ASCENT_E_ARG, before the device is looked at, no array touched) what the parent call refuses; nav_phi without nav_q or
 *   the reverse; either without gain_u; nav_q without xi_drift (the Monte Carlo call); and, with host pointers, a phi outside
 *   [0, 1], a q < 0 or a non-finite entry of either.  With device pointers the host does not read them: such a problem has every
 *   sample invalid at every node (n = 0, the statistics NaN, the nominal rows the nominal flight's) and NaN rows of stats_out in
 *   the Monte Carlo call, NaN rows of cov_out and jac_hist_out at every node in the covariance call; the work stays bounded and the other
 *   problems of the batch are not affected.  Garbage blobs as in the parent calls.
 * Host or device pointers; with device pointers and a stream both calls only enqueue (f_fly, f_history_drifting, f_disperse_stats,
 *   f_history_stats; f_fly, l_lincov_drifting).  Device workspace: the parent call's. */
int ascent_disperse_drifting_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                                   int32_t substeps, int32_t samples, const double *xi, const double *sigma,
                                   const double *sigma_u_or_null, const double *gain_u_or_null, const double *gain_t_or_null,
                                   const double *stretch_max_or_null, const double *ff_u_or_null, const double *ff_t_or_null,
                                   const double *ff_know_or_null, const double *xi_nav_or_null, const double *sigma_nav_or_null,
                                   const double *nav_phi_or_null, const double *nav_q_or_null, const double *xi_drift_or_null,
                                   int32_t node_stride, double *stats_out, double *samples_out_or_null, double *hist_out,
                                   double *hist_samples_out_or_null, int device_id, void *hip_stream_or_null, int ptr_is_device);
int ascent_covariance_drifting_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                                     int32_t substeps, const double *sigma, const double *sigma_u_or_null,
                                     const double *gain_u_or_null, const double *gain_t_or_null, const double *stretch_max_or_null,
                                     const double *ff_u_or_null, const double *ff_t_or_null, const double *ff_know_or_null,
                                     const double *sigma_nav_or_null, const double *nav_phi_or_null, const double *nav_q_or_null,
                                     int32_t node_stride, double *nominal_out, double *cov_out, double *jac_hist_out_or_null,
                                     int device_id, void *hip_stream_or_null, int ptr_is_device);

/* Navigation filter: the knowledge error estimated instead of driven.  A linear Kalman filter is designed along the flight
 * (ascent_navigation_filter), and the linear covariance corridor is swept with the estimation error e = z-hat - z of any filter
 * gains as the error the guidance law steers on (ascent_covariance_filtered_batch).  The model is that of
 * ascent_covariance_history_batch: linearised about the flight of ascent_fly_batch at the blob, clips ignored, the substeps m held,
 * the blob fixed in scaled units; Phi_k, g_k, Gamma_k, dz_k/dt_f and gamma_K the step records of ascent_guidance_gains.
 * Measurements: n_meas (1 .. ASCENT_NAVFILTER_MAX_MEAS) scalar measurements h_i . z + sigma_i v, linear in the scaled state, constant
 *   along the flight: meas_h [n_meas][7][batch], element (i, r, problem) at ((i*7 + r)*batch + problem), meas_sigma [n_meas][batch],
 *   every sigma_i > 0.  They are taken at every node j, 1 <= j <= K, with j % meas_stride == 0 and processed one after the other,
 *   i = 0 .. n_meas-1; no matrix is inverted.  A meas_stride above K is legal: no measurement is taken.
 *
 * ascent_navigation_filter (kernels f_fly, n_filter): the forward Riccati sweep.
 *   P-hat_0 = diag(sigma_nav^2), sigma_nav [7][batch];
 *   P-hat_k^- = Phi_k P-hat_{k-1} Phi_k' + sigma_u,k^2 g_k g_k' + diag(filter_q^2), sigma_u_or_null [K][batch] and filter_q_or_null
 *   [7][batch] (null: zero);
 *   at a measurement node, for i in order: s = h_i' P h_i + sigma_i^2, l_{k,i} = P h_i / s,
 *   P <- (I - l h_i') P (I - l h_i')' + sigma_i^2 l l' (Joseph form; P is kept exactly symmetric by averaging the two halves of an entry).
 *   gain_l_out [n_meas][7][K][batch], element (i, r, k-1, problem) at (((i*7 + r)*K + k-1)*batch + problem): l_{k,i}; exactly 0 at the
 *   nodes without a measurement.  pfilt_out_or_null [ASCENT_NAV_COV_ROWS][K][batch]: the upper triangle, row by row, of P-hat_k
 *   after the update.  summary_out [ASCENT_NAVFILTER_ROWS][batch]: 0 the status (0 ok, 2 frozen), 1 the first node whose innovation
 *   variance s was <= 0 or not finite, or whose sigma_i was not > 0 (0: none; 1 where t_f, sigma_nav or filter_q is not finite), 2 the number of
 *   measurement nodes, 3 the substeps m used.  From the failing node on the problem's rows of gain_l_out (those of the nodes
 *   without a measurement included) and pfilt_out are NaN; the work stays bounded and the other problems are not affected.
 *
 * ascent_covariance_filtered_batch (kernels f_fly, l_lincov_filtered): the truth under filter gains gain_l [n_meas][7][K][batch],
 *   the design's or any others; the gains of a node without a measurement are never read.  With e_0 = c[24..30]:
 *   corr_k = K_k . (dz_{k-1} + e_{k-1}), du_k = -corr_k + eps_k,
 *   dz_k = Phi_k dz_{k-1} + g_k du_k + Gamma_k dp + (dz_k/dt_f) dt_f, on step K with gain_t and stretch_max > 0 + gamma_K tau,
 *   tau = -k_t . (dz_{K-1} + e_{K-1});
 *   e_k^- = Phi_k e_{k-1} - g_k eps_k - Gamma_k dp - (dz_k/dt_f) dt_f (the filter knows the command and tau, not eps, dp or dt_f);
 *   at a measurement node, for i in order: e <- e + l_{k,i} (-h_i . e + sigma_i v_{k,i}), v unit white noise.
 *   The constants keep the ASCENT_LINCOV_COLS columns: 24..30 are e_0, with sigma_nav [7][batch] its standard deviations, and
 *   column 31 is exactly 0 in every row.  History nodes and nominal_out (the same bits), jac_hist_out_or_null and cov_out as
 *   ascent_covariance_history_batch defines them, the noise part of cov_out now from the 14 x 14 covariance of [dz; e] under eps and
 *   v.  nav_cov_out [ASCENT_NAV_COV_ROWS][NJ][batch]: the upper triangle, row by row, of the covariance of e_j after the update
 *   at node j.  nav_jac_out_or_null [7][ASCENT_LINCOV_COLS][NJ][batch], element (r, c, i, problem) at (((r*32 + c)*NJ + i)*batch +
 *   problem): d e_j / d c.  Fed the design's own gains with sigma 0 on the fields and t_f, filter_q null and the same sigma_u and
 *   sigma_nav, nav_cov_out is the design's pfilt_out up to rounding: the filter is consistent.
 *   The order of every addition is fixed: a node's rows do not depend on node_stride, the batch, host or device pointers, or on
 *   which optional outputs were asked for.  Without gain_u the ten quantities do not depend on the filter.
 * Both refuse (ASCENT_E_ARG, before the device is looked at, no array touched) what ascent_covariance_history_batch refuses of the
 *   arguments they share, n_meas outside 1 .. ASCENT_NAVFILTER_MAX_MEAS, meas_stride < 1, a null required pointer, gain_t or
 *   stretch_max without gain_u and, with host pointers, a meas_sigma that is not > 0 and finite or a non-finite entry of meas_h,
 *   sigma_nav or filter_q.  With device pointers the host does not read these arrays: such a problem has NaN rows at every node
 *   of the covariance call; the filter call gives status 2 and NaN rows from node 1 for a non-finite sigma_nav or filter_q, which
 *   enter P-hat before the first node, and from its first measurement node for meas_h and meas_sigma, which are not read before it
 *   (never, with a meas_stride above K: status 0).  terminal = 2 is accepted.  Garbage blobs: the work is bounded
 *   as in ascent_flight_jacobian; a non-finite t_f gives NaN rows at every node, a gain K_k or l_{k,i} that is not finite NaN rows
 *   from the node where it enters.
 * Host or device pointers; with device pointers and a stream each call only enqueues its two kernels.  Device workspace: that of
 *   ascent_flight_jacobian. */
#define ASCENT_NAVFILTER_MAX_MEAS 4
#define ASCENT_NAVFILTER_ROWS 4
#define ASCENT_NAV_COV_ROWS 28
int ascent_navigation_filter(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob, int32_t substeps,
                             const double *sigma_nav, const double *sigma_u_or_null, const double *filter_q_or_null,
                             const double *meas_h, const double *meas_sigma, int32_t n_meas, int32_t meas_stride, double *gain_l_out,
                             double *pfilt_out_or_null, double *summary_out, int device_id, void *hip_stream_or_null,
                             int ptr_is_device);
int ascent_covariance_filtered_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                                     int32_t substeps, const double *sigma, const double *sigma_u_or_null,
                                     const double *gain_u_or_null, const double *gain_t_or_null, const double *stretch_max_or_null,
                                     const double *sigma_nav, const double *gain_l, const double *meas_h, const double *meas_sigma,
                                     int32_t n_meas, int32_t meas_stride, int32_t node_stride, double *nominal_out, double *cov_out,
                                     double *nav_cov_out, double *jac_hist_out_or_null, double *nav_jac_out_or_null, int device_id,
                                     void *hip_stream_or_null, int ptr_is_device);

/* Order statistics of sample rows: quantiles and limit counts, exact (nothing is summed in floating point), on caller arrays.
 * values [quantities Q][groups G][samples][batch], element (q, i, s, problem) at (((q*G + i)*samples + s)*batch + problem): with
 *   G = 1 the layout of samples_out, with Q = ASCENT_HISTORY_QUANTITIES and G = NJ that of hist_samples_out.
 * Sample s of (group i, problem) is valid if its rows q < valid_quantities (V, 0 .. Q; 0: every sample) are finite there: V = 9,
 *   G = 1 is the rule of stats_out, V = 10 that of hist_out.  n: the valid samples.  count_out [G][batch]: n.
 * Per (q, i, problem) the values of the valid samples in ascending order x_(0) <= .. <= x_(n-1), NaN (rows q >= V only) last, as
 *   np.sort orders them; which of -0 and +0 comes first is unspecified.
 * probs: n_probs (1 .. 16) probabilities in [0, 1], ALWAYS a host array, read during the call.  For probability pi:
 *   h = pi (double)(n - 1), lo = floor(h), g = h - lo, hi = min(lo + 1, n - 1),
 *   quant_out[((j*Q + q)*G + i)*batch + problem] = x_(lo) + g (x_(hi) - x_(lo)) -- one subtraction, one multiplication, one
 *   addition, each rounded once, never fused: numpy's default "linear" quantile up to the rounding of its interpolation.
 *   n = 0: NaN.  n = 1: the sample.  pi = 0 the minimum, pi = 1 the maximum (g = 0).
 * limits_or_null [n_limits (1 .. 16)][Q][batch], the same limit at every group; below_out [n_limits][Q][G][batch]: the number
 *   of valid samples with value <= limit.  A NaN limit counts 0, +inf every valid sample that is not NaN.  Both or neither.
 * A result depends on the set of valid values only: not on the batch size, the problem's place in it, the kind of pointer or
 *   timing.
 * Refuses (ASCENT_E_ARG, before the device is looked at, no array touched): a null values, probs, count_out or quant_out; Q, G
 *   or batch < 1; V outside 0 .. Q; samples outside 1 .. ASCENT_DISPERSE_MAX_SAMPLES; n_probs outside 1 .. 16; a probability
 *   outside [0, 1] or not finite; limits without below_out or the reverse; n_limits outside 1 .. 16 where limits are given.
 * Host or device pointers; with device pointers and a stream the call only enqueues (q_sort: the rows of a tile of problems
 *   sorted in LDS, up to 16384 samples; q_select: radix select, one workgroup per row, above that).  No device workspace. */
int ascent_sample_quantiles(const double *values, int32_t quantities, int32_t groups, int32_t valid_quantities, int32_t samples,
                            int64_t batch, const double *probs, int32_t n_probs, const double *limits_or_null, int32_t n_limits,
                            double *count_out, double *quant_out, double *below_out_or_null, int device_id,
                            void *hip_stream_or_null, int ptr_is_device);

/* Monte Carlo dispersion with quantiles and limit counts: the flight of the existing calls, then ascent_sample_quantiles over
 * its sample rows, which never leave the device.  Arguments p .. xi_drift_or_null: those of ascent_disperse_drifting_batch, every
 * _or_null optional -- nav_phi null: the flight of ascent_disperse_history_batch (node_stride > 0) or of ascent_disperse_batch /
 * _guided_batch / _navigated_batch (node_stride = 0: open loop without gain_u, navigated with any of ff_u .. sigma_nav); the
 * "both or neither" and "only with gain_u" rules are theirs.  nav_phi needs node_stride > 0, as in the drifting call.
 * node_stride: 0 no history, else 1 .. K.  stats_out [ASCENT_DISPERSE_STAT_ROWS][batch] and hist_out_or_null
 *   [ASCENT_HISTORY_ROWS][NJ][batch] (with node_stride > 0, where it is required as in the parent call, and only then): the bits
 *   of that call.
 * probs, n_probs, n_limits: as in ascent_sample_quantiles.  limits_or_null [n_limits][ASCENT_GUIDED_SAMPLE_ROWS][batch] with
 *   below_out_or_null of the same shape, hist_limits_or_null [n_limits][ASCENT_HISTORY_QUANTITIES][batch] with
 *   hist_below_out_or_null [n_limits][ASCENT_HISTORY_QUANTITIES][NJ][batch]; quant_out [n_probs][ASCENT_GUIDED_SAMPLE_ROWS][batch];
 *   hist_quant_out_or_null [n_probs][ASCENT_HISTORY_QUANTITIES][NJ][batch] (node_stride > 0 only; hist_below_out needs it).
 * The end rows use the validity rule of stats_out (their count is its row 0), the history rows that of hist_out (row 0 of it).
 *   Rows 9 .. 11 of quant_out are exactly 0 in the open-loop flight (NaN where no sample is valid).
 * Refuses what the parent calls and ascent_sample_quantiles refuse of these arguments.
 * Host or device pointers; with device pointers and a stream the call only enqueues: the parent's kernels with the sample rows
 *   directed to the workspace, then the selection.  Device workspace: ascent_disperse_quantiles_bytes, the parent call's and
 *   (ASCENT_GUIDED_SAMPLE_ROWS + ASCENT_HISTORY_QUANTITIES NJ) samples batch doubles; a problem's results do not depend on
 *   the batch, so a caller short of memory splits the batch. */
int ascent_disperse_quantiles_batch(const ascent_params *p, int64_t batch, const ascent_opts *o, const double *sol_blob,
                                    int32_t substeps, int32_t samples, const double *xi, const double *sigma,
                                    const double *sigma_u_or_null, const double *gain_u_or_null, const double *gain_t_or_null,
                                    const double *stretch_max_or_null, const double *ff_u_or_null, const double *ff_t_or_null,
                                    const double *ff_know_or_null, const double *xi_nav_or_null, const double *sigma_nav_or_null,
                                    const double *nav_phi_or_null, const double *nav_q_or_null, const double *xi_drift_or_null,
                                    int32_t node_stride, double *stats_out, double *hist_out_or_null, const double *probs,
                                    int32_t n_probs, const double *limits_or_null, const double *hist_limits_or_null,
                                    int32_t n_limits, double *quant_out, double *below_out_or_null, double *hist_quant_out_or_null,
                                    double *hist_below_out_or_null, int device_id, void *hip_stream_or_null, int ptr_is_device);
/* The device workspace of that call in bytes; no device work.  Negative (ASCENT_E_ARG) for batch < 1, n_nodes outside
 * 3 .. 65536, samples outside 1 .. ASCENT_DISPERSE_MAX_SAMPLES or node_stride outside 0 .. n_nodes - 1. */
int64_t ascent_disperse_quantiles_bytes(int64_t batch, int32_t n_nodes, int32_t samples, int32_t node_stride);

/* Generic bordered block-tridiagonal solve (parity surface of the linear algebra):
 *     [ T   B ] [x]   [r]        T: n_nodes x n_nodes blocks of size bs (<= 16): diag[i] on the diagonal, lower[i] = block
 *     [ B'  d ] [y] = [s]           (i, i-1) (lower[0] ignored), upper[i] = block (i, i+1) (upper[n-1] ignored);
 *                                B: nb border columns (1 + nb <= 16), d: nb x nb (border_diag, row-major).
 * Layouts (host pointers, row-major, system index slowest): diag / lower / upper [batch][n_nodes][bs][bs],
 * border [batch][n_nodes][bs][nb], border_diag [batch][nb][nb], rhs and sol [batch][n_nodes*bs + nb].
 * algo 0: block elimination serial in the node index, one wavefront per system; algo 1: parallel cyclic reduction over
 * the nodes (one wavefront per node, log2(n_nodes) levels).  Blocks are padded to 16x16 and multiplied with
 * v_mfma_f64_16x16x4_f64; no pivoting inside blocks (returns ASCENT_E_ARG "singular pivot" if one vanishes); cyclic reduction exposes no inertia -- the interior-point solver uses it for a handful of NLPs only
 * and guards it with a curvature test along the step (a weaker guarantee than the exact inertia of the Riccati recursions); the
 * border is closed by a Schur complement on the host.  The interior-point solver does not call this (it uses a
 * Riccati recursion in the 7x7 value function); ascent_last_kernel_ms reports the device time of the solve. */
int ascent_kkt_solve(int64_t batch, int32_t n_nodes, int32_t bs, int32_t nb, const double *diag, const double *lower,
                     const double *upper, const double *border, const double *border_diag, const double *rhs,
                     double *sol, int device_id, int algo);

/* Test hook: the lane reductions of the persistent kernels on caller data (host pointers).  in: n records of 64 doubles, one
 * wavefront each; out: [n][ASCENT_REDUCE_PROBE_ROWS][64], per lane
 *   rows 0-2   sum / max / min over the lane's row of 16 lanes, by the DPP helpers the kernels use
 *   rows 3-5   the same by the __shfl_xor butterflies they replaced
 *   rows 6-8   sum / max / min over the wavefront by the helpers (DPP inside a row, shuffles across rows)
 *   rows 9-11  the same by shuffles alone
 *   rows 12,13 the inclusive prefix sum over the lane's row of 16: on DPP row shifts, and with __shfl_up
 * The two versions of each quantity agree bit for bit (NaN where either is NaN): tests/test_gpu_reduce_probe.py. */
#define ASCENT_REDUCE_PROBE_ROWS 14
int ascent_reduce_probe(const double *in, int64_t n, double *out, int device_id);

/* Device time (ms) of the solve kernel of the most recent ascent_solve_batch on this device,
 * measured with HIP events recorded on the launch stream around the kernel; waits for that
 * kernel to finish; < 0 if there was none. */
double ascent_last_kernel_ms(int device_id);

#ifdef __cplusplus
}
#endif
#endif /* ASCENT_H */
