#!/usr/bin/env python3
"""Apollo-11 lunar-module ascent to the 87 x 17 km orbit through the GEKKO-style surface.

This is this repository's own counterpart of the reference script: the same problem, declared with
the same modelling calls, solved by libascent on an MI355X instead of GEKKO/APMonitor/IPOPT.  It prints
the quantities the reference prints (/root/reference/Launch_Optimiser.py:178-194) and writes the same
three figures (:208-242).  Usage:  python examples/apollo11.py [--no-plots] [--outdir DIR] [--fly] [--trim] [--disperse] [--guide [--feedforward] [--lincov [--filter]]] [--corridor]
--fly also integrates the ODEs under the control just found (RK4 on the device) and prints where that flight ends.
--trim corrects (t_f, u) so that the flown control reaches the target orbit (trim_batch) and prints t_f and the flown apsides
before and after.
--disperse trims, then flies the trimmed control 1024 times with 50 N (1-sigma) of thrust error and 1e-3 of error on every control
step (disperse_batch) and prints the Monte Carlo and the linear 1-sigma of the flown apsides side by side.
--guide trims, computes the neighbouring-optimal feedback gains (guidance_gains) and flies the same 1024 dispersed samples open loop
and under that feedback; prints both 1-sigmas of the flown apsides and the control authority the feedback took.
--guide --feedforward adds, from the same draws, the thrust feed-forward (guidance_gains(feedforward="Ft")) with the thrust known
exactly, and with the thrust known to 10 N (1-sigma) under a navigation bias of NAV_BIAS (1-sigma, scaled units).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "compat"))
from gekko import GEKKO  # noqa: E402  (the compatibility package; resolves to gekko_shim.GEKKO)

# ---- physical data (SI) -----------------------------------------------------------------------------
MOON = dict(G=6.674e-11, M=7.346e22, R0=1738100.0)
VEHICLE = dict(Ft=15346.0, M0=4821.0, M_dot=5.053, fuel=2376.0, ang_acc_max=5e-4)
ORBIT = dict(periapsis=17703.0, apoapsis=88615.0)
BURN_LIMIT = 470.0          # s, fuel-limited maximum burn: time scale of the free final time
NT = 200
# --guide --feedforward: 1-sigma bias of each sample's state knowledge, scaled units (x, y, vx, vy, angle, angle rate, mass);
# a position unit is the insertion altitude, 17703 m, a velocity unit 17703 m/s: 17.7 m and 1.8 cm/s
NAV_BIAS = (1e-3, 1e-3, 1e-6, 1e-6, 0.0, 0.0, 0.0)
# --guide --lincov --filter: 1-sigma of the position and velocity fixes, scaled units (5.3 m and 5.3 cm/s), taken at every FIX_STRIDE-th node
FIX_SIGMA = (3e-4, 3e-4, 3e-6, 3e-6)
FIX_STRIDE = 10


def build(nt=NT, solver=None):
    m = GEKKO(solver=solver) if solver is not None else GEKKO()
    m.time = np.linspace(0, 1, nt)
    m.options.NODES, m.options.SOLVER, m.options.IMODE = 2, 3, 6
    m.options.MAX_ITER, m.options.MV_TYPE = 20000, 0
    m.options.OTOL = m.options.RTOL = 1e-3

    tf = m.FV(value=0, lb=0, ub=1)
    tf.STATUS = 1
    G, M, R0 = (m.Const(MOON[k], name=k) for k in ("G", "M", "R0"))
    Ft, M0 = m.Const(VEHICLE["Ft"], name="Ft"), m.Const(VEHICLE["M0"], name="M0")
    m.Const(VEHICLE["M_dot"], name="M_dot")
    mflow = VEHICLE["M_dot"] / VEHICLE["fuel"]
    S = m.Const(ORBIT["periapsis"], name="distance Scale")       # lengths are scaled by the insertion altitude
    m.Const(ORBIT["periapsis"], name="Rfmin")
    mS = m.Const(VEHICLE["fuel"], name="mass Scale")
    aS = m.Const(VEHICLE["ang_acc_max"] / 3)
    v_ins = np.sqrt(MOON["G"] * MOON["M"] / (MOON["R0"] + 0.5 * (ORBIT["periapsis"] + ORBIT["apoapsis"])))

    mass = m.Var(value=0, lb=0, ub=1, name="mass")
    y, ydot, ydd = m.Var(value=0, name="y"), m.Var(name="ydot"), m.Var(name="ydoubledot")
    x, xdot, xdd = m.Var(value=0, name="x"), m.Var(name="xdot"), m.Var(name="xdoubledot")
    angle, angledot = m.Var(value=0, lb=0, ub=np.pi / 3, name="angle"), m.Var(name="angledot")
    u = m.MV(name="angledoubledot", lb=-1, ub=1)
    u.STATUS, u.DCOST = 1, 1e-5

    scale = tf * BURN_LIMIT                      # d/dtau = tf * T * d/dt
    for var, rate in ((y, ydot), (ydot, ydd), (x, xdot), (xdot, xdd), (angle, angledot)):
        m.Equation(var.dt() == scale * rate)
    m.Equation(angledot.dt() == scale * u * aS)
    m.Equation(mass.dt() == mflow * BURN_LIMIT * tf)

    X, Y = x * S, y * S + R0                     # metres, Moon-centred; launch site on the +Y axis
    r = (X ** 2 + Y ** 2) ** (1 / 2)
    thrust = Ft / ((M0 - mS * mass) * r)         # thrust acceleration / r
    grav = G * M / (X ** 2 + Y ** 2) ** (3 / 2)
    m.Equation(ydd == (thrust * (Y * m.cos(3 * angle) + X * m.sin(3 * angle)) - Y * grav) / S)
    m.Equation(xdd == (thrust * (X * m.cos(3 * angle) - Y * m.sin(3 * angle)) - X * grav) / S)

    for v in (y, x, ydot, xdot, angle, mass):
        m.fix(v, pos=0, val=0)

    only_last = np.zeros(nt); only_last[-1] = 1                     # terminal constraints act on the last node
    slack_elsewhere = np.full(nt, S + R0 + 1.0); slack_elsewhere[-1] = 0
    p_rad, p_vel = m.Param(value=slack_elsewhere), m.Param(value=only_last)
    m.Equation(((y + R0 / S) ** 2 + x ** 2) ** (1 / 2) + p_rad >= (R0 + S) / S)
    m.Equation(xdot ** 2 + ydot ** 2 >= (v_ins / S) ** 2 * p_vel)
    m.Equation((Y * (ydot * S) + X * (xdot * S)) * p_vel == 0)
    m.Minimize(tf)
    return m, dict(tf=tf, x=x, y=y, xdot=xdot, ydot=ydot, xdd=xdd, ydd=ydd, angle=angle, mass=mass), v_ins


def report(m, v, v_ins):
    """The reference's prints, in its order and wording."""
    S, T = ORBIT["periapsis"], BURN_LIMIT
    tfv = v["tf"].value[0]
    print("Optimal Solution (final time): " + str(tfv * T))
    print(v_ins)
    for label, var in (("final y", "y"), ("final x", "x"), ("final ydot", "ydot"), ("final xdot", "xdot"),
                       ("final ydoubledot", "ydd"), ("final xdoubledot", "xdd")):
        print(label, v[var].value[-1] * S)
    print("final time", tfv * T)
    return tfv * T


def fly(m, scheme):
    """Flight verification of the solved case: the solution's control flown with RK4 on the device (fly_batch)."""
    from lunar_module_ascent_trajectory_optimiser_amd import fly_batch
    res = m.result
    f = fly_batch(res.params, res.flight_blob(), res.nt, scheme=scheme, formulation=m._formulation)
    print("flown with RK4, %d substeps per step: the control ends %.4g m and %.4g m/s from the NLP's last node"
          % (f.substeps[0], f.miss_position[0], f.miss_velocity[0]))
    print("flown burnout orbit (periapsis / apoapsis altitude): %.1f m / %.1f m" % (f.flown_periapsis_alt[0], f.flown_apoapsis_alt[0]))
    print("the NLP's own burnout orbit:                         %.1f m / %.1f m" % (f.nlp_periapsis_alt[0], f.nlp_apoapsis_alt[0]))
    print("largest local error of a collocation step: %.4g m, %.4g m/s (position: step %d)"
          % (f.max_local_position_error[0], f.max_local_velocity_error[0], f.max_local_step[0]))
    return f


def trim(m, scheme):
    """The solved case trimmed: t_f and the control corrected so that the flown trajectory meets the terminal conditions."""
    from lunar_module_ascent_trajectory_optimiser_amd import fly_batch, trim_batch
    res = m.result
    blob, T = res.flight_blob(), res.params[0, 11]
    kw = dict(scheme=scheme, formulation=m._formulation)
    before = fly_batch(res.params, blob, res.nt, want_traj=False, want_local=False, **kw)
    t = trim_batch(res.params, blob, res.nt, **kw)
    print("trim: status %d after %d rounds, flown conditions %.3g -> %.3g (scaled), %d of %d controls free, max |du| %.4g"
          % (t.status[0], t.rounds[0], t.residual_before[0], t.residual[0], t.free_controls[0], res.nt - 1, t.max_delta_u[0]))
    print("final time                                  before %.4f s   after %.4f s" % (res.tf[0] * T, t.tf[0] * T))
    print("flown periapsis / apoapsis altitude (m)     before %.1f / %.1f   after %.3f / %.3f"
          % (before.flown_periapsis_alt[0], before.flown_apoapsis_alt[0], t.flown_periapsis_alt[0], t.flown_apoapsis_alt[0]))
    return t


def corridor_report(name, d, params, tf, outdir=None, figure=None):
    """What the samples of one dispersed flight did on the way (d.history, disperse_batch(history=True)): four lines, and with
    outdir the figure `figure` (corridor_<name>.png if not named) -- nominal altitude against downrange with the min / max and
    +-1-sigma bands."""
    h, K = d.history, d.history.nodes[-1]
    t = h.nodes * tf * params[0, 11] / K
    ALT, ANG = 7, 4
    sd = h.std[0, :, ALT]
    i = int(np.nanargmax(sd))
    print("%s: widest 1-sigma altitude band at node %d (t = %.1f s): +-%.1f m" % (name, h.nodes[i], t[i], sd[i]))
    i = int(np.nanargmin(h.min[0, :, ALT]))
    print("%s: lowest altitude any sample reached: %.2f m at node %d (t = %.1f s); nominal there %.2f m"
          % (name, h.min[0, i, ALT], h.nodes[i], t[i], h.nominal[0, i, ALT]))
    out = np.maximum(np.maximum(-h.min[0, :, ANG], h.max[0, :, ANG] - params[0, 12]), 0.0)
    i = int(np.nanargmax(out))
    print("%s: largest excursion of the angle beyond [0, angle_ub]: %.3g (angle_ub %.4g) at node %d" % (name, out[i], params[0, 12], h.nodes[i]))
    i = int(np.argmax(h.clipped[0]))
    print("%s: step with the most clipped commands: step %d (t = %.1f s), %d of %d samples" % (name, h.nodes[i], t[i], h.clipped[0, i], h.n_valid[0, i]))
    if outdir is not None:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        x = -h.nominal[0, :, 0] * ORBIT["periapsis"]                  # downrange positive, as plots() has it
        fig, ax = plt.subplots()
        ax.fill_between(x, h.min[0, :, ALT], h.max[0, :, ALT], color=(0.9, 0.4, 0, 0.25), label="min / max")
        ax.fill_between(x, h.mean[0, :, ALT] - sd, h.mean[0, :, ALT] + sd, color=(0.9, 0.4, 0, 0.5), label="+-1 sigma")
        ax.plot(x, h.nominal[0, :, ALT], color="k", lw=0.8, label="nominal")
        ax.set(title="Dispersion corridor (%s)" % name, xlabel="downrange / m", ylabel="altitude / m")
        ax.legend()
        ax.grid()
        fig.savefig(os.path.join(outdir, figure or "corridor_%s.png" % name.replace(" ", "_")), dpi=300)


QUANTILE_POINTS = (0.00135, 0.5, 0.99865)       # the -3-sigma point, the median and the +3-sigma point of a normal distribution
PERIAPSIS_LIMIT = 15000.0                       # m: a flown periapsis below it counts as a violation


def quantile_keywords():
    """disperse_batch's keywords for quantile_report: the three points, and the limit on the flown periapsis (column 7)"""
    lim = np.full((1, 12), np.nan)
    lim[0, 7] = PERIAPSIS_LIMIT
    return dict(quantiles=QUANTILE_POINTS, limits=lim)


def quantile_report(name, d):
    """The order statistics of one dispersed flight (disperse_batch(quantiles=..., limits=...)): the 0.135 / 50 / 99.865 % points of
    the flown apsides, the fraction of samples whose periapsis ends below PERIAPSIS_LIMIT and, with a history, the 0.135 % ..
    99.865 % altitude band at the node where it is widest."""
    for what, q in (("periapsis", 7), ("apoapsis", 8)):
        print("%s: flown %s 0.135 %% / 50 %% / 99.865 %% points: %.1f / %.1f / %.1f m" % ((name, what) + tuple(d.quantiles[0, :, q])))
    print("%s: flown periapsis below %.0f m: %d of %d valid samples (%.3f %%)"
          % (name, PERIAPSIS_LIMIT, d.below[0, 0, 7], d.n_valid[0], 100.0 * d.below[0, 0, 7] / max(int(d.n_valid[0]), 1)))
    if d.history is not None:
        h, ALT = d.history, 7
        band = h.quantiles[0, :, 2, ALT] - h.quantiles[0, :, 0, ALT]
        i = int(np.nanargmax(band))
        print("%s: widest 0.135 %% .. 99.865 %% altitude band at node %d: %.1f .. %.1f m (median %.1f m, nominal %.1f m)"
              % (name, h.nodes[i], h.quantiles[0, i, 0, ALT], h.quantiles[0, i, 2, ALT], h.quantiles[0, i, 1, ALT], h.nominal[0, i, ALT]))


def disperse(m, scheme, samples=1024, corridor=False, outdir=None, quantiles=False):
    """The trimmed solution under a dispersed thrust and control: Monte Carlo on the device beside the flight Jacobian's linear
    prediction from the same draws.  corridor: with the per-node history, and its lines (corridor_report).  quantiles: with the
    order statistics selected on the device, and their lines (quantile_report)."""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch, flight_jacobian, trim_batch
    res = m.result
    kw = dict(scheme=scheme, formulation=m._formulation)
    t = trim_batch(res.params, res.flight_blob(), res.nt, **kw)
    thrust = np.zeros(16)
    thrust[3] = 50.0
    if quantiles:
        kw = dict(kw, **quantile_keywords())
    d = disperse_batch(res.params, t.blob, res.nt, param_sigma=thrust, control_sigma=1e-3, samples=samples, history=corridor, **kw)
    kw = dict(scheme=scheme, formulation=m._formulation)
    lin = np.sqrt(np.diagonal(d.linear_covariance(flight_jacobian(res.params, t.blob, res.nt, **kw)), axis1=1, axis2=2))
    print("dispersion: %d of %d samples valid; thrust 1-sigma 50 N, control 1-sigma 1e-3 per step" % (d.n_valid[0], samples))
    print("flown altitude (m)      nominal   Monte Carlo 1-sigma   linear 1-sigma   mean shift          min          max")
    for name, q in (("periapsis", 7), ("apoapsis", 8)):
        print("%-18s %12.1f %21.1f %16.1f %12.1f %12.1f %12.1f"
              % (name, d.nominal[0, q], d.std[0, q], lin[0, q], d.mean[0, q] - d.nominal[0, q], d.min[0, q], d.max[0, q]))
    if corridor:
        corridor_report("open loop", d, res.params, t.tf[0], outdir, "corridor.png")
    if quantiles:
        quantile_report("open loop", d)
    return d


def lincov_report(name, lc, d, params, tf, outdir=None, figure=None):
    """The linear covariance corridor lc (linear_corridor) beside the Monte Carlo history of the same flight (d.history): the
    altitude's 1-sigma band of both at the node where the sampled one is widest, and with outdir both bands in one figure."""
    h, K, ALT = d.history, d.history.nodes[-1], 7
    mc, lin = h.std[0, :, ALT], lc.std[0, :, ALT]
    i = int(np.nanargmax(mc))
    print("%s: linear 1-sigma altitude band at node %d (t = %.1f s): +-%.1f m; Monte Carlo +-%.1f m (%d samples)"
          % (name, h.nodes[i], h.nodes[i] * tf * params[0, 11] / K, lin[i], mc[i], h.n_valid[0, i]))
    print("%s: largest gap between the two bands over the nodes: %.2f m of %.1f m at node %d"
          % (name, np.nanmax(np.abs(lin - mc)), mc[int(np.nanargmax(np.abs(lin - mc)))], h.nodes[int(np.nanargmax(np.abs(lin - mc)))]))
    if outdir is not None:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        x = -h.nominal[0, :, 0] * ORBIT["periapsis"]
        fig, ax = plt.subplots()
        ax.fill_between(x, -mc, mc, color=(0.9, 0.4, 0, 0.4), label="Monte Carlo +-1 sigma")
        ax.plot(x, lin, color="k", lw=0.8, label="linear covariance +-1 sigma")
        ax.plot(x, -lin, color="k", lw=0.8)
        ax.set(title="Altitude dispersion about the nominal (%s)" % name, xlabel="downrange / m", ylabel="altitude deviation / m")
        ax.legend()
        ax.grid()
        fig.savefig(os.path.join(outdir, figure or "lincov_%s.png" % name.replace(" ", "_")), dpi=300)


def guide(m, scheme, samples=1024, weight=1e12, stretch_max=2.0, feedforward=False, corridor=False, outdir=None, lincov=False,
          nav_tau=None, knowledge_tau=None, quantiles=False, navfilter=False):
    """The trimmed solution under the same dispersions, open loop and steering back to the nominal with a cutoff on the state.
    The cutoff channel stretches the last step only, T / K = 2.2 s here: 50 N of 15 kN over a 435 s burn is 1.4 s (1-sigma) of burn
    time, so the stretch is allowed +-2 steps; at stretch_max = 0.5 it sits on its bound for most samples.
    corridor: every flight flown with its per-node history, and the lines of corridor_report for each.
    lincov: the open and the closed loop flown once more with their history, beside linear_corridor's band (lincov_report).
    nav_tau, knowledge_tau (seconds; with feedforward, corridor and lincov): the navigation bias as a stationary first-order
    Gauss-Markov process of that correlation time and the thrust estimate converging from its 10 N with that time constant
    (steady sigma 0): the sampled and the linear altitude band side by side, next to those of the frozen bias.
    quantiles: every flight flown with its order statistics, and the lines of quantile_report for each.
    navfilter (with lincov): a Kalman filter on position and velocity fixes every tenth node (navigation_filter), and the closed
    loop steering on its estimate (linear_corridor(filter=...)): what the filter believes of its error at burnout beside what the
    error truly is under the thrust dispersion the filter does not model, and the burnout altitude with and without the filter."""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch, guidance_gains, linear_corridor, navigation_filter, trim_batch
    res = m.result
    kw = dict(scheme=scheme, formulation=m._formulation)
    t = trim_batch(res.params, res.flight_blob(), res.nt, **kw)
    g = guidance_gains(res.params, t.blob, res.nt, cond_weights=(weight,) * 3, control_weight=1.0, cutoff_weight=1.0, stretch_max=stretch_max, **kw)
    thrust = np.zeros(16)
    thrust[3] = 50.0
    dkw = dict(param_sigma=thrust, control_sigma=1e-3, samples=samples, history=corridor, **kw)
    if quantiles:
        dkw.update(quantile_keywords())
    op = disperse_batch(res.params, t.blob, res.nt, **dkw)
    cl = disperse_batch(res.params, t.blob, res.nt, guidance=g, keep_samples=True, **dkw)
    print("guidance: status %d, %d of %d controls free, largest steering gain %.4g, largest cutoff gain %.4g (weights %g, 1, 1)"
          % (g.status[0], g.free_controls[0], res.nt - 1, g.max_gain[0], g.max_cutoff_gain[0], weight))
    print("closed loop: %d of %d samples valid; thrust 1-sigma 50 N, control 1-sigma 1e-3 per step" % (cl.n_valid[0], samples))
    print("flown altitude (m)      nominal   open loop 1-sigma   closed loop 1-sigma   closed loop min / max")
    for name, q in (("periapsis", 7), ("apoapsis", 8)):
        print("%-18s %12.1f %19.1f %21.2f %14.1f / %.1f" % (name, cl.nominal[0, q], op.std[0, q], cl.std[0, q], cl.min[0, q], cl.max[0, q]))
    e = cl.effort[0]
    print("control authority: a command clipped on %.2f steps per flight, largest |K.dz| %.3g, cutoff stretch 1-sigma %.3g (largest %.3g of %g)"
          % (e[:, 0].mean(), np.nanmax(e[:, 1]), np.nanstd(e[:, 2]), np.nanmax(np.abs(e[:, 2])), stretch_max))
    if corridor:
        corridor_report("open loop", op, res.params, t.tf[0], outdir)
        corridor_report("closed loop", cl, res.params, t.tf[0], outdir, "corridor.png")
    if quantiles:
        quantile_report("open loop", op)
        quantile_report("closed loop", cl)
    if feedforward:
        # the same draws with the feed-forward: the feedback gains are the same bits, the samples now plan with their own thrust
        gf = guidance_gains(res.params, t.blob, res.nt, cond_weights=(weight,) * 3, control_weight=1.0, cutoff_weight=1.0, stretch_max=stretch_max,
                            feedforward="Ft", **kw)
        known = disperse_batch(res.params, t.blob, res.nt, guidance=gf, keep_samples=True, **dkw)
        nav = disperse_batch(res.params, t.blob, res.nt, guidance=gf, keep_samples=True, knowledge_sigma=10.0, nav_sigma=NAV_BIAS, **dkw)
        lin = np.sqrt(np.diagonal(nav.linear_covariance(gf.jacobian, gf.jacobian_nav)[0]))
        print("feed-forward: largest |f_k| %.4g per N, |f_t| %.4g per N" % (gf.max_feedforward[0], gf.max_cutoff_feedforward[0]))
        print("flown altitude 1-sigma (m)   open loop   feedback only   + feed-forward, thrust known   + known to 10 N, navigation bias (linear)")
        for name, q in (("periapsis", 7), ("apoapsis", 8)):
            print("%-24s %13.1f %15.2f %30.2f %25.2f (%.2f)" % (name, op.std[0, q], cl.std[0, q], known.std[0, q], nav.std[0, q], lin[q]))
        print("commands clipped per flight: feedback only %.2f, thrust known %.2f, 10 N and navigation bias %.2f"
              % (e[:, 0].mean(), known.effort[0, :, 0].mean(), nav.effort[0, :, 0].mean()))
        if corridor:
            corridor_report("thrust known", known, res.params, t.tf[0], outdir)
            corridor_report("known to 10 N", nav, res.params, t.tf[0], outdir)
        if quantiles:
            quantile_report("thrust known", known)
            quantile_report("known to 10 N", nav)
        if corridor and lincov and (nav_tau is not None or knowledge_tau is not None):
            # the same errors, time-varying: the bias a stationary process, the thrust estimate converging to the truth
            nkw = dict(guidance=gf, knowledge_sigma=10.0, nav_sigma=NAV_BIAS, nav_tau=nav_tau, knowledge_tau=knowledge_tau,
                       knowledge_steady_sigma=None if knowledge_tau is None else 0.0)
            lkw = dict(param_sigma=thrust, control_sigma=1e-3, **kw)
            drift = disperse_batch(res.params, t.blob, res.nt, keep_samples=True, **nkw, **dkw)
            print("time-varying navigation error: nav_tau %s s, knowledge_tau %s s" % (nav_tau, knowledge_tau))
            print("flown altitude 1-sigma (m)   frozen bias   time-varying")
            for name, q in (("periapsis", 7), ("apoapsis", 8)):
                print("%-24s %15.2f %14.2f" % (name, nav.std[0, q], drift.std[0, q]))
            lincov_report("frozen bias", linear_corridor(res.params, t.blob, res.nt, guidance=gf, knowledge_sigma=10.0, nav_sigma=NAV_BIAS, **lkw),
                          nav, res.params, t.tf[0], outdir)
            lincov_report("time-varying", linear_corridor(res.params, t.blob, res.nt, **nkw, **lkw), drift, res.params, t.tf[0], outdir)
            for name, d_, lc_ in (("frozen bias", nav, linear_corridor(res.params, t.blob, res.nt, guidance=gf, knowledge_sigma=10.0, nav_sigma=NAV_BIAS, history=res.nt - 1, **lkw)),
                                  ("time-varying", drift, linear_corridor(res.params, t.blob, res.nt, history=res.nt - 1, **nkw, **lkw))):
                print("%s: closed-loop 1-sigma altitude at burnout: linear +-%.2f m; Monte Carlo +-%.2f m" % (name, lc_.std[0, -1, 7], d_.history.std[0, -1, 7]))
    if lincov:
        lkw = dict(param_sigma=thrust, control_sigma=1e-3, **kw)
        hkw = dict({k: v for k, v in dkw.items() if k not in ("quantiles", "limits")}, history=True)
        lincov_report("open loop", linear_corridor(res.params, t.blob, res.nt, **lkw), op if corridor else disperse_batch(res.params, t.blob, res.nt, **hkw),
                      res.params, t.tf[0], outdir)
        lincov_report("closed loop", linear_corridor(res.params, t.blob, res.nt, guidance=g, **lkw),
                      cl if corridor else disperse_batch(res.params, t.blob, res.nt, guidance=g, **hkw), res.params, t.tf[0], outdir, "lincov.png")
    if lincov and navfilter:
        S = ORBIT["periapsis"]
        nf = navigation_filter(res.params, t.blob, res.nt, nav_sigma=NAV_BIAS, meas_rows=np.eye(7)[:4], meas_sigma=FIX_SIGMA, meas_stride=FIX_STRIDE,
                               control_sigma=1e-3, **kw)
        lkw = dict(param_sigma=thrust, control_sigma=1e-3, history=res.nt - 1, **kw)
        bias = linear_corridor(res.params, t.blob, res.nt, guidance=g, nav_sigma=NAV_BIAS, **lkw)
        filt = linear_corridor(res.params, t.blob, res.nt, guidance=g, filter=nf, **lkw)
        print("navigation filter: status %d, fixes of %.1f m and %.1f cm/s (1-sigma) at every %dth node, %d of them"
              % (nf.status[0], FIX_SIGMA[0] * S, FIX_SIGMA[2] * S * 100, FIX_STRIDE, nf.meas_nodes[0]))
        print("knowledge error at burnout (1-sigma)   true   the filter's own")
        for name, q, unit, f in (("x (m)", 0, S, 1.0), ("y (m)", 1, S, 1.0), ("xdot (cm/s)", 2, S, 100.0), ("ydot (cm/s)", 3, S, 100.0)):
            print("%-30s %12.3f %14.3f" % (name, filt.nav_std[0, -1, q] * unit * f, nf.std[0, -1, q] * unit * f))
        print("closed-loop 1-sigma altitude at burnout: with the filter +-%.2f m; with the frozen navigation bias +-%.2f m"
              % (filt.std[0, -1, 7], bias.std[0, -1, 7]))
    return op, cl, g


def plots(m, v, outdir):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    S, R0 = ORBIT["periapsis"], MOON["R0"]
    xs = -np.asarray(v["x"].value) * S                    # downrange positive, as the reference plots it
    ys = np.asarray(v["y"].value) * S + R0
    theta = 3 * np.asarray(v["angle"].value) * 180 / np.pi
    t = m.time * v["tf"].value[0] * BURN_LIMIT
    fig, ax = plt.subplots()
    ax.add_patch(plt.Circle((0, 0), R0))
    ax.plot(xs, ys, color=(0.9, 0.4, 0))
    ax.set(ylim=(R0 - 30000, R0 + 20000), xlim=(-5000, 300000), title="Position", xlabel="x", ylabel="y", aspect="equal")
    ax.grid()
    fig.savefig(os.path.join(outdir, "takeoff_contextualized.png"), dpi=300)
    fig, ax = plt.subplots()
    ax.plot(t, theta)
    ax.set(title="Angle", xlabel="time", ylabel="Angle / degrees")
    ax.grid()
    fig.savefig(os.path.join(outdir, "Angle_vs_Time.png"), dpi=300)
    fig, ax = plt.subplots()
    ax.plot(xs, ys)
    ax.set(title="Position", xlabel="x", ylabel="y", ylim=(R0 - 10000, R0 + 20000), aspect="equal")
    ax.grid()
    fig.savefig(os.path.join(outdir, "takeoff_trajectory.png"), dpi=300)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-plots", action="store_true")
    ap.add_argument("--outdir", default=".")
    ap.add_argument("--no-dcost", action="store_true", help="ignore the MV's DCOST = 1e-5 (Launch_Optimiser.py:99; applied as an l1 move penalty by default)")
    ap.add_argument("--scheme", type=int, default=0, help="0 backward Euler (the reference's NODES=2), 1 trapezoid, 2 Hermite-Simpson")
    ap.add_argument("--fly", action="store_true", help="fly the solution's control with RK4 on the device and print what it reaches")
    ap.add_argument("--trim", action="store_true", help="trim t_f and the control so that the flown trajectory reaches its orbit; prints before / after")
    ap.add_argument("--disperse", action="store_true", help="trim, then fly the trimmed control under 50 N of thrust and 1e-3 of control error 1024 times; prints Monte Carlo and linear 1-sigma of the flown apsides")
    ap.add_argument("--guide", action="store_true", help="trim, compute LQ feedback gains and fly 1024 dispersed samples open loop and closed loop; prints both 1-sigmas of the flown apsides")
    ap.add_argument("--feedforward", action="store_true", help="with --guide: also fly the same draws with the thrust feed-forward, once with the thrust known exactly and once known to 10 N (1-sigma) under a navigation bias of 1-sigma %g (scaled; %.1f m) on both positions and %g (scaled; %.1f cm/s) on both velocities" % (NAV_BIAS[0], NAV_BIAS[0] * ORBIT["periapsis"], NAV_BIAS[2], NAV_BIAS[2] * ORBIT["periapsis"] * 100))
    ap.add_argument("--corridor", action="store_true", help="with --disperse or --guide: reduce the samples at every node as well (disperse_batch(history=True)); prints, per flight flown, the widest 1-sigma altitude band, the lowest altitude any sample reached, the largest excursion of the angle beyond its bounds and the step with the most clipped commands, and writes corridor.png (with --guide: of the closed loop; the other flights as corridor_<flight>.png)")
    ap.add_argument("--quantiles", action="store_true", help="with --disperse or --guide: select order statistics of the samples on the device (disperse_batch(quantiles=..., limits=...)); prints, per flight flown, the 0.135 / 50 / 99.865 %%%% points of the flown periapsis and apoapsis and the fraction of samples whose flown periapsis is below %.0f km, and with --corridor the 0.135 %%%% .. 99.865 %%%% altitude band at the node where it is widest" % (PERIAPSIS_LIMIT / 1000))
    ap.add_argument("--nav-tau", type=float, default=None, metavar="SECONDS", help="with --guide --feedforward --corridor --lincov: the navigation bias as a stationary first-order Gauss-Markov process of this correlation time; prints the sampled and the linear altitude band beside those of the frozen bias")
    ap.add_argument("--knowledge-tau", type=float, default=None, metavar="SECONDS", help="with --guide --feedforward --corridor --lincov: the 10 N error of the thrust estimate decays with this time constant")
    ap.add_argument("--filter", action="store_true", help="with --guide --lincov: a Kalman filter on position and velocity fixes (navigation_filter) and the closed loop steering on its estimate (linear_corridor(filter=...)); prints the true and the filter's own 1-sigma of the position and velocity knowledge at burnout, and the burnout altitude 1-sigma with the filter and with the frozen navigation bias")
    ap.add_argument("--lincov", action="store_true", help="with --guide: the linear covariance corridor (linear_corridor) of the open and the closed loop beside their Monte Carlo history; prints both 1-sigma altitude bands at the node where the sampled one is widest, and writes lincov.png (closed loop) and lincov_open_loop.png")
    a = ap.parse_args()
    if a.corridor and not (a.disperse or a.guide):
        ap.error("--corridor needs --disperse or --guide")
    if a.quantiles and not (a.disperse or a.guide):
        ap.error("--quantiles needs --disperse or --guide")
    if a.lincov and not a.guide:
        ap.error("--lincov needs --guide")
    if a.filter and not (a.guide and a.lincov):
        ap.error("--filter needs --guide --lincov")
    if (a.nav_tau is not None or a.knowledge_tau is not None) and not (a.guide and a.feedforward and a.corridor and a.lincov):
        ap.error("--nav-tau and --knowledge-tau need --guide --feedforward --corridor --lincov")
    figdir = None if a.no_plots else a.outdir
    model, variables, v_ins = build()
    if a.no_dcost:
        model.options.ASCENT_DCOST = 0
    if a.scheme:
        model.options.ASCENT_SCHEME = a.scheme
    model.solve(disp=True)
    report(model, variables, v_ins)
    if a.fly:
        fly(model, a.scheme)
    if a.trim:
        trim(model, a.scheme)
    if a.disperse:
        disperse(model, a.scheme, corridor=a.corridor, outdir=figdir, quantiles=a.quantiles)
    if a.guide:
        guide(model, a.scheme, feedforward=a.feedforward, corridor=a.corridor, outdir=figdir, lincov=a.lincov, nav_tau=a.nav_tau,
              knowledge_tau=a.knowledge_tau, quantiles=a.quantiles, navfilter=a.filter)
    if not a.no_plots:
        plots(model, variables, a.outdir)
