"""CPU reference of the flight verification (include/ascent.h: ascent_fly_batch): the model's ODEs integrated under the
control of a solution blob, written from the reference script's equations, not from the kernel and not from oracle/.

Right-hand side (Launch_Optimiser.py:114-136, per second: the script's d/dtau = tf * final_time * d/dt divided through):
    x' = xdot, y' = ydot, angle' = angledot, angledot' = u * ang_acc_max / 3, mass' = mdot / fuel_mass,
    X = x S, Y = y S + R0, r = sqrt(X^2 + Y^2), S = r_peri,
    ydot' = (Ft / ((M0 - mass_scalar mass) r) (Y cos 3a + X sin 3a) - Y G M / r^3) / S,
    xdot' = (Ft / ((M0 - mass_scalar mass) r) (X cos 3a - Y sin 3a) - X G M / r^3) / S.
Node 0 is the zero state; step k flies dt = tf T_scale / K seconds with u_k held.  Formulation 1 (the v1 script): the angle is
held at (angle_ub / 2)(u_k + 1) over step k and angledot is 0.

Two integrators: (i) "rk4": classical RK4 with the library's step rule (m substeps per collocation step; m = 0: ceil(dt / 0.5 s)
clamped to 1 .. 4096); (ii) "dop853": scipy's DOP853 at rtol 1e-13, atol 1e-15, restarted at every node.
"""
from __future__ import annotations

import math

import numpy as np

FIELDS = ("G", "M", "R0", "Ft", "M0", "mdot", "fuel_mass", "mass_scalar", "ang_acc_max", "r_peri", "r_apo", "T_scale",
          "angle_ub", "tf_lb", "tf_ub", "dcost")
SUMMARY = ("miss_pos_m", "miss_vel_ms", "flown_periapsis_alt_m", "flown_apoapsis_alt_m", "nlp_periapsis_alt_m",
           "nlp_apoapsis_alt_m", "max_local_pos_m", "max_local_vel_ms", "max_local_step", "substeps")
MAX_SUBSTEPS = 4096


def rhs(p, z, u, formulation=0):
    """dz/dt per second at z = (x, y, xdot, ydot, angle, angledot, mass), p = the 16 parameters in FIELDS order"""
    G, M, R0, Ft, M0, mdot, fuel, ms, accmax, S = p[:10]
    x, y, xd, yd, a, w, m = z
    X, Y = x * S, y * S + R0
    r = math.sqrt(X * X + Y * Y)
    thrust = Ft / ((M0 - ms * m) * r)
    grav = G * M / r ** 3
    c, s = math.cos(3.0 * a), math.sin(3.0 * a)
    ydd = (thrust * (Y * c + X * s) - Y * grav) / S
    xdd = (thrust * (X * c - Y * s) - X * grav) / S
    if formulation == 1:
        return np.array([xd, yd, xdd, ydd, 0.0, 0.0, mdot / fuel])
    return np.array([xd, yd, xdd, ydd, w, u * accmax / 3.0, mdot / fuel])


def substeps_of(dt, substeps=0):
    if substeps > 0:
        return int(substeps)
    if not math.isfinite(dt):
        return 1
    return int(min(max(math.ceil(dt / 0.5), 1), MAX_SUBSTEPS))


def _step(p, z, u, dt, m, formulation, integrator):
    z = np.array(z, dtype=np.float64)
    if formulation == 1:
        z[4], z[5] = 0.5 * p[12] * (u + 1.0), 0.0
    if integrator == "rk4":
        h = dt / m
        for _ in range(m):
            k1 = rhs(p, z, u, formulation)
            k2 = rhs(p, z + 0.5 * h * k1, u, formulation)
            k3 = rhs(p, z + 0.5 * h * k2, u, formulation)
            k4 = rhs(p, z + h * k3, u, formulation)
            z = z + h / 6.0 * (k1 + 2.0 * (k2 + k3) + k4)
        return z
    from scipy.integrate import solve_ivp
    r = solve_ivp(lambda t, s: rhs(p, s, u, formulation), (0.0, dt), z, method="DOP853", rtol=1e-13, atol=1e-15)
    assert r.success, r.message
    return r.y[:, -1]


def apsides(p, x, y, xd, yd):
    """periapsis / apoapsis altitude above R0 (m) of the two-body orbit through a scaled state, from the specific energy and
    the eccentricity vector (1 + 2 E h^2 / GM^2 loses eps / e^2 near the circle); energy >= 0: apoapsis +inf"""
    G, M, R0, S = p[0], p[1], p[2], p[9]
    X, Y, VX, VY = x * S, y * S + R0, xd * S, yd * S
    GM = G * M
    r = math.hypot(X, Y)
    v2, rv = VX * VX + VY * VY, X * VX + Y * VY
    E = 0.5 * v2 - GM / r
    h = X * VY - Y * VX
    e = math.hypot((v2 / GM - 1.0 / r) * X - rv / GM * VX, (v2 / GM - 1.0 / r) * Y - rv / GM * VY)
    if E >= 0.0:
        return h * h / (GM * (1.0 + e)) - R0, math.inf
    a = -GM / (2.0 * E)
    return a * (1.0 - e) - R0, a * (1.0 + e) - R0


def blob_parts(blob, nt):
    K = nt - 1
    return blob[:7 * K].reshape(K, 7), blob[7 * K:8 * K], float(blob[21 * K])


def make_blob(z, u, tf):
    """a blob (21K+10,) that holds states (K, 7), controls (K,) and tf; everything else zero"""
    K = len(u)
    b = np.zeros(21 * K + 10)
    b[:7 * K] = np.asarray(z, dtype=np.float64).ravel()
    b[7 * K:8 * K] = u
    b[21 * K] = tf
    return b


def fly(p16, blob, nt, formulation=0, substeps=0, integrator="rk4", want_local=True):
    """-> dict(traj (10, nt) in TRAJ_FIELDS order, local (K, 7) or None, summary (10,) in SUMMARY order, m)"""
    p = [float(v) for v in p16]
    K = nt - 1
    zs, us, tf = blob_parts(np.asarray(blob, dtype=np.float64), nt)
    S, T = p[9], p[11]
    dt = (tf * T) / K
    m = substeps_of(dt, substeps)

    def row(z, u):
        f = rhs(p, z, u, formulation)
        return [z[0], z[1], z[2], z[3], f[2], f[3], z[4], z[5], u, z[6]]

    z = np.zeros(7)
    traj = np.zeros((nt, 10))
    traj[0] = row(z, 0.0)
    for k in range(K):
        z = _step(p, z, us[k], dt, m, formulation, integrator)
        traj[k + 1] = row(z, us[k])
    local = None
    summary = np.full(10, np.nan)
    if want_local:
        local = np.zeros((K, 7))
        for k in range(K):
            za = zs[k - 1] if k else np.zeros(7)
            local[k] = _step(p, za, us[k], dt, m, formulation, integrator) - zs[k]
        ep, ev = np.hypot(local[:, 0], local[:, 1]), np.hypot(local[:, 2], local[:, 3])
        summary[6], summary[7], summary[8] = S * ep.max(), S * ev.max(), float(np.argmax(ep) + 1)
    zn = zs[-1]
    summary[0] = S * math.hypot(z[0] - zn[0], z[1] - zn[1])
    summary[1] = S * math.hypot(z[2] - zn[2], z[3] - zn[3])
    summary[2], summary[3] = apsides(p, *z[:4])
    summary[4], summary[5] = apsides(p, *zn[:4])
    summary[9] = float(m)
    return dict(traj=traj.T.copy(), local=local, summary=summary, m=m)


def synthetic_exact_blob(p16, nt, tf=0.9, seed=0):
    """A blob whose states are themselves an accurate (DOP853) flight of an arbitrary bounded control: a smooth pitch-over
    pattern plus seeded noise, |u| <= 1.  Its local errors and miss are the integrator's own error, whatever any solver does."""
    rng = np.random.default_rng(seed)
    K = nt - 1
    tau = (np.arange(K) + 0.5) / K
    u = np.clip(0.6 * np.cos(2.0 * np.pi * tau) * np.exp(-2.0 * tau) + 0.2 * rng.uniform(-1.0, 1.0, K), -1.0, 1.0)
    p = [float(v) for v in p16]
    dt = (tf * p[11]) / K
    z = np.zeros(7)
    zs = np.zeros((K, 7))
    for k in range(K):
        z = _step(p, z, u[k], dt, 1, 0, "dop853")
        zs[k] = z
    return make_blob(zs, u, tf)
