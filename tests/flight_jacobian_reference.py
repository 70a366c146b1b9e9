"""CPU reference of the flight Jacobian and the trim (include/ascent.h: ascent_flight_jacobian, ascent_trim_batch).

The arithmetic of tests/flight_reference.py (the model's right-hand side, classical RK4 with m substeps per collocation step,
the control held over a step, formulation 1's reset of the angle, the two-body apsides) restated with numpy so that it accepts
complex numbers and many perturbed copies at once, and differentiated by the complex step: for an analytic f,
Im f(x + i h) / h = f'(x) to rounding with h = 1e-30 -- no truncation error and no cancellation.  Nothing here comes from the
kernel's tangent recursion or from its chain rule: the parameters enter as the 16 SI fields, exactly as flight_reference.rhs
reads them.  The trim at the end is the algorithm of include/ascent.h built on that Jacobian with dense numpy algebra.
"""
from __future__ import annotations

import math

import numpy as np

import flight_reference as fr

H = 1e-30
NROW, NCOL = 9, 24          # rows: flown z_K (7, scaled), periapsis, apoapsis altitude (m); columns: z_0 (7), 16 fields, t_f


def rhs(p, z, u, formulation=0):
    """flight_reference.rhs for arrays: p (16, n), z (7, n), u (n,) -> (7, n); complex allowed"""
    G, M, R0, Ft, M0, mdot, fuel, ms, accmax, S = p[:10]
    x, y, xd, yd, a, w, m = z
    X, Y = x * S, y * S + R0
    r = np.sqrt(X * X + Y * Y)
    thrust = Ft / ((M0 - ms * m) * r)
    grav = G * M / r ** 3
    c, s = np.cos(3.0 * a), np.sin(3.0 * a)
    ydd = (thrust * (Y * c + X * s) - Y * grav) / S
    xdd = (thrust * (X * c - Y * s) - X * grav) / S
    zero = np.zeros_like(xd)
    if formulation == 1:
        return np.stack([xd, yd, xdd, ydd, zero, zero, mdot / fuel + zero])
    return np.stack([xd, yd, xdd, ydd, w, u * accmax / 3.0 + zero, mdot / fuel + zero])


def step(p, z, u, dt, m, formulation):
    if formulation == 1:
        z = z.copy()
        z[4], z[5] = 0.5 * p[12] * (u + 1.0), 0.0
    h = dt / m
    for _ in range(m):
        k1 = rhs(p, z, u, formulation)
        k2 = rhs(p, z + 0.5 * h * k1, u, formulation)
        k3 = rhs(p, z + 0.5 * h * k2, u, formulation)
        k4 = rhs(p, z + h * k3, u, formulation)
        z = z + h / 6.0 * (k1 + 2.0 * (k2 + k3) + k4)
    return z


def apsides(p, z):
    """flight_reference.apsides for arrays; the branch is taken on the real part of the specific energy; energy >= 0: the
    apoapsis is NaN here (its derivative does not exist)"""
    G, M, R0, S = p[0], p[1], p[2], p[9]
    X, Y, VX, VY = z[0] * S, z[1] * S + R0, z[2] * S, z[3] * S
    GM = G * M
    r = np.sqrt(X * X + Y * Y)
    v2, rv = VX * VX + VY * VY, X * VX + Y * VY
    E = 0.5 * v2 - GM / r
    h = X * VY - Y * VX
    # e from the eccentricity vector (1 + 2 E h^2 / GM^2 loses eps / e^2 near the circle); sqrt of the sum of squares, not abs:
    # it stays analytic for the complex step
    ex, ey = (v2 / GM - 1.0 / r) * X - rv / GM * VX, (v2 / GM - 1.0 / r) * Y - rv / GM * VY
    e = np.sqrt(ex * ex + ey * ey)
    bound = np.real(E) < 0.0
    with np.errstate(all="ignore"):
        a = -GM / (2.0 * E)
        peri = np.where(bound, a * (1.0 - e) - R0, h * h / (GM * (1.0 + e)) - R0)
        apo = np.where(bound, a * (1.0 + e) - R0, np.nan)
    return peri, apo


def flight(p, z0, tf, us, m, formulation, nodes=False):
    """p (16, n), z0 (7, n), tf (n,), us (K, n) -> the nine end quantities (9, n) [and every node's state (K, 7, n)]"""
    K = us.shape[0]
    dt = (tf * p[11]) / K
    z = z0
    zs = []
    for k in range(K):
        z = step(p, z, us[k], dt, m, formulation)
        if nodes:
            zs.append(z)
    peri, apo = apsides(p, z)
    out = np.concatenate([z, peri[None], apo[None]])
    return (out, np.stack(zs)) if nodes else out


def jacobian(p16, blob, nt, formulation=0, substeps=0):
    """-> dict(jac (9, 24), jac_u (9, K), end (9,), m): the Jacobian of the flown end quantities at the blob by complex step;
    parameter columns per SI unit with the blob held fixed in scaled units"""
    p16 = np.asarray(p16, dtype=np.float64)
    K = nt - 1
    _, us, tf = fr.blob_parts(np.asarray(blob, dtype=np.float64), nt)
    if not math.isfinite(tf):
        return dict(jac=np.full((NROW, NCOL), np.nan), jac_u=np.full((NROW, K), np.nan), end=np.full(NROW, np.nan), m=1)
    m = fr.substeps_of((tf * p16[11]) / K, substeps)
    n = NCOL + K + 1                        # the last copy is unperturbed
    p = np.repeat(p16[:, None], n, axis=1).astype(np.complex128)
    z0 = np.zeros((7, n), dtype=np.complex128)
    t = np.full(n, tf, dtype=np.complex128)
    u = np.repeat(us[:, None], n, axis=1).astype(np.complex128)
    for i in range(7):
        z0[i, i] += 1j * H
    for i in range(16):
        p[i, 7 + i] += 1j * H
    t[23] += 1j * H
    for k in range(K):
        u[k, NCOL + k] += 1j * H
    with np.errstate(all="ignore"):
        out = flight(p, z0, t, u, m, formulation)
    d = out.imag / H
    end = out[:, -1].real.copy()
    if not np.real(_energy(p16, end)) < 0.0:
        d[8] = np.nan
    jac, jac_u = d[:, :NCOL].copy(), d[:, NCOL:NCOL + K].copy()
    zero_cols = [7 + 10, 7 + 13, 7 + 14, 7 + 15, 7 + (8 if formulation == 1 else 12)]
    assert np.all(np.nan_to_num(jac[:8, zero_cols]) == 0.0)     # fields the flight does not read
    jac[:, zero_cols] = 0.0
    return dict(jac=jac, jac_u=jac_u, end=end, m=m)


def _energy(p16, end):
    G, M, R0, S = p16[0], p16[1], p16[2], p16[9]
    X, Y, VX, VY = end[0] * S, end[1] * S + R0, end[2] * S, end[3] * S
    return 0.5 * (VX * VX + VY * VY) - G * M / math.hypot(X, Y)


def fly_nodes(p16, us, tf, nt, formulation=0, substeps=0):
    """real flight of a control: (end (9,), states (K, 7), m)"""
    p16 = np.asarray(p16, dtype=np.float64)
    K = nt - 1
    m = fr.substeps_of((tf * p16[11]) / K, substeps)
    with np.errstate(all="ignore"):
        out, zs = flight(p16[:, None], np.zeros((7, 1)), np.array([tf]), np.asarray(us, dtype=np.float64)[:, None], m, formulation,
                         nodes=True)
    return out[:, 0], zs[:, :, 0], m


def conditions(p16, z, terminal=0):
    """the three terminal conditions (e3, g1, g2) of include/ascent.h at a scaled state and their gradient (3, 4) with respect
    to (x, y, xdot, ydot): r.v = 0, |r| = rho_f, |v|^2 = vp2 (terminal 0: circular speed of the mean radius; 1: vis-viva speed
    at the periapsis of the (r_peri, r_apo) ellipse)"""
    G, M, R0, S, ra = p16[0], p16[1], p16[2], p16[9], p16[10]
    GM = G * M
    if terminal == 0:
        vp2 = GM / (R0 + 0.5 * (S + ra)) / (S * S)
    else:
        rp, rA = R0 + S, R0 + ra
        vp2 = GM * (2.0 / rp - 2.0 / (rA + rp)) / (S * S)
    rho0, rhof = R0 / S, (R0 + S) / S
    x, y, vx, vy = z[:4]
    et = y + rho0
    rho = math.hypot(x, et) if math.isfinite(x) and math.isfinite(et) else math.nan
    c = np.array([et * vy + x * vx, rho - rhof, vx * vx + vy * vy - vp2])
    g = np.array([[vx, vy, x, et], [x / rho, et / rho, 0.0, 0.0], [0.0, 0.0, 2.0 * vx, 2.0 * vy]])
    return c, g


TRIM_ROWS = 10


def trim(p16, blob, nt, formulation=0, terminal=0, substeps=0, rounds=6, tol=1e-10):
    """-> dict(blob, summary (10,), history): include/ascent.h: ascent_trim_batch for one problem"""
    p16 = np.asarray(p16, dtype=np.float64)
    K = nt - 1
    blob = np.array(blob, dtype=np.float64)
    _, u0, tf0 = fr.blob_parts(blob, nt)
    u, tf = u0.copy(), tf0
    flag, used, c0, nfree, hist = 0, 0, math.nan, 0.0, []
    for r in range(rounds):
        b = blob.copy()
        b[7 * K:8 * K], b[21 * K] = u, tf
        J = jacobian(p16, b, nt, formulation, substeps)
        c, g = conditions(p16, J["end"], terminal)
        fin = bool(np.all(np.isfinite(c)))
        cn = float(np.abs(c).max()) if fin else math.nan
        if r == 0:
            c0 = cn
        nfree = float((np.abs(u) < 0.999).sum())
        hist.append(cn)
        if not fin:
            flag = 2
            break
        if cn <= tol:
            flag = 1
            break
        A = g @ np.concatenate([J["jac"][:4, 23:24], J["jac_u"][:4]], axis=1)          # (3, K + 1)
        w = np.concatenate([[1.0], (np.abs(u) < 0.999).astype(np.float64)])
        N = (A * w) @ A.T
        try:
            Lc = np.linalg.cholesky(N)
            if not (np.diag(Lc) ** 2 > 1e-300).all():
                raise np.linalg.LinAlgError
            y = np.linalg.solve(N, c)
        except np.linalg.LinAlgError:
            flag = 2
            break
        if not np.all(np.isfinite(y)):
            flag = 2
            break
        delta = -w * (A.T @ y)
        tf = tf + delta[0]
        u = np.where(w[1:] > 0, np.clip(u + delta[1:], -1.0, 1.0), u)
        used += 1
    end, zs, _ = fly_nodes(p16, u, tf, nt, formulation, substeps) if math.isfinite(tf) else (np.full(9, np.nan), np.full((K, 7), np.nan), 1)
    c, _ = conditions(p16, end, terminal)
    fin = bool(np.all(np.isfinite(c)))
    cn = float(np.abs(c).max()) if fin else math.nan
    out = blob.copy()
    out[:7 * K] = zs.ravel()
    out[7 * K:8 * K], out[21 * K] = u, tf
    peri, apo = fr.apsides(p16, *end[:4]) if fin else (math.nan, math.nan)
    ang = zs[:, 4]
    viol = float(np.max(np.maximum(np.maximum(-ang, ang - p16[12]), 0.0))) if np.all(np.isfinite(ang)) else math.nan
    with np.errstate(invalid="ignore"):
        du = float(np.nanmax(np.abs(u - u0))) if np.isfinite(np.abs(u - u0)).any() else 0.0
    summary = np.array([2.0 if (flag == 2 or not fin) else (0.0 if cn <= tol else 1.0), float(used), cn, c0, (tf - tf0) * p16[11],
                        du, nfree, peri, apo, viol])
    return dict(blob=out, summary=summary, history=hist, tf=tf, u=u)
