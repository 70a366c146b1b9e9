"""CPU reference of the per-node Monte Carlo history (include/ascent.h: ascent_disperse_history_batch) for one problem.

A flight loop of its own over flight_reference.rhs that records, after every step, the ten quantities of the node the step ends
at: the flown state, the altitude, the executed control and the correction of the step.  The perturbations are
dispersion_reference.perturbed's, the beliefs feedforward_reference.beliefs', and the command law is stated as
feedforward_reference.fly_navigated states it (with all-zero gains and no feed-forward it is the open-loop flight of
dispersion_reference.fly_rows, bit for bit in float64).  Nothing here comes from the kernels: the statistics are numpy's over
the samples valid at the node.  `dtype` switches the flight between float64 and numpy's longdouble, as in guidance_reference."""
from __future__ import annotations

import math

import numpy as np

import dispersion_reference as dr
import feedforward_reference as ffr
import flight_reference as fr
import guidance_reference as gr

NQ, ROWS = 10, 52


def altitude(p, x, y):
    """metres above R0 of a scaled position, the radius relation of flight_reference.apsides: p[9] = r_peri, p[2] = R0"""
    X, Y = x * p[9], y * p[9] + p[2]
    return np.sqrt(X * X + Y * Y) - p[2]


def fly_history(p, z0, us, noise, tf, m, nodes, gain_u=None, gain_t=None, smax=0.0, ff_u=None, ff_t=None, theta_hat=0.0, nu=None,
                nu_on=None, formulation=0, dtype=np.float64):
    """One flight, arguments as feedforward_reference.fly_navigated; gain_u None: open loop.  -> (hist (K, 10) of dtype: row k - 1
    is node k, clipped (K,) bool, margin (K,): the distance of the step's command from the clip, inf where the step has neither
    gain nor feed-forward)"""
    rhs = gr._rhs(dtype)
    p = [float(v) for v in p] if dtype is np.float64 else np.asarray(p, dtype=np.float64).astype(dtype)
    K = len(us)
    z = np.array(z0, dtype=dtype)
    th = dtype(theta_hat)
    hist, clipped, margin = np.full((K, NQ), np.nan, dtype=dtype), np.zeros(K, dtype=bool), np.full(K, math.inf)
    with np.errstate(all="ignore"):
        dt = (dtype(tf) * p[11]) / K
        try:
            for k in range(K):
                dz = z - np.asarray(nodes[k], dtype=dtype)
                if nu_on is not None:
                    for i in range(7):
                        if nu_on[i]:
                            dz[i] = dz[i] + dtype(nu[i])
                kk = np.zeros(7, dtype=dtype) if gain_u is None else np.asarray(gain_u[k], dtype=dtype)
                fk = dtype(0) if ff_u is None else dtype(ff_u[k])
                uc = dtype(us[k])
                corr = dtype(0)
                if np.any(kk != 0) or fk != 0:
                    dot = dtype(0)
                    for i in range(7):
                        dot = dot + kk[i] * dz[i]
                    w = uc - dot
                    if fk != 0:
                        w = w - fk * th
                        dot = dot + fk * th
                    uc = min(dtype(1), max(dtype(-1), w)) if math.isfinite(dot) else dtype(np.nan)
                    clipped[k] = bool(uc != w)
                    margin[k] = abs(abs(float(w)) - 1.0) if math.isfinite(w) else 0.0
                    corr = dot
                u = uc + dtype(noise[k]) if noise[k] != 0 else uc
                h = dt / m
                if k == K - 1 and gain_t is not None and smax > 0:
                    dtau = dtype(0)
                    for i in range(7):
                        dtau = dtau - dtype(gain_t[i]) * dz[i]
                    if ff_t is not None and ff_t != 0:
                        dtau = dtau - dtype(ff_t) * th
                    st = min(dtype(smax), max(dtype(-smax), dtau)) if math.isfinite(dtau) else dtype(np.nan)
                    h = (dt * (1 + st)) / m
                u = float(u) if dtype is np.float64 else u
                if formulation == 1:
                    z[4], z[5] = 0.5 * p[12] * (u + 1.0), 0.0
                for _ in range(m):
                    k1 = rhs(p, z, u, formulation)
                    k2 = rhs(p, z + 0.5 * h * k1, u, formulation)
                    k3 = rhs(p, z + 0.5 * h * k2, u, formulation)
                    k4 = rhs(p, z + h * k3, u, formulation)
                    z = z + h / 6.0 * (k1 + 2.0 * (k2 + k3) + k4)
                hist[k, :7] = z
                hist[k, 7], hist[k, 8], hist[k, 9] = altitude(p, z[0], z[1]), u, corr
        except (ValueError, ZeroDivisionError, OverflowError):       # math.* on a non-finite state: the rest stays NaN
            pass
    return hist, clipped, margin


def statistics(nominal, samples, clipped):
    """the 52 rows of hist_out per node, (K, 52), from the nominal rows (K, 10), every sample's (samples, K, 10) and the clipped
    flags (samples, K): numpy over the samples valid at the node"""
    K = nominal.shape[0]
    out = np.full((K, ROWS), np.nan)
    for k in range(K):
        valid = np.isfinite(samples[:, k]).all(axis=1)
        v = samples[valid, k]
        n = len(v)
        out[k, 0] = n
        out[k, 1:11] = nominal[k]
        out[k, 51] = np.count_nonzero(clipped[valid, k])
        if n >= 1:
            out[k, 11:21] = v.mean(axis=0)
            out[k, 31:41], out[k, 41:51] = v.min(axis=0), v.max(axis=0)
        if n >= 2:
            out[k, 21:31] = v.var(axis=0, ddof=1)
    return out


def history(p16, blob, nt, xi, sigma, sigma_u=None, gain_u=None, gain_t=None, smax=0.0, ff_u=None, ff_t=None, know=None, xi_nav=None,
            sigma_nav=None, formulation=0, substeps=0, dtype=np.float64):
    """-> dict(samples (samples, K, 10), clipped (samples, K), margin (samples, K), nominal (K, 10), stats (K, 52), m, nodes):
    one problem at stride 1; arguments as feedforward_reference.disperse_navigated, gain_u None for the open-loop flight"""
    p16 = np.asarray(p16, dtype=np.float64)
    K = nt - 1
    _, us, tf = fr.blob_parts(np.asarray(blob, dtype=np.float64), nt)
    xi, sigma = np.asarray(xi, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    m = fr.substeps_of((tf * p16[11]) / K, substeps)
    S = xi.shape[1]
    smp, clip, marg = np.full((S, K, NQ), np.nan, dtype=dtype), np.zeros((S, K), dtype=bool), np.full((S, K), math.inf)
    if not math.isfinite(tf):
        nominal = np.full((K, NQ), np.nan)
        return dict(samples=smp, clipped=clip, margin=marg, nominal=nominal, stats=statistics(nominal, smp.astype(np.float64), clip), m=m,
                    nodes=None)
    nodes = gr.nominal_nodes(p16, us, tf, m, formulation, dtype)
    nominal, _, _ = fly_history(p16, np.zeros(7), us, np.zeros(K), tf, m, nodes, formulation=formulation, dtype=dtype)
    th, nu, on = ffr.beliefs(xi, sigma, know, xi_nav, sigma_nav) if gain_u is not None else (np.zeros(S), np.zeros((S, 7)), np.zeros(7, dtype=bool))
    noise = np.zeros((K, S))
    if sigma_u is not None:
        su = np.asarray(sigma_u, dtype=np.float64)
        noise[su != 0.0] = su[su != 0.0, None] * xi[dr.NCOL:dr.NCOL + K][su != 0.0]
    for s in range(S):
        p, z0, _, t = dr.perturbed(p16, us, tf, xi, sigma, None, s)
        if math.isfinite(t):
            smp[s], clip[s], marg[s] = fly_history(p, z0, us, noise[:, s], t, m, nodes, gain_u, gain_t, smax, ff_u, ff_t, th[s], nu[s], on,
                                                   formulation, dtype)
    nominal = np.asarray(nominal, dtype=np.float64)
    return dict(samples=smp, clipped=clip, margin=marg, nominal=nominal, stats=statistics(nominal, smp.astype(np.float64), clip), m=m,
                nodes=nodes)
