"""CPU reference of the Monte Carlo dispersion (include/ascent.h: ascent_disperse_batch) for one problem.

Built on flight_reference.rhs and flight_reference.apsides, with a loop of its own: the flight of sample s starts from the
perturbed initial state, reads the perturbed 16 SI fields exactly as flight_reference.rhs reads them, flies the perturbed t_f
and the perturbed controls, and holds the substeps m of the nominal flight (flight_reference.substeps_of at the blob's t_f and
the nominal T_scale).  Nothing here comes from the kernel: the statistics are numpy's mean / cov / min / max over the valid
samples.
"""
from __future__ import annotations

import math

import numpy as np

import flight_reference as fr

NROW, NCOL, STAT_ROWS = 9, 24, 82
IU = np.triu_indices(NROW)


def fly_rows(p, z0, us, tf, m, formulation=0):
    """the nine rows of one flight: p the 16 fields, z0 (7,), us (K,), tf scaled, m substeps per step (held)"""
    p = [float(v) for v in p]
    K = len(us)
    z = np.array(z0, dtype=np.float64)
    with np.errstate(all="ignore"):
        dt = (tf * p[11]) / K
        h = dt / m
        try:
            for k in range(K):
                u = float(us[k])
                if formulation == 1:
                    z[4], z[5] = 0.5 * p[12] * (u + 1.0), 0.0
                for _ in range(m):
                    k1 = fr.rhs(p, z, u, formulation)
                    k2 = fr.rhs(p, z + 0.5 * h * k1, u, formulation)
                    k3 = fr.rhs(p, z + 0.5 * h * k2, u, formulation)
                    k4 = fr.rhs(p, z + h * k3, u, formulation)
                    z = z + h / 6.0 * (k1 + 2.0 * (k2 + k3) + k4)
            peri, apo = fr.apsides(p, *z[:4])
        except (ValueError, ZeroDivisionError, OverflowError):       # math.* on a non-finite state
            return np.full(NROW, np.nan)
    return np.concatenate([z, [peri, apo]])


def perturbed(p16, us, tf, xi, sigma, sigma_u, s):
    """(p, z0, us, tf) of sample s: sigma * xi added where sigma is non-zero, the nominal value itself elsewhere"""
    p16 = np.asarray(p16, dtype=np.float64)
    z0, p, u = np.zeros(7), p16.copy(), np.array(us, dtype=np.float64)
    for i in range(7):
        if sigma[i] != 0.0:
            z0[i] = sigma[i] * xi[i, s]
    for i in range(16):
        if sigma[7 + i] != 0.0:
            p[i] = p16[i] + sigma[7 + i] * xi[7 + i, s]
    if sigma[23] != 0.0:
        tf = tf + sigma[23] * xi[23, s]
    if sigma_u is not None:
        for k in range(len(u)):
            if sigma_u[k] != 0.0:
                u[k] = u[k] + sigma_u[k] * xi[NCOL + k, s]
    return p, z0, u, tf


def statistics(nominal, rows):
    """the 82 rows of stats_out from the nominal rows (9,) and every sample's rows (samples, 9)"""
    out = np.full(STAT_ROWS, np.nan)
    valid = np.isfinite(rows).all(axis=1)
    v = rows[valid]
    n = len(v)
    out[0] = n
    out[1:10] = nominal
    if n >= 1:
        out[10:19] = v.mean(axis=0)
        out[64:73], out[73:82] = v.min(axis=0), v.max(axis=0)
    if n >= 2:
        out[19:64] = np.cov(v.T)[IU]
    return out


def disperse(p16, blob, nt, xi, sigma, sigma_u=None, formulation=0, substeps=0):
    """-> dict(samples (samples, 9), stats (82,), nominal (9,), m): one problem; xi (24 + K, samples) ((24, samples) without
    sigma_u), sigma (24,), sigma_u (K,) or None"""
    p16 = np.asarray(p16, dtype=np.float64)
    K = nt - 1
    _, us, tf = fr.blob_parts(np.asarray(blob, dtype=np.float64), nt)
    xi, sigma = np.asarray(xi, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    m = fr.substeps_of((tf * p16[11]) / K, substeps)
    nominal = fly_rows(p16, np.zeros(7), us, tf, m, formulation) if math.isfinite(tf) else np.full(NROW, np.nan)
    rows = np.empty((xi.shape[1], NROW))
    for s in range(xi.shape[1]):
        p, z0, u, t = perturbed(p16, us, tf, xi, sigma, sigma_u, s)
        rows[s] = fly_rows(p, z0, u, t, m, formulation) if math.isfinite(t) else np.nan
    return dict(samples=rows, stats=statistics(nominal, rows), nominal=nominal, m=m)


def relative_sigma(p16, rel=1e-3):
    """sigma (24,) with rel * |field| on every parameter the flight reads, rel on z_0 and t_f (scaled units)"""
    p16 = np.asarray(p16, dtype=np.float64)
    sigma = np.zeros(NCOL)
    sigma[:7] = rel
    reads = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12]          # not r_apo, tf_lb, tf_ub, dcost
    sigma[[7 + i for i in reads]] = rel * np.abs(p16[reads])
    sigma[23] = rel
    return sigma
