"""CPU reference of the time-varying navigation error (include/ascent.h: ascent_disperse_drifting_batch and
ascent_covariance_drifting_batch) for one problem.

The eight knowledge channels are first-order Gauss-Markov sequences n_k = phi n_{k-1} + q omega_{k-1}; step k steers on n_k.
fly_drifting is history_reference.fly_history's loop with the per-step nu_k and theta-hat_k.  corridor_drifting is
lincov_reference.corridor's Jacobian recursion with the forcing of the columns 24..31 scaled by phi^k, and the part of the noise
that the driving draws add is formed by superposition: one linear run of the step recursion per unit impulse of eps_k and of
omega_a,k on guidance_reference.records, then sum var * outer(response, response).  The covariances C and D of the kernel's
recursion are never formed.  Nothing here comes from the kernels.  `dtype` switches float64 and numpy's longdouble."""
from __future__ import annotations

import math

import numpy as np

import dispersion_reference as dr
import feedforward_reference as ffr
import flight_reference as fr
import guidance_reference as gr
import history_reference as hr
import lincov_reference as lr

NQ, NC, NA = 10, 32, 8


def frozen(phi, q):
    """(8,) bool: channels that are never updated; both arrays None: all of them"""
    if phi is None:
        return np.ones(NA, dtype=bool)
    return (np.asarray(phi, dtype=np.float64) == 1.0) & (np.asarray(q, dtype=np.float64) == 0.0)


def sequences(K, xi_nav, sigma_nav, phi, q, omega, dtype=np.float64):
    """-> (n (samples, K + 1, 8) of dtype: n[:, k] is n_k, applied (8,) bool).  n_0 = sigma_nav * xi_nav where sigma_nav is not
    zero; a frozen channel stays there; omega (8, K, samples), row k the draw behind step k + 1, read only where q is not zero."""
    S = np.asarray(omega if omega is not None else xi_nav).shape[-1]
    sn = np.zeros(NA) if sigma_nav is None else np.asarray(sigma_nav, dtype=np.float64)
    fz = frozen(phi, q)
    n = np.zeros((S, K + 1, NA), dtype=dtype)
    applied = np.zeros(NA, dtype=bool)
    for a in range(NA):
        if sn[a] != 0:
            n[:, 0, a] = dtype(sn[a]) * np.asarray(xi_nav[a], dtype=np.float64).astype(dtype)
            applied[a] = True
        if fz[a]:
            n[:, 1:, a] = n[:, :1, a]
            continue
        ph, qa = dtype(phi[a]), dtype(q[a])
        applied[a] = applied[a] or q[a] != 0
        for k in range(1, K + 1):
            n[:, k, a] = ph * n[:, k - 1, a]
            if q[a] != 0:
                n[:, k, a] = n[:, k, a] + qa * np.asarray(omega[a][k - 1], dtype=np.float64).astype(dtype)
    return n, applied


def fly_drifting(p, z0, us, noise, tf, m, nodes, gain_u=None, gain_t=None, smax=0.0, ff_u=None, ff_t=None, theta_hat=None, nu=None,
                 nu_on=None, formulation=0, dtype=np.float64):
    """history_reference.fly_history with theta_hat (K,) and nu (K, 7): row k - 1 is what step k steers on (the cutoff stretch of
    step K uses row K - 1 as well).  -> (hist (K, 10), clipped (K,), margin (K,)) as there."""
    rhs = gr._rhs(dtype)
    p = [float(v) for v in p] if dtype is np.float64 else np.asarray(p, dtype=np.float64).astype(dtype)
    K = len(us)
    z = np.array(z0, dtype=dtype)
    hist, clipped, margin = np.full((K, NQ), np.nan, dtype=dtype), np.zeros(K, dtype=bool), np.full(K, math.inf)
    with np.errstate(all="ignore"):
        dt = (dtype(tf) * p[11]) / K
        try:
            for k in range(K):
                th = dtype(0) if theta_hat is None else dtype(theta_hat[k])
                dz = z - np.asarray(nodes[k], dtype=dtype)
                if nu_on is not None:
                    for i in range(7):
                        if nu_on[i]:
                            dz[i] = dz[i] + dtype(nu[k][i])
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
                hist[k, 7], hist[k, 8], hist[k, 9] = hr.altitude(p, z[0], z[1]), u, corr
        except (ValueError, ZeroDivisionError, OverflowError):       # math.* on a non-finite state: the rest stays NaN
            pass
    return hist, clipped, margin


def history_drifting(p16, blob, nt, xi, sigma, sigma_u, gain_u, gain_t=None, smax=0.0, ff_u=None, ff_t=None, know=None, xi_nav=None,
                     sigma_nav=None, phi=None, q=None, omega=None, formulation=0, substeps=0, dtype=np.float64):
    """history_reference.history with the drifting channels phi, q (8,) and their draws omega (8, K, samples): -> the same dict.
    The blob's t_f must be finite."""
    p16 = np.asarray(p16, dtype=np.float64)
    K = nt - 1
    _, us, tf = fr.blob_parts(np.asarray(blob, dtype=np.float64), nt)
    xi, sigma = np.asarray(xi, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    m = fr.substeps_of((tf * p16[11]) / K, substeps)
    S = xi.shape[1]
    smp, clip, marg = np.full((S, K, NQ), np.nan, dtype=dtype), np.zeros((S, K), dtype=bool), np.full((S, K), math.inf)
    nodes = gr.nominal_nodes(p16, us, tf, m, formulation, dtype)
    nominal, _, _ = hr.fly_history(p16, np.zeros(7), us, np.zeros(K), tf, m, nodes, formulation=formulation, dtype=dtype)
    th_all, _, _ = ffr.beliefs(xi, sigma, know, xi_nav, sigma_nav)          # a frozen channel 7: the navigated call's theta-hat
    no7 = None if sigma_nav is None else np.concatenate([np.asarray(sigma_nav, dtype=np.float64)[:7], [0.0]])
    th_w, _, _ = ffr.beliefs(xi, sigma, know, xi_nav, no7)                  # w . dp alone
    n, on = sequences(K, xi_nav, sigma_nav, phi, q, omega if omega is not None else np.zeros((NA, K, S)), dtype)
    fz7 = frozen(phi, q)[7]
    noise = np.zeros((K, S))
    if sigma_u is not None:
        su = np.asarray(sigma_u, dtype=np.float64)
        noise[su != 0.0] = su[su != 0.0, None] * xi[dr.NCOL:dr.NCOL + K][su != 0.0]
    for s in range(S):
        p, z0, _, t = dr.perturbed(p16, us, tf, xi, sigma, None, s)
        if math.isfinite(t):
            th = np.full(K, th_all[s], dtype=dtype) if fz7 else dtype(th_w[s]) + n[s, 1:, 7]
            smp[s], clip[s], marg[s] = fly_drifting(p, z0, us, noise[:, s], t, m, nodes, gain_u, gain_t, smax, ff_u, ff_t, th,
                                                    n[s, 1:, :7], on[:7], formulation, dtype)
    nominal = np.asarray(nominal, dtype=np.float64)
    return dict(samples=smp, clipped=clip, margin=marg, nominal=nominal, stats=hr.statistics(nominal, smp.astype(np.float64), clip), m=m,
                nodes=nodes, n=n)


def corridor_drifting(p16, blob, nt, sigma, sigma_u=None, gain_u=None, gain_t=None, smax=0.0, ff_u=None, ff_t=None, know=None,
                      sigma_nav=None, phi=None, q=None, formulation=0, substeps=0, dtype=np.float64, rec=None):
    """lincov_reference.corridor with the drifting channels phi, q (8,) or None.  -> dict(S (K, 10, 32), cov, noise (K, 10, 10),
    nominal (K, 10), rec, m_eps (K, 10, K): the response of y_j to a unit eps_k, r_om (K, 10, 8, K): to a unit q_a omega_a,k
    (k the step the draw enters, 1-based at index k - 1), var_n (K + 1, 8): the variance of n_k the drive alone builds up).
    noise = the execution-error part (lincov_reference.corridor's own, so that frozen channels give its bits; its superposition
    from m_eps is checked against it in the tests) + sum_a sum_k q_a^2 r r'."""
    if rec is None:
        rec = gr.records(p16, blob, nt, formulation, substeps, dtype)
    base = lr.corridor(p16, blob, nt, sigma, sigma_u, gain_u, gain_t, smax, ff_u, ff_t, know, sigma_nav, formulation, substeps, dtype, rec)
    K = nt - 1
    f = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
    ph = np.ones(NA, dtype=dtype) if phi is None else f(phi)
    q2 = np.zeros(NA, dtype=dtype) if q is None else f(q) ** 2
    Ku = np.zeros((K, 7), dtype=dtype) if gain_u is None else f(gain_u)
    fu = np.zeros(K, dtype=dtype) if ff_u is None or gain_u is None else f(ff_u)
    stretch = gain_u is not None and gain_t is not None and smax > 0
    kt = f(gain_t) if stretch else np.zeros(7, dtype=dtype)
    ft = dtype(ff_t) if stretch and ff_t is not None else dtype(0)
    su2 = np.zeros(K, dtype=dtype) if sigma_u is None else f(sigma_u) ** 2
    var = np.concatenate([f(sigma), np.zeros(8, dtype=dtype) if sigma_nav is None else f(sigma_nav)]) ** 2
    thw = np.zeros(NC, dtype=dtype)
    if know is not None:
        thw[lr.C_P:lr.C_TF] = f(know)
    D = np.zeros((7, NC), dtype=dtype)
    D[np.arange(7), lr.C_Z0 + np.arange(7)] = 1
    pw = np.ones(NA, dtype=dtype)
    NI = K + NA * K                                        # impulses: eps_1 .. eps_K | omega_a,k at K + a * K + k - 1
    Z, Nn = np.zeros((7, NI), dtype=dtype), np.zeros((NA, NI), dtype=dtype)
    wgt = np.concatenate([np.zeros(K, dtype=dtype), np.repeat(q2, K)])      # the drive's part alone
    S, cov, noise = np.zeros((K, NQ, NC), dtype=dtype), np.zeros((K, NQ, NQ), dtype=dtype), np.zeros((K, NQ, NQ), dtype=dtype)
    resp = np.zeros((K, NQ, NI), dtype=dtype)
    var_n = np.zeros((K + 1, NA), dtype=dtype)
    with np.errstate(all="ignore"):
        for k in range(1, K + 1):
            Phi, g = rec["Phi"][k - 1], rec["g"][k - 1]
            pw = pw * ph                                   # once per step, ascending: phi = 1 leaves the bits alone
            th = thw.copy()
            th[lr.C_E] = pw[7]
            N = np.zeros((7, NC), dtype=dtype)
            N[np.arange(7), lr.C_NU + np.arange(7)] = pw[:7]
            corr = Ku[k - 1] @ (D + N) + fu[k - 1] * th
            Dn = Phi @ D - np.outer(g, corr)
            Dn[:, lr.C_P:lr.C_TF] += rec["dp"][k - 1]
            Dn[:, lr.C_TF] += rec["dtf"][k - 1]
            # the impulses: n_k first, then the step
            Nn = ph[:, None] * Nn
            for a in range(NA):
                Nn[a, K + a * K + k - 1] = 1
            kap = np.concatenate([Ku[k - 1], [fu[k - 1]]])
            ic = Ku[k - 1] @ Z + kap @ Nn
            e = np.zeros(NI, dtype=dtype)
            e[k - 1] = 1
            du = -ic + e
            Zn = Phi @ Z + np.outer(g, du)
            if k == K and stretch:
                tau = -(kt @ (D + N)) - ft * th
                Dn = Dn + np.outer(rec["gamma"], tau)
                Zn = Zn + np.outer(rec["gamma"], -(kt @ Z) - np.concatenate([kt, [ft]]) @ Nn)
            z = rec["nodes"][k]
            ga, direct = lr.altitude_gradient(p16, z, dtype)
            y = np.zeros((NQ, NC), dtype=dtype)
            y[:7] = Dn
            y[7] = ga @ Dn
            y[7, lr.C_P:lr.C_TF] += direct
            y[8], y[9] = -corr, corr
            S[k - 1] = y
            resp[k - 1] = np.concatenate([Zn, (ga @ Zn)[None], du[None], ic[None]])
            no = (resp[k - 1] * wgt) @ resp[k - 1].T
            noise[k - 1] = base["noise"][k - 1] + (no + no.T) / 2
            c = (y * var) @ y.T
            cov[k - 1] = (c + c.T) / 2 + noise[k - 1]
            D, Z = Dn, Zn
            var_n[k] = np.array([(Nn[a, K + a * K:K + (a + 1) * K] ** 2).sum() * q2[a] for a in range(NA)], dtype=dtype)
    return dict(S=S, cov=cov, noise=noise, nominal=base["nominal"], rec=rec, Q=base["Q"], m_eps=resp[:, :, :K],
                r_om=resp[:, :, K:].reshape(K, NQ, NA, K), var_n=var_n, su2=su2, q2=q2)
