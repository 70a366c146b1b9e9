"""CPU reference of the time-varying navigation error (include/ascent.h: ascent_disperse_drifting_batch and
ascent_covariance_drifting_batch) for one problem.

The eight knowledge channels are first-order Gauss-Markov sequences n_k = phi n_{k-1} + q omega_{k-1}; step k steers on n_k.
history_drifting hands guidance_reference.fly a nu_k and a theta-hat_k per step.  corridor_drifting is
lincov_reference.corridor's Jacobian recursion with the forcing of the columns 24..31 scaled by phi^k, and the part of the noise
that the driving draws add is formed by superposition: one linear run of the step recursion per unit impulse of eps_k and of
omega_a,k on guidance_reference.records, then sum var * outer(response, response).  The covariances C and D of the kernel's
recursion are never formed.  Nothing here comes from the kernels.  `dtype` switches float64 and numpy's longdouble."""
from __future__ import annotations

import numpy as np

import feedforward_reference as ffr
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


def history_drifting(p16, blob, nt, xi, sigma, sigma_u, gain_u, gain_t=None, smax=0.0, ff_u=None, ff_t=None, know=None, xi_nav=None,
                     sigma_nav=None, phi=None, q=None, omega=None, formulation=0, substeps=0, dtype=np.float64):
    """history_reference.history with the drifting channels phi, q (8,) and their draws omega (8, K, samples): -> the same dict.
    The blob's t_f must be finite."""
    K, S = nt - 1, np.shape(xi)[1]
    th_all, _, _ = ffr.beliefs(xi, sigma, know, xi_nav, sigma_nav)          # a frozen channel 7: the navigated call's theta-hat
    no7 = None if sigma_nav is None else np.concatenate([np.asarray(sigma_nav, dtype=np.float64)[:7], [0.0]])
    th_w, _, _ = ffr.beliefs(xi, sigma, know, xi_nav, no7)                  # w . dp alone
    n, on = sequences(K, xi_nav, sigma_nav, phi, q, omega if omega is not None else np.zeros((NA, K, S)), dtype)
    th = np.broadcast_to(th_all.astype(dtype)[:, None], (S, K)) if frozen(phi, q)[7] else th_w.astype(dtype)[:, None] + n[:, 1:, 7]
    m, nodes, nominal, flights = gr.fly_samples(p16, blob, nt, xi, sigma, sigma_u, (gain_u, gain_t, smax, ff_u, ff_t), th, n[:, 1:, :7], on[:7],
                                                formulation, substeps, dtype)
    return dict(hr.history_result(m, nodes, nominal.hist, flights, dtype, K), n=n)


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
    Ku, fu, stretch, kt, ft, su2, var = lr.law_arrays(K, sigma, sigma_u, gain_u, gain_t, smax, ff_u, ff_t, sigma_nav, dtype)
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
