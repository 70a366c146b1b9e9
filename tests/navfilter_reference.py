"""CPU reference of the navigation filter (include/ascent.h: ascent_navigation_filter, ascent_covariance_filtered_batch) for one
problem, on guidance_reference.records.

design() is the plain Riccati recursion of the header.  corridor() takes a route the kernels do not take, explicit superposition:
the linear system of [dz; e] is propagated for every unit source at once -- the 32 constants, every execution error eps_k and every
measurement noise v_{k,i}, one column each -- and every covariance is the sum over the sources of (variance of the source) x (outer
product of its response).  recursion() is the 14 x 14 covariance recursion the kernel's header states, kept here only so that the
CPU tests can hold the superposition against it.  Nothing here comes from the kernels.  `dtype` switches records and arithmetic
between float64 and numpy's longdouble; the difference of the two runs is what the GPU tests derive their bounds from."""
from __future__ import annotations

import numpy as np

import guidance_reference as gr
import history_reference as hr
import lincov_reference as lr

NQ, NC = lr.NQ, lr.NC
C_P, C_TF, C_E0 = lr.C_P, lr.C_TF, lr.C_NU
TRIU7 = np.triu_indices(7)


def _f(a, dtype):
    return np.asarray(a, dtype=np.float64).astype(dtype)


def meas_nodes(K, meas_stride):
    """the 1-based nodes at which the measurements are taken"""
    return [j for j in range(1, K + 1) if j % meas_stride == 0]


def design(rec, sigma_nav, meas_h, meas_sigma, meas_stride=1, sigma_u=None, filter_q=None, dtype=np.float64):
    """-> dict(gain_l (K, M, 7), P (K, 7, 7) after the update at node k = 1 .. K, s (list of (node, i, s)), status, first_bad).  The
    recursion of the header: P^- = Phi P Phi' + sigma_u^2 g g' + diag(q^2); s = h' P h + sigma^2, l = P h / s, Joseph update."""
    K = len(rec["us"])
    h, sg = _f(meas_h, dtype), _f(meas_sigma, dtype)
    M = len(sg)
    su2 = np.zeros(K, dtype=dtype) if sigma_u is None else _f(sigma_u, dtype) ** 2
    q2 = np.zeros(7, dtype=dtype) if filter_q is None else _f(filter_q, dtype) ** 2
    P = np.diag(_f(sigma_nav, dtype) ** 2)
    I = np.eye(7, dtype=dtype)
    gl, Ps, ss, first_bad = np.zeros((K, M, 7), dtype=dtype), np.zeros((K, 7, 7), dtype=dtype), [], 0
    with np.errstate(all="ignore"):
        for k in range(1, K + 1):
            Phi, g = rec["Phi"][k - 1], rec["g"][k - 1]
            P = Phi @ P @ Phi.T + su2[k - 1] * np.outer(g, g) + np.diag(q2)
            P = (P + P.T) / 2
            if k % meas_stride == 0:
                for i in range(M):
                    s = h[i] @ P @ h[i] + sg[i] ** 2
                    ss.append((k, i, s))
                    if not first_bad and not (sg[i] > 0 and s > 0 and np.isfinite(s)):
                        first_bad = k
                    l = P @ h[i] / s
                    A = I - np.outer(l, h[i])
                    P = A @ P @ A.T + sg[i] ** 2 * np.outer(l, l)
                    P = (P + P.T) / 2
                    gl[k - 1, i] = l
            Ps[k - 1] = P
    if first_bad:
        gl[first_bad - 1:] = np.nan
        Ps[first_bad - 1:] = np.nan
    return dict(gain_l=gl, P=Ps, s=ss, status=2 if first_bad else 0, first_bad=first_bad)


def _law(K, sigma, sigma_u, gain_u, gain_t, smax, sigma_nav, dtype):
    sn8 = np.concatenate([np.asarray(sigma_nav, dtype=np.float64), [0.0]])
    Ku, _, stretch, kt, _, su2, var = lr.law_arrays(K, sigma, sigma_u, gain_u, gain_t, smax, None, None, sn8, dtype)
    return Ku, stretch, kt, su2, var


def corridor(p16, blob, nt, sigma, sigma_nav, gain_l, meas_h, meas_sigma, meas_stride=1, sigma_u=None, gain_u=None, gain_t=None, smax=0.0,
             formulation=0, substeps=0, dtype=np.float64, rec=None):
    """Superposition.  -> dict(S (K, 10, 32), cov (K, 10, 10), noise (K, 10, 10) the part of cov from eps and v, nav_jac (K, 7, 32),
    nav_cov (K, 7, 7), nav_noise (K, 7, 7), nominal (K, 10), rec): row j - 1 is node j.  sigma (24,), sigma_nav (7,) of e_0, gain_l
    (K, M, 7) read at the measurement nodes only, meas_h (M, 7), meas_sigma (M,), sigma_u (K,) or None, gain_u (K, 7) or None."""
    if rec is None:
        rec = gr.records(p16, blob, nt, formulation, substeps, dtype)
    K = nt - 1
    Ku, stretch, kt, su2, var = _law(K, sigma, sigma_u, gain_u, gain_t, smax, sigma_nav, dtype)
    h, sg, gl = _f(meas_h, dtype), _f(meas_sigma, dtype), _f(gain_l, dtype)
    M = len(sg)
    mn = meas_nodes(K, meas_stride)
    NS = NC + K + len(mn) * M                              # sources: the constants | eps_1 .. eps_K | v_{k,i}, node by node
    svar = np.concatenate([var, su2, np.ones(len(mn) * M, dtype=dtype)])
    D, E = np.zeros((7, NS), dtype=dtype), np.zeros((7, NS), dtype=dtype)
    D[np.arange(7), np.arange(7)] = 1
    E[np.arange(7), C_E0 + np.arange(7)] = 1
    out = dict(S=np.zeros((K, NQ, NC), dtype=dtype), cov=np.zeros((K, NQ, NQ), dtype=dtype), noise=np.zeros((K, NQ, NQ), dtype=dtype),
               nav_jac=np.zeros((K, 7, NC), dtype=dtype), nav_cov=np.zeros((K, 7, 7), dtype=dtype), nav_noise=np.zeros((K, 7, 7), dtype=dtype),
               nominal=np.zeros((K, NQ), dtype=dtype), rec=rec)
    p = np.asarray(p16, dtype=np.float64).astype(dtype)
    sym = lambda a: (a + a.T) / 2
    with np.errstate(all="ignore"):
        for k in range(1, K + 1):
            Phi, g = rec["Phi"][k - 1], rec["g"][k - 1]
            eps = np.zeros(NS, dtype=dtype)
            eps[NC + k - 1] = 1
            corr = Ku[k - 1] @ (D + E)
            du = -corr + eps
            forced = np.zeros((7, NS), dtype=dtype)
            forced[:, C_P:C_TF] = rec["dp"][k - 1]
            forced[:, C_TF] = rec["dtf"][k - 1]
            Dn = Phi @ D + np.outer(g, du) + forced
            if k == K and stretch:
                Dn = Dn + np.outer(rec["gamma"], -(kt @ (D + E)))
            En = Phi @ E - np.outer(g, eps) - forced
            if k in mn:
                for i in range(M):
                    v = np.zeros(NS, dtype=dtype)
                    v[NC + K + mn.index(k) * M + i] = 1
                    En = En + np.outer(gl[k - 1, i], -(h[i] @ En) + sg[i] * v)
            z = rec["nodes"][k]
            ga, direct = lr.altitude_gradient(p16, z, dtype)
            y = np.zeros((NQ, NS), dtype=dtype)
            y[:7] = Dn
            y[7] = ga @ Dn
            y[7, C_P:C_TF] += direct
            y[8], y[9] = du, corr
            out["S"][k - 1], out["nav_jac"][k - 1] = y[:, :NC], En[:, :NC]
            out["cov"][k - 1], out["noise"][k - 1] = sym((y * svar) @ y.T), sym((y[:, NC:] * svar[NC:]) @ y[:, NC:].T)
            out["nav_cov"][k - 1], out["nav_noise"][k - 1] = sym((En * svar) @ En.T), sym((En[:, NC:] * svar[NC:]) @ En[:, NC:].T)
            out["nominal"][k - 1, :7] = z
            out["nominal"][k - 1, 7], out["nominal"][k - 1, 8] = hr.altitude(p, z[0], z[1]), rec["us"][k - 1]
            D, E = Dn, En
    return out


def recursion(rec, sigma_u, gain_u, gain_t, smax, gain_l, meas_h, meas_sigma, meas_stride=1, dtype=np.float64):
    """The covariance of w = [dz; e] under eps and v as a 14 x 14 recursion: -> Q (K, 14, 14) after the update at node k = 1 .. K.
    Q_k^- = F Q F' + sigma_u^2 [g; -g][g; -g]', F = [A, -g K'; 0, Phi]; per measurement Q <- U Q U' + sigma^2 [0; l][0; l]',
    U = diag(I, I - l h')."""
    K = len(rec["us"])
    Ku, stretch, kt, su2, _ = _law(K, np.zeros(24), sigma_u, gain_u, gain_t, smax, np.zeros(7), dtype)
    h, sg, gl = _f(meas_h, dtype), _f(meas_sigma, dtype), _f(gain_l, dtype)
    Q, out = np.zeros((14, 14), dtype=dtype), np.zeros((K, 14, 14), dtype=dtype)
    for k in range(1, K + 1):
        Phi, g = rec["Phi"][k - 1], rec["g"][k - 1]
        B = -np.outer(g, Ku[k - 1])
        if k == K and stretch:
            B = B - np.outer(rec["gamma"], kt)
        F = np.zeros((14, 14), dtype=dtype)
        F[:7, :7], F[:7, 7:], F[7:, 7:] = Phi + B, B, Phi
        ge = np.concatenate([g, -g])
        Q = F @ Q @ F.T + su2[k - 1] * np.outer(ge, ge)
        if k % meas_stride == 0:
            for i in range(len(sg)):
                U = np.eye(14, dtype=dtype)
                U[7:, 7:] -= np.outer(gl[k - 1, i], h[i])
                le = np.concatenate([np.zeros(7, dtype=dtype), gl[k - 1, i]])
                Q = U @ Q @ U.T + sg[i] ** 2 * np.outer(le, le)
        Q = (Q + Q.T) / 2
        out[k - 1] = Q
    return out


def gain_scales(gain_l):
    """(K, M): max(1, the infinity norm) of every gain column, the scale a gain is compared in"""
    return np.maximum(1.0, np.abs(np.asarray(gain_l, dtype=np.float64)).max(axis=2))
