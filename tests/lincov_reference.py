"""CPU reference of the linear covariance corridor (include/ascent.h: ascent_covariance_history_batch) for one problem.

The recursion of the header in dense numpy over all 32 columns at once (the kernel carries a compressed column space and expands
it at the nodes; nothing of that is here): the step records are guidance_reference.records' complex-step derivatives about the
reference's own nominal flight, the altitude's gradient and its direct terms the complex step on history_reference.altitude.
Nothing here comes from the kernels.  `dtype` switches records and recursion between float64 and numpy's longdouble; the
difference of the two runs is what the GPU tests derive their bounds from."""
from __future__ import annotations

import numpy as np

import guidance_reference as gr
import history_reference as hr

NQ, NC = 10, 32
C_Z0, C_P, C_TF, C_NU, C_E = 0, 7, 23, 24, 31
TRIU = np.triu_indices(NQ)


def altitude_gradient(p16, z, dtype=np.float64):
    """-> (ga (7,): d altitude / d z at the scaled state z, direct (16,): its direct dependence on the fields), complex step"""
    ct = gr._complex(dtype)
    p = np.asarray(p16, dtype=np.float64).astype(dtype)
    h = dtype(gr.H)
    ga, direct = np.zeros(7, dtype=dtype), np.zeros(16, dtype=dtype)
    for i in (0, 1):
        zz = np.asarray(z, dtype=dtype).astype(ct)
        zz[i] += 1j * h
        ga[i] = hr.altitude(p.astype(ct), zz[0], zz[1]).imag / h
    for i in (2, 9):
        pp = p.astype(ct)
        pp[i] += 1j * h
        direct[i] = hr.altitude(pp, ct(z[0]), ct(z[1])).imag / h
    return ga, direct


def law_arrays(K, sigma, sigma_u, gain_u, gain_t, smax, ff_u, ff_t, sigma_nav, dtype):
    """The law and the sigmas as the recursions take them, absent parts as zeros: -> (Ku (K, 7), fu (K,), stretch: whether step K
    stretches the cutoff, kt (7,), ft, su2 (K,) = sigma_u^2, var (32,): the variances of the 32 constants).  Without gain_u there
    is no law at all: no feed-forward and no stretch either."""
    f = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
    Ku = np.zeros((K, 7), dtype=dtype) if gain_u is None else f(gain_u)
    fu = np.zeros(K, dtype=dtype) if ff_u is None or gain_u is None else f(ff_u)
    stretch = gain_u is not None and gain_t is not None and smax > 0
    kt = f(gain_t) if stretch else np.zeros(7, dtype=dtype)
    ft = dtype(ff_t) if stretch and ff_t is not None else dtype(0)
    su2 = np.zeros(K, dtype=dtype) if sigma_u is None else f(sigma_u) ** 2
    var = np.concatenate([f(sigma), np.zeros(8, dtype=dtype) if sigma_nav is None else f(sigma_nav)]) ** 2
    return Ku, fu, stretch, kt, ft, su2, var


def corridor(p16, blob, nt, sigma, sigma_u=None, gain_u=None, gain_t=None, smax=0.0, ff_u=None, ff_t=None, know=None, sigma_nav=None,
             formulation=0, substeps=0, dtype=np.float64, rec=None):
    """-> dict(S (K, 10, 32) d y_j / d c, cov (K, 10, 10), noise (K, 10, 10) the part N_j of cov, Q (K + 1, 7, 7), nominal (K, 10),
    rec): every node 1 .. K (row j - 1 is node j).  sigma (24,), sigma_u (K,) or None, gain_u (K, 7) or None for the open loop,
    gain_t (7,), smax, ff_u (K,), ff_t, know (16,), sigma_nav (8,) or None, as history_reference.history takes them."""
    if rec is None:
        rec = gr.records(p16, blob, nt, formulation, substeps, dtype)
    K = nt - 1
    Ku, fu, stretch, kt, ft, su2, var = law_arrays(K, sigma, sigma_u, gain_u, gain_t, smax, ff_u, ff_t, sigma_nav, dtype)
    th = np.zeros(NC, dtype=dtype)                        # theta-hat = w . dp + e
    if know is not None:
        th[C_P:C_TF] = np.asarray(know, dtype=np.float64).astype(dtype)
    th[C_E] = 1
    N = np.zeros((7, NC), dtype=dtype)                    # the knowledge bias as the feedback sees it
    N[np.arange(7), C_NU + np.arange(7)] = 1
    D = np.zeros((7, NC), dtype=dtype)
    D[np.arange(7), C_Z0 + np.arange(7)] = 1
    Q = np.zeros((7, 7), dtype=dtype)
    S, cov, noise, Qs = np.zeros((K, NQ, NC), dtype=dtype), np.zeros((K, NQ, NQ), dtype=dtype), np.zeros((K, NQ, NQ), dtype=dtype), [Q]
    nominal = np.zeros((K, NQ), dtype=dtype)
    with np.errstate(all="ignore"):
        for k in range(1, K + 1):
            Phi, g = rec["Phi"][k - 1], rec["g"][k - 1]
            corr = Ku[k - 1] @ (D + N) + fu[k - 1] * th
            A = Phi - np.outer(g, Ku[k - 1])
            Dn = Phi @ D - np.outer(g, corr)
            Dn[:, C_P:C_TF] += rec["dp"][k - 1]
            Dn[:, C_TF] += rec["dtf"][k - 1]
            if k == K and stretch:
                tau = -(kt @ (D + N)) - ft * th
                Dn = Dn + np.outer(rec["gamma"], tau)
                A = A - np.outer(rec["gamma"], kt)
            z = rec["nodes"][k]
            ga, direct = altitude_gradient(p16, z, dtype)
            y = np.zeros((NQ, NC), dtype=dtype)
            y[:7] = Dn
            y[7] = ga @ Dn
            y[7, C_P:C_TF] += direct
            y[8], y[9] = -corr, corr
            Y = np.concatenate([A, (ga @ A)[None], -Ku[k - 1][None], Ku[k - 1][None]])      # d y_k / d dz_{k-1}
            ye = np.concatenate([g, [ga @ g, 1, 0]]).astype(dtype)                          # d y_k / d eps_k
            n = Y @ Q @ Y.T + su2[k - 1] * np.outer(ye, ye)
            noise[k - 1] = (n + n.T) / 2
            S[k - 1] = y
            c = (y * var) @ y.T
            cov[k - 1] = (c + c.T) / 2 + noise[k - 1]
            Q = A @ Q @ A.T + su2[k - 1] * np.outer(g, g)
            Q = (Q + Q.T) / 2
            Qs.append(Q)
            D = Dn
            p = np.asarray(p16, dtype=np.float64).astype(dtype)
            nominal[k - 1, :7] = z
            nominal[k - 1, 7], nominal[k - 1, 8] = hr.altitude(p, z[0], z[1]), rec["us"][k - 1]
    return dict(S=S, cov=cov, noise=noise, Q=np.array(Qs), nominal=nominal, rec=rec)


def row_scales(p16, gain_u, ff_u, K):
    """(K, 10): the scale of each quantity at each node in the tests' bounds -- 1 (scaled units) for the state, r_peri for the
    altitude, max(1, |K_j|_1 + |f_j|) for the control and the correction"""
    s = np.ones((K, NQ))
    s[:, 7] = p16[9]
    k1 = np.zeros(K) if gain_u is None else np.abs(np.asarray(gain_u, dtype=np.float64)).sum(axis=1)
    if ff_u is not None and gain_u is not None:
        k1 = k1 + np.abs(np.asarray(ff_u, dtype=np.float64))
    s[:, 8:] = np.maximum(1.0, k1)[:, None]
    return s
