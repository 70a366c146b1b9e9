"""CPU reference of the guidance feed-forward and the navigation errors (include/ascent.h: ascent_guidance_feedforward,
ascent_disperse_navigated_batch) for one problem.

On the records of guidance_reference.records: the augmented Riccati recursion of the header -- the value function
1/2 [dz; theta]' [[P, p], [p', pi0]] [dz; theta] --, the closed-loop Jacobian with its navigation block as the forward product
of the closed-loop step maps on the state augmented by every constant input, and the navigated flight as a loop of its own over
flight_reference.rhs.  Nothing here comes from the kernels.  `dtype` switches a computation between float64 and numpy's
longdouble, as in guidance_reference."""
from __future__ import annotations

import numpy as np

import flight_jacobian_reference as jr
import guidance_reference as gr

NAV_ROWS = 8
GUIDE_FF_ROWS = 7


def forcing(rec, direction):
    """pi_k = Gamma_k d (K, 7): the steps' derivative with respect to the 16 SI fields along d; the direct dependence of the
    apsides on the fields (rec["end_p"]) is not part of it"""
    dtype = rec["Phi"].dtype.type
    return rec["dp"] @ np.asarray(direction, dtype=np.float64).astype(dtype)


def gains(rec, p16, weights, direction, dtype=np.float64):
    """The augmented recursion on records of the same dtype.  -> dict(gain_u (K, 7), gain_t (7,), ff_u (K,), ff_t, summary (7,),
    P (K + 1, 7, 7), p (K + 1, 7), pi0 (K + 1,): the value function at node k)"""
    w = np.asarray(weights, dtype=np.float64)
    d = np.asarray(direction, dtype=np.float64)
    K = len(rec["us"])
    nfree = float((np.abs(rec["us"]) < 0.999).sum())
    nan = dict(gain_u=np.full((K, 7), np.nan), gain_t=np.full(7, np.nan), ff_u=np.full(K, np.nan), ff_t=np.nan,
               summary=np.array([2.0, nfree, np.nan, np.nan, float(rec["m"]), np.nan, np.nan]), P=None, p=None, pi0=None)
    if not (np.all(np.isfinite(w)) and np.all(w[:3] >= 0) and w[3] > 0 and w[4] > 0 and w[5] >= 0 and np.all(np.isfinite(d))):
        return nan
    q, ru, rt, smax = w[:3].astype(dtype), dtype(w[3]), dtype(w[4]), w[5]
    c = gr.cond_grad(p16, rec["nodes"][K], dtype)
    pis = forcing(rec, d)
    P = np.zeros((7, 7), dtype=dtype)
    for i in range(3):
        P = P + q[i] * np.outer(c[i], c[i])
    p, pi0 = np.zeros(7, dtype=dtype), dtype(0)
    Ps, ps, p0s = [None] * (K + 1), [None] * (K + 1), [None] * (K + 1)
    Ps[K], ps[K], p0s[K] = P, p, pi0
    gu, gt = np.zeros((K, 7), dtype=dtype), np.zeros(7, dtype=dtype)
    fu, ft = np.zeros(K, dtype=dtype), dtype(0)
    with np.errstate(all="ignore"):
        for k in range(K, 0, -1):
            Phi, pk = rec["Phi"][k - 1], pis[k - 1]
            cols, R = [], []
            f1, f2 = bool(abs(rec["us"][k - 1]) < 0.999), bool(k == K and smax > 0)
            if f1:
                cols.append(rec["g"][k - 1]); R.append(ru)
            if f2:
                cols.append(rec["gamma"]); R.append(rt)
            a = P @ pk + p
            Pn = Phi.T @ (P @ Phi)
            pn = Phi.T @ a
            p0n = pi0 + pk @ (P @ pk) + 2 * (p @ pk)
            if cols:
                Bm = np.stack(cols, axis=1)
                PB = P @ Bm
                S = np.diag(np.array(R, dtype=dtype)) + Bm.T @ PB
                h = PB.T @ Phi
                e = Bm.T @ a
                if not np.all(np.isfinite(S.astype(np.float64))) or not np.all(np.diag(S) > 0):
                    return nan
                if len(cols) == 2:
                    det = S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]
                    if not det > 0:
                        return nan
                    G = np.stack([(S[1, 1] * h[0] - S[0, 1] * h[1]) / det, (S[0, 0] * h[1] - S[0, 1] * h[0]) / det])
                    f = np.array([(S[1, 1] * e[0] - S[0, 1] * e[1]) / det, (S[0, 0] * e[1] - S[0, 1] * e[0]) / det], dtype=dtype)
                else:
                    G = h / S[0, 0]
                    f = e / S[0, 0]
                Pn = Pn - G.T @ S @ G
                pn = pn - G.T @ (S @ f)
                p0n = p0n - f @ (S @ f)
                if f1:
                    gu[k - 1], fu[k - 1] = G[0], f[0]
                if f2:
                    gt, ft = G[-1], f[-1]
            P, p, pi0 = 0.5 * (Pn + Pn.T), pn, p0n
            Ps[k - 1], ps[k - 1], p0s[k - 1] = P, p, pi0
    summary = np.array([0.0, nfree, float(np.abs(gu).max()), float(np.abs(gt).max()), float(rec["m"]), float(np.abs(fu).max()), abs(float(ft))])
    return dict(gain_u=gu, gain_t=gt, ff_u=fu, ff_t=ft, summary=summary, P=Ps, p=np.array(ps), pi0=np.array(p0s))


def closed_loop_jacobian(rec, G, know, p16, formulation=0):
    """-> dict(jac (9, 24), jac_u (9, K), jac_nav (9, 8)): the derivative of the nine end quantities of the linear closed loop
    under du_k = -K_k (dz + nu) - f_k theta-hat, tau = -k_t (dz + nu) - f_t theta-hat, theta-hat = know . dp + eps, with respect
    to dz_0 (7), dp (16 SI fields), dt_f, the execution errors e_k (K), nu (7) and eps.  Forward: X_k = d dz_k / d (every input),
    X_0 = [I | 0], X_k = A_k X_{k-1} + (the step's own dependence on the inputs), A_k the closed-loop step map."""
    K = len(rec["us"])
    dtype = rec["Phi"].dtype.type
    gu, gt, fu, ft = G["gain_u"], G["gain_t"], G["ff_u"], G["ff_t"]
    w = np.asarray(know, dtype=np.float64).astype(dtype)
    n = 7 + 16 + 1 + K + 7 + 1
    iP, iT, iE, iN, iK = 7, 23, 24, 24 + K, 24 + K + 7
    X = np.zeros((7, n), dtype=dtype)
    X[:, :7] = np.eye(7, dtype=dtype)
    with np.errstate(all="ignore"):
        for k in range(1, K + 1):
            g = rec["g"][k - 1]
            A = rec["Phi"][k - 1] - np.outer(g, gu[k - 1])
            if k == K:
                A = A - np.outer(rec["gamma"], gt)
            Xn = A @ X
            Xn[:, iP:iP + 16] += rec["dp"][k - 1] - np.outer(g * fu[k - 1], w)
            Xn[:, iT] += rec["dtf"][k - 1]
            Xn[:, iE + k - 1] += g
            Xn[:, iN:iN + 7] -= np.outer(g, gu[k - 1])
            Xn[:, iK] -= g * fu[k - 1]
            if k == K:
                Xn[:, iP:iP + 16] -= np.outer(rec["gamma"] * ft, w)
                Xn[:, iN:iN + 7] -= np.outer(rec["gamma"], gt)
                Xn[:, iK] -= rec["gamma"] * ft
            X = Xn
        full = rec["end_z"] @ X
    full[:, iP:iP + 16] += rec["end_p"]
    jac, jac_u, jac_nav = full[:, :24].copy(), full[:, iE:iE + K].copy(), full[:, iN:].copy()
    if not jr._energy(np.asarray(p16, dtype=np.float64), np.asarray(rec["end"], dtype=np.float64)) < 0.0:
        jac[8], jac_u[8], jac_nav[8] = np.nan, np.nan, np.nan
    return dict(jac=jac, jac_u=jac_u, jac_nav=jac_nav)


def beliefs(xi, sigma, know, xi_nav, sigma_nav):
    """-> (theta_hat (samples,), nu (samples, 7), nu_on (7,)) by the rules of the header: a draw counts where its sigma is non-zero"""
    xi, sigma = np.asarray(xi, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    S = xi.shape[1]
    th, nu, on = np.zeros(S), np.zeros((S, 7)), np.zeros(7, dtype=bool)
    if know is not None:
        for i in range(16):
            if sigma[7 + i] != 0:
                th = th + (know[i] * sigma[7 + i]) * xi[7 + i]
    if sigma_nav is not None:
        sn, xn = np.asarray(sigma_nav, dtype=np.float64), np.asarray(xi_nav, dtype=np.float64)
        for i in range(7):
            if sn[i] != 0:
                on[i] = True
                nu[:, i] = sn[i] * xn[i]
        if sn[7] != 0:
            th = th + sn[7] * xn[7]
    return th, nu, on


def disperse_navigated(p16, blob, nt, xi, sigma, sigma_u, gain_u, gain_t=None, smax=0.0, ff_u=None, ff_t=None, know=None, xi_nav=None,
                       sigma_nav=None, formulation=0, substeps=0, dtype=np.float64):
    """-> dict(samples (samples, 9), effort (samples, 4), stats (82,), nominal (9,), m, nodes): guidance_reference.disperse_guided
    with the feed-forward and the navigation errors of ascent_disperse_navigated_batch"""
    th, nu, on = beliefs(xi, sigma, know, xi_nav, sigma_nav)
    return gr.dispersion_result(*gr.fly_samples(p16, blob, nt, xi, sigma, sigma_u, (gain_u, gain_t, smax, ff_u, ff_t), th, nu, on, formulation,
                                                substeps, dtype), dtype)


def simulate_linear(rec, G, direction, dz0, theta, theta_hat=None, ff_u=None, ff_t=None):
    """the linear closed loop dz_k = Phi_k dz_{k-1} + g_k du_k + pi_k theta + [k = K] gamma tau under the law of the header, with
    theta_hat (None: theta itself) and, optionally, other feed-forward gains than G's: -> (dz_K, du (K,), tau)"""
    K = len(rec["us"])
    pis = forcing(rec, direction)
    fu = G["ff_u"] if ff_u is None else ff_u
    ft = G["ff_t"] if ff_t is None else ff_t
    th = theta if theta_hat is None else theta_hat
    dz = np.array(dz0, dtype=rec["Phi"].dtype)
    du = np.zeros(K, dtype=dz.dtype)
    tau = dz.dtype.type(0)
    for k in range(1, K + 1):
        du[k - 1] = -(G["gain_u"][k - 1] @ dz) - fu[k - 1] * th
        nxt = rec["Phi"][k - 1] @ dz + rec["g"][k - 1] * du[k - 1] + pis[k - 1] * theta
        if k == K:
            tau = -(G["gain_t"] @ dz) - ft * th
            nxt = nxt + rec["gamma"] * tau
        dz = nxt
    return dz, du, tau


def linear_cost(rec, p16, weights, G, direction, dz0, theta, theta_hat=None, ff_u=None, ff_t=None):
    w = np.asarray(weights, dtype=np.float64)
    dzK, du, tau = simulate_linear(rec, G, direction, dz0, theta, theta_hat, ff_u, ff_t)
    c = gr.cond_grad(p16, rec["nodes"][-1], rec["Phi"].dtype.type)
    return 0.5 * float(np.sum(w[:3] * (c @ dzK) ** 2)) + 0.5 * w[3] * float(du @ du) + 0.5 * w[4] * float(tau) ** 2
