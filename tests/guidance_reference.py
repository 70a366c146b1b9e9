"""CPU reference of the closed-loop guidance (include/ascent.h: ascent_guidance_gains, ascent_disperse_guided_batch) for one
problem.

Step records by the complex step on flight_jacobian_reference.step -- Phi_k = dz_k/dz_{k-1}, g_k = dz_k/du_k, the derivative
with respect to the 16 SI fields and the scaled t_f -- about the reference's own nominal flight; the Riccati recursion of the
header in dense numpy; the closed-loop Jacobian as the product of the closed-loop step maps; and the closed-loop flight as a
loop of its own over flight_reference.rhs.  Nothing here comes from the kernels.  `dtype` switches the whole computation
(nominal flight, records, recursion; the closed-loop flight) between float64 and numpy's longdouble: the difference of the two
runs measures what double precision loses on the case at hand, and the GPU tests derive their bounds from it.

The closed-loop flight is written once, in fly, for the four sample drivers: disperse_guided here,
feedforward_reference.disperse_navigated, history_reference.history and navdrift_reference.history_drifting all go through
fly_samples and differ in the beliefs they form and the statistics they take.  Where the tests find two of them equal bit for
bit (guided against navigated end rows, frozen drifting channels against the history) they pin that plumbing and nothing
else: it is one law flown twice.  The independent evidence for the law is dispersion_reference.fly_rows, an open-loop flight
built directly on flight_reference that shares nothing with fly; the two "...agrees_with_the_closed_loop_jacobian_to_second_order"
tests; and the central differences of the flight in test_lincov_reference (test_jacobian_is_the_central_difference_of_the_flight)
and test_navdrift_reference (test_impulse_response_is_the_central_difference_of_the_flight), which judge it against the
linearisations derived from the step records.
"""
from __future__ import annotations

import collections
import math

import numpy as np

import dispersion_reference as dr
import flight_jacobian_reference as jr
import flight_reference as fr

H = 1e-30
GUIDE_ROWS = 5
NQ = 10                        # quantities per node: the state, the altitude, the executed control, the correction
NREC = 7 + 16 + 1 + 1          # perturbed copies of a step: z_{k-1} (7), the 16 fields, t_f, u_k


def _complex(dtype):
    return np.clongdouble if dtype is np.longdouble else np.complex128


def records(p16, blob, nt, formulation=0, substeps=0, dtype=np.float64):
    """-> dict(nodes (K + 1, 7) the nominal flight, node 0 first; Phi (K, 7, 7); g (K, 7); dp (K, 7, 16) per SI unit; dtf (K, 7)
    per scaled t_f; gamma (7,) = dt dz_K/d dt; end_z (9, 7), end_p (9, 16): the derivative of the nine end quantities with
    respect to z_K and, directly, to the fields; us, tf, m)"""
    ct = _complex(dtype)
    p16 = np.asarray(p16, dtype=np.float64)
    K = nt - 1
    _, us, tf = fr.blob_parts(np.asarray(blob, dtype=np.float64), nt)
    m = fr.substeps_of((tf * p16[11]) / K, substeps)
    pn = p16.astype(dtype)
    with np.errstate(all="ignore"):
        z = np.zeros((7, 1), dtype=dtype)
        nodes = [z[:, 0]]
        dt = (dtype(tf) * pn[11]) / K
        for k in range(K):
            z = jr.step(pn[:, None], z, np.array([us[k]], dtype=dtype), dt, m, formulation)
            nodes.append(z[:, 0])
        nodes = np.array(nodes)
        # every step at once: K blocks of NREC perturbed copies
        n = K * NREC
        p = np.repeat(pn[:, None], n, axis=1).astype(ct)
        z0 = np.repeat(nodes[:K].T, NREC, axis=1).astype(ct)
        u = np.repeat(us.astype(dtype), NREC).astype(ct)
        t = np.full(n, tf, dtype=ct)
        base = np.arange(K) * NREC
        for i in range(7):
            z0[i, base + i] += 1j * H
        for i in range(16):
            p[i, base + 7 + i] += 1j * H
        t[base + 23] += 1j * H
        u[base + 24] += 1j * H
        out = jr.step(p, z0, u, (t * p[11]) / K, m, formulation)
        d = (out.imag / dtype(H)).reshape(7, K, NREC).transpose(1, 0, 2)          # (K, 7, NREC)
        # the nine end quantities at z_K: identity and the apsides by complex step
        pe = np.repeat(pn[:, None], 23, axis=1).astype(ct)
        ze = np.repeat(nodes[K][:, None], 23, axis=1).astype(ct)
        for i in range(7):
            ze[i, i] += 1j * H
        for i in range(16):
            pe[i, 7 + i] += 1j * H
        peri, apo = jr.apsides(pe, ze)
        da = np.stack([peri.imag, apo.imag]) / dtype(H)
        end = np.zeros((9, 23), dtype=dtype)
        end[:7, :7] = np.eye(7, dtype=dtype)
        end[7:] = da
    Phi, g, dp, dtf = d[:, :, :7], d[:, :, 24], d[:, :, 7:23], d[:, :, 23]
    gamma = dtf[K - 1] * dtype(tf)          # dt dz/d dt = t_f dz/d t_f on the last step (dt is linear in t_f)
    return dict(nodes=nodes, Phi=Phi, g=g, dp=dp, dtf=dtf, gamma=gamma, end_z=end[:, :7], end_p=end[:, 7:], us=us, tf=tf, m=m,
                end=np.concatenate([nodes[K], [peri[0].real, apo[0].real]]))


def cond_grad(p16, zK, dtype=np.float64):
    """gradients c_i (3, 7) of the trim's conditions e3, g1, g2 at a scaled state"""
    p = np.asarray(p16, dtype=np.float64).astype(dtype)
    x, y, vx, vy = zK[:4]
    et = y + p[2] / p[9]
    rho = np.sqrt(x * x + et * et)
    c = np.zeros((3, 7), dtype=dtype)
    c[0, :4] = [vx, vy, x, et]
    c[1, :2] = [x / rho, et / rho]
    c[2, 2:4] = [2 * vx, 2 * vy]
    return c


def gains(rec, p16, weights, dtype=np.float64):
    """The recursion of include/ascent.h on records of the same dtype.  weights (6,): q_e3, q_g1, q_g2, r_u, r_t, stretch_max.
    -> dict(gain_u (K, 7), gain_t (7,), summary (5,), P (K + 1, 7, 7) with P[k] the value matrix at node k, S list)"""
    w = np.asarray(weights, dtype=np.float64)
    K = len(rec["us"])
    nfree = float((np.abs(rec["us"]) < 0.999).sum())
    nan = dict(gain_u=np.full((K, 7), np.nan), gain_t=np.full(7, np.nan), summary=np.array([2.0, nfree, np.nan, np.nan, float(rec["m"])]),
               P=None)
    if not (np.all(np.isfinite(w)) and np.all(w[:3] >= 0) and w[3] > 0 and w[4] > 0 and w[5] >= 0):
        return nan
    q, ru, rt, smax = w[:3].astype(dtype), dtype(w[3]), dtype(w[4]), w[5]
    c = cond_grad(p16, rec["nodes"][K], dtype)
    P = np.zeros((7, 7), dtype=dtype)
    for i in range(3):
        P = P + q[i] * np.outer(c[i], c[i])
    Ps = [None] * (K + 1)
    Ps[K] = P
    gu, gt = np.zeros((K, 7), dtype=dtype), np.zeros(7, dtype=dtype)
    with np.errstate(all="ignore"):
        for k in range(K, 0, -1):
            Phi = rec["Phi"][k - 1]
            cols, R = [], []
            f1, f2 = bool(abs(rec["us"][k - 1]) < 0.999), bool(k == K and smax > 0)
            if f1:
                cols.append(rec["g"][k - 1]); R.append(ru)
            if f2:
                cols.append(rec["gamma"]); R.append(rt)
            Pn = Phi.T @ (P @ Phi)
            if cols:
                Bm = np.stack(cols, axis=1)
                PB = P @ Bm
                S = np.diag(np.array(R, dtype=dtype)) + Bm.T @ PB
                h = PB.T @ Phi
                if not np.all(np.isfinite(S.astype(np.float64))) or not np.all(np.diag(S) > 0):
                    return nan
                if len(cols) == 2:
                    det = S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]
                    if not det > 0:
                        return nan
                    G = np.stack([(S[1, 1] * h[0] - S[0, 1] * h[1]) / det, (S[0, 0] * h[1] - S[0, 1] * h[0]) / det])
                else:
                    G = h / S[0, 0]
                Pn = Pn - G.T @ S @ G
                if f1:
                    gu[k - 1] = G[0]
                if f2:
                    gt = G[-1]
            P = 0.5 * (Pn + Pn.T)
            Ps[k - 1] = P
    summary = np.array([0.0, nfree, float(np.abs(gu).max()), float(np.abs(gt).max()), float(rec["m"])])
    return dict(gain_u=gu, gain_t=gt, summary=summary, P=Ps)


def closed_loop_jacobian(rec, gain_u, gain_t, p16, formulation=0):
    """-> dict(jac (9, 24), jac_u (9, K)) in the conventions of flight_jacobian_reference.jacobian: Lambda_K = d end / d z_K,
    Lambda_{k-1} = Lambda_k (Phi_k - g_k K_k' - [k = K] gamma k_t'); columns: Lambda_0 | sum_k Lambda_k dz_k/dp + the direct
    dependence of the apsides | sum_k Lambda_k dz_k/dt_f; jac_u column k-1: Lambda_k g_k (the execution error of step k)"""
    K = len(rec["us"])
    dtype = rec["Phi"].dtype.type
    L = rec["end_z"].copy()
    jac = np.zeros((9, 24), dtype=dtype)
    jac_u = np.zeros((9, K), dtype=dtype)
    jac[:, 7:23] = rec["end_p"]
    with np.errstate(all="ignore"):
        for k in range(K, 0, -1):
            jac_u[:, k - 1] = L @ rec["g"][k - 1]
            jac[:, 7:23] += L @ rec["dp"][k - 1]
            jac[:, 23] += L @ rec["dtf"][k - 1]
            A = rec["Phi"][k - 1] - np.outer(rec["g"][k - 1], gain_u[k - 1])
            if k == K:
                A = A - np.outer(rec["gamma"], gain_t)
            L = L @ A
    jac[:, :7] = L
    if not jr._energy(np.asarray(p16, dtype=np.float64), np.asarray(rec["end"], dtype=np.float64)) < 0.0:
        jac[8], jac_u[8] = np.nan, np.nan
    zero_cols = [7 + 10, 7 + 13, 7 + 14, 7 + 15, 7 + (8 if formulation == 1 else 12)]
    jac[:, zero_cols] = 0.0
    return dict(jac=jac, jac_u=jac_u)


def _rhs(dtype):
    if dtype is np.float64:
        return fr.rhs
    return lambda p, z, u, formulation: jr.rhs(np.asarray(p, dtype=dtype), z, dtype(u), formulation)


def altitude(p, x, y):
    """metres above R0 of a scaled position, the radius relation of flight_reference.apsides: p[9] = r_peri, p[2] = R0"""
    X, Y = x * p[9], y * p[9] + p[2]
    return np.sqrt(X * X + Y * Y) - p[2]


# What one flight leaves behind: hist (K, 10) of dtype, row k - 1 the ten quantities of node k (NaN from the step that failed on);
# clipped (K,) bool and margin (K,), the distance of the step's command from the clip (inf where the step has neither gain nor
# feed-forward); corr (K,), the correction of every step that was begun (hist[:, 9] holds it only for the steps that ended);
# stretch, the applied cutoff stretch; p, the fields as the flight read them; error, the exception of math.* that ended it, or None.
Flight = collections.namedtuple("Flight", "hist clipped margin corr stretch p error")


def fly(p, z0, us, noise, tf, m, nodes, gain_u=None, gain_t=None, smax=0.0, ff_u=None, ff_t=None, theta_hat=0.0, nu=None, nu_on=None,
        formulation=0, dtype=np.float64):
    """One closed-loop flight, the command law of include/ascent.h: p the sample's 16 fields, z0 (7,), us (K,) the nominal controls,
    noise (K,) the execution errors (sigma_u xi), tf the sample's scaled t_f, m held, nodes (K + 1, 7) the nominal flight the
    feedback refers to (None: there is no law), gain_u (K, 7) or None for the open loop, gain_t (7,) or None, smax, ff_u (K,) or
    None, ff_t or None, theta_hat a scalar or (K,), nu (7,) or (K, 7) and nu_on (7,) bool: where the bias is applied; row k - 1 of a
    per-step theta_hat or nu is what step k steers on (the cutoff stretch of step K uses row K - 1 as well).  -> Flight"""
    rhs = _rhs(dtype)
    p = [float(v) for v in p] if dtype is np.float64 else np.asarray(p, dtype=np.float64).astype(dtype)
    K = len(us)
    z = np.array(z0, dtype=dtype)
    theta_hat = 0.0 if theta_hat is None else theta_hat
    hist, clipped, margin = np.full((K, NQ), np.nan, dtype=dtype), np.zeros(K, dtype=bool), np.full(K, math.inf)
    corrs, stretch, error = np.zeros(K, dtype=dtype), 0.0, None
    with np.errstate(all="ignore"):
        dt = (dtype(tf) * p[11]) / K
        try:
            for k in range(K):
                th = dtype(theta_hat if np.ndim(theta_hat) == 0 else theta_hat[k])
                if nodes is not None:
                    dz = z - np.asarray(nodes[k], dtype=dtype)
                if nu_on is not None:
                    nuk = nu if np.ndim(nu) == 1 else nu[k]
                    for i in range(7):
                        if nu_on[i]:
                            dz[i] = dz[i] + dtype(nuk[i])
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
                    corr = corrs[k] = dot
                u = uc + dtype(noise[k]) if noise[k] != 0 else uc
                h = dt / m
                if k == K - 1 and gain_t is not None and smax > 0:
                    dtau = dtype(0)
                    for i in range(7):
                        dtau = dtau - dtype(gain_t[i]) * dz[i]
                    if ff_t is not None and ff_t != 0:
                        dtau = dtau - dtype(ff_t) * th
                    st = min(dtype(smax), max(dtype(-smax), dtau)) if math.isfinite(dtau) else dtype(np.nan)
                    stretch = float(st)
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
        except (ValueError, ZeroDivisionError, OverflowError) as e:       # math.* on a non-finite state: the rest stays NaN
            error = e
    return Flight(hist, clipped, margin, corrs, stretch, p, error)


def end_rows(f):
    """(9,): the flown end state and its apsides -- flight_reference.apsides in float64, flight_jacobian_reference.apsides in
    longdouble --, NaN where math.* gave up in the flight or here"""
    dtype = f.hist.dtype.type
    z = f.hist[-1, :7]
    if f.error is not None:
        return np.full(9, np.nan)
    with np.errstate(all="ignore"):
        try:
            if dtype is np.float64:
                peri, apo = fr.apsides(f.p, *z[:4])
            else:
                pa, aa = jr.apsides(f.p[:, None], z[:, None])
                peri, apo = pa[0], (aa[0] if np.isfinite(aa[0]) else np.inf)
        except (ValueError, ZeroDivisionError, OverflowError):
            return np.full(9, np.nan)
    return np.concatenate([z, [peri, apo]]).astype(dtype)


def effort(f):
    """(4,): clipped steps, max |K . dz + f theta-hat| (NaN once a correction is NaN), stretch, and -- the reference's own -- the
    smallest distance of a command from the clip, | |u_k - K . dz - f theta-hat| - 1 | (0 for a command that is not finite, inf
    where no row steers); of a flight that math.* ended, what had accumulated when it did"""
    with np.errstate(all="ignore"):
        c = np.abs(f.corr.astype(np.float64))
    return np.array([float(np.count_nonzero(f.clipped)), math.nan if np.isnan(c).any() else c.max(), f.stretch, f.margin.min()])


def _nominal(p16, us, tf, m, formulation, dtype):
    """the nominal flight: zero start, no law, no noise; an exception of math.* is passed on"""
    f = fly(p16, np.zeros(7), us, np.zeros(len(us)), tf, m, None, formulation=formulation, dtype=dtype)
    if f.error is not None:
        raise f.error
    return f


def nominal_nodes(p16, us, tf, m, formulation=0, dtype=np.float64):
    """(K + 1, 7): the states of the nominal flight at the nodes 0 .. K"""
    return np.concatenate([np.zeros((1, 7), dtype=dtype), _nominal(p16, us, tf, m, formulation, dtype).hist[:, :7]])


def fly_samples(p16, blob, nt, xi, sigma, sigma_u, law, theta_hat=None, nu=None, nu_on=None, formulation=0, substeps=0,
                dtype=np.float64, finite_tf=False):
    """What the four sample drivers share: the blob's parts and the held m, the nominal flight and its nodes, the execution errors
    sigma_u xi, and one flight per sample of dispersion_reference.perturbed under law = (gain_u, gain_t, smax, ff_u, ff_t),
    steering on theta_hat[s] and nu[s] where nu_on.  -> (m, nodes, nominal, flights): Flights, None for a sample
    whose t_f is not finite; finite_tf: nodes, nominal and flights are None where the blob's own t_f is not finite."""
    p16 = np.asarray(p16, dtype=np.float64)
    K = nt - 1
    _, us, tf = fr.blob_parts(np.asarray(blob, dtype=np.float64), nt)
    xi, sigma = np.asarray(xi, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    m = fr.substeps_of((tf * p16[11]) / K, substeps)
    S = xi.shape[1]
    if finite_tf and not math.isfinite(tf):
        return m, None, None, None
    nominal = _nominal(p16, us, tf, m, formulation, dtype)
    nodes = np.concatenate([np.zeros((1, 7), dtype=dtype), nominal.hist[:, :7]])
    theta_hat = np.zeros(S) if theta_hat is None else theta_hat
    nu = np.zeros((S, 7)) if nu is None else nu
    noise = np.zeros((K, S))          # the execution errors sigma_u xi, applied where sigma_u is non-zero
    if sigma_u is not None:
        su = np.asarray(sigma_u, dtype=np.float64)
        noise[su != 0.0] = su[su != 0.0, None] * xi[dr.NCOL:dr.NCOL + K][su != 0.0]
    flights = []
    for s in range(S):
        p, z0, _, t = dr.perturbed(p16, us, tf, xi, sigma, None, s)
        flights.append(fly(p, z0, us, noise[:, s], t, m, nodes, *law, theta_hat[s], nu[s], nu_on,
                           formulation, dtype) if math.isfinite(t) else None)
    return m, nodes, nominal, flights


def dispersion_result(m, nodes, nominal, flights, dtype):
    """the dict of disperse_guided and feedforward_reference.disperse_navigated from fly_samples' flights"""
    rows, eff = np.full((len(flights), 9), np.nan, dtype=dtype), np.full((len(flights), 4), np.nan)
    for s, f in enumerate(flights):
        if f is not None:
            rows[s], eff[s] = end_rows(f), effort(f)
    nominal = end_rows(nominal)
    return dict(samples=rows, effort=eff, stats=dr.statistics(nominal.astype(np.float64), rows.astype(np.float64)), nominal=nominal, m=m,
                nodes=nodes)


def disperse_guided(p16, blob, nt, xi, sigma, sigma_u, gain_u, gain_t=None, smax=0.0, formulation=0, substeps=0, dtype=np.float64):
    """-> dict(samples (samples, 9), effort (samples, 4), stats (82,), nominal (9,), m, nodes): one problem, arguments as
    dispersion_reference.disperse plus the feedback.  The nominal flight the feedback refers to is flown here with the same loop."""
    m, nodes, nominal, flights = fly_samples(p16, blob, nt, xi, sigma, sigma_u, (gain_u, gain_t, smax, None, None), formulation=formulation,
                                             substeps=substeps, dtype=dtype, finite_tf=True)
    if flights is None:
        rows = np.full((np.shape(xi)[1], 9), np.nan)
        return dict(samples=rows, effort=np.full((len(rows), 4), np.nan), stats=dr.statistics(np.full(9, np.nan), rows), nominal=np.full(9, np.nan), m=m)
    return dispersion_result(m, nodes, nominal, flights, dtype)


def simulate_linear(rec, gain_u, gain_t, dz0):
    """the linear closed loop dz_k = Phi_k dz_{k-1} + g_k du_k + [k = K] gamma tau under du_k = -K_k dz_{k-1}, tau = -k_t
    dz_{K-1}: -> (dz_K, du (K,), tau)"""
    K = len(rec["us"])
    dz = np.array(dz0, dtype=rec["Phi"].dtype)
    du = np.zeros(K, dtype=dz.dtype)
    tau = dz.dtype.type(0)
    for k in range(1, K + 1):
        du[k - 1] = -(gain_u[k - 1] @ dz)
        nxt = rec["Phi"][k - 1] @ dz + rec["g"][k - 1] * du[k - 1]
        if k == K:
            tau = -(gain_t @ dz)
            nxt = nxt + rec["gamma"] * tau
        dz = nxt
    return dz, du, tau


def linear_cost(rec, p16, weights, gain_u, gain_t, dz0):
    w = np.asarray(weights, dtype=np.float64)
    dzK, du, tau = simulate_linear(rec, gain_u, gain_t, dz0)
    c = cond_grad(p16, rec["nodes"][-1], rec["Phi"].dtype.type)
    return 0.5 * float(np.sum(w[:3] * (c @ dzK) ** 2)) + 0.5 * w[3] * float(du @ du) + 0.5 * w[4] * float(tau) ** 2


def rel_gap(a, b):
    """largest |a - b| over the largest |b| per row (last axis), the measure the GPU bounds use"""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    scale = np.abs(b).max(axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        r = np.abs(a - b) / np.where(scale > 0, scale, 1)
    return float(np.nanmax(r))
