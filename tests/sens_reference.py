"""CPU reference of the post-optimal sensitivity dJ*/dp = dL/dp at a fixed solution blob (include/ascent.h:
ascent_param_sensitivity), built from the oracles' constraint residuals, not from the kernel's derivatives.

The equality-constraint residuals of an oracle are differentiated with respect to each SI parameter at the fixed blob by
central differences with one Richardson extrapolation, and contracted with the blob's multipliers (defects: lambda,
terminal conditions: nu3, nu1, nu2).  The terms that the oracles carry as bounds or objective, not as residuals, are added
in closed form in the blob's sign convention (L = J + lambda'c + nu'c_T - zL'(v - lb) - zU'(ub - v)):
angle_ub: -sum zU_angle; tf_lb: +zL_tf; tf_ub: -zU_tf; move penalty: d/d dcost = w sum |u_k - u_{k-1}|;
formulation 1's algebraic angle row angle_k - (angle_ub/2)(u_k + 1): -lambda_angle (u_k + 1)/2.

Residual sources: oracle.c_oracle.constraints (schemes 0 / 1, formulation 0, terminal 0), oracle.ascent_general.GeneralNLP
(Hermite-Simpson, terminals 1 / 2), oracle.ascent_numpy.AscentNLP (formulation 1).
"""
from __future__ import annotations

import numpy as np

from oracle import c_oracle
from oracle.ascent_general import GeneralNLP
from oracle.ascent_numpy import AscentNLP, Params

FIELDS = c_oracle.PARAM_FIELDS
IA = 4
TERMINAL_NAMES = {0: "reference", 1: "periapsis", 2: "ellipse"}


def _blob_parts(blob, nt):
    K = nt - 1
    z = blob[:7 * K].reshape(K, 7)
    u = blob[7 * K:8 * K]
    lam = blob[8 * K:15 * K].reshape(K, 7)
    zb = blob[15 * K:21 * K].reshape(K, 6)
    sc = blob[21 * K:]
    return z, u, lam, zb, sc


def _residual_fn(nt, blob, scheme, formulation, terminal):
    """-> (f(params16) -> residual vector, multiplier vector of the same length, rows per node of the defect part)"""
    K = nt - 1
    z, u, lam, zb, sc = _blob_parts(blob, nt)
    nu3, nu1, nu2 = sc[7], sc[8], sc[9]
    if formulation == 1:
        keep = [0, 1, 2, 3, 6]                                   # x y xdot ydot mass: AscentNLP's v1 states
        v = np.concatenate([np.hstack([z[:, keep], z[:, IA:IA + 1]]).ravel(), [sc[0], sc[3], sc[4]]])
        mult = np.concatenate([lam[:, keep].ravel(), [nu3, nu1, nu2]])

        def f(p16):
            P = Params(**dict(zip(FIELDS, p16)))
            nlp = AscentNLP(P, nt=nt, formulation=1, scheme=0)
            if terminal == 1:
                nlp.d["vp2"] = GeneralNLP(P, phases=((K, "burn"),), terminal="periapsis").v2_t
            return nlp.constraints(v)
        return f, mult, 5
    if scheme in (0, 1) and terminal == 0:
        mult = np.concatenate([lam.ravel(), [nu3, nu1, nu2]])
        return (lambda p16: c_oracle.constraints(np.ascontiguousarray(p16), nt, blob, scheme)), mult, 7
    v = np.concatenate([np.hstack([z, u[:, None]]).ravel(), [sc[0], sc[3], sc[4]]])
    mult = np.concatenate([lam.ravel(), [nu3, nu1, nu2] if terminal != 2 else [nu1, nu2]])

    def f(p16):
        P = Params(**dict(zip(FIELDS, p16)))
        return GeneralNLP(P, phases=((K, "burn"),), scheme=scheme, dcost=0.0, terminal=TERMINAL_NAMES[terminal]).constraints(v)
    return f, mult, 7


def reference_gradient(params16, nt, blob, scheme=0, formulation=0, terminal=0, move_penalty=False, rel_step=1e-3):
    """(g, scale): g[16] = dL/dp in the units of ascent_param_sensitivity (scaled objective per SI unit); scale[16] =
    sum over every per-node and closed-form contribution of |term| (the size against which cancellation is judged)."""
    p0 = np.asarray(params16, dtype=np.float64)
    blob = np.ascontiguousarray(blob, dtype=np.float64)
    K = nt - 1
    z, u, lam, zb, sc = _blob_parts(blob, nt)
    f, mult, _ = _residual_fn(nt, blob, scheme, formulation, terminal)
    g = np.zeros(16)
    scale = np.zeros(16)
    for i in range(16):
        h = rel_step * abs(p0[i]) if p0[i] != 0.0 else rel_step

        def cd(hh):
            pp, pm = p0.copy(), p0.copy()
            pp[i] += hh
            pm[i] -= hh
            return (f(pp) - f(pm)) / (2.0 * hh)
        d = (4.0 * cd(0.5 * h) - cd(h)) / 3.0
        terms = mult * d
        g[i] = terms.sum()
        scale[i] = np.abs(terms).sum()
    closed = np.zeros(16)
    absc = np.zeros(16)
    ia, itl, itu, idc = FIELDS.index("angle_ub"), FIELDS.index("tf_lb"), FIELDS.index("tf_ub"), FIELDS.index("dcost")
    closed[ia] -= zb[:, 1].sum()
    absc[ia] += np.abs(zb[:, 1]).sum()
    if formulation == 1:
        t = -0.5 * lam[:, IA] * (u + 1.0)
        closed[ia] += t.sum()
        absc[ia] += np.abs(t).sum()
    closed[itl] += sc[1]
    closed[itu] -= sc[2]
    absc[itl] += abs(sc[1])
    absc[itu] += abs(sc[2])
    if move_penalty:
        u0 = -1.0 if formulation == 1 else 0.0
        tv = np.abs(np.diff(np.concatenate([[u0], u]))).sum()
        if formulation == 1:
            closed[idc] += 0.5 * p0[ia] * tv
            closed[ia] += 0.5 * p0[idc] * tv
            absc[ia] += 0.5 * p0[idc] * tv
        else:
            closed[idc] += tv
        absc[idc] += abs(closed[idc])
    return g + closed, scale + absc


def objective(params16, nt, blob, formulation=0, move_penalty=False):
    """J* at the blob: tf, plus the move penalty taken from the controls."""
    K = nt - 1
    J = blob[21 * K]
    if move_penalty:
        p = np.asarray(params16)
        u0 = -1.0 if formulation == 1 else 0.0
        w = p[15] * p[12] * 0.5 if formulation == 1 else p[15]
        J = J + w * np.abs(np.diff(np.concatenate([[u0], blob[7 * K:8 * K]]))).sum()
    return J
