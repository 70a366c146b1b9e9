"""TEST INFRASTRUCTURE ONLY -- the Newton step of the barrier problem for every terminal mode (ascent_opts.terminal 0 / 1 / 2)
from a generic sparse LU of the full KKT matrix (numpy / scipy, no device): conftest.generic_lu_newton_step with the terminal
block of oracle/ascent_general.py::GeneralNLP, whose hand-written terminal Jacobian and Hessian tests/test_general_oracle.py
checks against central differences.  Nothing here is stage-structured: no Riccati recursion, no border elimination, no unit
pivot -- with terminal "ellipse" the r.v = 0 row and its multiplier simply do not exist.

Besides the step it reports what a comparison with it may rest on: the inertia of the KKT matrix by eigenvalue count, and the
reference's own float64 error (one step of iterative refinement, residual in numpy.longdouble)."""
import functools

import numpy as np

# ascent_opts.terminal (include/ascent.h) -> GeneralNLP(terminal=...): the one place where the two namings meet
TERMINAL_NAMES = {0: "reference", 1: "periapsis", 2: "ellipse"}


def sections(K):
    """The four sections of a blob the step tests compare separately: states and controls | defect multipliers | bound
    multipliers | the ten scalars (t_f and its two bound multipliers, s1 s2, z_s1 z_s2, nu3 nu1 nu2)."""
    return (0, 8 * K), (8 * K, 15 * K), (15 * K, 21 * K), (21 * K, 21 * K + 10)


@functools.lru_cache(maxsize=None)
def _general_nlp(prow, K, scheme, terminal, dcost):
    """One GeneralNLP per (problem, grid, scheme, terminal mode, weight): the sympy-generated step functions behind it are
    built once per scheme (seconds for Hermite-Simpson), the object itself costs milliseconds."""
    from oracle.ascent_general import GeneralNLP
    from oracle.ascent_numpy import Params
    from oracle.c_oracle import PARAM_FIELDS
    P = Params(**dict(zip(PARAM_FIELDS, prow)))
    return GeneralNLP(P, ((K, "burn"),), scheme, dcost=dcost, terminal=TERMINAL_NAMES[terminal])


def _nlp_of(P, K, scheme, terminal, move_penalty):
    from oracle.c_oracle import pack_params
    if terminal == 0 and scheme < 2 and not move_penalty:      # conftest.generic_lu_newton_step's own choice for these: the
        from oracle.ascent_numpy import AscentNLP              # hand-written numpy oracle (same variable layout)
        return AscentNLP(P, K + 1, 0, scheme=scheme)
    return _general_nlp(tuple(float(x) for x in pack_params(P)), K, scheme, terminal, float(P.dcost) if move_penalty else 0.0)


class _System:
    """The KKT system of one call: matrix (sparse), right-hand side, the NLP and what maps a solution back into the blob layout"""


def _system(P, nt, blob, mu, dw, scheme, terminal, move_penalty, without_terminal_hessian):
    import scipy.sparse as sp
    K = nt - 1
    nlp = _nlp_of(P, K, scheme, terminal, move_penalty)
    two_rows = TERMINAL_NAMES[terminal] == "ellipse"
    v = np.zeros(nlp.n); lam = np.zeros(nlp.m); zL = np.zeros(nlp.n); zU = np.zeros(nlp.n)
    Wk = v[:8 * K].reshape(K, 8)
    Wk[:, :7] = blob[:7 * K].reshape(K, 7); Wk[:, 7] = blob[7 * K:8 * K]
    lam[:7 * K] = blob[8 * K:15 * K]
    zb = blob[15 * K:21 * K].reshape(K, 6); sc = blob[21 * K:]
    base = np.arange(K) * 8
    zL[base + 4], zU[base + 4], zL[base + 6], zU[base + 6], zL[base + 7], zU[base + 7] = zb.T
    v[nlp.itf], zL[nlp.itf], zU[nlp.itf] = sc[0], sc[1], sc[2]
    v[nlp.is1], v[nlp.is2], zL[nlp.is1], zL[nlp.is2] = sc[3], sc[4], sc[5], sc[6]
    if two_rows:
        lam[-2], lam[-1] = sc[8], sc[9]
    else:
        lam[-3], lam[-2], lam[-1] = sc[7], sc[8], sc[9]
    if move_penalty:
        du_ = np.diff(np.concatenate([[0.0], blob[7 * K:8 * K]]))
        v[nlp.ip], v[nlp.in_] = np.maximum(du_, 0.0) + 1e-4, np.maximum(-du_, 0.0) + 1e-4
        zL[nlp.ip] = zL[nlp.in_] = P.dcost
        lam[nlp.rmove] = 0.0
    hasL, hasU = np.isfinite(nlp.lb), np.isfinite(nlp.ub)
    dL = np.where(hasL, v - nlp.lb, 1.0); dU = np.where(hasU, nlp.ub - v, 1.0)
    c = nlp.constraints(v)
    lamW = lam
    if without_terminal_hessian:
        lamW = lam.copy()
        lamW[-(2 if two_rows else 3):] = 0.0
    J = nlp.jacobian(v); W = nlp.hessian(v, lamW)
    Sig = np.where(hasL, zL / dL, 0) + np.where(hasU, zU / dU, 0)
    gphi = nlp.grad_objective(v) - np.where(hasL, mu / dL, 0) + np.where(hasU, mu / dU, 0)
    Kmat = sp.bmat([[W + sp.diags(Sig + dw), J.T], [J, None]], format="csc")
    rhs = -np.concatenate([gphi + J.T @ lam, c])
    y = _System()
    y.Kmat, y.rhs, y.nlp, y.K, y.two_rows = Kmat, rhs, nlp, K, two_rows
    y.hasL, y.hasU, y.dL, y.dU, y.zL, y.zU, y.base = hasL, hasU, dL, dU, zL, zU, base
    return y


def lu_newton_step(P, nt, blob, mu, dw, scheme, terminal, move_penalty=False, without_terminal_hessian=False):
    """(step, inertia_ok, ref_err) at a primal-dual iterate in the blob layout of include/ascent.h.

    step: the Newton step of the barrier problem, same layout; the blob mapping and the warm-start rule of the slack pairs
      (move_penalty) are conftest.generic_lu_newton_step's.  terminal 2 has two terminal rows: nu3 has no row, lam[-2], lam[-1]
      = nu1, nu2, and the step carries d nu3 = 0 in row 21K+7 -- what the kernels' unit pivot must leave there.
    inertia_ok: the dense KKT matrix has n positive and m negative eigenvalues (numpy.linalg.eigvalsh; no stage structure).
    ref_err: per section of sections(K), the size of the correction one step of iterative refinement makes to `step`, the
      residual of the linear system formed in numpy.longdouble: this reference's own rounding error for this system.
    without_terminal_hessian: a deliberately wrong step -- the terminal constraints' contribution left out of the Lagrangian
      Hessian, everything else as it is --, only there to show that a comparison with `step` would notice such a kernel."""
    import scipy.sparse.linalg as spla
    y = _system(P, nt, blob, mu, dw, scheme, terminal, move_penalty, without_terminal_hessian)
    Kmat, rhs, nlp, K, two_rows = y.Kmat, y.rhs, y.nlp, y.K, y.two_rows
    hasL, hasU, dL, dU, zL, zU, base = y.hasL, y.hasU, y.dL, y.dU, y.zL, y.zU, y.base
    lu = spla.splu(Kmat)
    sol = lu.solve(rhs)

    def to_blob(s, homogeneous):
        """The solution of the linear system (or a correction to it: homogeneous) in the blob layout"""
        dx, dlam = s[:nlp.n], s[nlp.n:]
        if homogeneous:
            dzL = np.where(hasL, -zL / dL * dx, 0); dzU = np.where(hasU, zU / dU * dx, 0)
        else:
            dzL = np.where(hasL, mu / dL - zL - zL / dL * dx, 0)
            dzU = np.where(hasU, mu / dU - zU + zU / dU * dx, 0)
        step = np.zeros_like(blob)
        dW = dx[:8 * K].reshape(K, 8)
        step[:7 * K] = dW[:, :7].ravel(); step[7 * K:8 * K] = dW[:, 7]
        step[8 * K:15 * K] = dlam[:7 * K]
        step[15 * K:21 * K] = np.stack([dzL[base + 4], dzU[base + 4], dzL[base + 6], dzU[base + 6], dzL[base + 7], dzU[base + 7]], 1).ravel()
        step[21 * K:] = [dx[nlp.itf], dzL[nlp.itf], dzU[nlp.itf], dx[nlp.is1], dx[nlp.is2], dzL[nlp.is1], dzL[nlp.is2],
                         0.0 if two_rows else dlam[-3], dlam[-2], dlam[-1]]
        return step

    step = to_blob(sol, False)
    Kd = Kmat.toarray()
    ev = np.linalg.eigvalsh(Kd)
    inertia_ok = bool((ev > 0).sum() == nlp.n and (ev < 0).sum() == nlp.m)
    resid = rhs.astype(np.longdouble) - Kd.astype(np.longdouble) @ sol.astype(np.longdouble)
    corr = to_blob(lu.solve(np.asarray(resid, dtype=np.float64)), True)
    ref_err = np.array([np.abs(corr[lo:hi]).max() for lo, hi in sections(K)])
    return step, inertia_ok, ref_err


def stagewise_inertia_ok(P, nt, blob, mu, dw, scheme, terminal, move_penalty=False):
    """What a stage-wise factorisation with a (t_f, nu3) border can certify -- the C oracle's and every kernel's inertia test: all
    pivots of the recursion over the nodes positive AND the border's 2 x 2 Schur complement indefinite.  That is the right inertia of
    the KKT matrix WITHOUT the t_f column and the nu3 row (n - 1 positive, m - 1 negative eigenvalues; terminal 2, which has no nu3
    row: n - 1, m) and of the whole matrix: sufficient for the inertia lu_newton_step reports, not necessary -- an inner block with
    one negative direction and a positive definite Schur complement has the right total too, and the recursions refuse it."""
    y = _system(P, nt, blob, mu, dw, scheme, terminal, move_penalty, False)
    n, m = y.nlp.n, y.nlp.m
    Kd = y.Kmat.toarray()
    drop = [y.nlp.itf] + ([] if y.two_rows else [n + m - 3])
    keep = np.setdiff1d(np.arange(n + m), drop)
    ev, evi = np.linalg.eigvalsh(Kd), np.linalg.eigvalsh(Kd[np.ix_(keep, keep)])
    return bool((ev > 0).sum() == n and (ev < 0).sum() == m and (evi > 0).sum() == n - 1 and (evi < 0).sum() == m - len(drop) + 1)
