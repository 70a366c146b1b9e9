"""CPU reference of the per-node Monte Carlo history (include/ascent.h: ascent_disperse_history_batch) for one problem.

The flight is guidance_reference.fly, which records, after every step, the ten quantities of the node the step ends at: the
flown state, the altitude, the executed control and the correction of the step.  The perturbations are
dispersion_reference.perturbed's, the beliefs feedforward_reference.beliefs' (with all-zero gains and no feed-forward the
flight is the open-loop one of dispersion_reference.fly_rows, bit for bit in float64).  Nothing here comes from the kernels:
the statistics are numpy's over the samples valid at the node.  `dtype` switches the flight between float64 and numpy's
longdouble, as in guidance_reference."""
from __future__ import annotations

import math

import numpy as np

import feedforward_reference as ffr
import guidance_reference as gr

NQ, ROWS = 10, 52


altitude = gr.altitude


def fly_history(p, z0, us, noise, tf, m, nodes, gain_u=None, gain_t=None, smax=0.0, ff_u=None, ff_t=None, theta_hat=0.0, nu=None,
                nu_on=None, formulation=0, dtype=np.float64):
    """One flight, the arguments of guidance_reference.fly; gain_u None: open loop.  -> (hist (K, 10) of dtype: row k - 1 is node k,
    clipped (K,) bool, margin (K,): the distance of the step's command from the clip, inf where the step has neither gain nor
    feed-forward)"""
    return gr.fly(p, z0, us, noise, tf, m, nodes, gain_u, gain_t, smax, ff_u, ff_t, theta_hat, nu, nu_on, formulation, dtype)[:3]


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


def history_result(m, nodes, nominal, flights, dtype, K):
    """the dict of history and navdrift_reference.history_drifting from guidance_reference.fly_samples' flights; nominal (K, 10)"""
    S = len(flights)
    smp, clip, marg = np.full((S, K, NQ), np.nan, dtype=dtype), np.zeros((S, K), dtype=bool), np.full((S, K), math.inf)
    for s, f in enumerate(flights):
        if f is not None:
            smp[s], clip[s], marg[s] = f.hist, f.clipped, f.margin
    nominal = np.asarray(nominal, dtype=np.float64)
    return dict(samples=smp, clipped=clip, margin=marg, nominal=nominal, stats=statistics(nominal, smp.astype(np.float64), clip), m=m,
                nodes=nodes)


def history(p16, blob, nt, xi, sigma, sigma_u=None, gain_u=None, gain_t=None, smax=0.0, ff_u=None, ff_t=None, know=None, xi_nav=None,
            sigma_nav=None, formulation=0, substeps=0, dtype=np.float64):
    """-> dict(samples (samples, K, 10), clipped (samples, K), margin (samples, K), nominal (K, 10), stats (K, 52), m, nodes):
    one problem at stride 1; arguments as feedforward_reference.disperse_navigated, gain_u None for the open-loop flight"""
    K, S = nt - 1, np.shape(xi)[1]
    th, nu, on = ffr.beliefs(xi, sigma, know, xi_nav, sigma_nav) if gain_u is not None else (None, None, None)
    m, nodes, nominal, flights = gr.fly_samples(p16, blob, nt, xi, sigma, sigma_u, (gain_u, gain_t, smax, ff_u, ff_t), th, nu, on, formulation,
                                                substeps, dtype, finite_tf=True)
    if flights is None:
        return history_result(m, None, np.full((K, NQ), np.nan), [None] * S, dtype, K)
    return history_result(m, nodes, nominal.hist, flights, dtype, K)
