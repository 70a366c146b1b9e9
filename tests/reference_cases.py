"""The cases the CPU reference tests share: the nominal fields, a bounded synthetic blob, the prototype problem, and the law
the reference computes for itself.  A plain module, imported by the test files; no fixtures and no GPU."""
import functools

import numpy as np

import feedforward_reference as ffr
import flight_jacobian_reference as jr
import flight_reference as fr
import guidance_reference as gr
from oracle.ascent_numpy import Params

E_FT = np.eye(16)[3]


def p16():
    return np.array([getattr(Params(), f) for f in fr.FIELDS], dtype=np.float64)


def blob(nt=18, seed=4):
    """an arbitrary bounded control with free and (two) saturated steps"""
    b = fr.synthetic_exact_blob(p16(), nt, tf=0.9, seed=seed)
    K = nt - 1
    b[7 * K + 3], b[7 * K + K - 2] = 1.0, -1.0
    return b


@functools.lru_cache(maxsize=None)
def prototype_case():
    """backward Euler, nt = 50, the C oracle's solution trimmed with numpy to 1e-12 (m = 18), and its records"""
    from oracle import c_oracle
    c_oracle.build()
    nt = 50
    p = c_oracle.pack_params(Params())
    r = c_oracle.solve_batch(p[None], nt, 300, 1e-9, want_blob=True)
    assert r["status"][0] == 0
    t = jr.trim(p, r["blob"][0], nt, 0, 0, 0, 8, 1e-12)
    assert t["summary"][0] == 0
    return p, t["blob"], nt, gr.records(p, t["blob"], nt), gr.records(p, t["blob"], nt, dtype=np.longdouble)


def law(kind, rec, p16):
    """keyword arguments of lincov_reference.corridor for a kind of flight; the gains are the reference's own at q = 1e6"""
    if kind == "open":
        return {}
    G = ffr.gains(rec, p16, np.array([1e6, 1e6, 1e6, 1.0, 1.0, 0.5]), E_FT, np.longdouble)
    assert G["summary"][0] == 0
    kw = dict(gain_u=G["gain_u"].astype(np.float64), gain_t=G["gain_t"].astype(np.float64), smax=0.5)
    if kind == "navigated":
        kw.update(ff_u=G["ff_u"].astype(np.float64), ff_t=float(G["ff_t"]), know=E_FT)
    return kw
