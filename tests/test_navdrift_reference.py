"""The CPU reference of the time-varying navigation error (tests/navdrift_reference.py) checked against what it extends and
against closed forms: frozen channels give history_reference's and lincov_reference's bits, the marginal variance of the
channels is the AR(1) closed form, and the recursion in Q, C and D that the kernel carries -- written out here in numpy -- is the
superposition the reference forms.  No GPU."""
import numpy as np
import pytest

import guidance_reference as gr
import history_reference as hr
import lincov_reference as lr
import navdrift_reference as nd
from reference_cases import blob as _blob, law as _law, p16 as _p16

NT, K, M = 18, 17, 2
LD = np.longdouble
SIGMA_NAV = np.array([1e-5, 2e-5, 0.0, 1e-5, 1e-4, 0.0, 1e-5, 5.0])
PHI = np.array([0.9, 0.5, 0.8, 1.0, 0.0, 0.97, 1.0, 0.7])
Q = np.array([1e-5 * np.sqrt(1 - 0.81), 0.0, 3e-6, 0.0, 1e-4, 2e-6, 0.0, 5.0 * np.sqrt(1 - 0.49)])
#   stationary | decaying | zero-start walk | frozen | phi = 0 | zero-start | frozen | stationary


def _draws(S, seed=5):
    r = np.random.default_rng(seed)
    return r.standard_normal((24 + K, S)), r.standard_normal((8, S)), r.standard_normal((8, K, S))


@pytest.mark.parametrize("form", [0, 1])
def test_frozen_channels_fly_history_references_flight(form):
    """phi = 1, q = 0 and the arrays None: every sample's rows are history_reference.history's, array_equal in float64; the draws
    of a frozen channel are NaN and never read"""
    p16, blob = _p16(), _blob()
    law = _law("navigated", gr.records(p16, blob, NT, form, M, LD), p16)
    xi, xi_nav, _ = _draws(3)
    sigma = np.zeros(24)
    sigma[:7], sigma[10] = 1e-6, 20.0
    su = np.full(K, 1e-4)
    args = (p16, blob, NT, xi, sigma, su, law["gain_u"], law["gain_t"], law["smax"], law["ff_u"], law["ff_t"], law["know"], xi_nav, SIGMA_NAV)
    base = hr.history(*args, formulation=form, substeps=M)
    for phi, q, om in ((None, None, None), (np.ones(8), np.zeros(8), np.full((8, K, 3), np.nan))):
        got = nd.history_drifting(*args, phi, q, om, formulation=form, substeps=M)
        assert np.array_equal(got["samples"], base["samples"]) and np.array_equal(got["clipped"], base["clipped"])
        assert np.array_equal(got["stats"], base["stats"], equal_nan=True) and np.isfinite(got["samples"]).all()


@pytest.mark.parametrize("kind", ["guided", "navigated"])
def test_frozen_channels_give_lincov_references_corridor(kind):
    p16, blob = _p16(), _blob()
    rec = gr.records(p16, blob, NT, 0, M)
    law = _law(kind, gr.records(p16, blob, NT, 0, M, LD), p16)
    sigma = np.full(24, 1e-6)
    su = np.full(K, 1e-3)
    base = lr.corridor(p16, blob, NT, sigma, su, sigma_nav=SIGMA_NAV, substeps=M, rec=rec, **law)
    for phi, q in ((None, None), (np.ones(8), np.zeros(8))):
        got = nd.corridor_drifting(p16, blob, NT, sigma, su, sigma_nav=SIGMA_NAV, phi=phi, q=q, substeps=M, rec=rec, **law)
        for key in ("S", "cov", "noise", "nominal"):
            assert np.array_equal(got[key], base[key]), key
        assert np.all(got["var_n"] == 0)


def test_marginal_variance_is_the_ar1_closed_form():
    """var n_a,k of the drive alone, from the superposition's impulse responses, against q^2 (1 - phi^2k) / (1 - phi^2) (k q^2 at
    phi = 1); and with the initial sigma^2 phi^2k added, a stationary drive q = sigma sqrt(1 - phi^2) keeps sigma^2 for every k"""
    p16, blob = _p16(), _blob()
    rec = gr.records(p16, blob, NT, 0, M)
    law = _law("navigated", gr.records(p16, blob, NT, 0, M, LD), p16)
    phi, q = PHI.copy(), Q.copy()
    phi[3], q[3] = 1.0, 2e-6          # a random walk instead of the frozen channel
    got = nd.corridor_drifting(p16, blob, NT, np.zeros(24), None, sigma_nav=SIGMA_NAV, phi=phi, q=q, substeps=M, rec=rec, **law)
    k = np.arange(K + 1)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        closed = np.where(phi == 1.0, k * q ** 2, q ** 2 * (1 - phi ** (2 * k)) / (1 - phi ** 2))
    assert np.abs(got["var_n"] - closed).max() <= 1e-14 * closed.max()
    assert np.allclose(got["var_n"], closed, rtol=1e-13, atol=0)
    total = got["var_n"] + SIGMA_NAV ** 2 * phi ** (2 * k)
    for a in (0, 7):                   # the two stationary channels
        assert np.allclose(total[:, a], SIGMA_NAV[a] ** 2, rtol=1e-13, atol=0), a
    # the Monte Carlo sequences have that variance: 4000 samples, four standard errors of a variance estimate
    S = 4000
    _, xi_nav, om = _draws(S, 11)
    n, on = nd.sequences(K, xi_nav, SIGMA_NAV, phi, q, om)
    assert list(on) == [True] * 8
    v = n.var(axis=0, ddof=0)
    assert np.all(np.abs(v[1:] - total[1:]) <= 4 * np.sqrt(2.0 / S) * total[1:] + 1e-300)


def _recursion(rec, p16, law, su, phi, q, dtype):
    """N_j (K, 10, 10) by the recursion of include/ascent.h: D, C and Q, and the node rows through C_{j-1} Phi_n and D_j"""
    f = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
    Ku, fu, kt, ft = f(law["gain_u"]), f(law.get("ff_u", np.zeros(K))), f(law["gain_t"]), dtype(law.get("ff_t", 0.0))
    ph, q2, su2 = f(phi), f(q) ** 2, f(su) ** 2
    D, Cm, Qm = np.zeros(8, dtype=dtype), np.zeros((7, 8), dtype=dtype), np.zeros((7, 7), dtype=dtype)
    out = np.zeros((K, 10, 10), dtype=dtype)
    for k in range(1, K + 1):
        Phi, g = rec["Phi"][k - 1], rec["g"][k - 1]
        kap = np.concatenate([Ku[k - 1], [fu[k - 1]]])
        A = Phi - np.outer(g, Ku[k - 1])
        B = -np.outer(g, kap)
        if k == K:
            A = A - np.outer(rec["gamma"], kt)
            B = B - np.outer(rec["gamma"], np.concatenate([kt, [ft]]))
        Dk = ph * D * ph + q2
        Ct = Cm * ph                                       # Cov(dz_{k-1}, n_k)
        ga, _ = lr.altitude_gradient(p16, rec["nodes"][k], dtype)
        # y_k = Y dz_{k-1} + W n_k + ye eps_k
        Y = np.concatenate([A, (ga @ A)[None], -Ku[k - 1][None], Ku[k - 1][None]])
        W = np.concatenate([B, (ga @ B)[None], -kap[None], kap[None]])
        ye = np.concatenate([g, [ga @ g, 1, 0]]).astype(dtype)
        n = Y @ Qm @ Y.T + Y @ Ct @ W.T + (Y @ Ct @ W.T).T + (W * Dk) @ W.T + su2[k - 1] * np.outer(ye, ye)
        out[k - 1] = (n + n.T) / 2
        Qn = A @ Qm @ A.T + A @ Ct @ B.T + (A @ Ct @ B.T).T + (B * Dk) @ B.T + su2[k - 1] * np.outer(g, g)
        Cm = A @ Ct + B * Dk
        Qm, D = (Qn + Qn.T) / 2, Dk
    return out


def test_recursion_in_q_c_d_is_the_superposition():
    """The recursion the kernel carries against the reference's superposition, both in float64, within 100 x the reference's own
    float64-against-longdouble gap (floor 1e-10) in units of sqrt(N_aa N_bb); and the execution-error part alone, superposed
    from m_eps, against lincov_reference's Q recursion, which the reference takes for that part"""
    p16, blob = _p16(), _blob()
    rec, recl = gr.records(p16, blob, NT, 0, M), gr.records(p16, blob, NT, 0, M, LD)
    law = _law("navigated", recl, p16)
    su = np.full(K, 1e-3)
    su[5] = 0.0
    kw = dict(sigma_nav=SIGMA_NAV, phi=PHI, q=Q, substeps=M)
    r64 = nd.corridor_drifting(p16, blob, NT, np.zeros(24), su, rec=rec, **kw, **law)
    rld = nd.corridor_drifting(p16, blob, NT, np.zeros(24), su, rec=recl, dtype=LD, **kw, **law)
    sd = np.sqrt(np.einsum("jaa->ja", rld["noise"]).astype(np.float64))
    den = np.where(sd[:, :, None] * sd[:, None, :] > 0, sd[:, :, None] * sd[:, None, :], 1.0)
    gap = float((np.abs((r64["noise"] - rld["noise"]).astype(np.float64)) / den).max())
    rcs = _recursion(rec, p16, law, su, PHI, Q, np.float64)
    err = float((np.abs(rcs - rld["noise"].astype(np.float64)) / den).max())
    print("reference gap", gap, "recursion against superposition", err)
    assert err <= max(1e-10, 100 * gap)
    assert np.any(r64["noise"] != lr.corridor(p16, blob, NT, np.zeros(24), su, sigma_nav=SIGMA_NAV, substeps=M, rec=rec, **law)["noise"])
    eps = np.einsum("jak,k,jbk->jab", r64["m_eps"], su ** 2, r64["m_eps"])
    base = lr.corridor(p16, blob, NT, np.zeros(24), su, substeps=M, rec=rec, **law)["noise"]
    assert (np.abs(eps - base) / den).max() <= 1e-12


def test_impulse_response_is_the_central_difference_of_the_flight():
    """r_jak of the reference against a pair of flights of history_drifting whose omega_a,k is +-1 and everything else zero, with q_a
    small enough to stay linear: channel 0 at the first step, channel 7 in the middle, channel 4 at the last step"""
    p16, blob = _p16(), _blob()
    recl = gr.records(p16, blob, NT, 0, M, LD)
    law = _law("navigated", recl, p16)
    phi = np.array([0.9, 1, 1, 1, 0.5, 1, 1, 0.7])
    q = np.array([1e-7, 0, 0, 0, 1e-7, 0, 0, 1e-4 * p16[3]])
    ref = nd.corridor_drifting(p16, blob, NT, np.zeros(24), None, phi=phi, q=q, substeps=M, rec=recl, dtype=LD, **law)
    scale = lr.row_scales(p16, law["gain_u"], law["ff_u"], K)
    xi = np.zeros((24 + K, 2))
    for a, k in ((0, 1), (7, 9), (4, K)):
        om = np.zeros((8, K, 2))
        om[a, k - 1] = (1.0, -1.0)
        h = nd.history_drifting(p16, blob, NT, xi, np.zeros(24), None, law["gain_u"], law["gain_t"], law["smax"], law["ff_u"], law["ff_t"],
                                law["know"], None, None, phi, q, om, substeps=M, dtype=LD)
        assert not h["clipped"].any()
        fd = (h["samples"][0] - h["samples"][1]) / (2 * LD(q[a]))
        r = ref["r_om"][:, :, a, k - 1]
        d = np.abs(((fd - r) / scale).astype(np.float64))
        assert np.all(r[:k - 1] == 0) and np.any(r[k - 1:] != 0)
        assert d.max() <= 1e-6 * max(1.0, np.abs((r / scale).astype(np.float64)).max()), (a, k, d.max())
