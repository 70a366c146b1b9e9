"""The CPU reference of the navigation filter (tests/navfilter_reference.py) checked against itself by two routes and against
what a filter must satisfy: the superposition against the 14 x 14 covariance recursion, the consistency identity (the truth fed
the design's own gains under the design's own assumptions has the covariance the design believes), and the optimality of the
design's gains.  No GPU."""
import numpy as np
import pytest

import guidance_reference as gr
import navfilter_reference as nr
from reference_cases import blob as _blob, law as _law, p16 as _p16

NT, K, M = 18, 17, 2
LD = np.longdouble
H4 = np.eye(7)[[0, 1, 2, 3]]                   # the unit rows of x, y, xdot, ydot
SIG_M, SIG_NAV = 1e-4, 1e-3


def _design(rec, n_meas, stride, su=None, q=None, dtype=np.float64):
    return nr.design(rec, np.full(7, SIG_NAV), H4[:n_meas], np.full(n_meas, SIG_M), stride, su, q, dtype)


@pytest.mark.parametrize("kind", ["open", "guided"])
@pytest.mark.parametrize("n_meas,stride", [(1, 1), (2, 4), (4, 1), (4, K + 1)])
def test_superposition_equals_the_recursion(kind, n_meas, stride):
    """The covariance of [dz; e] under eps and v: the sum over the unit sources of their responses' outer products against
    F Q F' / U Q U'.  Both in longdouble on the same records, every node; within 1e-12 of sqrt(Q_aa Q_bb).  (In float64 the
    guided recursion without a measurement reaches 4e-11: the estimate then follows the state exactly, dz + e = 0, which the
    superposition keeps and the recursion has to cancel through gains of 1e3.)  The gains are the design's, halved so that they
    are not the optimal ones."""
    p16, blob = _p16(), _blob()
    rec = gr.records(p16, blob, NT, 0, M, LD)
    law = _law(kind, rec, p16)
    su = np.full(K, 1e-3)
    su[5] = 0.0
    d = _design(rec, n_meas, stride, su, dtype=LD)
    assert d["status"] == 0 and all(s > 0 for _, _, s in d["s"])
    gl = 0.5 * d["gain_l"].astype(np.float64)
    ref = nr.corridor(p16, blob, NT, np.zeros(24), np.zeros(7), gl, H4[:n_meas], np.full(n_meas, SIG_M), stride, su, rec=rec, dtype=LD, **law)
    Q = nr.recursion(rec, su, law.get("gain_u"), law.get("gain_t"), law.get("smax", 0.0), gl, H4[:n_meas], np.full(n_meas, SIG_M), stride, LD)
    for name, a, b in (("dz", ref["noise"][:, :7, :7], Q[:, :7, :7]), ("e", ref["nav_noise"], Q[:, 7:, 7:])):
        # in units of sqrt(Q_aa Q_bb) of the superposition; a state no source reaches (the mass: g has no mass row) is exactly 0
        # there and rounding in the recursion, so a standard deviation below 1e-9 of the node's largest takes the largest
        sd = np.sqrt(np.einsum("jaa->ja", a))
        sd = np.where(sd < 1e-9 * sd.max(axis=1, keepdims=True), sd.max(axis=1, keepdims=True), sd)
        den = np.where(sd[:, :, None] * sd[:, None, :] > 0, sd[:, :, None] * sd[:, None, :], 1.0)
        err = float((np.abs(a - b) / den).astype(np.float64).max())
        print(kind, n_meas, stride, name, "superposition against the recursion", err)
        assert err <= 1e-12


def _rel(a, b, sd):
    """the largest difference of two stacks of covariances in units of sd_a sd_b"""
    return float((np.abs(a - b) / (sd[:, :, None] * sd[:, None, :])).astype(np.float64).max())


@pytest.mark.parametrize("kind", ["open", "guided"])
@pytest.mark.parametrize("n_meas,stride", [(1, 1), (2, 4), (4, 1), (4, K + 1)])
def test_consistency_identity(kind, n_meas, stride):
    """Truth fed the design's own gains, dp = dt_f = 0, filter_q = 0, the same sigma_u and e_0 ~ sigma_nav: nav_cov equals P-hat at
    every node, whatever the guidance law does with the estimate and however z_0 is dispersed.  Entries in units of
    sqrt(P_aa P_bb).  In float64 the two agree to the larger of 1e-12 and 100 x the distance of the float64 runs from the longdouble
    ones (the unobserved states grow along the flight and the update cancels: with x and y alone measured every fourth node that
    distance is 7e-11) -- the convention of the GPU tests, here between two routes of the reference; and the difference is
    rounding, not the model: in longdouble, whose unit roundoff is 2^-11 of float64's, it is below 1e-15 or a hundredth of the
    float64 one (seen: 1e-18 .. 3e-14 against 8e-15 .. 7e-11)."""
    p16, blob = _p16(), _blob()
    law = _law(kind, gr.records(p16, blob, NT, 0, M, LD), p16)
    su = np.full(K, 1e-3)
    sigma = np.zeros(24)
    sigma[:7] = 1e-3                            # the dispersion of z_0 is no error of the estimate
    run = {}
    for dt in (np.float64, LD):
        rec = gr.records(p16, blob, NT, 0, M, dt)
        d = _design(rec, n_meas, stride, su, dtype=dt)
        assert d["status"] == 0
        ref = nr.corridor(p16, blob, NT, sigma, np.full(7, SIG_NAV), d["gain_l"], H4[:n_meas], np.full(n_meas, SIG_M), stride, su, rec=rec,
                          dtype=dt, **law)
        run[dt] = (ref["nav_cov"], d["P"])
    sd = np.sqrt(np.einsum("jaa->ja", run[LD][1]))
    err_ld, err = _rel(*run[LD], sd), _rel(*run[np.float64], sd)
    gap = max(_rel(run[np.float64][0], run[LD][0], sd), _rel(run[np.float64][1], run[LD][1], sd))
    print(kind, n_meas, stride, "true covariance of e against P-hat: longdouble", err_ld, "float64", err, "float64 against longdouble", gap)
    assert err_ld <= max(1e-15, 1e-2 * err) and err <= max(1e-12, 100.0 * gap)


def test_halving_the_gains_never_lowers_the_error():
    """The design's gains minimise trace(nav_cov) at every node: with half of them it is larger at every node from the first
    measurement on, and equal before it."""
    p16, blob = _p16(), _blob()
    rec = gr.records(p16, blob, NT, 0, M)
    su = np.full(K, 1e-3)
    for n_meas, stride in ((1, 1), (4, 1), (4, 4)):
        d = _design(rec, n_meas, stride, su)
        run = lambda gl: nr.corridor(p16, blob, NT, np.zeros(24), np.full(7, SIG_NAV), gl, H4[:n_meas], np.full(n_meas, SIG_M), stride, su,
                                     rec=rec)["nav_cov"]
        full, half = np.einsum("jaa->j", run(d["gain_l"])), np.einsum("jaa->j", run(0.5 * d["gain_l"]))
        assert np.all(half[stride - 1:] > full[stride - 1:]) and np.array_equal(half[:stride - 1], full[:stride - 1])


def test_design_flags_a_vanishing_innovation_variance():
    """h = 0 with sigma = 0 gives s = 0: status 2, first_bad the first measurement node, NaN from it on and the rows before it kept"""
    p16, blob = _p16(), _blob()
    rec = gr.records(p16, blob, NT, 0, M)
    d = nr.design(rec, np.full(7, SIG_NAV), np.zeros((1, 7)), np.zeros(1), 4)
    assert d["status"] == 2 and d["first_bad"] == 4
    assert np.isnan(d["P"][3:]).all() and np.isnan(d["gain_l"][3:]).all() and np.isfinite(d["P"][:3]).all() and np.all(d["gain_l"][:3] == 0)
