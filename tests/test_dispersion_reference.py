"""The CPU reference of the Monte Carlo dispersion (tests/dispersion_reference.py) checked against tests/flight_reference.py
(the unperturbed flight), against the complex-step Jacobian of tests/flight_jacobian_reference.py (second-order agreement) and
for the substeps it holds.  No GPU."""
import numpy as np
import pytest

import dispersion_reference as dr
import flight_jacobian_reference as jr
import flight_reference as fr
from oracle.ascent_numpy import Params


def _p16():
    return np.array([getattr(Params(), f) for f in fr.FIELDS], dtype=np.float64)


@pytest.mark.parametrize("form", [0, 1])
def test_zero_sigma_is_the_flight_reference(form):
    """Every sigma = 0, whatever xi holds (a NaN among it): all samples equal flight_reference.fly's last node and summary rows
    2 / 3 exactly; mean = nominal, covariance 0, n = samples."""
    nt, K = 18, 17
    p16 = _p16()
    blob = fr.synthetic_exact_blob(p16, nt, tf=0.9, seed=3)
    xi = np.random.default_rng(1).standard_normal((24 + K, 5))
    xi[10, 2] = np.nan
    for m in (0, 3):
        d = dr.disperse(p16, blob, nt, xi, np.zeros(24), np.zeros(K), form, m)
        f = fr.fly(p16, blob, nt, formulation=form, substeps=m, want_local=False)
        want = np.concatenate([f["traj"][[0, 1, 2, 3, 6, 7, 9], -1], f["summary"][2:4]])
        assert d["m"] == f["m"]
        assert np.array_equal(d["nominal"], want) and np.array_equal(d["samples"], np.tile(want, (5, 1)))
        st = d["stats"]
        assert st[0] == 5 and np.array_equal(st[1:10], want) and np.array_equal(st[64:73], want) and np.array_equal(st[73:82], want)
        assert np.allclose(st[10:19], want, rtol=1e-15, atol=0) and np.abs(st[19:64]).max() <= 1e-28 * np.abs(want).max() ** 2


@pytest.mark.parametrize("form", [0, 1])
def test_one_sample_agrees_with_the_jacobian_to_second_order(form):
    """remainder(sigma) = sample - nominal - J (sigma o xi): halving sigma with the same xi divides it by 4, within [3, 5], on
    every row whose remainder is above 1e-9 of the row's scale at both sigmas (below that the remainder is rounding of the
    flight, not curvature) -- and the position, velocity and apsis rows are all above it at the sigmas chosen here, relative
    1e-4 and 5e-5 (of every field the flight reads; absolute on z_0, t_f and every control).  At 1e-3 the third-order term shows:
    z_0 carries an angular rate that turns the thrust by 0.4 rad over the burn, and a ratio falls outside [3, 5]."""
    nt, K, m = 18, 17, 2
    p16 = _p16()
    blob = fr.synthetic_exact_blob(p16, nt, tf=0.9, seed=4)
    xi = np.random.default_rng(2).standard_normal((24 + K, 1))
    J = jr.jacobian(p16, blob, nt, form, m)
    rem = []
    for rel in (1e-4, 5e-5):
        sigma, su = dr.relative_sigma(p16, rel), np.full(K, rel)
        d = dr.disperse(p16, blob, nt, xi, sigma, su, form, m)
        assert d["stats"][0] == 1
        lin = J["jac"] @ (sigma * xi[:24, 0]) + J["jac_u"] @ (su * xi[24:, 0])
        rem.append(d["samples"][0] - d["nominal"] - lin)
    scale = np.maximum(np.abs(d["nominal"]), 1.0)
    big = (np.abs(rem[0]) > 1e-9 * scale) & (np.abs(rem[1]) > 1e-9 * scale)
    print("form", form, "remainders", rem[0], rem[1], "rows checked", np.flatnonzero(big))
    assert big[[0, 1, 2, 3, 7, 8]].all()
    ratio = rem[0][big] / rem[1][big]
    print("ratios", ratio)
    assert np.all((ratio >= 3.0) & (ratio <= 5.0))


def test_substeps_of_the_nominal_flight_are_held():
    """nt = 18, substeps = 0, t_f dispersed by 5 %: the m of flight_reference.substeps_of at a sample's own t_f differs from the
    nominal m for some sample; that sample is flown with the nominal m all the same."""
    nt, K = 18, 17
    p16 = _p16()
    blob = fr.synthetic_exact_blob(p16, nt, tf=0.9, seed=5)
    tf = blob[21 * K]
    xi = np.random.default_rng(3).standard_normal((24, 6))
    sigma = np.zeros(24)
    sigma[23] = 0.05 * tf
    d = dr.disperse(p16, blob, nt, xi, sigma, None, 0, 0)
    m = d["m"]
    assert m == fr.substeps_of(tf * p16[11] / K)
    own = [fr.substeps_of((tf + sigma[23] * xi[23, s]) * p16[11] / K) for s in range(6)]
    differ = [s for s in range(6) if own[s] != m]
    print("nominal m", m, "own m of the samples", own)
    assert differ
    s = differ[0]
    us = blob[7 * K:8 * K]
    held = dr.fly_rows(p16, np.zeros(7), us, tf + sigma[23] * xi[23, s], m)
    recomputed = dr.fly_rows(p16, np.zeros(7), us, tf + sigma[23] * xi[23, s], own[s])
    assert np.array_equal(d["samples"][s], held) and not np.array_equal(held, recomputed)


def test_invalid_samples_are_left_out():
    """A NaN draw on a field with sigma != 0 makes that sample invalid: n = samples - 1 and the statistics are those of the
    others; with one valid sample the covariance is NaN and the mean defined; with none everything but the nominal rows is NaN."""
    nt, K = 18, 17
    p16 = _p16()
    blob = fr.synthetic_exact_blob(p16, nt, tf=0.9, seed=6)
    xi = np.random.default_rng(4).standard_normal((24, 4))
    sigma = np.zeros(24)
    sigma[7 + 3] = 50.0
    a = dr.disperse(p16, blob, nt, xi[:, [0, 1, 3]], sigma, None, 0, 1)
    xi[7 + 3, 2] = np.nan
    b = dr.disperse(p16, blob, nt, xi, sigma, None, 0, 1)
    assert b["stats"][0] == 3 and np.isnan(b["samples"][2]).any()
    assert np.array_equal(a["stats"][1:], b["stats"][1:])
    one = dr.statistics(b["nominal"], b["samples"][1:3])
    assert one[0] == 1 and np.isnan(one[19:64]).all() and np.array_equal(one[10:19], b["samples"][1])
    none = dr.statistics(b["nominal"], b["samples"][2:3])
    assert none[0] == 0 and np.isnan(none[10:]).all() and np.array_equal(none[1:10], b["nominal"])
