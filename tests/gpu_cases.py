"""The cases, inputs and measures the GPU test modules share.  A plain module, imported by the test files; it holds no test and
no fixture of its own (parity_writer makes one for the module that calls it).  Solved cases and gains are computed once per
process (lru_cache) and handed out read-only."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import dispersion_reference as dr
import flight_reference as fr
import lincov_reference as lr

# (nt, scheme, form) of the closed-loop modules: one chunk whose last step is half the grid; a chunk that holds one step
# (K = 17), every (scheme, formulation) pair; three chunks
CASES = [(3, 0, 0), (3, 0, 1)] + [(18, s, f) for s, f in ((0, 0), (1, 0), (2, 0), (0, 1))] + [(34, 0, 0)]
M = 2                      # substeps of the parity tests
REL = 1e-3                 # relative sigma of the parameters the flight reads; absolute sigma of z_0, t_f (scaled) and every control
SAMPLE_BOUND = 1e-10       # tests/test_gpu_flight.py's bound for the same arithmetic: scaled units; times r_peri for the altitudes
FLOOR = 1e-10              # the same bound (SAMPLE_BOUND) in the scales of tests/test_gpu_lincov.py
FD_STEPS = (1e-5, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10, 1e-11)          # relative steps tried; truncation falls and rounding rises along them


def parity_writer(env_name, store, sort_keys=False):
    """-> a module-scoped autouse fixture that, when the module is done, writes `store` as JSON to the file the environment
    variable names, if it names one"""
    @pytest.fixture(scope="module", autouse=True)
    def _write_parity():
        yield
        path = os.environ.get(env_name)
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                json.dump(store, f, indent=1, sort_keys=sort_keys)
    return _write_parity


def points(n=2, dcost=None):
    """the nominal point and sweep corners (config 3), tf_ub = 1.2; dcost: the DCOST column of every row"""
    from lunar_module_ascent_trajectory_optimiser_amd import AscentParams, sweep_isp_drymass
    nom = AscentParams(tf_ub=1.2).as_row()
    sw = sweep_isp_drymass()
    P = np.vstack([nom, sw[0], sw[4095], sw[63], sw[4032]])[:n].copy()
    if dcost is not None:
        P[:, 15] = dcost
    return P


@functools.lru_cache(maxsize=None)
def solved(nt, scheme, form, terminal=0, n=2):
    """(P, blob): solved once per case and shared; never written to.  tol 1e-10: the slack the interior-point method leaves on
    the terminal inequalities, which the comparison of the flown apsides with the NLP's own sees, is then 1.5e-4 m."""
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch
    P = points(n)
    r = solve_batch(P, nt, tol=1e-10, max_iter=500, want_blob=True, scheme=scheme, formulation=form, terminal=terminal)
    assert (r.status == 0).all(), r.status
    P.setflags(write=False)
    r.blob.setflags(write=False)
    return P, r.blob


def synthetic():
    """the nt = 3 blob of the flight Jacobian's smallest-grid test"""
    return points(1), fr.make_blob(np.zeros((2, 7)), np.array([0.4, -0.7]), 0.05)[:, None]


@functools.lru_cache(maxsize=None)
def case(nt, scheme, form, n=2):
    """(P, blob): the synthetic blob at nt = 3, else GPU-solved and trimmed to 1e-12; shared, never written to"""
    from lunar_module_ascent_trajectory_optimiser_amd import trim_batch
    if nt == 3:
        return synthetic()
    P, blob = solved(nt, scheme, form, n=n)
    t = trim_batch(P, blob, nt, scheme=scheme, formulation=form, substeps=M, rounds=8, tol=1e-12)
    assert (t.status == 0).all(), t.summary
    t.blob.setflags(write=False)
    return P, t.blob


def weights(q, smax=0.5):
    return dict(cond_weights=(q, q, q), control_weight=1.0, cutoff_weight=1.0, stretch_max=smax)


@functools.lru_cache(maxsize=None)
def gains(nt, scheme, form, kind, q, n=2, substeps=M, jacobian=False):
    """the device's own gains of a case; navigated: with the feed-forward of the thrust; open: None"""
    from lunar_module_ascent_trajectory_optimiser_amd import guidance_gains
    if kind == "open":
        return None
    P, blob = case(nt, scheme, form, n)
    g = guidance_gains(P, blob, nt, scheme=scheme, formulation=form, substeps=substeps, want_jacobian=jacobian,
                       **(dict(feedforward="Ft") if kind == "navigated" else {}), **weights(q))
    assert (g.status == 0).all()
    return g


def sigmas(P, rel=REL, tf_rel=None, blob=None):
    """keyword arguments of disperse_batch: all four groups non-zero"""
    sig = np.array([dr.relative_sigma(p, rel) for p in P])
    tf = sig[:, 23] if tf_rel is None else tf_rel * blob[-10]
    return dict(z0_sigma=sig[:, :7].copy(), param_sigma=sig[:, 7:23].copy(), tf_sigma=np.array(tf), control_sigma=rel)


def xi(K, samples, seed=11):
    return np.random.default_rng(seed).standard_normal((24 + K, samples))


def guided(P, blob, nt, scheme, form, g, xi, kw, substeps=M, keep=True):
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch
    return disperse_batch(P, blob, nt, xi=xi, keep_samples=keep, scheme=scheme, formulation=form, substeps=substeps, guidance=g, **kw)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def same(a, b):
    """the same bits, NaN positions included: two arrays of one shape, None and None, or two dicts of those key by key"""
    if isinstance(a, dict):
        return all(same(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def stats(d):
    return np.concatenate([d.n_valid[:, None], d.nominal, d.mean, d.cov.reshape(-1, 81), d.min, d.max], axis=1)


def sample_error(dev, ref, S):
    """largest difference of (samples, 9) rows in units of the bound's scale; rows that are not finite must agree as they are"""
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(dev)) and np.array_equal(ref[~fin], dev[~fin], equal_nan=True)
    d = np.where(fin, np.abs(np.where(fin, dev, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    d[:, 7:] /= S
    return d.max()


def scaled_error(dev, ref, r_peri, scale89):
    """largest difference of (samples, K, 10) histories in units of the bound's scale: scaled units for the state, r_peri for the
    altitude, scale89 (K,) for the control and the correction; entries that are not finite must agree as they are"""
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(dev)) and np.array_equal(ref[~fin], dev[~fin], equal_nan=True)
    d = np.where(fin, np.abs(np.where(fin, dev, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    d[:, :, 7] /= r_peri
    d[:, :, 8:] /= scale89[None, :, None]
    return float(d.max()) if d.size else 0.0


def numpy_stats(samples):
    """count, mean, unbiased covariance, min, max over the valid rows of (samples, 9)"""
    v = samples[np.isfinite(samples).all(axis=1)]
    n = len(v)
    nan9 = np.full(9, np.nan)
    return (n, v.mean(axis=0) if n else nan9, np.atleast_2d(np.cov(v.T)) if n >= 2 else np.full((9, 9), np.nan),
            v.min(axis=0) if n else nan9, v.max(axis=0) if n else nan9)


def check_statistics(d, j, samples=None):
    """problem j of a DispersionResult against numpy on (its own) samples: the error in units of the bound 1e-11 range_i
    (range_i range_j for the covariance); extrema and count exact"""
    n, mean, cov, lo, hi = numpy_stats(d.samples[j] if samples is None else samples)
    assert d.n_valid[j] == n
    assert np.array_equal(d.min[j], lo, equal_nan=True) and np.array_equal(d.max[j], hi, equal_nan=True)
    if n == 0:
        assert np.isnan(d.mean[j]).all() and np.isnan(d.cov[j]).all()
        return 0.0
    rng = hi - lo
    em = np.abs(d.mean[j] - mean)
    assert np.all(em <= 1e-11 * rng), (em, rng)
    worst = float(np.max(np.divide(em, rng, out=np.zeros(9), where=rng > 0)))
    if n < 2:
        assert np.isnan(d.cov[j]).all()
        return worst
    ec, rr = np.abs(d.cov[j] - cov), np.outer(rng, rng)
    assert np.all(ec <= 1e-11 * rr), (ec, rr)
    assert np.array_equal(d.cov[j], d.cov[j].T)
    return max(worst, float(np.max(np.divide(ec, rr, out=np.zeros((9, 9)), where=rr > 0))))


def col_scales(p16):
    """(32,) the size of a unit relative step of every constant: the field's own (1 where it is zero), the thrust for the error of
    theta-hat, 1 in scaled units"""
    s = np.ones(lr.NC)
    s[lr.C_P:lr.C_TF] = np.where(p16 != 0, np.abs(p16), 1.0)
    s[lr.C_E] = abs(p16[3])
    return s


def norm_jac(S, rows, cols):
    return np.asarray(S * cols[None, None, :] / rows[:, :, None], dtype=np.float64)


def norm_cov(Cv, rows):
    return np.asarray(Cv / (rows[:, :, None] * rows[:, None, :]), dtype=np.float64)
