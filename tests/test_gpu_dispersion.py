"""Monte Carlo dispersion (ascent_disperse_batch) on the GPU: every sample against the CPU reference
(tests/dispersion_reference.py), the reduction against numpy on the device's own samples, the bitwise properties the header
promises, invalid samples, the covariance against the linear prediction of the flight Jacobian, and the front ends.

The differences seen are collected in PARITY; with ASCENT_DISPERSION_PARITY_OUT=<file> they are written there as JSON when the
module is done (profiles/dispersion_parity.json is such a file)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import dispersion_reference as dr
import flight_jacobian_reference as jr
import flight_reference as fr
from gpu_cases import (REL, SAMPLE_BOUND, check_statistics as _check_statistics, parity_writer, points as _points,
                       sample_error as _sample_error, sigmas as _sigmas, solved as _solved, synthetic as _synthetic, xi as _xi)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = {"samples_vs_reference": {}, "statistics_vs_numpy": {}, "covariance_vs_reference": {}, "covariance_vs_linear": {}}
CASES = [(nt, scheme, form) for nt in (18, 34) for scheme, form in ((0, 0), (1, 0), (2, 0), (0, 1))]
_write_parity = parity_writer("ASCENT_DISPERSION_PARITY_OUT", PARITY)


def _reference(P, blob, nt, xi, kw, form, substeps, j):
    K = nt - 1
    sigma = np.concatenate([kw["z0_sigma"][j], kw["param_sigma"][j], [kw["tf_sigma"][j]]])
    return dr.disperse(P[j], blob[:, j], nt, xi, sigma, np.full(K, kw["control_sigma"]), form, substeps)


def _check_samples(name, P, blob, nt, form, scheme, substeps, kw, samples=65):
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch
    K = nt - 1
    xi = _xi(K, samples)
    d = disperse_batch(P, blob, nt, xi=xi, keep_samples=True, scheme=scheme, formulation=form, substeps=substeps, **kw)
    assert d.samples.shape == (P.shape[0], samples, 9) and d.cov.shape == (P.shape[0], 9, 9)
    worst = 0.0
    for j in range(P.shape[0]):
        ref = _reference(P, blob, nt, xi, kw, form, substeps, j)
        worst = max(worst, _sample_error(d.samples[j], ref["samples"], P[j, 9]),
                    _sample_error(d.nominal[j][None], ref["nominal"][None], P[j, 9]))
        assert d.n_valid[j] == ref["stats"][0]
    PARITY["samples_vs_reference"][name] = worst
    print(name, "samples against the reference, worst difference (scaled; altitudes / r_peri)", worst)
    assert worst <= SAMPLE_BOUND


@pytest.mark.parametrize("nt,scheme,form", CASES)
def test_samples_match_reference(nt, scheme, form):
    """65 samples, all four sigma groups non-zero, substeps = 2, two problems: every row of samples_out against the CPU reference
    within 1e-10 in scaled units (times r_peri for the two altitude rows)."""
    P, blob = _solved(nt, scheme, form)
    _check_samples(f"nt{nt}_scheme{scheme}_form{form}", P, blob, nt, form, scheme, 2, _sigmas(P))


@pytest.mark.parametrize("form", [0, 1])
def test_samples_match_reference_on_the_smallest_grid(form):
    P, blob = _synthetic()
    _check_samples(f"nt3_synthetic_form{form}", P, blob, 3, form, 0, 2, _sigmas(P))


def test_samples_match_reference_with_held_substeps():
    """substeps = 0 and t_f dispersed by 5 %: the nominal m (about 50 at nt = 18) is held although most samples' own t_f would
    pick another; one problem."""
    nt, K = 18, 17
    P, blob = _solved(nt, 0, 0)
    P, blob = P[:1], blob[:, :1]
    kw = _sigmas(P, tf_rel=0.05, blob=blob)
    xi = _xi(K, 65)
    m = fr.substeps_of(blob[21 * K, 0] * P[0, 11] / K)
    own = [fr.substeps_of((blob[21 * K, 0] + kw["tf_sigma"][0] * xi[23, s]) * P[0, 11] / K) for s in range(65)]
    assert any(o != m for o in own)
    _check_samples("nt18_scheme0_form0_substeps0_tf5pct", P, blob, nt, 0, 0, 0, kw)


@pytest.mark.parametrize("samples", [1, 2, 63, 64, 65, 129, 192, 193, 257, 300, 1024])
def test_statistics_match_numpy_on_the_device_samples(samples):
    """The reduction alone: mean, unbiased covariance, min, max, count of stats_out against numpy over the valid rows of the
    same call's samples_out.  Bounds: means 1e-11 range_i, covariances 1e-11 range_i range_j (n eps <= 1.2e-13 for n <= 1024,
    times 100 for the subtraction in the covariance), extrema and count exact.  The sample counts straddle the wavefront (64), the
    workgroup (256) and several partial records, and take every workgroup size (one to four wavefronts: up to 64, 128, 192
    samples, and beyond); n < 2 gives a NaN covariance and a defined mean."""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch
    nt = 18
    worst = 0.0
    for scheme, form in ((0, 0), (0, 1)):
        P, blob = _solved(nt, scheme, form)
        d = disperse_batch(P, blob, nt, xi=_xi(nt - 1, samples, 5), keep_samples=True, scheme=scheme, formulation=form, substeps=2, **_sigmas(P))
        assert (d.n_valid == samples).all()
        for j in range(2):
            worst = max(worst, _check_statistics(d, j))
        if samples == 1:
            assert np.array_equal(d.mean, d.samples[:, 0])
    PARITY["statistics_vs_numpy"][f"samples{samples}"] = worst
    print("samples", samples, "statistics against numpy, worst error / range", worst)


@pytest.mark.parametrize("nt,scheme,form", CASES + [(3, 0, 0), (3, 0, 1)])
def test_zero_sigma_is_the_nominal_flight_bit_for_bit(nt, scheme, form):
    """All sigma = 0, xi whatever (a NaN in it): every sample equals the nominal rows bit for bit, mean == nominal, covariance
    exactly 0, extrema == nominal; the nominal rows are ascent_fly_batch's last node and its summary rows 2 / 3, bit for bit.
    substeps 0 (automatic) and 2; 300 samples: two workgroups."""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch, fly_batch
    P, blob = _synthetic() if nt == 3 else _solved(nt, scheme, form)
    B, K = P.shape[0], nt - 1
    xi = _xi(K, 300, 3)
    xi[9, 17] = np.nan
    for m in (0, 2):
        kw = dict(scheme=scheme, formulation=form, substeps=m)
        f = fly_batch(P, blob, nt, want_local=False, **kw)
        nominal = np.concatenate([f.traj[:, [0, 1, 2, 3, 6, 7, 9], -1], f.summary[:, 2:4]], axis=1)
        for sig in (dict(), dict(param_sigma=np.zeros(16), control_sigma=0.0, tf_sigma=0.0, z0_sigma=np.zeros(7))):
            d = disperse_batch(P, blob, nt, xi=xi, keep_samples=True, **kw, **sig)
            assert np.array_equal(d.nominal, nominal)
            assert np.array_equal(d.samples, np.repeat(nominal[:, None, :], 300, axis=1))
            assert (d.n_valid == 300).all() and np.array_equal(d.mean, nominal) and np.all(d.cov == 0.0)
            assert np.array_equal(d.min, nominal) and np.array_equal(d.max, nominal)


def test_batch_independence_pointers_and_optional_output():
    """Each of 5 problems alone and repeated through a batch of 70 gives the same bits; host pointers and device pointers on
    torch's stream give the same bits; with and without samples_out the statistics are the same bits.  300 samples."""
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import _lib, disperse_batch
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    nt, K, B, S = 34, 33, 5, 300
    P, blob = _solved(nt, 0, 0, n=5)
    xi = _xi(K, S, 8)
    kw = _sigmas(P)

    def stats(d):
        return np.concatenate([d.n_valid[:, None], d.nominal, d.mean, d.cov.reshape(-1, 81), d.min, d.max], axis=1)

    host = disperse_batch(P, blob, nt, xi=xi, keep_samples=True, **kw)
    assert (host.n_valid == S).all()
    without = disperse_batch(P, blob, nt, xi=xi, **kw)
    assert without.samples is None and np.array_equal(stats(without), stats(host))
    for q in range(B):
        one = disperse_batch(P[q:q + 1], blob[:, q:q + 1], nt, xi=xi, keep_samples=True, **{k: v[q:q + 1] if isinstance(v, np.ndarray) else v for k, v in kw.items()})
        assert np.array_equal(stats(one)[0], stats(host)[q]) and np.array_equal(one.samples[0], host.samples[q])
    idx = np.arange(70) % B
    big = disperse_batch(P[idx], np.ascontiguousarray(blob[:, idx]), nt, xi=xi, keep_samples=True,
                         **{k: v[idx] if isinstance(v, np.ndarray) else v for k, v in kw.items()})
    assert np.array_equal(stats(big), stats(host)[idx]) and np.array_equal(big.samples, host.samples[idx])
    # device pointers on torch's stream
    L = _lib.load()
    sig = np.ascontiguousarray(np.concatenate([kw["z0_sigma"], kw["param_sigma"], kw["tf_sigma"][:, None]], axis=1).T)
    sig_u = np.full((K, B), kw["control_sigma"])
    pt, bt, xt, st, ut = (torch.from_numpy(np.array(a)).cuda() for a in (P, blob, xi, sig, sig_u))
    out = torch.empty((82, B), dtype=torch.float64, device="cuda")
    smp = torch.empty((9, S, B), dtype=torch.float64, device="cuda")
    o = _opts(nt, 0, 1.0, 0, 0.0)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.ascent_disperse_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), 0, S, xt.data_ptr(), st.data_ptr(), ut.data_ptr(),
                                       out.data_ptr(), smp.data_ptr(), 0, C.c_void_p(stream), 1))
    torch.cuda.synchronize()
    s = out.cpu().numpy().T
    assert np.array_equal(s[:, 0], host.n_valid) and np.array_equal(s[:, 1:10], host.nominal) and np.array_equal(s[:, 10:19], host.mean)
    assert np.array_equal(s[:, 19:64], host.cov[:, np.triu_indices(9)[0], np.triu_indices(9)[1]])
    assert np.array_equal(s[:, 64:73], host.min) and np.array_equal(s[:, 73:82], host.max)
    assert np.array_equal(smp.cpu().numpy().transpose(2, 1, 0), host.samples)


def test_invalid_samples_are_left_out():
    """A NaN in xi's thrust row for one sample, nothing provoked: problems with sigma_Ft != 0 report n = samples - 1 and their
    statistics are those of the run without that sample, to the bounds of the reduction test; a problem of the same batch with
    sigma_Ft = 0 reports n = samples and is untouched bit for bit."""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch
    nt, K, S, bad = 18, 17, 300, 131
    P, blob = _solved(nt, 0, 0)
    kw = _sigmas(P)
    kw["param_sigma"][1, 3] = 0.0
    xi = _xi(K, S, 9)
    clean = disperse_batch(P, blob, nt, xi=xi, keep_samples=True, substeps=2, **kw)
    xn = xi.copy()
    xn[7 + 3, bad] = np.nan
    d = disperse_batch(P, blob, nt, xi=xn, keep_samples=True, substeps=2, **kw)
    assert d.n_valid[0] == S - 1 and d.n_valid[1] == S and not np.isfinite(d.samples[0, bad]).all()
    keep = np.arange(S) != bad
    assert np.array_equal(d.samples[0, keep], clean.samples[0, keep])
    _check_statistics(d, 0, clean.samples[0, keep])
    for a in ("n_valid", "nominal", "mean", "cov", "min", "max", "samples"):
        assert np.array_equal(getattr(d, a)[1], getattr(clean, a)[1]), a


def test_a_blob_without_a_final_time_gives_no_valid_sample():
    """t_f = NaN in one blob of two: the call returns ASCENT_OK, that problem has n = 0 and NaN statistics (its nominal rows are
    NaN as well), the other is untouched bit for bit."""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch
    nt, K = 18, 17
    P, blob = _solved(nt, 0, 0)
    kw = _sigmas(P)
    xi = _xi(K, 65, 10)
    good = disperse_batch(P, blob, nt, xi=xi, substeps=2, **kw)
    b = np.array(blob)
    b[21 * K, 0] = np.nan
    d = disperse_batch(P, b, nt, xi=xi, keep_samples=True, **kw)
    assert d.n_valid[0] == 0 and np.isnan(d.mean[0]).all() and np.isnan(d.cov[0]).all() and np.isnan(d.min[0]).all() and np.isnan(d.max[0]).all()
    assert np.isnan(d.nominal[0, :4]).all() and not np.isfinite(d.samples[0]).all(axis=1).any()
    d2 = disperse_batch(P, b, nt, xi=xi, substeps=2, **kw)
    for a in ("n_valid", "nominal", "mean", "cov", "min", "max"):
        assert np.array_equal(getattr(d2, a)[1], getattr(good, a)[1]), a


def _linear_mismatch(cov, lin):
    """largest |cov - lin|_ij / sqrt(cov_ii cov_jj) over the rows that vary at all"""
    sd = np.sqrt(np.diag(cov))
    on = sd > 0
    assert np.all(lin[~on][:, ~on] == 0.0)
    return float(np.max(np.abs(cov - lin)[np.ix_(on, on)] / np.outer(sd[on], sd[on])))


@functools.lru_cache(maxsize=None)
def _reference_covariances(rel, nt=18, scheme=0, form=0):
    """entirely on the CPU, on the blob of (nt, scheme, form), problem 0, the xi of the tests below: dispersion_reference's
    samples and covariance, and the linear covariance from flight_jacobian_reference"""
    K = nt - 1
    P, blob = _solved(nt, scheme, form)
    xi = _xi(K, 256, 12)
    kw = _sigmas(P, rel)
    ref = _reference(P, blob, nt, xi, kw, form, 2, 0)
    assert ref["stats"][0] == 256           # the reference keeps every sample at this sigma
    cov = np.zeros((9, 9))
    cov[dr.IU] = ref["stats"][19:64]
    cov = cov + cov.T - np.diag(np.diag(cov))
    J = jr.jacobian(P[0], blob[:, 0], nt, form, 2)
    A = np.concatenate([J["jac"] * np.concatenate([kw["z0_sigma"][0], kw["param_sigma"][0], [kw["tf_sigma"][0]]]), J["jac_u"] * rel], axis=1)
    return dict(cov=cov, lin=A @ np.cov(xi) @ A.T, rng=ref["samples"].max(axis=0) - ref["samples"].min(axis=0))


def _reference_linear_mismatch(rel, nt=18, scheme=0, form=0):
    r = _reference_covariances(rel, nt, scheme, form)
    return _linear_mismatch(r["cov"], r["lin"])


@pytest.mark.parametrize("rel", [1e-3, 1e-5])
@pytest.mark.parametrize("nt,scheme,form", CASES)
def test_covariance_matches_the_reference_on_the_same_blob(nt, scheme, form, rel):
    """The device's covariance against the CPU reference's on the same blob, same xi, same sigma (problem 0), entry by entry.
    The bound follows from two bounds this file already holds.  Every device sample is within d_i = 1e-10 (times r_peri for the
    altitudes) of the reference's (SAMPLE_BOUND), so with e the difference of the samples, cov(x + e) - cov(x) = cov(e, x) +
    cov(x, e) + cov(e, e), and by Cauchy-Schwarz with sd(e_i) <= d_i sqrt(n / (n - 1)):
        |cov_dev - cov_ref|_ij <= 1.01 (d_i sd_j + d_j sd_i + d_i d_j);
    the device's reduction adds 1e-11 range_i range_j (the bound of the reduction test).  sd and range are the reference's.
    At rel = 1e-5 this is 1e-5 of sd_i sd_j for the rows that vary least, 5e-9 for those that vary most.  The agreement of the
    mismatch against the linear prediction (the quantity of the test below) is recorded beside it."""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch, flight_jacobian
    P, blob = _solved(nt, scheme, form)
    r = _reference_covariances(rel, nt, scheme, form)
    kw = dict(scheme=scheme, formulation=form, substeps=2)
    d = disperse_batch(P, blob, nt, xi=_xi(nt - 1, 256, 12), **kw, **_sigmas(P, rel))
    assert d.n_valid[0] == 256
    sd = np.sqrt(np.diag(r["cov"]))
    dl = np.full(9, SAMPLE_BOUND)
    dl[7:] *= P[0, 9]
    bound = 1.01 * (np.outer(dl, sd) + np.outer(sd, dl) + np.outer(dl, dl)) + 1e-11 * np.outer(r["rng"], r["rng"])
    err = np.abs(d.cov[0] - r["cov"])
    lin = d.linear_covariance(flight_jacobian(P, blob, nt, **kw))[0]
    on = sd > 0
    scale = np.outer(sd[on], sd[on])
    fig = dict(cov_error_over_bound=float(np.max(err / np.where(bound > 0, bound, 1.0))),
               cov_error_over_sd_sd=float(np.max(err[np.ix_(on, on)] / scale)),
               linear_error_over_sd_sd=float(np.max(np.abs(lin - r["lin"])[np.ix_(on, on)] / scale)),
               mismatch_device=_linear_mismatch(d.cov[0], lin), mismatch_reference=_linear_mismatch(r["cov"], r["lin"]))
    PARITY["covariance_vs_reference"][f"rel{rel:g}_nt{nt}_scheme{scheme}_form{form}"] = fig
    print(nt, scheme, form, "rel", rel, "covariance against the reference's on the same blob:", fig)
    assert np.all(err <= bound), (err, bound)


@pytest.mark.parametrize("rel", [1e-3, 1e-5])
@pytest.mark.parametrize("nt,scheme,form", CASES)
def test_covariance_against_the_linear_prediction(nt, scheme, form, rel):
    """256 samples at the sigma of the sample test (rel = 1e-3) and at a hundredth of it: cov against
    linear_covariance(flight_jacobian(...)) entry by entry, relative to sqrt(cov_ii cov_jj), within 10 x the same quantity
    measured on the CPU (dispersion_reference against flight_jacobian_reference, same xi).  Every one of the 256 samples must be
    valid.

    rel = 1e-3: the CPU figure is taken at nt = 18, (0, 0) -- the remainder is second order in sigma and 10 x leaves room for the
    other cases' curvature.  There the dispersion is far from linear (the z_0 sigma carries an angular rate of 1e-3 (scaled) that
    turns the thrust by some 0.4 rad (scaled) over the burn), the reference's own mismatch is 3.0 and the check is weak.

    rel = 1e-5: the CPU figure is taken on the case's own blob.  The curvature does not carry over from one blob to another at
    this size: the trapezoidal and Hermite-Simpson solutions burn out so close to the flown apoapsis, where the apoapsis altitude
    has no linear term in the radial velocity, that its variance is second order even at 1e-5 (entry (8, 8): 0.77 .. 0.89 on
    the CPU, 0.18 still at 1e-6), where backward Euler's gives 0.021 and the formulation-1 blob 5.5e-4.  The factor 10 is kept.
    Neither bound is sharp; the sharp check of the same covariance is the test above."""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch, flight_jacobian
    P, blob = _solved(nt, scheme, form)
    K = nt - 1
    own = rel != REL
    bound_ref = _reference_linear_mismatch(rel, nt, scheme, form) if own else _reference_linear_mismatch(rel)
    kw = dict(scheme=scheme, formulation=form, substeps=2)
    d = disperse_batch(P, blob, nt, xi=_xi(K, 256, 12), **kw, **_sigmas(P, rel))
    assert (d.n_valid == 256).all()
    lin = d.linear_covariance(flight_jacobian(P, blob, nt, **kw))
    worst = max(_linear_mismatch(d.cov[j], lin[j]) for j in range(2))
    name = f"reference_nt{nt}_scheme{scheme}_form{form}" if own else "reference_nt18_scheme0_form0"
    PARITY["covariance_vs_linear"][f"rel{rel:g}_nt{nt}_scheme{scheme}_form{form}"] = {"device": worst, name: bound_ref}
    print(nt, scheme, form, "rel", rel, "covariance against the linear prediction: device", worst, name, bound_ref)
    assert worst <= 10.0 * bound_ref


def test_front_ends_agree_and_terminal_2_is_accepted():
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch, solve_batch
    nt = 18
    P = _points(2)
    r = solve_batch(P, nt, want_blob=True)
    assert (r.status == 0).all()
    kw = dict(param_sigma=dr.relative_sigma(P[0])[7:23], control_sigma=1e-3, samples=100, seed=4)
    a, b = r.disperse(**kw), disperse_batch(P, r.blob, nt, **kw)
    assert a.xi.shape == (24 + nt - 1, 100) and np.array_equal(a.xi, np.random.default_rng(4).standard_normal((24 + nt - 1, 100)))
    for f in ("n_valid", "nominal", "mean", "cov", "min", "max", "xi", "param_sigma", "control_sigma", "tf_sigma", "z0_sigma"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.samples is None and (a.n_valid == 100).all() and np.all(a.std[:, :4] > 0) and a.std.shape == (2, 9)
    assert np.all(a.tf_sigma == 0.0) and np.all(a.z0_sigma == 0.0) and a.param_sigma.shape == (2, 16) and a.control_sigma.shape == (2, nt - 1)
    # without its blob a result disperses the blob rebuilt from its trajectory: the same flight
    r2 = solve_batch(P, nt)
    c = r2.disperse(**kw)
    assert np.array_equal(c.mean, a.mean) and np.array_equal(c.cov, a.cov)
    t2 = disperse_batch(P, r.blob, nt, terminal=2, **kw)
    assert np.array_equal(t2.mean, a.mean) and np.array_equal(t2.cov, a.cov)


def test_the_example_disperses():
    """examples/apollo11.py --disperse trims the solved model's blob, disperses it and prints both 1-sigmas."""
    import importlib.util
    import io
    from contextlib import redirect_stdout
    spec = importlib.util.spec_from_file_location("apollo11_example_disperse", os.path.join(ROOT, "examples", "apollo11.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    m, _, _ = ex.build()
    out = io.StringIO()
    with redirect_stdout(out):
        m.solve(disp=False)
        d = ex.disperse(m, 0)
    text = out.getvalue()
    print(text)
    assert d.n_valid[0] == 1024 and "Monte Carlo 1-sigma" in text and "periapsis" in text and "apoapsis" in text
    assert np.all(d.std[0, 7:] > 0) and abs(d.nominal[0, 8] - 17703.0) <= 0.05
