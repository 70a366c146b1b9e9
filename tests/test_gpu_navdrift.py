"""The time-varying navigation error on the GPU (ascent_disperse_drifting_batch, ascent_covariance_drifting_batch): frozen
channels give the parent calls' bits, every sample against the CPU reference (tests/navdrift_reference.py) flown with the
device's own gains, the reduction against numpy, the impulse response of the flight kernel against the noise model the covariance
kernel sums, the covariance kernel against the reference's superposition, the bitwise promises of the header, bounded garbage.

The cases are five of gpu_cases.CASES at q = 1e6 and the K = 17 backward-Euler one at q = 1e12 as well, navigated with
the feed-forward of the thrust, substeps = 2, two problems, 300 samples.  The entry points are called through ctypes, because
phi and q are set directly: a random walk (phi = 1, q > 0) has no time constant.  Bounds that depend on the conditioning of the
case are computed here from the reference alone -- its float64 run against its longdouble run -- never from the device.  The
differences seen are collected in PARITY; with ASCENT_NAVDRIFT_PARITY_OUT=<file> they are written there as JSON when the module
is done (profiles/navdrift_parity.json is such a file)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import guidance_reference as gr
import lincov_reference as lr
import navdrift_reference as nd
from gpu_cases import (FD_STEPS, FLOOR, M, SAMPLE_BOUND, case as _case, col_scales as _col_scales, gains as _gains,
                       norm_cov as _norm_cov, norm_jac as _norm_jac, parity_writer, ptr as _ptr, same as _same,
                       scaled_error as _scaled_error, sigmas as _sigmas, weights as _weights, xi as _xi)

pytestmark = pytest.mark.gpu

PARITY = {"samples_vs_reference": {}, "impulse_response": {}, "corridor_vs_reference": {}}
CASES = [(3, 0, 0, 1e6), (18, 0, 0, 1e6), (18, 2, 0, 1e6), (18, 0, 1, 1e6), (34, 0, 0, 1e6), (18, 0, 0, 1e12)]
S = 300                    # not a multiple of the wavefront or the workgroup, and more than one workgroup
LD = np.longdouble
# the channel mix: stationary | decaying | frozen | zero-start random walk | phi = 0 | zero-start | frozen | stationary (theta-hat)
PHI = np.array([0.9, 0.5, 1.0, 1.0, 0.0, 0.97, 1.0, 0.7])
START = np.array([1.0, 2.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0])          # sigma_nav in units of the case's sigma
DRIVE = np.array([np.sqrt(1 - 0.81), 0.0, 0.0, 0.3, 1.0, 0.2, 0.0, np.sqrt(1 - 0.49)])
FROZEN = (PHI == 1.0) & (DRIVE == 0.0)
_write_parity = parity_writer("ASCENT_NAVDRIFT_PARITY_OUT", PARITY)


def _rel(q):
    """the relative sigma of a case: small enough that no command of the reference comes near the clip (asserted there)"""
    return 1e-6 if q <= 1e6 else 1e-9


def _inputs(P, nt, q, rel=None, control=True):
    """the sigma arrays of a case as the C ABI takes them: sigma [24][B], sigma_u [K][B], sigma_nav, phi, q [8][B]"""
    rel = _rel(q) if rel is None else rel
    B, K = P.shape[0], nt - 1
    kw = _sigmas(P, rel)
    sig = np.ascontiguousarray(np.concatenate([kw["z0_sigma"], kw["param_sigma"], kw["tf_sigma"][:, None]], axis=1).T)
    unit = np.concatenate([np.full((B, 7), rel), rel * np.abs(P[:, 3:4])], axis=1)          # scaled units; the thrust for theta-hat
    return dict(sigma=sig, sigma_u=np.full((K, B), rel) if control else None, sigma_nav=np.ascontiguousarray((unit * START).T),
                phi=np.ascontiguousarray(np.tile(PHI, (B, 1)).T), q=np.ascontiguousarray((unit * DRIVE).T))


def _draws(K, samples=S):
    r = np.random.default_rng(17)
    om = r.standard_normal((8, K, samples))
    om[FROZEN | (DRIVE == 0.0)] = np.nan          # rows that must not be read
    return _xi(K, samples), r.standard_normal((8, samples)), om


def _law_arrays(g, K, B):
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _feedback_arrays, _feedforward_arrays
    return _feedback_arrays(g, K, B) + _feedforward_arrays(g, K, B)


def _mc(P, blob, nt, scheme, form, g, xi, xi_nav, om, inp, stride=1, optional=True, parent=False, drift=True, substeps=M):
    """ascent_disperse_drifting_batch (parent: ascent_disperse_history_batch; drift False: phi, q and the draws null) with host
    pointers -> dict(stats (82, B), samples (12, S, B), hist (52, NJ, B), hist_samples (10, NJ, S, B)); optional False: the two
    optional outputs null"""
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts, history_nodes
    L = _lib.load()
    B, K, Sx = P.shape[0], nt - 1, xi.shape[1]
    o = _opts(nt, 0, 1.0, 0, 0.0, scheme, form)
    NJ = len(history_nodes(K, stride))
    out = dict(stats=np.full((82, B), 7.25), samples=np.full((12, Sx, B), 7.25) if optional else None, hist=np.full((52, NJ, B), 7.25),
               hist_samples=np.full((10, NJ, Sx, B), 7.25) if optional else None)
    law = [np.ascontiguousarray(a) if a is not None else None for a in _law_arrays(g, K, B)]
    keep = [np.ascontiguousarray(a) if a is not None else None for a in (P, blob, xi, inp["sigma"], inp["sigma_u"], xi_nav, inp["sigma_nav"],
                                                                         inp["phi"], inp["q"], om)]
    Pc, bc, xc, sg, su, xn, sn, ph, qq, omc = keep
    head = [_ptr(Pc), B, C.byref(o), _ptr(bc), substeps, Sx, _ptr(xc), _ptr(sg), _ptr(su)] + [_ptr(a) for a in law] + [_ptr(xn), _ptr(sn)]
    tail = [stride, _ptr(out["stats"]), _ptr(out["samples"]), _ptr(out["hist"]), _ptr(out["hist_samples"]), 0, None, 0]
    if parent:
        _lib.check(L.ascent_disperse_history_batch(*head, *tail))
    else:
        _lib.check(L.ascent_disperse_drifting_batch(*head, *([_ptr(ph), _ptr(qq), _ptr(omc)] if drift else [None] * 3), *tail))
    return out


def _lc(P, blob, nt, scheme, form, g, inp, stride=1, jac=True, parent=False, drift=True, substeps=M):
    """ascent_covariance_drifting_batch likewise -> dict(nominal (10, NJ, B), cov (55, NJ, B), jac (10, 32, NJ, B))"""
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts, history_nodes
    L = _lib.load()
    B, K = P.shape[0], nt - 1
    o = _opts(nt, 0, 1.0, 0, 0.0, scheme, form)
    NJ = len(history_nodes(K, stride))
    out = dict(nominal=np.full((10, NJ, B), 7.25), cov=np.full((55, NJ, B), 7.25), jac=np.full((10, 32, NJ, B), 7.25) if jac else None)
    law = [np.ascontiguousarray(a) if a is not None else None for a in _law_arrays(g, K, B)]
    keep = [np.ascontiguousarray(a) if a is not None else None for a in (P, blob, inp["sigma"], inp["sigma_u"], inp["sigma_nav"], inp["phi"], inp["q"])]
    Pc, bc, sg, su, sn, ph, qq = keep
    head = [_ptr(Pc), B, C.byref(o), _ptr(bc), substeps, _ptr(sg), _ptr(su)] + [_ptr(a) for a in law] + [_ptr(sn)]
    tail = [stride, _ptr(out["nominal"]), _ptr(out["cov"]), _ptr(out["jac"]), 0, None, 0]
    if parent:
        _lib.check(L.ascent_covariance_history_batch(*head, *tail))
    else:
        _lib.check(L.ascent_covariance_drifting_batch(*head, *([_ptr(ph), _ptr(qq)] if drift else [None] * 2), *tail))
    return out


@pytest.mark.parametrize("nt,scheme,form,q", CASES)
def test_frozen_is_the_parents_bits(nt, scheme, form, q):
    """phi = 1 and q = 0 through the new kernels, and the arrays null, against ascent_disperse_history_batch and
    ascent_covariance_history_batch on the same inputs: every output array, NaN positions included; the draws are all NaN"""
    P, blob = _case(nt, scheme, form)
    K = nt - 1
    g = _gains(nt, scheme, form, "navigated", q)
    inp = _inputs(P, nt, q)
    frozen = dict(inp, phi=np.ones_like(inp["phi"]), q=np.zeros_like(inp["q"]))
    xi, xn, _ = _draws(K)
    nan = np.full((8, K, S), np.nan)
    base = _mc(P, blob, nt, scheme, form, g, xi, xn, None, inp, parent=True)
    assert np.isfinite(base["hist_samples"]).all() and not np.any(base["stats"] == 7.25)
    assert _same(_mc(P, blob, nt, scheme, form, g, xi, xn, nan, frozen), base)
    assert _same(_mc(P, blob, nt, scheme, form, g, xi, xn, None, inp, drift=False), base)
    for control in (True, False):
        inp = _inputs(P, nt, q, 1e-3, control)
        frozen = dict(inp, phi=np.ones_like(inp["phi"]), q=np.zeros_like(inp["q"]))
        base = _lc(P, blob, nt, scheme, form, g, inp, parent=True)
        assert np.isfinite(base["cov"]).all()
        assert _same(_lc(P, blob, nt, scheme, form, g, frozen), base)
        assert _same(_lc(P, blob, nt, scheme, form, g, inp, drift=False), base)


def _moments(n_valid, mean, second, lo, hi, v, what):
    """Count, mean, variance (or covariance) and extrema of the device against the rows v (samples, rows) it reduced, with the
    bounds of tests/test_gpu_history.py: count and extrema exact, means within 1e-11 of the range, second moments within 1e-11 of
    the product of the ranges.  The sigmas of this module are small (no command may come near the clip), so the range of a row
    can be 1e-11 of the row itself: the moments of v are formed in longdouble, so that numpy's own rounding stays out, and a mean
    is allowed the one unit in its last place that it cannot do without as a float64.  -> the worst error over its bound"""
    ok = np.isfinite(v).all(axis=1)
    v = v[ok].astype(LD)
    assert n_valid == len(v) == len(ok), what          # every sample of these cases is valid
    assert np.array_equal(lo, v.min(axis=0).astype(np.float64)) and np.array_equal(hi, v.max(axis=0).astype(np.float64)), what
    rng = (v.max(axis=0) - v.min(axis=0)).astype(np.float64)
    m = v.mean(axis=0)
    em = np.abs(mean - m).astype(np.float64)
    bm = 1e-11 * rng + np.spacing(np.abs(mean))
    assert np.all(em <= bm), (what, em, bm)
    worst = float((em / bm).max())
    c = (v - m).T @ (v - m) / (len(v) - 1)
    if second.ndim == 1:
        c, br = np.diagonal(c), 1e-11 * rng * rng
    else:
        br = 1e-11 * rng[:, None] * rng[None, :]
    ec = np.abs(second - c).astype(np.float64)
    assert np.all(ec <= br), (what, ec, br)
    return max(worst, float(np.max(np.divide(ec, br, out=np.zeros_like(ec), where=br > 0))))


def _reference_args(P, blob, nt, g, j, xi, xn, om, inp, n=None):
    K = nt - 1
    sl = slice(None) if n is None else slice(0, n)
    return [P[j], blob[:, j], nt, xi[:, sl], inp["sigma"][:, j], None if inp["sigma_u"] is None else inp["sigma_u"][:, j], g.gain_u[j], g.gain_t[j],
            float(g.stretch_max[j]), g.ff_u[j], float(g.ff_t[j]), g.ff_know[j], xn[:, sl], inp["sigma_nav"][:, j], inp["phi"][:, j], inp["q"][:, j],
            np.nan_to_num(om[:, :, sl], nan=0.0)]


@pytest.mark.parametrize("nt,scheme,form,q", CASES)
def test_samples_match_reference_and_the_reduction_matches_numpy(nt, scheme, form, q):
    """hist_samples_out at stride 1 against navdrift_reference.history_drifting in longdouble, all 300 samples of both problems.
    Bound, the project's convention: the larger of 1e-10 and 100 x the reference's own float64-against-longdouble difference (on
    the first 40 samples: fewer samples can only lower the bound), in lincov_reference.row_scales.  No command of the reference is
    within 1e-6 of the clip, so no sample is excluded and row 51 is zero.  Then hist_out and stats_out against the moments of the
    device's own samples (_moments: the bounds of tests/test_gpu_history.py)."""
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _cov_from_upper, _history_result
    P, blob = _case(nt, scheme, form)
    K = nt - 1
    g = _gains(nt, scheme, form, "navigated", q)
    inp = _inputs(P, nt, q)
    xi, xn, om = _draws(K)
    dev = _mc(P, blob, nt, scheme, form, g, xi, xn, om, inp)
    h = _history_result(K, 1, dev["hist"], dev["hist_samples"])
    st = dev["stats"].T
    d = types.SimpleNamespace(history=h, n_valid=st[:, 0].astype(np.int64), mean=st[:, 10:19], cov=_cov_from_upper(st[:, 19:64]), min=st[:, 64:73],
                              max=st[:, 73:82], samples=np.ascontiguousarray(dev["samples"][:9].transpose(2, 1, 0)))
    assert (h.n_valid == S).all() and (h.clipped == 0).all()
    name, fig = f"nt{nt}_scheme{scheme}_form{form}_q{q:g}", {}
    for j in range(P.shape[0]):
        refl = nd.history_drifting(*_reference_args(P, blob, nt, g, j, xi, xn, om, inp), formulation=form, substeps=M, dtype=LD)
        assert refl["margin"].min() > 1e-6 and not refl["clipped"].any(), refl["margin"].min()
        n = 40
        ref = nd.history_drifting(*_reference_args(P, blob, nt, g, j, xi, xn, om, inp, n), formulation=form, substeps=M)
        rows = lr.row_scales(P[j], g.gain_u[j], g.ff_u[j], K)
        gap = _scaled_error(ref["samples"], refl["samples"][:n].astype(np.float64), P[j, 9], rows[:, 8])
        bound = max(SAMPLE_BOUND, 100.0 * gap)
        err = _scaled_error(h.samples[j], refl["samples"].astype(np.float64), P[j, 9], rows[:, 8])
        drift = float(np.abs(refl["n"][:, 1:, :].astype(np.float64) - refl["n"][:, :1, :].astype(np.float64)).max(axis=(0, 1))[~FROZEN].min())
        fig[f"problem{j}"] = dict(device_error=err, reference_gap=gap, bound=bound, smallest_margin=float(refl["margin"].min()),
                                  hist_statistics_error_over_bound=max(_moments(h.n_valid[j, i], h.mean[j, i], h.var[j, i], h.min[j, i], h.max[j, i], h.samples[j, :, i],
                                                                                            (name, j, "node", i + 1)) for i in range(K)),
                                  stats_error_over_bound=_moments(d.n_valid[j], d.mean[j], d.cov[j], d.min[j], d.max[j], d.samples[j], (name, j, "end")))
        print(name, "problem", j, fig[f"problem{j}"])
        assert drift > 0.0
    PARITY["samples_vs_reference"][name] = fig
    for k, v in fig.items():
        assert v["device_error"] <= v["bound"], (name, k, v)


def test_impulse_response_of_the_flight_kernel_is_the_noise_model():
    """nt = 18, q = 1e6, every sigma zero: sample pairs whose xi_drift is +-1 at one (a, k) and zero elsewhere, every channel at the
    first step, the chunk boundary of the covariance sweep (k = 16) and the last step, q_a = h of the channel's scale for every h
    of gpu_cases.FD_STEPS.  The central difference, the best step taken per entry, against the reference's r_jak (longdouble
    complex-step records).  Bound: 10 x what the reference's own float64 flight pairs (navdrift_reference.history_drifting) show by the
    same measure, from problem 0.  The flight kernel knows nothing of the covariance kernel: this ties the two noise models."""
    nt, scheme, form, q = 18, 0, 0, 1e6
    K = nt - 1
    P, blob = _case(nt, scheme, form)
    B = P.shape[0]
    g = _gains(nt, scheme, form, "navigated", q)
    pairs = [(a, k) for a in range(8) for k in (1, 16, K)]
    Sx = 2 * len(pairs)
    om = np.zeros((8, K, Sx))
    for i, (a, k) in enumerate(pairs):
        om[a, k - 1, 2 * i], om[a, k - 1, 2 * i + 1] = 1.0, -1.0
    phi = np.where(FROZEN, 0.8, PHI)                        # every channel drifts here
    unit = np.concatenate([np.ones((B, 7)), np.abs(P[:, 3:4])], axis=1)
    xi, xn = np.zeros((24 + K, Sx)), np.zeros((8, Sx))
    zero = dict(sigma=np.zeros((24, B)), sigma_u=None, sigma_nav=np.zeros((8, B)), phi=np.ascontiguousarray(np.tile(phi, (B, 1)).T))

    def best(fd_by_h, want, rows):
        d = np.min([np.abs(fd - want) for fd in fd_by_h], axis=0) / rows[:, :, None]
        return float(d.max())

    dev_fd = {j: [] for j in range(B)}
    ref_fd = []
    for h in FD_STEPS:
        inp = dict(zero, q=np.ascontiguousarray((unit * h).T))
        out = _mc(P, blob, nt, scheme, form, g, xi, xn, om, inp)
        assert (out["hist"][51] == 0).all() and (out["hist"][0] == Sx).all()
        for j in range(B):
            smp = out["hist_samples"][:, :, :, j].transpose(2, 1, 0)          # (S, K, 10)
            dev_fd[j].append((smp[0::2] - smp[1::2]).transpose(1, 2, 0) / (2.0 * h * unit[j][[a for a, _ in pairs]]))
        r = nd.history_drifting(*_reference_args(P, blob, nt, g, 0, xi, xn, om, inp), formulation=form, substeps=M)["samples"]
        ref_fd.append((r[0::2] - r[1::2]).transpose(1, 2, 0) / (2.0 * h * unit[0][[a for a, _ in pairs]]))
    fig = {}
    for j in range(B):
        law = dict(gain_u=g.gain_u[j], gain_t=g.gain_t[j], smax=float(g.stretch_max[j]), ff_u=g.ff_u[j], ff_t=float(g.ff_t[j]), know=g.ff_know[j])
        ref = nd.corridor_drifting(P[j], blob[:, j], nt, np.zeros(24), None, phi=phi, q=np.ones(8), formulation=form, substeps=M, dtype=LD, **law)
        want = np.stack([ref["r_om"][:, :, a, k - 1] for a, k in pairs], axis=2).astype(np.float64)          # (K, 10, pairs), per unit n
        rows = lr.row_scales(P[j], g.gain_u[j], g.ff_u[j], K) / 1.0
        # per unit of the channel's own scale, as the Jacobian's columns are compared
        sc = unit[j][[a for a, _ in pairs]]
        if j == 0:
            bound = 10.0 * best([f * sc for f in ref_fd], want * sc, rows)
        fig[f"problem{j}"] = dict(device_difference=best([f * sc for f in dev_fd[j]], want * sc, rows), largest_entry=float(np.abs(want * sc / rows[:, :, None]).max()))
    fig["bound"] = bound
    print(fig)
    PARITY["impulse_response"] = fig
    for j in range(B):
        assert fig[f"problem{j}"]["device_difference"] <= bound, fig


@functools.lru_cache(maxsize=None)
def _compared(nt, scheme, form, q):
    """The stride-1 corridor of a case against the longdouble reference at unit relative sigmas: every sigma one unit of its
    column's scale (test_gpu_lincov._unit_sigmas), sigma_u = 1, the initial knowledge errors and the steady sigmas behind q one
    unit as well.  noise: only sigma_u and the drift on; drift: only the drift on, so that an error in C or D cannot hide behind Q."""
    P, blob = _case(nt, scheme, form)
    B, K = P.shape[0], nt - 1
    g = _gains(nt, scheme, form, "navigated", q)
    cs = np.array([_col_scales(p) for p in P])
    full = dict(sigma=np.ascontiguousarray(cs[:, :24].T), sigma_u=np.ones((K, B)), sigma_nav=np.ascontiguousarray((cs[:, 24:] * START).T),
                phi=np.ascontiguousarray(np.tile(PHI, (B, 1)).T), q=np.ascontiguousarray((cs[:, 24:] * DRIVE).T))
    noise = dict(full, sigma=np.zeros((24, B)), sigma_nav=None)
    drift = dict(noise, sigma_u=None)
    dev = {k: _lc(P, blob, nt, scheme, form, g, v, jac=k == "full") for k, v in (("full", full), ("noise", noise), ("drift", drift))}
    iu = np.triu_indices(10)

    def square(c):
        m = np.zeros((K, 10, 10))
        m[:, iu[0], iu[1]] = c
        m[:, iu[1], iu[0]] = c
        return m
    fig = {}
    for j in range(B):
        law = dict(gain_u=g.gain_u[j], gain_t=g.gain_t[j], smax=float(g.stretch_max[j]), ff_u=g.ff_u[j], ff_t=float(g.ff_t[j]), know=g.ff_know[j])
        rows = lr.row_scales(P[j], g.gain_u[j], g.ff_u[j], K)
        out = {}
        ref = {}
        for dt in (np.float64, LD):
            rec = gr.records(P[j], blob[:, j], nt, form, M, dt)
            ref[dt] = {k: nd.corridor_drifting(P[j], blob[:, j], nt, v["sigma"][:, j], None if v["sigma_u"] is None else v["sigma_u"][:, j],
                                               sigma_nav=None if v["sigma_nav"] is None else v["sigma_nav"][:, j], phi=v["phi"][:, j], q=v["q"][:, j],
                                               formulation=form, substeps=M, dtype=dt, rec=rec, **law)
                       for k, v in (("full", full), ("noise", noise), ("drift", drift))}
        for name, key, of_ref, of_dev, norm in (("jacobian", "full", "S", dev["full"]["jac"][:, :, :, j].transpose(2, 0, 1), lambda a: _norm_jac(a, rows, cs[j])),
                                                ("covariance", "full", "cov", square(dev["full"]["cov"][:, :, j].T), lambda a: _norm_cov(a, rows)),
                                                ("noise", "noise", "cov", square(dev["noise"]["cov"][:, :, j].T), lambda a: _norm_cov(a, rows)),
                                                ("drift", "drift", "cov", square(dev["drift"]["cov"][:, :, j].T), lambda a: _norm_cov(a, rows))):
            want = norm(ref[LD][key][of_ref])
            gap = float(np.abs(norm(ref[np.float64][key][of_ref]) - want).max())
            assert np.isfinite(of_dev).all()
            out[name] = dict(device_error=float(np.abs(norm(of_dev) - want).max()), reference_gap=gap, bound=max(FLOOR, 100.0 * gap),
                             largest_entry=float(np.abs(want).max()))
        fig[f"problem{j}"] = out
        print(nt, scheme, form, q, "problem", j, out)
    PARITY["corridor_vs_reference"][f"nt{nt}_scheme{scheme}_form{form}_q{q:g}"] = fig
    return dev, fig


@pytest.mark.parametrize("nt,scheme,form,q", CASES)
def test_jacobian_and_covariance_match_reference(nt, scheme, form, q):
    """jac_hist_out, cov_out, the noise-only covariance and the drift-only covariance (control_sigma null) at stride 1 against
    navdrift_reference.corridor_drifting in longdouble, which forms the drift's part by superposition and never carries C or D.
    Bound: the larger of 1e-10 and 100 x the reference's own float64-against-longdouble gap, in the scales of
    tests/test_gpu_lincov.py; the gap is recorded.  cov_out holds the upper triangle only, so the exact symmetry of Q inside the
    kernel cannot be observed through the ABI: it holds by construction (one lane forms both halves of an entry and stores their
    average to both places), and what is checked here is the upper triangle against the reference."""
    dev, fig = _compared(nt, scheme, form, q)
    for k, v in fig.items():
        for name, f in v.items():
            assert f["device_error"] <= f["bound"], (k, name, f)
        assert v["drift"]["largest_entry"] > 1e3 * v["drift"]["bound"], (k, v["drift"])          # frozen, this covariance is zero


def _mc_all(o):
    return np.concatenate([o["hist"].transpose(2, 1, 0)] + ([] if o["hist_samples"] is None else [o["hist_samples"].transpose(3, 1, 0, 2).reshape(
        o["hist"].shape[2], o["hist"].shape[1], -1)]), axis=2)


def _lc_all(o):
    return np.concatenate([o["nominal"].transpose(2, 1, 0), o["cov"].transpose(2, 1, 0)] + ([] if o["jac"] is None else [
        o["jac"].transpose(3, 2, 0, 1).reshape(o["cov"].shape[2], o["cov"].shape[1], -1)]), axis=2)


def test_a_nodes_rows_do_not_depend_on_stride_batch_pointers_or_optional_outputs():
    """nt = 34 (three chunks), five problems, all channels of the mix drifting: strides 4 (the last node is not a multiple) and K
    against stride 1; each problem alone and through a batch of 70; without the optional outputs; device pointers on torch's
    stream.  Bitwise, both calls."""
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult, _lib, guidance_gains
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts, history_nodes
    nt, K, B, q = 34, 33, 5, 1e6
    P, blob = _case(nt, 0, 0, 5)
    g = guidance_gains(P, blob, nt, substeps=M, want_jacobian=False, feedforward="Ft", **_weights(q))
    assert (g.status == 0).all()
    sub = lambda idx: GuidanceResult(g.gain_u[idx], g.gain_t[idx], g.summary[idx], g.stretch_max[idx], None, g.ff_u[idx], g.ff_t[idx],
                                     g.ff_dir[idx], g.ff_know[idx])
    inp = _inputs(P, nt, q)
    take = lambda idx: {k: None if v is None else np.ascontiguousarray(v[:, idx]) for k, v in inp.items()}
    xi, xn, om = _draws(K, 70)
    mc1, lc1 = _mc(P, blob, nt, 0, 0, g, xi, xn, om, inp), _lc(P, blob, nt, 0, 0, g, inp)
    assert np.isfinite(_mc_all(mc1)).all() and np.isfinite(_lc_all(lc1)).all()
    for stride in (4, K):
        at = history_nodes(K, stride) - 1
        mcs, lcs = _mc(P, blob, nt, 0, 0, g, xi, xn, om, inp, stride=stride), _lc(P, blob, nt, 0, 0, g, inp, stride=stride)
        assert np.array_equal(_mc_all(mcs), _mc_all(mc1)[:, at]) and np.array_equal(_lc_all(lcs), _lc_all(lc1)[:, at])
        assert np.array_equal(mcs["stats"], mc1["stats"]) and np.array_equal(mcs["samples"], mc1["samples"])
        bare_mc, bare_lc = _mc(P, blob, nt, 0, 0, g, xi, xn, om, inp, stride=stride, optional=False), _lc(P, blob, nt, 0, 0, g, inp, stride=stride, jac=False)
        assert np.array_equal(bare_mc["hist"], mcs["hist"]) and np.array_equal(bare_mc["stats"], mcs["stats"])
        assert np.array_equal(bare_lc["cov"], lcs["cov"]) and np.array_equal(bare_lc["nominal"], lcs["nominal"])
    stride = 4
    at = history_nodes(K, stride) - 1
    for j in (0, 3):
        s1 = slice(j, j + 1)
        one_mc = _mc(P[s1], blob[:, s1], nt, 0, 0, sub(s1), xi, xn, om, take(s1), stride=stride)
        one_lc = _lc(P[s1], blob[:, s1], nt, 0, 0, sub(s1), take(s1), stride=stride)
        assert np.array_equal(_mc_all(one_mc)[0], _mc_all(mc1)[j, at]) and np.array_equal(_lc_all(one_lc)[0], _lc_all(lc1)[j, at])
    idx = np.arange(70) % B
    big_mc = _mc(P[idx], np.ascontiguousarray(blob[:, idx]), nt, 0, 0, sub(idx), xi, xn, om, take(idx), stride=stride, optional=False)
    big_lc = _lc(P[idx], np.ascontiguousarray(blob[:, idx]), nt, 0, 0, sub(idx), take(idx), stride=stride)
    assert np.array_equal(big_mc["hist"].transpose(2, 1, 0), mc1["hist"].transpose(2, 1, 0)[idx][:, at]) and np.array_equal(_lc_all(big_lc), _lc_all(lc1)[idx][:, at])
    # device pointers on torch's stream
    L = _lib.load()
    _lib.require_single_hip_runtime()
    o = _opts(nt, 0, 1.0, 0, 0.0)
    stream = torch.cuda.current_stream().cuda_stream
    NJ, Sx = len(at), xi.shape[1]
    dv = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    law = [dv(a) for a in _law_arrays(g, K, B)]
    pt, bt, xt, sg, su, xnt, sn, ph, qq, omt = (dv(a) for a in (P, blob, xi, inp["sigma"], inp["sigma_u"], xn, inp["sigma_nav"], inp["phi"], inp["q"], om))
    new = lambda *shape: torch.full(shape, 7.25, dtype=torch.float64, device="cuda")
    stats, smp, hist, hsmp = new(82, B), new(12, Sx, B), new(52, NJ, B), new(10, NJ, Sx, B)
    _lib.check(L.ascent_disperse_drifting_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), M, Sx, xt.data_ptr(), sg.data_ptr(), su.data_ptr(),
                                                *[a.data_ptr() for a in law], xnt.data_ptr(), sn.data_ptr(), ph.data_ptr(), qq.data_ptr(),
                                                omt.data_ptr(), stride, stats.data_ptr(), smp.data_ptr(), hist.data_ptr(), hsmp.data_ptr(), 0,
                                                C.c_void_p(stream), 1))
    nom, cov, jac = new(10, NJ, B), new(55, NJ, B), new(10, 32, NJ, B)
    _lib.check(L.ascent_covariance_drifting_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), M, sg.data_ptr(), su.data_ptr(),
                                                  *[a.data_ptr() for a in law], sn.data_ptr(), ph.data_ptr(), qq.data_ptr(), stride,
                                                  nom.data_ptr(), cov.data_ptr(), jac.data_ptr(), 0, C.c_void_p(stream), 1))
    torch.cuda.synchronize()
    d_mc = dict(stats=stats.cpu().numpy(), samples=smp.cpu().numpy(), hist=hist.cpu().numpy(), hist_samples=hsmp.cpu().numpy())
    d_lc = dict(nominal=nom.cpu().numpy(), cov=cov.cpu().numpy(), jac=jac.cpu().numpy())
    assert np.array_equal(_mc_all(d_mc), _mc_all(mc1)[:, at]) and np.array_equal(d_mc["stats"], mc1["stats"]) and np.array_equal(d_mc["samples"], mc1["samples"])
    assert np.array_equal(_lc_all(d_lc), _lc_all(lc1)[:, at])


def test_bounded_garbage():
    """Nothing here provokes a fault: every case is bounded work that ends in NaN rows.  With device pointers the host does not
    read phi and q: NaN, phi = 2 and q = -1 in problem 0 give n = 0 and NaN statistics at every node (the nominal rows stay) and
    NaN rows of the covariance call, and leave problem 1's bits alone.  A blob without a final time behaves as in the parent calls."""
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    nt, K, B, q = 18, 17, 2, 1e6
    P, blob = _case(nt, 0, 0)
    g = _gains(nt, 0, 0, "navigated", q)
    inp = _inputs(P, nt, q)
    xi, xn, om = _draws(K, 70)
    good_mc, good_lc = _mc(P, blob, nt, 0, 0, g, xi, xn, om, inp), _lc(P, blob, nt, 0, 0, g, inp)
    L = _lib.load()
    _lib.require_single_hip_runtime()
    o = _opts(nt, 0, 1.0, 0, 0.0)
    dv = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    law = [dv(a) for a in _law_arrays(g, K, B)]
    pt, bt, xt, sg, su, xnt, sn, omt = (dv(a) for a in (P, blob, xi, inp["sigma"], inp["sigma_u"], xn, inp["sigma_nav"], np.nan_to_num(om)))
    new = lambda *shape: torch.full(shape, 7.25, dtype=torch.float64, device="cuda")
    for what, a, val in (("phi", 1, np.nan), ("phi", 0, 2.0), ("q", 7, -1.0), ("q", 4, np.inf)):
        bad = {k: inp[k].copy() for k in ("phi", "q")}
        bad[what][a, 0] = val
        ph, qq = dv(bad["phi"]), dv(bad["q"])
        stats, hist, hsmp = new(82, B), new(52, K, B), new(10, K, 70, B)
        _lib.check(L.ascent_disperse_drifting_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), M, 70, xt.data_ptr(), sg.data_ptr(), su.data_ptr(),
                                                    *[x.data_ptr() for x in law], xnt.data_ptr(), sn.data_ptr(), ph.data_ptr(), qq.data_ptr(),
                                                    omt.data_ptr(), 1, stats.data_ptr(), None, hist.data_ptr(), hsmp.data_ptr(), 0, None, 1))
        nom, cov, jac = new(10, K, B), new(55, K, B), new(10, 32, K, B)
        _lib.check(L.ascent_covariance_drifting_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), M, sg.data_ptr(), su.data_ptr(),
                                                      *[x.data_ptr() for x in law], sn.data_ptr(), ph.data_ptr(), qq.data_ptr(), 1,
                                                      nom.data_ptr(), cov.data_ptr(), jac.data_ptr(), 0, None, 1))
        torch.cuda.synchronize()
        hist, stats, cov, jac, nom = hist.cpu().numpy(), stats.cpu().numpy(), cov.cpu().numpy(), jac.cpu().numpy(), nom.cpu().numpy()
        assert np.all(hist[0, :, 0] == 0) and np.isnan(hist[11:51, :, 0]).all() and np.array_equal(hist[1:11, :, 0], good_mc["hist"][1:11, :, 0]), (what, val)
        assert stats[0, 0] == 0 and np.isnan(stats[10:, 0]).all() and np.isnan(hsmp.cpu().numpy()[:8, :, :, 0]).all()
        assert np.isnan(cov[:, :, 0]).all() and np.isnan(jac[:, :, :, 0]).all() and np.array_equal(nom, good_lc["nominal"])
        assert np.array_equal(hist[:, :, 1], good_mc["hist"][:, :, 1]) and np.array_equal(stats[:, 1], good_mc["stats"][:, 1])
        assert np.array_equal(cov[:, :, 1], good_lc["cov"][:, :, 1]) and np.array_equal(jac[:, :, :, 1], good_lc["jac"][:, :, :, 1])
    b = np.array(blob)
    b[21 * K, 0] = np.nan
    mc, lc = _mc(P, b, nt, 0, 0, g, xi, xn, om, inp), _lc(P, b, nt, 0, 0, g, inp)
    pm, pl = _mc(P, b, nt, 0, 0, g, xi, xn, None, inp, parent=True), _lc(P, b, nt, 0, 0, g, inp, parent=True)
    assert np.array_equal(mc["hist"][:, :, 0], pm["hist"][:, :, 0], equal_nan=True) and np.all(mc["hist"][0, :, 0] == 0)
    assert np.array_equal(lc["cov"][:, :, 0], pl["cov"][:, :, 0], equal_nan=True) and np.isnan(lc["cov"][:, :, 0]).all()
    assert np.array_equal(mc["hist"][:, :, 1], good_mc["hist"][:, :, 1]) and np.array_equal(lc["cov"][:, :, 1], good_lc["cov"][:, :, 1])


def test_front_end_makes_the_same_call():
    """disperse_batch and linear_corridor with time constants against the entry points called with the phi and q of the
    translation; without `history` the drifting dispersion runs at stride K and returns history None"""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch, linear_corridor
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _nav_drift
    nt, K, q = 18, 17, 1e6
    P, blob = _case(nt, 0, 0)
    B = P.shape[0]
    g = _gains(nt, 0, 0, "navigated", q)
    inp = _inputs(P, nt, q)
    tau = np.array([60.0, 10.0, np.inf, 60.0, 1e-300, 30.0, np.inf])
    steady = np.array([1e-6, 0.0, 0.0, 2e-6, 1e-6, 1e-6, 0.0])
    nav_s = np.ascontiguousarray(inp["sigma_nav"].T)
    phi, qd = _nav_drift(tau, 5.0, steady, None, nav_s, blob[21 * K] * P[:, 11] / K, B)
    assert np.all(phi[:, 4] == 0.0) and np.all(phi[:, [2, 6]] == 1.0) and np.all(qd[:, [1, 2, 6]] == 0.0) and np.all(qd[:, 7] > 0)
    xi, xn, _ = _draws(K, 70)
    om = np.random.default_rng(2).standard_normal((8, K, 70))
    direct = dict(inp, phi=np.ascontiguousarray(phi.T), q=np.ascontiguousarray(qd.T))
    kw = dict(z0_sigma=inp["sigma"][:7].T, param_sigma=inp["sigma"][7:23].T, tf_sigma=inp["sigma"][23], control_sigma=inp["sigma_u"].T,
              nav_sigma=nav_s[:, :7], knowledge_sigma=nav_s[:, 7], nav_tau=tau, knowledge_tau=5.0, nav_steady_sigma=steady, guidance=g, substeps=M)
    want = _mc(P, blob, nt, 0, 0, g, xi, xn, om, direct, stride=4)
    d = disperse_batch(P, blob, nt, xi=xi, xi_nav=xn, samples=70, history=4, keep_samples=True, keep_history_samples=True, **kw)
    assert np.array_equal(d.xi_drift, om) and np.array_equal(d.nav_phi, phi) and np.array_equal(d.nav_q, qd)
    assert np.array_equal(d.history.samples, want["hist_samples"].transpose(3, 2, 1, 0)) and np.array_equal(d.history.mean, want["hist"][11:21].transpose(2, 1, 0))
    assert np.array_equal(d.mean, want["stats"][10:19].T) and np.array_equal(d.effort, want["samples"][9:].transpose(2, 1, 0))
    end = disperse_batch(P, blob, nt, xi=xi, xi_nav=xn, samples=70, **kw)
    assert end.history is None and np.array_equal(end.mean, d.mean) and np.array_equal(end.cov, d.cov)
    lc = linear_corridor(P, blob, nt, history=4, **kw)
    w = _lc(P, blob, nt, 0, 0, g, direct, stride=4)
    assert np.array_equal(lc.jacobian, w["jac"].transpose(3, 2, 0, 1)) and np.array_equal(lc.nominal, w["nominal"].transpose(2, 1, 0))
    iu = np.triu_indices(10)
    assert np.array_equal(lc.cov[:, :, iu[0], iu[1]], w["cov"].transpose(2, 1, 0)) and np.array_equal(lc.cov, lc.cov.transpose(0, 1, 3, 2))
