"""The guidance feed-forward and the navigation errors on the GPU (ascent_guidance_feedforward, ascent_disperse_navigated_batch):
the bitwise promises of the header against ascent_guidance_gains and ascent_disperse_guided_batch, the feed-forward gains and
the closed-loop Jacobian with its navigation block against the CPU reference (tests/feedforward_reference.py), every navigated
sample against the reference flown with the device's own gains, bounded garbage, and what the feed-forward is worth.

Bounds that depend on the conditioning of the case are computed here from the reference alone -- its float64 run against its
longdouble run -- never from the device.  The differences seen are collected in PARITY; with ASCENT_FEEDFORWARD_PARITY_OUT=<file>
they are written there as JSON when the module is done (profiles/feedforward_parity.json is such a file)."""
import ctypes as C

import numpy as np
import pytest

import feedforward_reference as ffr
import guidance_reference as gr
from gpu_cases import (CASES, M, SAMPLE_BOUND, case as _case, check_statistics as _check_statistics, guided as _guided,
                       parity_writer, sample_error as _sample_error, sigmas as _sigmas, stats as _stats, weights as _weights,
                       xi as _xi)

pytestmark = pytest.mark.gpu

PARITY = {"feedforward_vs_reference": {}, "navigated_samples_vs_reference": {}, "effectiveness": {}}
E_FT = np.eye(16)[3]
_write_parity = parity_writer("ASCENT_FEEDFORWARD_PARITY_OUT", PARITY)


def _dense(P):
    """a dense direction per problem: every field moves by about 1e-3 of itself (1e-3 where it is zero)"""
    return np.random.default_rng(21).standard_normal(P.shape) * np.where(P != 0, np.abs(P), 1.0) * 1e-3


def _gains_bits(g, n=5):
    J = g.jacobian
    B = len(g.gain_t)
    return np.concatenate([g.gain_u.reshape(B, -1), g.gain_t, g.summary[:, :n]] + ([] if J is None else [
        J.dz0.reshape(B, -1), J.dparams.reshape(B, -1), J.dtf, J.dcontrols.reshape(B, -1)]), axis=1)


def _ff_bits(g):
    B = len(g.gain_t)
    return np.concatenate([_gains_bits(g, 7), g.ff_u, g.ff_t[:, None]] + ([] if g.jacobian_nav is None else [g.jacobian_nav.reshape(B, -1)]), axis=1)


@pytest.mark.parametrize("nt,scheme,form", CASES)
def test_feedback_gains_keep_their_bits_and_a_zero_direction_changes_nothing(nt, scheme, form):
    """q = 1e6 and 1e12, substeps 2: for ff_dir = e_Ft and for a dense random direction gain_u, gain_t and summary rows 0..4 are
    ascent_guidance_gains' bits; ff_dir = 0 gives zero feed-forward, a zero theta-hat column and the bits of the closed-loop
    Jacobian; with and without the optional outputs the other outputs are the same bits."""
    from lunar_module_ascent_trajectory_optimiser_amd import guidance_gains
    P, blob = _case(nt, scheme, form)
    kw = dict(scheme=scheme, formulation=form, substeps=M)
    for q in (1e6, 1e12):
        g = guidance_gains(P, blob, nt, **kw, **_weights(q))
        assert (g.status == 0).all() and g.ff_u is None and g.summary.shape[1] == 5
        for d in ("Ft", _dense(P)):
            gf = guidance_gains(P, blob, nt, feedforward=d, want_jacobian=False, **kw, **_weights(q))
            assert gf.summary.shape == (P.shape[0], 7) and gf.ff_u.shape == (P.shape[0], nt - 1) and gf.ff_t.shape == (P.shape[0],)
            assert np.array_equal(_gains_bits(gf), _gains_bits(g)[:, :_gains_bits(gf).shape[1]])
            assert np.array_equal(gf.max_feedforward, np.abs(gf.ff_u).max(axis=1)) and np.array_equal(gf.max_cutoff_feedforward, np.abs(gf.ff_t))
            sat = np.abs(blob[7 * (nt - 1):8 * (nt - 1)].T) >= 0.999
            assert np.all(gf.ff_u[sat] == 0.0) and np.all(gf.ff_u[~sat] != 0.0) and np.all(gf.ff_t != 0.0)
            gj = guidance_gains(P, blob, nt, feedforward=d, **kw, **_weights(q))
            for f in ("gain_u", "gain_t", "summary", "ff_u", "ff_t"):
                assert np.array_equal(getattr(gf, f), getattr(gj, f)), f
            assert gj.jacobian_nav.shape == (P.shape[0], 9, 8)
            assert np.array_equal(gj.jacobian.dz0, g.jacobian.dz0, equal_nan=True) and np.array_equal(gj.jacobian.dcontrols, g.jacobian.dcontrols, equal_nan=True)
        g0 = guidance_gains(P, blob, nt, feedforward=np.zeros(16), knowledge=E_FT, **kw, **_weights(q))
        assert np.all(g0.ff_u == 0.0) and np.all(g0.ff_t == 0.0) and np.all(g0.jacobian_nav[:, :, 7] == 0.0)
        assert np.array_equal(_gains_bits(g0), _gains_bits(g), equal_nan=True)


def _navigated_raw(P, blob, nt, scheme, form, g, xi, kw, substeps, ff_u=None, ff_t=None, ff_know=None, xi_nav=None, sigma_nav=None):
    """ascent_disperse_navigated_batch itself, host pointers, so that every new argument can be null: -> (stats (B, 82), samples (B, S, 12))"""
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts, _ptr
    L = _lib.load()
    B, K, S = P.shape[0], nt - 1, xi.shape[1]
    o = _opts(nt, 0, 1.0, 0, 0.0, scheme, form)
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    sig = c(np.concatenate([kw["z0_sigma"], kw["param_sigma"], kw["tf_sigma"][:, None]], axis=1).T)
    sig_u = np.full((K, B), kw["control_sigma"])
    gu, gt, sm = c(g.gain_u.transpose(2, 1, 0)), c(g.gain_t.T), c(g.stretch_max)
    stats, smp = np.empty((82, B)), np.empty((12, S, B))
    Pc, bc, xc = c(P), c(blob), c(xi)
    args = [c(ff_u), c(ff_t), c(ff_know), c(xi_nav), c(sigma_nav)]
    _lib.check(L.ascent_disperse_navigated_batch(_ptr(Pc), B, C.byref(o), _ptr(bc), substeps, S, _ptr(xc), _ptr(sig), _ptr(sig_u), _ptr(gu),
                                                 _ptr(gt), _ptr(sm), *[_ptr(a) for a in args], _ptr(stats), _ptr(smp), 0, None, 0))
    return stats.T, smp.transpose(2, 1, 0)


def _raw_matches(raw, d):
    s, a = raw
    iu = np.triu_indices(9)
    return (np.array_equal(s[:, 0], d.n_valid) and np.array_equal(s[:, 1:10], d.nominal) and np.array_equal(s[:, 10:19], d.mean, equal_nan=True)
            and np.array_equal(s[:, 19:64], d.cov[:, iu[0], iu[1]], equal_nan=True) and np.array_equal(s[:, 64:73], d.min, equal_nan=True)
            and np.array_equal(s[:, 73:82], d.max, equal_nan=True) and np.array_equal(a[:, :, :9], d.samples, equal_nan=True)
            and np.array_equal(a[:, :, 9:], d.effort, equal_nan=True))


@pytest.mark.parametrize("nt,scheme,form,samples", [(3, 0, 0, 1), (3, 0, 1, 65), (18, 0, 0, 257), (18, 2, 0, 65), (18, 0, 1, 257), (34, 0, 0, 65)])
def test_nothing_new_gives_the_bits_of_the_guided_dispersion(nt, scheme, form, samples):
    """The navigated call with every new argument null, and with all of them given but zero (the draws non-zero), gives
    ascent_disperse_guided_batch's statistics, samples and effort bit for bit; substeps 0 and 2, q = 1e9."""
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult, guidance_gains
    P, blob = _case(nt, scheme, form)
    B, K = P.shape[0], nt - 1
    xi, xn = _xi(K, samples, 3), np.random.default_rng(4).standard_normal((8, samples))
    kw = _sigmas(P)
    for m in (0, 2):
        g = guidance_gains(P, blob, nt, scheme=scheme, formulation=form, substeps=m, want_jacobian=False, **_weights(1e9))
        d = _guided(P, blob, nt, scheme, form, g, xi, kw, m)
        assert _raw_matches(_navigated_raw(P, blob, nt, scheme, form, g, xi, kw, m), d)
        z = _navigated_raw(P, blob, nt, scheme, form, g, xi, kw, m, np.zeros((K, B)), np.zeros(B), np.zeros((16, B)), xn, np.zeros((8, B)))
        assert _raw_matches(z, d)
        gz = GuidanceResult(g.gain_u, g.gain_t, g.summary, g.stretch_max, None, ff_u=np.zeros((B, K)), ff_t=np.zeros(B), ff_know=np.zeros((B, 16)))
        dz = _guided(P, blob, nt, scheme, form, gz, xi, dict(kw, nav_sigma=np.zeros(7), knowledge_sigma=0.0, xi_nav=xn), m)
        assert np.array_equal(_stats(dz), _stats(d), equal_nan=True) and np.array_equal(dz.samples, d.samples) and np.array_equal(dz.effort, d.effort)
        assert dz.nav_sigma.shape == (B, 8) and dz.xi_nav is not None and d.xi_nav is None


def _nav_kw(P):
    """navigation sigmas of 1e-6 (scaled) on every state and 1e-3 of the thrust on theta-hat"""
    return dict(nav_sigma=np.full(7, 1e-6), knowledge_sigma=1e-3 * P[:, 3])


def test_batch_independence_pointers_and_optional_outputs():
    """Each of 5 problems alone and repeated through a batch of 70 gives the same bits, feed-forward gains and navigated dispersion
    alike; host pointers and device pointers on torch's stream give the same bits; with and without samples_out the statistics are
    the same bits.  nt = 34, 257 samples, q = 1e9."""
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult, _lib, guidance_gains
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    nt, K, B, S = 34, 33, 5, 257
    P, blob = _case(nt, 0, 0, 5)
    xi, xn = _xi(K, S, 8), np.random.default_rng(9).standard_normal((8, S))
    kw = dict(_sigmas(P), xi_nav=xn, **_nav_kw(P))
    wk = _weights(1e9)
    take = lambda k, idx: {n: v[idx] if n in ("z0_sigma", "param_sigma", "tf_sigma", "knowledge_sigma") else v for n, v in k.items()}

    def sub(g, idx):
        return GuidanceResult(g.gain_u[idx], g.gain_t[idx], g.summary[idx], g.stretch_max[idx], None, ff_u=g.ff_u[idx], ff_t=g.ff_t[idx],
                              ff_know=g.ff_know[idx])

    g = guidance_gains(P, blob, nt, feedforward="Ft", **wk)
    assert (g.status == 0).all() and (g.substeps > 2).all()
    host = _guided(P, blob, nt, 0, 0, g, xi, kw, 0)
    assert (host.n_valid == S).all() and host.effort[:, :, 1].max() > 0
    without = _guided(P, blob, nt, 0, 0, g, xi, kw, 0, keep=False)
    assert without.samples is None and np.array_equal(_stats(without), _stats(host))
    for q in range(B):
        one = guidance_gains(P[q:q + 1], blob[:, q:q + 1], nt, feedforward="Ft", **wk)
        assert np.array_equal(_ff_bits(one)[0], _ff_bits(g)[q], equal_nan=True)
        d1 = _guided(P[q:q + 1], blob[:, q:q + 1], nt, 0, 0, one, xi, take(kw, slice(q, q + 1)), 0)
        assert np.array_equal(_stats(d1)[0], _stats(host)[q]) and np.array_equal(d1.samples[0], host.samples[q]) and np.array_equal(d1.effort[0], host.effort[q])
    idx = np.arange(70) % B
    bb = np.ascontiguousarray(blob[:, idx])
    big = guidance_gains(P[idx], bb, nt, feedforward="Ft", **wk)
    assert np.array_equal(_ff_bits(big), _ff_bits(g)[idx], equal_nan=True)
    dbig = _guided(P[idx], bb, nt, 0, 0, sub(g, idx), xi, take(kw, idx), 0)
    assert np.array_equal(_stats(dbig), _stats(host)[idx]) and np.array_equal(dbig.samples, host.samples[idx]) and np.array_equal(dbig.effort, host.effort[idx])
    # device pointers on torch's stream
    L = _lib.load()
    _lib.require_single_hip_runtime()
    o = _opts(nt, 0, 1.0, 0, 0.0)
    stream = torch.cuda.current_stream().cuda_stream
    w = np.ascontiguousarray(np.array([[1e9, 1e9, 1e9, 1.0, 1.0, 0.5]] * B).T)
    sig = np.ascontiguousarray(np.concatenate([kw["z0_sigma"], kw["param_sigma"], kw["tf_sigma"][:, None]], axis=1).T)
    sig_u = np.full((K, B), kw["control_sigma"])
    dirs = np.ascontiguousarray(np.tile(E_FT, (B, 1)).T)
    sn = np.ascontiguousarray(host.nav_sigma.T)
    pt, bt, wt, xt, st, ut, dt, nt_, snt = (torch.from_numpy(np.array(a)).cuda() for a in (P, blob, w, xi, sig, sig_u, dirs, xn, sn))
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    gu, gt, fu, ft, sm, jc, ju, jn = new(7, K, B), new(7, B), new(K, B), new(B), new(7, B), new(9, 24, B), new(9, K, B), new(9, 8, B)
    out, smp = new(82, B), new(12, S, B)
    _lib.check(L.ascent_guidance_feedforward(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), 0, wt.data_ptr(), dt.data_ptr(), dt.data_ptr(),
                                             gu.data_ptr(), gt.data_ptr(), fu.data_ptr(), ft.data_ptr(), sm.data_ptr(), jc.data_ptr(),
                                             ju.data_ptr(), jn.data_ptr(), 0, C.c_void_p(stream), 1))
    _lib.check(L.ascent_disperse_navigated_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), 0, S, xt.data_ptr(), st.data_ptr(), ut.data_ptr(),
                                                 gu.data_ptr(), gt.data_ptr(), wt[5].data_ptr(), fu.data_ptr(), ft.data_ptr(), dt.data_ptr(),
                                                 nt_.data_ptr(), snt.data_ptr(), out.data_ptr(), smp.data_ptr(), 0, C.c_void_p(stream), 1))
    torch.cuda.synchronize()
    assert np.array_equal(gu.cpu().numpy().transpose(2, 1, 0), g.gain_u) and np.array_equal(gt.cpu().numpy().T, g.gain_t)
    assert np.array_equal(fu.cpu().numpy().T, g.ff_u) and np.array_equal(ft.cpu().numpy(), g.ff_t) and np.array_equal(sm.cpu().numpy().T, g.summary)
    assert np.array_equal(jn.cpu().numpy().transpose(2, 0, 1), g.jacobian_nav) and np.array_equal(ju.cpu().numpy().transpose(2, 0, 1), g.jacobian.dcontrols)
    assert np.array_equal(jc.cpu().numpy().transpose(2, 0, 1)[:, :, 7:23], g.jacobian.dparams)
    assert _raw_matches((out.cpu().numpy().T, smp.cpu().numpy().transpose(2, 1, 0)), host)


@pytest.mark.parametrize("nt,scheme,form", CASES)
def test_feedforward_and_closed_loop_jacobian_match_reference(nt, scheme, form):
    """q = 1e6, r_u = r_t = 1, stretch_max = 0.5, substeps = 2, ff_dir = e_Ft known exactly (w = e_Ft).  Rows: [f_u(1..K), f_t] as
    one row, every row of jac_nav, every row of [jac_cl | jac_u_cl].  Per problem the bound is 100 x the reference's own
    float64-against-longdouble difference of that quantity on that blob, in units of each row's largest entry, with a floor of
    1e-13 -- the rule and the margin of test_gpu_guidance.test_gains_and_closed_loop_jacobian_match_reference --; the device is
    compared with the longdouble run."""
    from lunar_module_ascent_trajectory_optimiser_amd import guidance_gains
    P, blob = _case(nt, scheme, form)
    w = np.array([1e6, 1e6, 1e6, 1.0, 1.0, 0.5])
    g = guidance_gains(P, blob, nt, scheme=scheme, formulation=form, substeps=M, feedforward="Ft", **_weights(1e6))
    assert np.array_equal(g.ff_dir, np.tile(E_FT, (P.shape[0], 1))) and np.array_equal(g.ff_know, g.ff_dir)
    fig = {}
    for j in range(P.shape[0]):
        out = {}
        for dtype in (np.float64, np.longdouble):
            rec = gr.records(P[j], blob[:, j], nt, form, M, dtype)
            G = ffr.gains(rec, P[j], w, E_FT, dtype)
            J = ffr.closed_loop_jacobian(rec, G, E_FT, P[j], form)
            out[dtype] = dict(ff=np.concatenate([G["ff_u"], [G["ff_t"]]]), jac_nav=J["jac_nav"], jac=np.concatenate([J["jac"], J["jac_u"]], axis=1),
                              summary=G["summary"])
        dev = dict(ff=np.concatenate([g.ff_u[j], [g.ff_t[j]]]), jac_nav=g.jacobian_nav[j],
                   jac=np.concatenate([g.jacobian.dz0[j], g.jacobian.dparams[j], g.jacobian.dtf[j][:, None], g.jacobian.dcontrols[j]], axis=1))
        ref, refl = out[np.float64], out[np.longdouble]
        assert np.array_equal(g.summary[j, [0, 1, 4]], refl["summary"][[0, 1, 4]]) and g.summary[j, 0] == 0
        for name in ("ff", "jac_nav", "jac"):
            gap = gr.rel_gap(ref[name], refl[name])
            err = gr.rel_gap(dev[name], refl[name])
            bound = max(100.0 * gap, 1e-13)
            fig[f"problem{j}_{name}"] = dict(device_error=err, reference_gap=gap, bound=bound)
            print(nt, scheme, form, "problem", j, name, "device against longdouble reference", err, "reference float64 against longdouble", gap, "bound", bound)
    PARITY["feedforward_vs_reference"][f"nt{nt}_scheme{scheme}_form{form}"] = fig
    for k, v in fig.items():
        assert v["device_error"] <= v["bound"], (k, v)


@pytest.mark.parametrize("q", [1e6, 1e12])
@pytest.mark.parametrize("nt,scheme,form,samples", [c + (65,) for c in CASES] + [(3, 0, 0, 1), (18, 0, 0, 257)])
def test_navigated_samples_match_reference_flown_with_the_device_gains(nt, scheme, form, samples, q):
    """Every row of samples_out against the CPU reference flying the device's own gains and feed-forward, all four sigma groups at
    1e-3, the navigation sigmas at 1e-6 (scaled), a knowledge sigma of 1e-3 of the thrust, ff_dir = e_Ft, substeps = 2.  Bound: the
    larger of SAMPLE_BOUND and 100 x the float64-against-longdouble difference of the reference's navigated flight on the case (on
    the first 65 samples for the second problem of the 257-sample case), as
    test_gpu_guidance.test_guided_samples_match_reference_flown_with_the_device_gains; the correction and the stretch within the
    bound times |K_k|_1 + |f_k theta-hat| scale; the clipped-step count equal wherever the reference's commands stay that far from
    the clip.  Then the reduction against numpy on the device's samples."""
    from lunar_module_ascent_trajectory_optimiser_amd import guidance_gains
    P, blob = _case(nt, scheme, form)
    K = nt - 1
    g = guidance_gains(P, blob, nt, scheme=scheme, formulation=form, substeps=M, want_jacobian=False, feedforward="Ft", **_weights(q))
    assert (g.status == 0).all() and g.jacobian is None and g.jacobian_nav is None
    xi, xn = _xi(K, samples), np.random.default_rng(13).standard_normal((8, samples))
    kw = _sigmas(P)
    d = _guided(P, blob, nt, scheme, form, g, xi, dict(kw, xi_nav=xn, **_nav_kw(P)))
    assert d.samples.shape == (P.shape[0], samples, 9) and d.effort.shape == (P.shape[0], samples, 3) and np.all(d.nav_sigma[:, :7] == 1e-6)
    fig = {}
    for j in range(P.shape[0]):
        sigma = np.concatenate([kw["z0_sigma"][j], kw["param_sigma"][j], [kw["tf_sigma"][j]]])
        args = (P[j], blob[:, j], nt, xi, sigma, np.full(K, kw["control_sigma"]), g.gain_u[j], g.gain_t[j], 0.5, g.ff_u[j], g.ff_t[j], g.ff_know[j])
        ref = ffr.disperse_navigated(*args, xn, d.nav_sigma[j], form, M)
        n = samples if j == 0 else min(samples, 65)
        refl = ffr.disperse_navigated(*args[:3], xi[:, :n], *args[4:], xn[:, :n], d.nav_sigma[j], form, M, dtype=np.longdouble)
        gap = _sample_error(ref["samples"][:n], refl["samples"].astype(np.float64), P[j, 9])
        bound = max(SAMPLE_BOUND, 100.0 * gap)
        err = max(_sample_error(d.samples[j], ref["samples"], P[j, 9]), _sample_error(d.nominal[j][None], ref["nominal"][None], P[j, 9]))
        assert d.n_valid[j] == ref["stats"][0]
        th = np.abs(ffr.beliefs(xi, sigma, g.ff_know[j], xn, d.nav_sigma[j])[0]).max()
        k1, kt1 = np.abs(g.gain_u[j]).sum(axis=1).max() + np.abs(g.ff_u[j]).max() * th, np.abs(g.gain_t[j]).sum() + abs(g.ff_t[j]) * th
        e_fb, e_st = np.abs(d.effort[j, :, 1] - ref["effort"][:, 1]).max(), np.abs(d.effort[j, :, 2] - ref["effort"][:, 2]).max()
        far = ref["effort"][:, 3] > bound * k1
        fig[f"problem{j}"] = dict(device_error=err, reference_gap=gap, bound=bound, feedback_error=e_fb, stretch_error=e_st,
                                  clipped_steps_mean=float(ref["effort"][:, 0].mean()), count_checked=int(far.sum()))
        print(nt, scheme, form, samples, "q", q, "problem", j, fig[f"problem{j}"])
        assert np.array_equal(d.effort[j, far, 0], ref["effort"][far, 0])
        assert e_fb <= bound * k1 and e_st <= bound * kt1
        _check_statistics(d, j)
    PARITY["navigated_samples_vs_reference"][f"nt{nt}_scheme{scheme}_form{form}_samples{samples}_q{q:g}"] = fig
    for k, v in fig.items():
        assert v["device_error"] <= v["bound"], (k, v)


def test_bounded_garbage():
    """Nothing here provokes a fault; every case is bounded work that ends in NaN rows.  A NaN in one problem's ff_dir or ff_know
    freezes that problem alone (status 2, NaN gains, feed-forward and Jacobians); a NaN or an inf entry of ff_u, a NaN f_t, or a NaN
    navigation draw under a non-zero sigma makes that problem's samples invalid (n = 0) and leaves the other problem's statistics
    and samples untouched bit for bit."""
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult, guidance_gains
    nt, K = 18, 17
    P, blob = _case(nt, 0, 0)
    kw = _sigmas(P)
    xi, xn = _xi(K, 65, 10), np.random.default_rng(14).standard_normal((8, 65))
    wk = dict(substeps=M, **_weights(1e6))
    g = guidance_gains(P, blob, nt, feedforward="Ft", **wk)
    nav = dict(kw, xi_nav=xn, **_nav_kw(P))
    good = _guided(P, blob, nt, 0, 0, g, xi, nav)
    assert (good.n_valid == 65).all() and (g.status == 0).all()
    for field in ("feedforward", "knowledge"):
        a = np.tile(E_FT, (2, 1))
        a[0, 5] = np.nan
        gn = guidance_gains(P, blob, nt, **dict(dict(feedforward="Ft"), **{field: a}), **wk)
        assert gn.status[0] == 2 and np.isnan(gn.gain_u[0]).all() and np.isnan(gn.gain_t[0]).all() and np.isnan(gn.ff_u[0]).all() and np.isnan(gn.ff_t[0])
        assert np.isnan(gn.jacobian.dparams[0]).all() and np.isnan(gn.jacobian_nav[0]).all() and np.isnan(gn.summary[0, [2, 3, 5, 6]]).all()
        assert np.array_equal(_ff_bits(gn)[1], _ff_bits(g)[1], equal_nan=True)

    def with_ff(**ch):
        f = dict(ff_u=g.ff_u, ff_t=g.ff_t, ff_know=g.ff_know)
        return GuidanceResult(g.gain_u, g.gain_t, g.summary, g.stretch_max, None, **dict(f, **ch))

    for bad, k in ((np.nan, 5), (np.inf, 0), (np.nan, K - 1)):
        fu = g.ff_u.copy()
        fu[0, k] = bad
        d = _guided(P, blob, nt, 0, 0, with_ff(ff_u=fu), xi, nav)
        assert d.n_valid[0] == 0 and np.isnan(d.mean[0]).all() and not np.isfinite(d.samples[0]).all(axis=1).any()
        assert np.array_equal(_stats(d)[1], _stats(good)[1]) and np.array_equal(d.samples[1], good.samples[1])
    ft = g.ff_t.copy()
    ft[0] = np.nan
    d = _guided(P, blob, nt, 0, 0, with_ff(ff_t=ft), xi, nav)
    assert d.n_valid[0] == 0 and np.array_equal(_stats(d)[1], _stats(good)[1])
    # a NaN draw counts only where its sigma is not zero: row 2 (a state bias) and row 7 (theta-hat), problem 0 alone has the sigma
    for row in (2, 7):
        xb = xn.copy()
        xb[row] = np.nan
        ns = np.zeros((2, 7))
        ks = np.zeros(2)
        if row < 7:
            ns[0, row] = 1e-6
        else:
            ks[0] = 1.0
        base = _guided(P, blob, nt, 0, 0, g, xi, dict(kw, xi_nav=xn, nav_sigma=ns, knowledge_sigma=ks))
        d = _guided(P, blob, nt, 0, 0, g, xi, dict(kw, xi_nav=xb, nav_sigma=ns, knowledge_sigma=ks))
        assert base.n_valid[0] == 65 and d.n_valid[0] == 0 and np.isnan(d.mean[0]).all()
        assert np.array_equal(_stats(d)[1], _stats(base)[1]) and np.array_equal(d.samples[1], base.samples[1])


def test_what_the_feedforward_is_worth_end_to_end():
    """The figures of tests/test_feedforward_reference.py from the device: backward Euler, nt = 50, solved, trimmed to 1e-12 and
    flown on the GPU (m = 18), 128 samples of default_rng(0), 50 N of thrust sigma, 1e-3 per control step, q = 1e12, r_u = r_t = 1,
    stretch_max = 0.5: the periapsis 1-sigma with the thrust known at least 10 times below feedback only, with the thrust known to
    10 N (draws of default_rng(1)) strictly between the two, no command clipped; and the sample covariance of the 10 N case against
    linear_covariance with the navigation block."""
    from lunar_module_ascent_trajectory_optimiser_amd import AscentParams, disperse_batch, guidance_gains, solve_batch, trim_batch
    nt, K = 50, 49
    P = AscentParams().as_row()[None].copy()
    r = solve_batch(P, nt, want_blob=True)
    assert (r.status == 0).all()
    t = trim_batch(P, r.blob, nt, rounds=8, tol=1e-12)
    assert t.status[0] == 0
    xi = np.random.default_rng(0).standard_normal((24 + K, 128))
    xn = np.random.default_rng(1).standard_normal((8, 128))
    thrust = np.zeros(16)
    thrust[3] = 50.0
    dkw = dict(param_sigma=thrust, control_sigma=1e-3, xi=xi, keep_samples=True)
    g = guidance_gains(P, t.blob, nt, **_weights(1e12))
    gf = guidance_gains(P, t.blob, nt, feedforward="Ft", **_weights(1e12))
    assert g.status[0] == 0 and gf.status[0] == 0 and gf.substeps[0] == 18 and np.array_equal(gf.gain_u, g.gain_u)
    fb = disperse_batch(P, t.blob, nt, guidance=g, **dkw)
    known = disperse_batch(P, t.blob, nt, guidance=gf, **dkw)
    approx = disperse_batch(P, t.blob, nt, guidance=gf, knowledge_sigma=10.0, xi_nav=xn, **dkw)
    assert fb.n_valid[0] == 128 and known.n_valid[0] == 128 and approx.n_valid[0] == 128
    lin = np.sqrt(np.diagonal(approx.linear_covariance(gf.jacobian, gf.jacobian_nav)[0]))
    fig = dict(feedback_only=fb.std[0, 7:].tolist(), feedforward_known=known.std[0, 7:].tolist(), feedforward_10N=approx.std[0, 7:].tolist(),
               feedforward_10N_linear=lin[7:].tolist(), max_feedforward=float(gf.max_feedforward[0]), max_cutoff_feedforward=float(gf.max_cutoff_feedforward[0]),
               clipped_steps=[float(x.effort[0, :, 0].sum()) for x in (fb, known, approx)])
    PARITY["effectiveness"]["nt50_q1e12"] = fig
    print("1-sigma of the flown periapsis / apoapsis altitude (m):", fig)
    assert known.std[0, 7] * 10.0 <= fb.std[0, 7]
    assert known.std[0, 7] < approx.std[0, 7] < fb.std[0, 7]
    assert np.all(known.effort[0, :, 0] == 0) and np.all(approx.effort[0, :, 0] == 0)
