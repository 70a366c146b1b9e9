"""Closed-loop guidance on the GPU (ascent_guidance_gains, ascent_disperse_guided_batch): the gains and the closed-loop
Jacobian against the CPU reference (tests/guidance_reference.py), every guided sample against the reference flown with the
device's own gains, the bitwise properties the header promises, bounded garbage, what the feedback is worth, the front ends.

Bounds that depend on the conditioning of the case are computed here from the reference alone -- its float64 run against its
longdouble run -- never from the device.  The differences seen are collected in PARITY; with ASCENT_GUIDANCE_PARITY_OUT=<file>
they are written there as JSON when the module is done (profiles/guidance_parity.json is such a file)."""
import ctypes as C
import os

import numpy as np
import pytest

import guidance_reference as gr
from gpu_cases import (CASES, M, SAMPLE_BOUND, case as _case, check_statistics as _check_statistics, guided as _guided,
                       parity_writer, sample_error as _sample_error, sigmas as _sigmas, stats as _stats, weights as _weights,
                       xi as _xi)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = {"gains_vs_reference": {}, "guided_samples_vs_reference": {}, "effectiveness": {}}
_write_parity = parity_writer("ASCENT_GUIDANCE_PARITY_OUT", PARITY)


def _row_error(a, b):
    """largest |a - b| in units of the largest |b| of its row (last axis)"""
    return gr.rel_gap(a, b)


@pytest.mark.parametrize("nt,scheme,form", CASES)
def test_gains_and_closed_loop_jacobian_match_reference(nt, scheme, form):
    """q = 1e6, r_u = r_t = 1, stretch_max = 0.5, substeps = 2.  Rows: gain_u per state over the steps (the layout's rows), gain_t
    as one row, every row of [jac_cl | jac_u_cl].  Per problem the bound is 100 x the reference's own float64-against-longdouble
    difference of that quantity on that blob, in units of each row's largest entry, with a floor of 1e-13; the device is compared
    with the longdouble run.  Status, free-control count and m are equal."""
    from lunar_module_ascent_trajectory_optimiser_amd import guidance_gains
    P, blob = _case(nt, scheme, form)
    w = np.array([1e6, 1e6, 1e6, 1.0, 1.0, 0.5])
    g = guidance_gains(P, blob, nt, scheme=scheme, formulation=form, substeps=M, **_weights(1e6))
    K = nt - 1
    assert g.gain_u.shape == (P.shape[0], K, 7) and g.gain_t.shape == (P.shape[0], 7) and g.summary.shape == (P.shape[0], 5)
    fig = {}
    for j in range(P.shape[0]):
        out = {}
        for dtype in (np.float64, np.longdouble):
            rec = gr.records(P[j], blob[:, j], nt, form, M, dtype)
            G = gr.gains(rec, P[j], w, dtype)
            J = gr.closed_loop_jacobian(rec, G["gain_u"], G["gain_t"], P[j], form)
            out[dtype] = dict(gain_u=G["gain_u"].T, gain_t=G["gain_t"], jac=np.concatenate([J["jac"], J["jac_u"]], axis=1), summary=G["summary"])
        dev = dict(gain_u=g.gain_u[j].T, gain_t=g.gain_t[j],
                   jac=np.concatenate([g.jacobian.dz0[j], g.jacobian.dparams[j], g.jacobian.dtf[j][:, None], g.jacobian.dcontrols[j]], axis=1))
        ref, refl = out[np.float64], out[np.longdouble]
        assert np.array_equal(g.summary[j, [0, 1, 4]], refl["summary"][[0, 1, 4]]) and g.summary[j, 0] == 0
        sat = np.abs(blob[7 * K:8 * K, j]) >= 0.999
        assert np.all(g.gain_u[j][sat] == 0.0)
        for name in ("gain_u", "gain_t", "jac"):
            gap = _row_error(ref[name], refl[name])
            err = _row_error(dev[name], refl[name])
            bound = max(100.0 * gap, 1e-13)
            fig[f"problem{j}_{name}"] = dict(device_error=err, reference_gap=gap, bound=bound)
            print(nt, scheme, form, "problem", j, name, "device against longdouble reference", err, "reference float64 against longdouble", gap, "bound", bound)
        for i, name in ((2, "gain_u"), (3, "gain_t")):
            assert abs(g.summary[j, i] - refl["summary"][i]) <= fig[f"problem{j}_{name}"]["bound"] * np.abs(np.asarray(refl[name], dtype=np.float64)).max()
    PARITY["gains_vs_reference"][f"nt{nt}_scheme{scheme}_form{form}"] = fig
    for k, v in fig.items():
        assert v["device_error"] <= v["bound"], (k, v)


@pytest.mark.parametrize("q", [1e6, 1e12])
@pytest.mark.parametrize("nt,scheme,form,samples", [c + (65,) for c in CASES] + [(3, 0, 0, 1), (18, 0, 0, 257)])
def test_guided_samples_match_reference_flown_with_the_device_gains(nt, scheme, form, samples, q):
    """Every row of samples_out against the CPU reference flying the device's own gains (the conditioning of the Riccati
    recursion then drops out), all four sigma groups non-zero at 1e-3 as in tests/test_gpu_dispersion.py, substeps = 2.  Bound:
    the larger of that file's 1e-10 (scaled; times r_peri for the altitudes) and 100 x the float64-against-longdouble difference of
    the reference's guided flight on the case (on the first 65 samples for the second problem of the 257-sample case).  The effort
    rows: the feedback and the stretch within the bound times |K_k|_1, |k_t|_1; the clipped-step count equal wherever the
    reference's commands stay that far from the clip.  Then the reduction against numpy on the device's samples, with
    test_gpu_dispersion's bounds."""
    from lunar_module_ascent_trajectory_optimiser_amd import guidance_gains
    P, blob = _case(nt, scheme, form)
    K = nt - 1
    g = guidance_gains(P, blob, nt, scheme=scheme, formulation=form, substeps=M, want_jacobian=False, **_weights(q))
    assert (g.status == 0).all() and g.jacobian is None
    xi = _xi(K, samples)
    kw = _sigmas(P)
    d = _guided(P, blob, nt, scheme, form, g, xi, kw)
    assert d.samples.shape == (P.shape[0], samples, 9) and d.effort.shape == (P.shape[0], samples, 3)
    fig = {}
    for j in range(P.shape[0]):
        sigma = np.concatenate([kw["z0_sigma"][j], kw["param_sigma"][j], [kw["tf_sigma"][j]]])
        args = (P[j], blob[:, j], nt, xi, sigma, np.full(K, kw["control_sigma"]), g.gain_u[j], g.gain_t[j], 0.5, form, M)
        ref = gr.disperse_guided(*args)
        n = samples if j == 0 else min(samples, 65)          # the longdouble flight is slow: fewer samples can only lower the bound
        refl = gr.disperse_guided(*args[:3], xi[:, :n], *args[4:], dtype=np.longdouble)
        gap = _sample_error(ref["samples"][:n], refl["samples"].astype(np.float64), P[j, 9])
        bound = max(SAMPLE_BOUND, 100.0 * gap)
        err = max(_sample_error(d.samples[j], ref["samples"], P[j, 9]), _sample_error(d.nominal[j][None], ref["nominal"][None], P[j, 9]))
        assert d.n_valid[j] == ref["stats"][0]
        k1, kt1 = np.abs(g.gain_u[j]).sum(axis=1).max(), np.abs(g.gain_t[j]).sum()
        e_fb, e_st = np.abs(d.effort[j, :, 1] - ref["effort"][:, 1]).max(), np.abs(d.effort[j, :, 2] - ref["effort"][:, 2]).max()
        far = ref["effort"][:, 3] > bound * k1
        fig[f"problem{j}"] = dict(device_error=err, reference_gap=gap, bound=bound, feedback_error=e_fb, stretch_error=e_st,
                                  clipped_steps_mean=float(ref["effort"][:, 0].mean()), count_checked=int(far.sum()))
        print(nt, scheme, form, samples, "q", q, "problem", j, fig[f"problem{j}"])
        assert np.array_equal(d.effort[j, far, 0], ref["effort"][far, 0])
        assert e_fb <= bound * k1 and e_st <= bound * kt1
        _check_statistics(d, j)
    PARITY["guided_samples_vs_reference"][f"nt{nt}_scheme{scheme}_form{form}_samples{samples}_q{q:g}"] = fig
    for k, v in fig.items():
        assert v["device_error"] <= v["bound"], (k, v)


@pytest.mark.parametrize("nt,scheme,form", [(3, 0, 0), (3, 0, 1), (18, 0, 0), (18, 2, 0), (18, 0, 1), (34, 0, 0)])
def test_zero_gains_give_the_bits_of_the_open_loop_dispersion(nt, scheme, form):
    """All-zero gains with stretch_max = 0, with a zero gain_t and without one: statistics and the nine sample rows are
    ascent_disperse_batch's bit for bit, the effort rows zero; and the closed-loop Jacobian of zero gains (q = 0) is
    ascent_flight_jacobian's.  300 samples (two workgroups), substeps 0 and 2."""
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult, disperse_batch, flight_jacobian, guidance_gains
    P, blob = _case(nt, scheme, form)
    B, K = P.shape[0], nt - 1
    xi = _xi(K, 300, 3)
    kw = _sigmas(P)
    for m in (0, 2):
        okw = dict(scheme=scheme, formulation=form, substeps=m)
        op = disperse_batch(P, blob, nt, xi=xi, keep_samples=True, **okw, **kw)
        for gt in (np.zeros((B, 7)), None):
            g = GuidanceResult(np.zeros((B, K, 7)), gt, np.zeros((B, 5)), np.zeros(B), None)
            cl = _guided(P, blob, nt, scheme, form, g, xi, kw, m)
            assert np.array_equal(_stats(cl), _stats(op), equal_nan=True) and np.array_equal(cl.samples, op.samples, equal_nan=True)
            assert np.all(cl.effort == 0.0)
        g0 = guidance_gains(P, blob, nt, **okw, **_weights(0.0))
        J = flight_jacobian(P, blob, nt, **okw)
        assert np.all(g0.gain_u == 0.0) and np.all(g0.gain_t == 0.0) and (g0.status == 0).all()
        for f in ("dz0", "dparams", "dtf", "dcontrols"):
            assert np.array_equal(getattr(g0.jacobian, f), getattr(J, f), equal_nan=True), f


def test_batch_independence_pointers_and_optional_outputs():
    """Each of 5 problems alone and repeated through a batch of 70 gives the same bits, gains and guided dispersion alike; host
    pointers and device pointers on torch's stream give the same bits; with and without samples_out (and with and without the
    closed-loop Jacobian) the other outputs are the same bits.  nt = 34, 300 samples, q = 1e9."""
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult, _lib, guidance_gains
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    nt, K, B, S = 34, 33, 5, 300
    P, blob = _case(nt, 0, 0, 5)
    xi = _xi(K, S, 8)
    kw = _sigmas(P)
    wk = _weights(1e9)

    def gains(g):
        J = g.jacobian
        return np.concatenate([g.gain_u.reshape(len(g.gain_t), -1), g.gain_t, g.summary] + ([] if J is None else [
            J.dz0.reshape(len(g.gain_t), -1), J.dparams.reshape(len(g.gain_t), -1), J.dtf, J.dcontrols.reshape(len(g.gain_t), -1)]), axis=1)

    def sub(g, idx):
        return GuidanceResult(g.gain_u[idx], g.gain_t[idx], g.summary[idx], g.stretch_max[idx], None)

    g = guidance_gains(P, blob, nt, **wk)
    assert (g.status == 0).all() and (g.substeps > 2).all()
    gn = guidance_gains(P, blob, nt, want_jacobian=False, **wk)
    assert np.array_equal(gains(gn), gains(g)[:, :gains(gn).shape[1]])
    host = _guided(P, blob, nt, 0, 0, g, xi, kw, 0)
    assert (host.n_valid == S).all()
    without = _guided(P, blob, nt, 0, 0, g, xi, kw, 0, keep=False)
    assert without.samples is None and without.effort is None and np.array_equal(_stats(without), _stats(host))
    for q in range(B):
        one = guidance_gains(P[q:q + 1], blob[:, q:q + 1], nt, **wk)
        assert np.array_equal(gains(one)[0], gains(g)[q], equal_nan=True)
        d1 = _guided(P[q:q + 1], blob[:, q:q + 1], nt, 0, 0, one, xi, {k: v[q:q + 1] if isinstance(v, np.ndarray) else v for k, v in kw.items()}, 0)
        assert np.array_equal(_stats(d1)[0], _stats(host)[q]) and np.array_equal(d1.samples[0], host.samples[q]) and np.array_equal(d1.effort[0], host.effort[q])
    idx = np.arange(70) % B
    bb = np.ascontiguousarray(blob[:, idx])
    big = guidance_gains(P[idx], bb, nt, **wk)
    assert np.array_equal(gains(big), gains(g)[idx], equal_nan=True)
    dbig = _guided(P[idx], bb, nt, 0, 0, sub(g, idx), xi, {k: v[idx] if isinstance(v, np.ndarray) else v for k, v in kw.items()}, 0)
    assert np.array_equal(_stats(dbig), _stats(host)[idx]) and np.array_equal(dbig.samples, host.samples[idx]) and np.array_equal(dbig.effort, host.effort[idx])
    # device pointers on torch's stream
    L = _lib.load()
    _lib.require_single_hip_runtime()
    o = _opts(nt, 0, 1.0, 0, 0.0)
    stream = torch.cuda.current_stream().cuda_stream
    w = np.ascontiguousarray(np.array([[1e9, 1e9, 1e9, 1.0, 1.0, 0.5]] * B).T)
    sig = np.ascontiguousarray(np.concatenate([kw["z0_sigma"], kw["param_sigma"], kw["tf_sigma"][:, None]], axis=1).T)
    sig_u = np.full((K, B), kw["control_sigma"])
    pt, bt, wt, xt, st, ut = (torch.from_numpy(np.array(a)).cuda() for a in (P, blob, w, xi, sig, sig_u))
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    gu, gt, sm, jc, ju, out, smp = new(7, K, B), new(7, B), new(5, B), new(9, 24, B), new(9, K, B), new(82, B), new(12, S, B)
    _lib.check(L.ascent_guidance_gains(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), 0, wt.data_ptr(), gu.data_ptr(), gt.data_ptr(), sm.data_ptr(),
                                       jc.data_ptr(), ju.data_ptr(), 0, C.c_void_p(stream), 1))
    _lib.check(L.ascent_disperse_guided_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), 0, S, xt.data_ptr(), st.data_ptr(), ut.data_ptr(),
                                              gu.data_ptr(), gt.data_ptr(), wt[5].data_ptr(), out.data_ptr(), smp.data_ptr(), 0, C.c_void_p(stream), 1))
    torch.cuda.synchronize()
    assert np.array_equal(gu.cpu().numpy().transpose(2, 1, 0), g.gain_u) and np.array_equal(gt.cpu().numpy().T, g.gain_t)
    assert np.array_equal(sm.cpu().numpy().T, g.summary) and np.array_equal(ju.cpu().numpy().transpose(2, 0, 1), g.jacobian.dcontrols)
    assert np.array_equal(jc.cpu().numpy().transpose(2, 0, 1)[:, :, 7:23], g.jacobian.dparams)
    s = out.cpu().numpy().T
    assert np.array_equal(s[:, 0], host.n_valid) and np.array_equal(s[:, 1:10], host.nominal) and np.array_equal(s[:, 10:19], host.mean)
    assert np.array_equal(s[:, 19:64], host.cov[:, np.triu_indices(9)[0], np.triu_indices(9)[1]])
    assert np.array_equal(s[:, 64:73], host.min) and np.array_equal(s[:, 73:82], host.max)
    a = smp.cpu().numpy()
    assert np.array_equal(a[:9].transpose(2, 1, 0), host.samples) and np.array_equal(a[9:].transpose(2, 1, 0), host.effort)


def test_bounded_garbage():
    """Nothing here provokes a fault; every case is bounded work that ends in NaN rows.  A NaN or an inf in one problem's gains
    makes that problem's samples invalid (n = 0) and leaves the other problem's statistics untouched bit for bit; a t_f of NaN
    gives n = 0 and frozen gains; a weights column with r_u = 0 gives status 2 and NaN gains for that problem alone."""
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult, guidance_gains
    nt, K = 18, 17
    P, blob = _case(nt, 0, 0)
    kw = _sigmas(P)
    xi = _xi(K, 65, 10)
    g = guidance_gains(P, blob, nt, substeps=M, **_weights(1e6))
    good = _guided(P, blob, nt, 0, 0, g, xi, kw)
    assert (good.n_valid == 65).all()
    for bad, where in ((np.nan, (0, 5, 2)), (np.inf, (0, 0, 3)), (np.nan, (0, K - 1, 0))):
        gu = g.gain_u.copy()
        gu[where] = bad
        d = _guided(P, blob, nt, 0, 0, GuidanceResult(gu, g.gain_t, g.summary, g.stretch_max, None), xi, kw)
        assert d.n_valid[0] == 0 and np.isnan(d.mean[0]).all() and not np.isfinite(d.samples[0]).all(axis=1).any()
        assert np.array_equal(_stats(d)[1], _stats(good)[1]) and np.array_equal(d.samples[1], good.samples[1])
    gt = g.gain_t.copy()
    gt[0, 1] = np.nan
    d = _guided(P, blob, nt, 0, 0, GuidanceResult(g.gain_u, gt, g.summary, g.stretch_max, None), xi, kw)
    assert d.n_valid[0] == 0 and np.array_equal(_stats(d)[1], _stats(good)[1])
    b = np.array(blob)
    b[21 * K, 0] = np.nan
    gn = guidance_gains(P, b, nt, substeps=M, **_weights(1e6))
    assert gn.status[0] == 2 and np.isnan(gn.gain_u[0]).all() and np.isnan(gn.gain_t[0]).all() and np.isnan(gn.jacobian.dtf[0]).all()
    assert np.array_equal(gn.gain_u[1], g.gain_u[1]) and np.array_equal(gn.summary[1], g.summary[1])
    d = _guided(P, b, nt, 0, 0, g, xi, kw)
    assert d.n_valid[0] == 0 and np.isnan(d.mean[0]).all() and np.array_equal(_stats(d)[1], _stats(good)[1])
    gz = guidance_gains(P, blob, nt, substeps=M, cond_weights=(1e6, 1e6, 1e6), control_weight=np.array([0.0, 1.0]), cutoff_weight=1.0, stretch_max=0.5)
    assert gz.status[0] == 2 and np.isnan(gz.gain_u[0]).all() and np.isnan(gz.gain_t[0]).all() and np.isnan(gz.max_gain[0])
    assert gz.free_controls[0] == g.free_controls[0] and gz.substeps[0] == M
    assert gz.status[1] == 0 and np.array_equal(gz.gain_u[1], g.gain_u[1]) and np.array_equal(gz.jacobian.dcontrols[1], g.jacobian.dcontrols[1])


def test_what_the_feedback_is_worth_end_to_end():
    """The figures of tests/test_guidance_reference.py from the device: backward Euler, nt = 50, solved, trimmed to 1e-12 and
    flown on the GPU (m = 18), 128 samples of default_rng(0), 50 N of thrust sigma, 1e-3 per control step, q = 1e12, r_u = r_t =
    1, stretch_max = 0.5: the guided apoapsis sigma at least 100 times below the open-loop one, the periapsis sigma at least 4
    times; steering alone at q = 1e10 worse than open loop.  Also BatchResult.disperse(guidance=...)."""
    from lunar_module_ascent_trajectory_optimiser_amd import AscentParams, guidance_gains, solve_batch, trim_batch
    nt, K = 50, 49
    P = AscentParams().as_row()[None].copy()
    r = solve_batch(P, nt, want_blob=True)
    assert (r.status == 0).all()
    t = trim_batch(P, r.blob, nt, rounds=8, tol=1e-12)
    assert t.status[0] == 0
    xi = np.random.default_rng(0).standard_normal((24 + K, 128))
    thrust = np.zeros(16)
    thrust[3] = 50.0
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch
    dkw = dict(param_sigma=thrust, control_sigma=1e-3, xi=xi)
    op = disperse_batch(P, t.blob, nt, **dkw)
    g = guidance_gains(P, t.blob, nt, **_weights(1e12))
    cl = disperse_batch(P, t.blob, nt, guidance=g, keep_samples=True, **dkw)
    g0 = guidance_gains(P, t.blob, nt, **_weights(1e10, 0.0))
    st = disperse_batch(P, t.blob, nt, guidance=g0, **dkw)
    assert g.status[0] == 0 and g0.status[0] == 0 and g.substeps[0] == 18 and np.all(g0.gain_t == 0.0)
    assert op.n_valid[0] == 128 and cl.n_valid[0] == 128
    fig = dict(open_loop=op.std[0, 7:].tolist(), closed_loop=cl.std[0, 7:].tolist(), steering_only_q1e10=st.std[0, 7:].tolist(),
               steering_only_valid=int(st.n_valid[0]), max_gain=float(g.max_gain[0]), max_cutoff_gain=float(g.max_cutoff_gain[0]),
               clipped_steps_mean=float(cl.effort[0, :, 0].mean()), largest_stretch=float(np.abs(cl.effort[0, :, 2]).max()))
    PARITY["effectiveness"]["nt50_q1e12"] = fig
    print("1-sigma of the flown periapsis / apoapsis altitude (m):", fig)
    assert cl.std[0, 8] * 100.0 <= op.std[0, 8] and cl.std[0, 7] * 4.0 <= op.std[0, 7]
    assert st.n_valid[0] < 128 or st.std[0, 7] > op.std[0, 7]
    # the trimmed blob in a BatchResult's place: the method is the function
    r.blob = t.blob
    via = r.disperse(guidance=g, keep_samples=True, **dkw)
    assert np.array_equal(_stats(via), _stats(cl)) and np.array_equal(via.effort, cl.effort)


def test_the_example_guides():
    """examples/apollo11.py --guide trims the solved model's blob, computes the gains, flies 1024 samples open loop and closed loop
    and prints both 1-sigmas; the closed loop's are the smaller ones."""
    import importlib.util
    import io
    from contextlib import redirect_stdout
    spec = importlib.util.spec_from_file_location("apollo11_example_guide", os.path.join(ROOT, "examples", "apollo11.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    m, _, _ = ex.build()
    out = io.StringIO()
    with redirect_stdout(out):
        m.solve(disp=False)
        op, cl, g = ex.guide(m, 0)
    text = out.getvalue()
    print(text)
    assert cl.n_valid[0] == 1024 and "closed loop 1-sigma" in text and "control authority" in text and g.status[0] == 0
    assert np.all(cl.std[0, 7:] < op.std[0, 7:])
