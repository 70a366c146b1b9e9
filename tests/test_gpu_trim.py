"""Flight Jacobian and trim (ascent_flight_jacobian, ascent_trim_batch) on the GPU: the kernels against the complex-step CPU
reference (tests/flight_jacobian_reference.py) at the same blob, against central differences of ascent_fly_batch itself on the
device, the trimmed blob checked by the untouched flight, and the surfaces around them.

Errors are measured per row relative to the row's largest entry, the parameter columns taken as elasticities p d/dp and the
t_f column as t_f d/dt_f.  The differences seen are collected in PARITY; with ASCENT_TRIM_PARITY_OUT=<file> they are written
there as JSON when the module is done (profiles/trim_parity.json is such a file)."""
import ctypes as C
import os

import numpy as np
import pytest

import flight_jacobian_reference as jr
import flight_reference as fr
from gpu_cases import parity_writer, points as _points, solved as _solved

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = {"jacobian_vs_reference": {}, "jacobian_vs_device_differences": {}, "trim_vs_reference": {}, "trim_flown": {}}
# Bounds of the two comparisons with the reference: 100 x the largest value measured on the device (profiles/trim_parity.json:
# Jacobian 1.3e-11, formulation 1 at nt = 18; trim 2.6e-12), never looser than 1e-9.
JAC_BOUND = 1e-9
TRIM_BOUND = 2.6e-10
CASES = [(nt, scheme, form, term) for nt in (18, 34, 50) for scheme, form in ((0, 0), (1, 0), (2, 0), (0, 1)) for term in (0, 1)]
_write_parity = parity_writer("ASCENT_TRIM_PARITY_OUT", PARITY)


def _lib():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    return _lib


def _row_scale(jac, jac_u, p16, tf):
    el = np.concatenate([jac[:, :7], jac[:, 7:23] * p16, jac[:, 23:24] * tf, jac_u], axis=1)
    s = np.abs(el).max(axis=1)
    return np.where(s > 0, s, 1.0)


def _jac_error(J, j, ref, p16, tf):
    """largest error of problem j of a FlightJacobian against the reference dict, per row scale"""
    jac = np.concatenate([J.dz0[j], J.dparams[j], J.dtf[j][:, None]], axis=1)
    scale = _row_scale(ref["jac"], ref["jac_u"], p16, tf)
    w = np.concatenate([np.ones(7), p16, [tf]])
    e1 = (np.abs(jac - ref["jac"]) * w / scale[:, None]).max()
    e2 = (np.abs(J.dcontrols[j] - ref["jac_u"]) / scale[:, None]).max()
    return max(e1, e2)


@pytest.mark.parametrize("nt,scheme,form,term", CASES)
def test_jacobian_matches_reference(nt, scheme, form, term):
    """Kernel against the complex-step reference at the same GPU blob, substeps 0 (automatic), 1 and 3, two problems."""
    from lunar_module_ascent_trajectory_optimiser_amd import flight_jacobian
    P, blob = _solved(nt, scheme, form, term)
    K = nt - 1
    worst = 0.0
    for m in (0, 1, 3):
        J = flight_jacobian(P, blob, nt, scheme=scheme, formulation=form, terminal=term, substeps=m)
        assert J.dz0.shape == (2, 9, 7) and J.dparams.shape == (2, 9, 16) and J.dtf.shape == (2, 9) and J.dcontrols.shape == (2, 9, K)
        for j in range(2):
            ref = jr.jacobian(P[j], blob[:, j], nt, form, m)
            assert np.isfinite(ref["jac"]).all() and np.isfinite(J.dparams[j]).all()
            worst = max(worst, _jac_error(J, j, ref, P[j], blob[21 * K, j]))
            for f in (10, 13, 14, 15, 8 if form == 1 else 12):        # fields the flight does not read
                assert np.all(J.dparams[:, :, f] == 0.0)
    PARITY["jacobian_vs_reference"][f"nt{nt}_scheme{scheme}_form{form}_term{term}"] = worst
    print(nt, scheme, form, term, "jacobian error / row scale", worst)
    assert worst <= JAC_BOUND


@pytest.mark.parametrize("form", [0, 1])
def test_jacobian_on_the_smallest_grid(form):
    """nt = 3 (two steps, one partly filled chunk), a synthetic blob"""
    from lunar_module_ascent_trajectory_optimiser_amd import flight_jacobian
    P = _points(1)
    blob = fr.make_blob(np.zeros((2, 7)), np.array([0.4, -0.7]), 0.05)
    J = flight_jacobian(P, blob[:, None], 3, formulation=form, substeps=0)
    ref = jr.jacobian(P[0], blob, 3, form, 0)
    e = _jac_error(J, 0, ref, P[0], 0.05)
    PARITY["jacobian_vs_reference"][f"nt3_synthetic_form{form}"] = e
    print("nt 3 form", form, e)
    assert e <= JAC_BOUND


@pytest.mark.parametrize("form", [0, 1])
def test_jacobian_matches_central_differences_of_the_flight_on_the_device(form):
    """Central differences of ascent_fly_batch itself, all perturbed copies flown as one batch, explicit substeps m = 4 held
    fixed, nt = 34: every non-zero parameter column, t_f, and u_k at k = 1, 16, 17, K (both sides of the chunk boundaries);
    relative step 1e-6 (absolute for the controls).  <= 1e-6 of the row scale: the noise of these differences measured on
    the CPU is 2e-9."""
    from lunar_module_ascent_trajectory_optimiser_amd import flight_jacobian, fly_batch
    nt, K, m = 34, 33, 4
    P, blob = _solved(nt, 0, form, 0)
    p16, b0 = P[0], blob[:, 0]
    tf = b0[21 * K]
    J = flight_jacobian(P[:1], blob[:, :1], nt, formulation=form, substeps=m)
    cols = [("p", i) for i in range(16) if i not in (10, 13, 14, 15, 8 if form == 1 else 12) and p16[i] != 0.0]
    cols += [("tf", 0)] + [("u", k) for k in (1, 16, 17, K)]
    PP, BB, hs = [], [], []
    for kind, i in cols:
        for sgn in (1.0, -1.0):
            p, b = p16.copy(), b0.copy()
            if kind == "p":
                h = 1e-6 * p16[i]; p[i] += sgn * h
            elif kind == "tf":
                h = 1e-6 * tf; b[21 * K] += sgn * h
            else:
                h = 1e-6; b[7 * K + i - 1] += sgn * h
            PP.append(p); BB.append(b)
        hs.append(h)
    f = fly_batch(np.array(PP), np.ascontiguousarray(np.array(BB).T), nt, formulation=form, substeps=m, want_local=False)
    end = np.concatenate([f.traj[:, [0, 1, 2, 3, 6, 7, 9], -1], f.summary[:, 2:4]], axis=1)
    scale = _row_scale(np.concatenate([J.dz0[0], J.dparams[0], J.dtf[0][:, None]], axis=1), J.dcontrols[0], p16, tf)
    worst = 0.0
    for n, (kind, i) in enumerate(cols):
        fd = (end[2 * n] - end[2 * n + 1]) / (2 * hs[n])
        mine, w = (J.dparams[0, :, i], p16[i]) if kind == "p" else (J.dtf[0], tf) if kind == "tf" else (J.dcontrols[0, :, i - 1], 1.0)
        worst = max(worst, (np.abs(fd - mine) * w / scale).max())
    PARITY["jacobian_vs_device_differences"][f"form{form}"] = worst
    print("form", form, "jacobian against device central differences / row scale", worst)
    assert worst <= 1e-6


@pytest.mark.parametrize("nt,scheme,form,term", CASES)
def test_trim_matches_reference_trim(nt, scheme, form, term):
    """Kernel trim against the numpy trim from the same blob, substeps 0, 1 and 3, one of the two problems: t_f, u, the flown
    states and the summary (status, rounds and free controls equal; residuals to the bound in absolute scaled units; SI rows
    relative to r_peri)."""
    from lunar_module_ascent_trajectory_optimiser_amd import trim_batch
    P, blob = _solved(nt, scheme, form, term)
    K = nt - 1
    j = (nt + scheme + term) % 2
    worst = 0.0
    for m in (0, 1, 3):
        t = trim_batch(P, blob, nt, scheme=scheme, formulation=form, terminal=term, substeps=m)
        ref = jr.trim(P[j], blob[:, j], nt, form, term, m)
        s, rs = t.summary[j], ref["summary"]
        print(nt, scheme, form, term, "m", m, "device", s, "reference history", ref["history"])
        assert s[0] == rs[0] and s[1] == rs[1] and s[6] == rs[6], (s, rs)
        S = P[j, 9]
        d = [abs(t.tf[j] - ref["tf"]), np.abs(t.controls[j] - ref["u"]).max(), np.abs(t.blob[:7 * K, j] - ref["blob"][:7 * K]).max(),
             abs(s[2] - rs[2]), abs(s[3] - rs[3]), abs(s[4] - rs[4]) / P[j, 11], abs(s[5] - rs[5]), abs(s[7] - rs[7]) / S,
             abs(s[8] - rs[8]) / S, abs(s[9] - rs[9])]
        worst = max(worst, max(d))
        assert np.array_equal(t.blob[8 * K:21 * K, j], blob[8 * K:21 * K, j]) and np.array_equal(t.blob[21 * K + 1:, j], blob[21 * K + 1:, j])
    PARITY["trim_vs_reference"][f"nt{nt}_scheme{scheme}_form{form}_term{term}"] = worst
    print(nt, scheme, form, term, "trim difference", worst)
    assert worst <= TRIM_BOUND


@pytest.mark.parametrize("nt,scheme,form,term", CASES)
def test_trimmed_blob_flown_by_the_untouched_flight(nt, scheme, form, term):
    """ascent_fly_batch on trim_blob_out: the conditions recomputed in numpy from the flown end state are <= 1e-9, the flown
    apsides are the NLP's own (rows 4 / 5 of the flight of the untrimmed blob) to 1e-3 m, the local error is exactly 0, |u| <= 1
    and saturated controls are untouched.  Trimmed to tol 1e-12: a condition of 1e-10 in the scaled speed^2 is 0.03 m of
    periapsis.  Trimming the trimmed blob uses 0 rounds and returns the same bits."""
    from lunar_module_ascent_trajectory_optimiser_amd import trim_batch, fly_batch
    P, blob = _solved(nt, scheme, form, term)
    K = nt - 1
    kw = dict(scheme=scheme, formulation=form, terminal=term)
    t = trim_batch(P, blob, nt, tol=1e-12, **kw)
    assert (t.status == 0).all() and (t.rounds <= 6).all() and (t.residual <= 1e-12).all(), t.summary
    before, after = fly_batch(P, blob, nt, **kw), fly_batch(P, t.blob, nt, **kw)
    worst = dict(conditions=0.0, apsides_m=0.0)
    for j in range(P.shape[0]):
        c, _ = jr.conditions(P[j], after.traj[j, [0, 1, 2, 3], -1], term)
        worst["conditions"] = max(worst["conditions"], np.abs(c).max())
        worst["apsides_m"] = max(worst["apsides_m"], np.abs(after.summary[j, 2:4] - before.summary[j, 4:6]).max())
    PARITY["trim_flown"][f"nt{nt}_scheme{scheme}_form{form}_term{term}"] = worst
    print(nt, scheme, form, term, worst, "rounds", t.rounds, "delta t_f (s)", t.delta_tf_seconds)
    assert worst["conditions"] <= 1e-9 and worst["apsides_m"] <= 1e-3
    assert np.all(after.local_error == 0.0) and np.all(after.summary[:, 6:8] == 0.0) and np.all(after.summary[:, 0:2] == 0.0)
    assert np.array_equal(after.summary[:, 2:4], t.summary[:, 7:9])
    u0, u1 = blob[7 * K:8 * K], t.blob[7 * K:8 * K]
    sat = np.abs(u0) >= 0.999
    assert np.abs(u1).max() <= 1.0 and np.array_equal(u1[sat], u0[sat])
    again = trim_batch(P, t.blob, nt, tol=1e-12, **kw)
    assert (again.rounds == 0).all() and (again.status == 0).all()
    assert np.array_equal(again.blob, t.blob)


def test_device_pointers_null_controls_and_batch_independence():
    """Host and device pointers on torch's stream agree bit for bit (Jacobian and trim); jac_u_out = NULL changes nothing else;
    each of 5 problems alone and repeated through a batch of 70 gives the same bits."""
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import flight_jacobian, trim_batch
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    nt, K = 34, 33
    P, blob = _solved(nt, 0, 0, 0, 5)
    B = 5
    host = flight_jacobian(P, blob, nt)
    htrim = trim_batch(P, blob, nt)
    L, lib = _lib().load(), _lib()
    pt = torch.from_numpy(np.array(P)).cuda()
    bt = torch.from_numpy(np.array(blob)).cuda()
    jt = torch.empty((9, 24, B), dtype=torch.float64, device="cuda")
    ut = torch.empty((9, K, B), dtype=torch.float64, device="cuda")
    ot = torch.empty((21 * K + 10, B), dtype=torch.float64, device="cuda")
    st = torch.empty((10, B), dtype=torch.float64, device="cuda")
    o = _opts(nt, 0, 1.0, 0, 0.0)
    stream = torch.cuda.current_stream().cuda_stream
    lib.check(L.ascent_flight_jacobian(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), 0, jt.data_ptr(), ut.data_ptr(), 0, C.c_void_p(stream), 1))
    lib.check(L.ascent_trim_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), 0, 0, 0.0, ot.data_ptr(), st.data_ptr(), 0, C.c_void_p(stream), 1))
    torch.cuda.synchronize()
    j = jt.cpu().numpy().transpose(2, 0, 1)
    assert np.array_equal(j[:, :, :7], host.dz0) and np.array_equal(j[:, :, 7:23], host.dparams) and np.array_equal(j[:, :, 23], host.dtf)
    assert np.array_equal(ut.cpu().numpy().transpose(2, 0, 1), host.dcontrols)
    assert np.array_equal(ot.cpu().numpy(), htrim.blob) and np.array_equal(st.cpu().numpy().T, htrim.summary)
    only = flight_jacobian(P, blob, nt, want_controls=False)
    assert only.dcontrols is None and np.array_equal(only.dparams, host.dparams) and np.array_equal(only.dz0, host.dz0)
    assert np.array_equal(only.dtf, host.dtf)
    idx = np.arange(70) % 5
    Pb, bb = P[idx], np.ascontiguousarray(blob[:, idx])
    big, bigt = flight_jacobian(Pb, bb, nt), trim_batch(Pb, bb, nt)
    for q in range(5):
        one, onet = flight_jacobian(P[q:q + 1], blob[:, q:q + 1], nt), trim_batch(P[q:q + 1], blob[:, q:q + 1], nt)
        assert np.array_equal(one.dparams[0], host.dparams[q]) and np.array_equal(one.dcontrols[0], host.dcontrols[q])
        assert np.array_equal(onet.blob[:, 0], htrim.blob[:, q]) and np.array_equal(onet.summary[0], htrim.summary[q])
    assert np.array_equal(big.dparams, host.dparams[idx]) and np.array_equal(big.dcontrols, host.dcontrols[idx])
    assert np.array_equal(big.dz0, host.dz0[idx]) and np.array_equal(big.dtf, host.dtf[idx])
    assert np.array_equal(bigt.blob, htrim.blob[:, idx]) and np.array_equal(bigt.summary, htrim.summary[idx])


def test_unconverged_input_returns_and_freezes():
    """Blobs of solves stopped after 2 iterations, and blobs with t_f NaN, inf, 1e300 (4096 substeps on 49 steps: bounded) and
    -1: both calls return 0; the trim status is 2 or the rows are NaN for the non-finite and huge t_f, and a status of the
    three for the others."""
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch, flight_jacobian, trim_batch
    nt, K = 50, 49
    P = _points(3)
    r = solve_batch(P, nt, max_iter=2, coarse_nodes=-1, want_blob=True)
    assert (r.status != 0).all()
    J, t = flight_jacobian(P, r.blob, nt), trim_batch(P, r.blob, nt)
    assert J.dparams.shape == (3, 9, 16) and np.isin(t.status, (0, 1, 2)).all()
    good = _solved(nt, 0, 0, 0)[1][:, :1]
    for tf in (np.nan, np.inf, 1e300, -1.0):
        blob = np.array(good)
        blob[21 * K] = tf
        J, t = flight_jacobian(P[:1], blob, nt), trim_batch(P[:1], blob, nt)
        print("t_f", tf, "status", t.status, "rounds", t.rounds, "residual", t.residual)
        if tf == -1.0:
            assert np.isin(t.status, (0, 1, 2)).all()
        else:
            assert t.status[0] == 2 or np.isnan(t.summary[0]).all()
            assert t.rounds[0] == 0 and not np.isfinite(J.dparams[0, :4, :10]).any()


def test_sweep_converges_and_keeps_the_angle_in_bounds():
    """A 7 x 6 Isp x dry-mass sweep at nt = 50: every problem converges within 6 rounds and the trimmed flight keeps
    0 <= angle <= angle_ub (summary row 9 is 0); solve_batch(trim=True) is the same call."""
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch, sweep_isp_drymass, trim_batch
    nt = 50
    P = sweep_isp_drymass(7, 6)
    r = solve_batch(P, nt, want_blob=True, trim=True)
    assert (r.status == 0).all()
    t = r.trim
    print("sweep: rounds", t.rounds, "residual max", t.residual.max(), "max |du|", t.max_delta_u.max(), "dt_f (s)", t.delta_tf_seconds.min(),
          t.delta_tf_seconds.max())
    assert (t.status == 0).all() and (t.rounds <= 6).all() and (t.residual <= 1e-10).all()
    assert np.all(t.angle_violation == 0.0)
    direct = trim_batch(P, r.blob, nt)
    assert np.array_equal(direct.blob, t.blob) and np.array_equal(direct.summary, t.summary)


def test_the_example_trims():
    """examples/apollo11.py --trim goes through trim_batch on the solved model's blob and prints before / after."""
    import importlib.util
    import io
    from contextlib import redirect_stdout
    spec = importlib.util.spec_from_file_location("apollo11_example_trim", os.path.join(ROOT, "examples", "apollo11.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    m, _, _ = ex.build()
    out = io.StringIO()
    with redirect_stdout(out):
        m.solve(disp=False)
        t = ex.trim(m, 0)
    text = out.getvalue()
    assert t.status[0] == 0 and t.residual[0] <= 1e-10 and "before" in text and "after" in text
    assert abs(t.flown_apoapsis_alt[0] - 17703.0) <= 0.05 and abs(t.tf[0] * 470.0 - 435.23) <= 0.05, text
