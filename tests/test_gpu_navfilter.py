"""The navigation filter on the GPU (ascent_navigation_filter, ascent_covariance_filtered_batch; navigation_filter,
linear_corridor(filter=...)): the Kalman gains, the filter's own covariance, the corridor under the filter and the true covariance
of the estimation error against the CPU reference (tests/navfilter_reference.py: plain recursion for the design, explicit
superposition for the truth), the consistency of the two kernels with each other, the exact structure and the bitwise promises of
the header, and bounded garbage.

The cases are gpu_cases.CASES, substeps = 2, two problems, open loop and the device's own guidance gains at q = 1e6 and 1e12.  The
measurements are the unit rows of x, y, xdot, ydot, the first M of them, sigma_i = 1e-4 and sigma_nav = 1e-3 in scaled units; on the
CPU the reference design has s > 0 at every update and status 0 for every case (asserted where the reference is run).  The scales
are those of tests/test_gpu_lincov.py; the rows of e are in scaled units and a gain column is taken relative to max(1, its
infinity norm).  Every bound is max(FLOOR, 100 x the reference's own float64-against-longdouble difference of the same quantity),
computed from the reference alone.  The differences seen are collected in PARITY; with ASCENT_NAVFILTER_PARITY_OUT=<file> they are
written there as JSON when the module is done (profiles/navfilter_parity.json is such a file)."""
import ctypes as C
import functools

import numpy as np
import pytest

import guidance_reference as gr
import lincov_reference as lr
import navfilter_reference as nr
from gpu_cases import (CASES, FLOOR, M, case as _case, col_scales as _col_scales, gains as _gains, norm_cov as _norm_cov,
                       norm_jac as _norm_jac, parity_writer)

pytestmark = pytest.mark.gpu

PARITY = {"design_vs_reference": {}, "corridor_vs_reference": {}, "two_kernel_consistency": {}}
KINDS = [("open", 0.0), ("guided", 1e6), ("guided", 1e12)]
LD = np.longdouble
H4 = np.eye(7)[[0, 1, 2, 3]]
SIG_M, SIG_NAV, SIG_U = 1e-4, 1e-3, 1e-3
_write_parity = parity_writer("ASCENT_NAVFILTER_PARITY_OUT", PARITY)


def _filter(P, blob, nt, scheme, form, n_meas, stride, **kw):
    from lunar_module_ascent_trajectory_optimiser_amd import navigation_filter
    kw.setdefault("control_sigma", SIG_U)
    return navigation_filter(P, blob, nt, nav_sigma=SIG_NAV, meas_rows=H4[:n_meas], meas_sigma=SIG_M, meas_stride=stride, scheme=scheme,
                             formulation=form, substeps=M, **kw)


@functools.lru_cache(maxsize=None)
def _designed(nt, scheme, form, n_meas, stride):
    P, blob = _case(nt, scheme, form)
    nf = _filter(P, blob, nt, scheme, form, n_meas, stride)
    for a in (nf.gain_l, nf.cov):
        a.setflags(write=False)
    return nf


def _corridor(P, blob, nt, scheme, form, g, nf, **kw):
    from lunar_module_ascent_trajectory_optimiser_amd import linear_corridor
    kw.setdefault("substeps", M)
    return linear_corridor(P, blob, nt, guidance=g, filter=nf, scheme=scheme, formulation=form, **kw)


def _unit_sigmas(P):
    """every sigma of the 24 constants one unit of its column's scale, sigma_u = 1 (tests/test_gpu_lincov.py)"""
    cs = np.array([_col_scales(p) for p in P])
    return dict(z0_sigma=cs[:, :7], param_sigma=cs[:, lr.C_P:lr.C_TF], tf_sigma=cs[:, lr.C_TF], control_sigma=1.0)


def _all(lc):
    """everything a filtered LinearCorridor holds, as one array per problem and node"""
    B, NJ = lc.nominal.shape[:2]
    parts = [lc.nominal, lc.cov.reshape(B, NJ, -1), lc.nav_cov.reshape(B, NJ, -1)]
    parts += [] if lc.jacobian is None else [lc.jacobian.reshape(B, NJ, -1), lc.nav_jacobian.reshape(B, NJ, -1)]
    return np.concatenate(parts, axis=2)


def _law(g, j):
    return {} if g is None else dict(gain_u=g.gain_u[j], gain_t=g.gain_t[j], smax=float(g.stretch_max[j]))


def _figure(dev, ref, norm):
    """device error, the reference's own gap and the bound of one quantity; ref: {dtype: array}"""
    want = norm(ref[LD])
    gap = float(np.abs(norm(ref[np.float64]) - want).max())
    assert np.isfinite(dev).all()
    return dict(device_error=float(np.abs(norm(dev) - want).max()), reference_gap=gap, bound=max(FLOOR, 100.0 * gap),
                largest_entry=float(np.abs(want).max()))


REL_FLOOR = 1e-12


def _sd(Pk):
    """(K, 7) standard deviations of a stack of covariances, as the scale of a relative difference.  A state nothing reaches has none
    (formulation 1 sets the angle from the control and holds its rate at 0: their variances are exactly 0 after the first step), so
    one below 1e-9 of the node's largest takes the largest, as tests/test_navfilter_reference.py does"""
    sd = np.sqrt(np.einsum("kaa->ka", np.asarray(Pk, dtype=np.float64)))
    top = sd.max(axis=1, keepdims=True)
    return np.where(sd < 1e-9 * top, top, sd)


def _rel(a, b, sd):
    """the largest difference of two stacks of covariances in units of sd_a sd_b"""
    return float((np.abs(np.asarray(a - b, dtype=np.float64)) / (sd[:, :, None] * sd[:, None, :])).max())


@functools.lru_cache(maxsize=None)
def _design_compared(nt, scheme, form, n_meas, stride):
    """gain_l and pfilt_out of a case against the reference design.  -> (nf, per problem dict(gain / covariance: figures))"""
    P, blob = _case(nt, scheme, form)
    K = nt - 1
    nf = _designed(nt, scheme, form, n_meas, stride)
    assert nf.gain_l.shape == (P.shape[0], K, n_meas, 7) and nf.cov.shape == (P.shape[0], K, 7, 7)
    assert (nf.status == 0).all() and (nf.first_bad == 0).all() and (nf.meas_nodes == K // stride).all() and (nf.substeps == M).all()
    assert np.array_equal(nf.cov, nf.cov.transpose(0, 1, 3, 2))
    fig = {}
    for j in range(P.shape[0]):
        ref = {}
        for dt in (np.float64, LD):
            rec = gr.records(P[j], blob[:, j], nt, form, M, dt)
            ref[dt] = nr.design(rec, np.full(7, SIG_NAV), H4[:n_meas], np.full(n_meas, SIG_M), stride, np.full(K, SIG_U), None, dt)
            assert ref[dt]["status"] == 0 and all(s > 0 and np.isfinite(s) for _, _, s in ref[dt]["s"])
        gs = nr.gain_scales(ref[LD]["gain_l"])[:, :, None]
        fig[f"problem{j}"] = dict(gain=_figure(nf.gain_l[j], {dt: r["gain_l"] for dt, r in ref.items()}, lambda a: np.asarray(a / gs, dtype=np.float64)),
                                  covariance=_figure(nf.cov[j], {dt: r["P"] for dt, r in ref.items()}, lambda a: np.asarray(a, dtype=np.float64)))
        fig[f"problem{j}"]["covariance"]["relative_gap"] = _rel(ref[np.float64]["P"], ref[LD]["P"], _sd(ref[LD]["P"]))
        print(nt, scheme, form, n_meas, stride, "problem", j, fig[f"problem{j}"])
    PARITY["design_vs_reference"][f"nt{nt}_scheme{scheme}_form{form}_M{n_meas}_stride{stride}"] = fig
    return nf, fig


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("n_meas", [1, 2, 4])
@pytest.mark.parametrize("nt,scheme,form", CASES)
def test_gains_and_filter_covariance_match_reference(nt, scheme, form, n_meas, stride):
    """gain_l_out and pfilt_out, every node, against the longdouble recursion; sigma_u = 1e-3.  Check 1 of the issue at stride 1; the
    stride 4 skips nodes (K = 2: no measurement at all)."""
    _, fig = _design_compared(nt, scheme, form, n_meas, stride)
    for k, v in fig.items():
        for name, f in v.items():
            assert f["device_error"] <= f["bound"], (k, name, f)


@functools.lru_cache(maxsize=None)
def _compared(nt, scheme, form, kind, q, n_meas):
    """The stride-1 corridor under the device's own filter (measurements at every node) at unit relative sigmas against the
    longdouble superposition.  noise / nav_noise: the covariances with only eps (sigma_u = 1) and v on."""
    P, blob = _case(nt, scheme, form)
    K = nt - 1
    g = _gains(nt, scheme, form, kind, q)
    nf = _designed(nt, scheme, form, n_meas, 1)
    dev = _corridor(P, blob, nt, scheme, form, g, nf, **_unit_sigmas(P))
    only = _corridor(P, blob, nt, scheme, form, g, nf, control_sigma=1.0, nav_sigma=np.zeros(7), want_jacobian=False)
    B = P.shape[0]
    assert dev.jacobian.shape == (B, K, 10, 32) and dev.cov.shape == (B, K, 10, 10) and np.array_equal(dev.nodes, np.arange(1, K + 1))
    assert dev.nav_jacobian.shape == (B, K, 7, 32) and dev.nav_cov.shape == (B, K, 7, 7) and dev.nav_std.shape == (B, K, 7)
    assert only.jacobian is None and only.nav_jacobian is None
    fig = {}
    for j in range(B):
        law, cs = _law(g, j), _col_scales(P[j])
        ref, ref_only = {}, {}
        for dt in (np.float64, LD):
            rec = gr.records(P[j], blob[:, j], nt, form, M, dt)
            a = (P[j], blob[:, j], nt)
            kw = dict(formulation=form, substeps=M, dtype=dt, rec=rec, **law)
            ref[dt] = nr.corridor(*a, cs[:24], np.full(7, SIG_NAV), nf.gain_l[j], H4[:n_meas], np.full(n_meas, SIG_M), 1, np.ones(K), **kw)
            ref_only[dt] = nr.corridor(*a, np.zeros(24), np.zeros(7), nf.gain_l[j], H4[:n_meas], np.full(n_meas, SIG_M), 1, np.ones(K), **kw)
        rows = lr.row_scales(P[j], law.get("gain_u"), None, K)
        f64 = lambda a: np.asarray(a, dtype=np.float64)
        pick = lambda r, key: {dt: v[key] for dt, v in r.items()}
        out = dict(jacobian=_figure(dev.jacobian[j], pick(ref, "S"), lambda a: _norm_jac(a, rows, cs)),
                   covariance=_figure(dev.cov[j], pick(ref, "cov"), lambda a: _norm_cov(a, rows)),
                   noise=_figure(only.cov[j], pick(ref_only, "noise"), lambda a: _norm_cov(a, rows)),
                   nav_jacobian=_figure(dev.nav_jacobian[j], pick(ref, "nav_jac"), lambda a: f64(a * cs[None, None, :])),
                   nav_covariance=_figure(dev.nav_cov[j], pick(ref, "nav_cov"), f64),
                   nav_noise=_figure(only.nav_cov[j], pick(ref_only, "nav_noise"), f64))
        nom = np.abs(dev.nominal[j] - ref[np.float64]["nominal"].astype(np.float64)) / rows
        out["nominal"] = dict(device_error=float(nom[:, :8].max()), reference_gap=0.0, bound=FLOOR)
        fig[f"problem{j}"] = out
        print(nt, scheme, form, kind, q, n_meas, "problem", j, out)
    PARITY["corridor_vs_reference"][f"nt{nt}_scheme{scheme}_form{form}_{kind}_q{q:g}_M{n_meas}"] = fig
    return dev, only, fig


@pytest.mark.parametrize("n_meas", [1, 2, 4])
@pytest.mark.parametrize("kind,q", KINDS)
@pytest.mark.parametrize("nt,scheme,form", CASES)
def test_corridor_under_the_filter_matches_reference(nt, scheme, form, kind, q, n_meas):
    """cov_out, nav_cov_out, jac_hist_out and nav_jac_out at stride 1, every node, against the longdouble superposition flown with
    the device's own guidance gains and the device's own filter gains; every sigma one unit of its column's scale, sigma_u = 1,
    sigma_nav = 1e-3.  Exact on the way: cov_out and nav_cov_out symmetric by layout, column 31 exactly 0, the nominal rows the
    parent call's bits."""
    from lunar_module_ascent_trajectory_optimiser_amd import linear_corridor
    dev, only, fig = _compared(nt, scheme, form, kind, q, n_meas)
    for k, v in fig.items():
        for name, f in v.items():
            assert f["device_error"] <= f["bound"], (k, name, f)
    assert np.array_equal(dev.cov, dev.cov.transpose(0, 1, 3, 2)) and np.array_equal(dev.nav_cov, dev.nav_cov.transpose(0, 1, 3, 2))
    assert np.all(dev.jacobian[..., 31] == 0.0) and np.all(dev.nav_jacobian[..., 31] == 0.0)
    P, blob = _case(nt, scheme, form)
    parent = linear_corridor(P, blob, nt, guidance=_gains(nt, scheme, form, kind, q), scheme=scheme, formulation=form, substeps=M, **_unit_sigmas(P))
    assert np.array_equal(dev.nominal, parent.nominal) and np.array_equal(only.nominal, parent.nominal)


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("kind,q", KINDS)
@pytest.mark.parametrize("nt,scheme,form", CASES)
def test_two_kernel_consistency(nt, scheme, form, kind, q, stride):
    """l_lincov_filtered fed n_filter's own gains under the identity's conditions -- no sigma on the fields or t_f, filter_q null, the
    design's sigma_u and sigma_nav; z_0 dispersed, which is no error of the estimate -- returns nav_cov_out equal to pfilt_out at every
    node within the sum of the two reference bounds (the design's for P-hat, the superposition's for nav_cov, each max(FLOOR, 100 x its
    float64-against-longdouble gap), scaled units).  M = 4.
    The entries of P-hat are 1e-6 .. 1e-8 here, so that absolute bound alone would pass a relative error of 1e-4; the same difference
    is therefore also held in units of sqrt(P_aa P_bb) (_sd) against the sum of the two references' float64-against-longdouble gaps
    in those units, each max(REL_FLOOR, 100 x gap).  REL_FLOOR = 1e-12: K <= 33 steps, each entry a sum of about 100 products
    rounded to 1.1e-16, is 4e-13 if every rounding had the same sign."""
    P, blob = _case(nt, scheme, form)
    K, n_meas = nt - 1, 4
    g = _gains(nt, scheme, form, kind, q)
    nf, dfig = _design_compared(nt, scheme, form, n_meas, stride)
    lc = _corridor(P, blob, nt, scheme, form, g, nf, control_sigma=SIG_U, z0_sigma=1e-3, want_jacobian=False)
    out = {}
    for j in range(P.shape[0]):
        ref = {}
        for dt in (np.float64, LD):
            rec = gr.records(P[j], blob[:, j], nt, form, M, dt)
            sigma = np.zeros(24)
            sigma[:7] = 1e-3
            ref[dt] = nr.corridor(P[j], blob[:, j], nt, sigma, np.full(7, SIG_NAV), nf.gain_l[j], H4, np.full(n_meas, SIG_M), stride,
                                  np.full(K, SIG_U), formulation=form, substeps=M, dtype=dt, rec=rec, **_law(g, j))["nav_cov"]
        b2 = max(FLOOR, 100.0 * float(np.abs((ref[np.float64] - ref[LD]).astype(np.float64)).max()))
        b1 = dfig[f"problem{j}"]["covariance"]["bound"]
        d = np.abs(lc.nav_cov[j] - nf.cov[j])
        sd = _sd(ref[LD])
        r1 = max(REL_FLOOR, 100.0 * dfig[f"problem{j}"]["covariance"]["relative_gap"])
        r2 = max(REL_FLOOR, 100.0 * _rel(ref[np.float64], ref[LD], sd))
        out[f"problem{j}"] = dict(difference=float(d.max()), tolerance=b1 + b2, largest_entry=float(np.abs(nf.cov[j]).max()),
                                  relative_difference=_rel(lc.nav_cov[j], nf.cov[j], sd), relative_tolerance=r1 + r2)
        print(nt, scheme, form, kind, q, stride, "problem", j, out[f"problem{j}"])
    PARITY["two_kernel_consistency"][f"nt{nt}_scheme{scheme}_form{form}_{kind}_q{q:g}_stride{stride}"] = out
    for k, v in out.items():
        assert v["difference"] <= v["tolerance"] and v["relative_difference"] <= v["relative_tolerance"], (k, v)


def test_open_loop_rows_do_not_depend_on_the_filter():
    """gain_u null: the ten rows are the same bits under two different filters (M = 1 at every node; M = 4 every fourth node with
    the gains halved), their columns 24..30 and row 9 exactly 0, and the covariance's row 9 exactly 0.  K = 17 and K = 33."""
    from lunar_module_ascent_trajectory_optimiser_amd import NavigationFilter
    for nt in (18, 34):
        P, blob = _case(nt, 0, 0)
        a, b = _designed(nt, 0, 0, 1, 1), _designed(nt, 0, 0, 4, 4)
        b = NavigationFilter(0.5 * b.gain_l, b.cov, b.status, b.first_bad, b.meas_nodes, b.substeps, b.nav_sigma, b.meas_rows, b.meas_sigma,
                             b.meas_stride, b.control_sigma, b.process_sigma)
        la, lb = (_corridor(P, blob, nt, 0, 0, None, f, **_unit_sigmas(P)) for f in (a, b))
        assert np.array_equal(la.cov, lb.cov) and np.array_equal(la.jacobian, lb.jacobian) and np.array_equal(la.nominal, lb.nominal)
        assert not np.array_equal(la.nav_cov, lb.nav_cov)
        assert np.all(la.jacobian[..., 24:31] == 0.0) and np.all(la.jacobian[:, :, 9] == 0.0) and np.all(la.cov[:, :, 9] == 0.0)
        assert np.isfinite(_all(la)).all() and np.isfinite(_all(lb)).all()


@pytest.mark.parametrize("nt", [3, 18, 34])
def test_gains_are_zero_off_the_measurement_nodes(nt):
    """meas_stride 4: gain_l is exactly 0 at the other nodes and not at those; meas_stride K + 1: all-zero gains, no measurement
    node, and P-hat the pure propagation -- the same bits whatever M, and the reference's propagation within its bound."""
    P, blob = _case(nt, 0, 0)
    K = nt - 1
    nf = _designed(nt, 0, 0, 4, 4)
    on = np.arange(1, K + 1) % 4 == 0
    assert np.all(nf.gain_l[:, ~on] == 0.0) and np.all(np.abs(nf.gain_l[:, on]).max(axis=(2, 3)) > 0) and (nf.meas_nodes == K // 4).all()
    none4, none1 = _designed(nt, 0, 0, 4, K + 1), _designed(nt, 0, 0, 1, K + 1)
    assert np.all(none4.gain_l == 0.0) and np.all(none1.gain_l == 0.0) and (none4.meas_nodes == 0).all() and (none4.status == 0).all()
    assert np.array_equal(none4.cov, none1.cov)
    _, fig = _design_compared(nt, 0, 0, 4, K + 1)
    for k, v in fig.items():
        assert v["covariance"]["device_error"] <= v["covariance"]["bound"], (k, v)


def _device_calls(P, blob, nt, g, n_meas, meas_stride, node_stride, meas_sigma=None, meas_rows=None, want_optional=True, nav_sigma=None):
    """both entry points with device pointers on torch's stream -> (gain_l (M, 7, K, B), pfilt (28, K, B), summary (4, B), nominal,
    cov, nav_cov, jac, nav_jac) as numpy arrays in the C ABI's layouts; the corridor is fed the filter call's gains on the device.
    want_optional False: pfilt_out, jac_hist_out and nav_jac_out are null, and their arrays here keep the 7.25 they were filled with.
    nav_sigma (7, B): sigma_nav of both calls instead of SIG_NAV"""
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts, history_nodes
    L = _lib.load()
    _lib.require_single_hip_runtime()
    B, K = P.shape[0], nt - 1
    NJ = len(history_nodes(K, node_stride))
    o = _opts(nt, 0, 1.0, 0, 0.0)
    stream = torch.cuda.current_stream().cuda_stream
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    new = lambda *shape: torch.full(shape, 7.25, dtype=torch.float64, device="cuda")
    cs = np.array([_col_scales(p) for p in P])
    h = np.broadcast_to(H4[:n_meas] if meas_rows is None else meas_rows, (B, n_meas, 7))
    sg = np.broadcast_to(np.full(n_meas, SIG_M) if meas_sigma is None else meas_sigma, (B, n_meas))
    pt, bt, sn, su, ht, st, sig = (dev(P), dev(blob), dev(np.full((7, B), SIG_NAV) if nav_sigma is None else nav_sigma), dev(np.full((K, B), SIG_U)), dev(np.moveaxis(h, 0, -1)),
                                  dev(sg.T), dev(cs[:, :24].T))
    law = [None] * 3 if g is None else [dev(g.gain_u.transpose(2, 1, 0)), dev(g.gain_t.T), dev(g.stretch_max)]
    gl, pf, sm = new(n_meas, 7, K, B), new(28, K, B), new(4, B)
    _lib.check(L.ascent_navigation_filter(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), M, sn.data_ptr(), su.data_ptr(), None, ht.data_ptr(),
                                          st.data_ptr(), n_meas, meas_stride, gl.data_ptr(), pf.data_ptr() if want_optional else None, sm.data_ptr(), 0,
                                          C.c_void_p(stream), 1))
    nom, cov, ncov, jac, njac = new(10, NJ, B), new(55, NJ, B), new(28, NJ, B), new(10, 32, NJ, B), new(7, 32, NJ, B)
    opt = [jac.data_ptr(), njac.data_ptr()] if want_optional else [None, None]
    _lib.check(L.ascent_covariance_filtered_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), M, sig.data_ptr(), su.data_ptr(),
                                                  *[None if a is None else a.data_ptr() for a in law], sn.data_ptr(), gl.data_ptr(), ht.data_ptr(),
                                                  st.data_ptr(), n_meas, meas_stride, node_stride, nom.data_ptr(), cov.data_ptr(), ncov.data_ptr(),
                                                  *opt, 0, C.c_void_p(stream), 1))
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (gl, pf, sm, nom, cov, ncov, jac, njac))


def _host_pair(P, blob, nt, g, n_meas, meas_stride, history=True, **kw):
    """the same two calls with host pointers through the front ends: (nf, lc); sigma of the 24 constants one unit of its scale"""
    nf = _filter(P, blob, nt, 0, 0, n_meas, meas_stride)
    u = _unit_sigmas(P)
    u["control_sigma"] = SIG_U
    return nf, _corridor(P, blob, nt, 0, 0, g, nf, history=history, **u, **kw)


def test_batch_independence_pointers_strides_and_optional_outputs():
    """nt = 34 (three chunks), guided at q = 1e6, M = 4 every fourth node, node stride 5 (the last node is not a multiple).  A problem
    gives the same bits alone as inside batches of 2 and 65; a node's rows do not depend on node_stride (1, 5, K); host pointers and
    device pointers on torch's stream give the same bits; with pfilt_out, jac_hist_out and nav_jac_out null the other outputs
    (gain_l_out and summary_out of the filter call among them) are the same bits and the arrays not handed over are not written."""
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult
    nt, K, n_meas, ms = 34, 33, 4, 4
    P, blob = _case(nt, 0, 0)
    g = _gains(nt, 0, 0, "guided", 1e6)
    sub = lambda idx: GuidanceResult(g.gain_u[idx], g.gain_t[idx], g.summary[idx], g.stretch_max[idx], None)
    nf, full = _host_pair(P, blob, nt, g, n_meas, ms)
    assert np.isfinite(_all(full)).all() and (nf.status == 0).all()
    for idx in (np.array([0]), np.array([1]), np.arange(65) % 2):
        nf_i, lc_i = _host_pair(P[idx], np.ascontiguousarray(blob[:, idx]), nt, sub(idx), n_meas, ms)
        assert np.array_equal(nf_i.gain_l, nf.gain_l[idx]) and np.array_equal(nf_i.cov, nf.cov[idx]) and np.array_equal(_all(lc_i), _all(full)[idx])
    for stride, nodes in ((5, [5, 10, 15, 20, 25, 30, 33]), (K, [K])):
        _, lc = _host_pair(P, blob, nt, g, n_meas, ms, history=stride)
        assert np.array_equal(lc.nodes, nodes) and np.array_equal(_all(lc), _all(full)[:, np.searchsorted(full.nodes, nodes)])
        _, bare = _host_pair(P, blob, nt, g, n_meas, ms, history=stride, want_jacobian=False)
        assert bare.jacobian is None and np.array_equal(bare.cov, lc.cov) and np.array_equal(bare.nav_cov, lc.nav_cov)
        assert np.array_equal(bare.nominal, lc.nominal)
    _, lc = _host_pair(P, blob, nt, g, n_meas, ms, history=5)
    iu, i7 = np.triu_indices(10), np.triu_indices(7)
    for opt in (True, False):
        gl, pf, sm, nom, cov, ncov, jac, njac = _device_calls(P, blob, nt, g, n_meas, ms, 5, want_optional=opt)
        assert np.array_equal(gl.transpose(3, 2, 0, 1), nf.gain_l)
        assert np.array_equal(sm, np.stack([nf.status, nf.first_bad, nf.meas_nodes, nf.substeps]))
        assert np.array_equal(nom.transpose(2, 1, 0), lc.nominal) and np.array_equal(cov.transpose(2, 1, 0), lc.cov[:, :, iu[0], iu[1]])
        assert np.array_equal(ncov.transpose(2, 1, 0), lc.nav_cov[:, :, i7[0], i7[1]])
        if opt:
            assert np.array_equal(jac.transpose(3, 2, 0, 1), lc.jacobian) and np.array_equal(njac.transpose(3, 2, 0, 1), lc.nav_jacobian)
            assert np.array_equal(pf.transpose(2, 1, 0), nf.cov[:, :, i7[0], i7[1]])
        else:
            assert np.all(jac == 7.25) and np.all(njac == 7.25) and np.all(pf == 7.25)


def test_bounded_garbage():
    """Nothing here provokes a fault; every case is bounded work that ends in NaN rows.  A t_f of NaN gives NaN rows at every node of
    both calls (status 2) and leaves the neighbour's bits untouched; a NaN in one gain_l entry at node 9 gives NaN rows from node 9
    on and leaves the nodes before it and the other problem as they were; with device pointers a sigma_i = 0 together with
    h_i = 0 (s = 0) gives status 2 and first_bad equal to that node, the first measurement node."""
    from lunar_module_ascent_trajectory_optimiser_amd import NavigationFilter
    nt, K, n_meas = 18, 17, 2
    P, blob = _case(nt, 0, 0)
    g = _gains(nt, 0, 0, "guided", 1e6)
    nf, good = _host_pair(P, blob, nt, g, n_meas, 1)
    assert np.isfinite(_all(good)).all() and np.isfinite(nf.gain_l).all() and np.isfinite(nf.cov).all()
    b = np.array(blob)
    b[21 * K, 0] = np.nan
    nf_b, lc = _host_pair(P, b, nt, g, n_meas, 1)
    assert nf_b.status[0] == 2 and nf_b.status[1] == 0 and np.isnan(nf_b.gain_l[0]).all() and np.isnan(nf_b.cov[0]).all()
    assert np.array_equal(nf_b.gain_l[1], nf.gain_l[1]) and np.array_equal(nf_b.cov[1], nf.cov[1])
    u = _unit_sigmas(P)
    u["control_sigma"] = SIG_U
    lc = _corridor(P, b, nt, 0, 0, g, nf, **u)
    assert np.isnan(lc.cov[0]).all() and np.isnan(lc.jacobian[0]).all() and np.isnan(lc.nav_cov[0]).all() and np.isnan(lc.nav_jacobian[0]).all()
    assert np.isnan(lc.nominal[0, :, :8]).all() and np.array_equal(_all(lc)[1], _all(good)[1])
    node = 9
    gl = nf.gain_l.copy()
    gl[0, node - 1, 1, 3] = np.nan
    bad = NavigationFilter(gl, nf.cov, nf.status, nf.first_bad, nf.meas_nodes, nf.substeps, nf.nav_sigma, nf.meas_rows, nf.meas_sigma, 1,
                           nf.control_sigma, None)
    lc = _corridor(P, blob, nt, 0, 0, g, bad, **u)
    assert np.array_equal(_all(lc)[0, :node - 1], _all(good)[0, :node - 1]) and np.array_equal(_all(lc)[1], _all(good)[1])
    assert np.isnan(lc.cov[0, node - 1:]).all() and np.isnan(lc.nav_cov[0, node - 1:]).all()
    assert np.isnan(lc.jacobian[0, node - 1:]).all() and np.isnan(lc.nav_jacobian[0, node - 1:]).all()
    assert np.array_equal(lc.nominal, good.nominal)
    # s = 0 at the first measurement node (4), problem 0 only; device pointers, so the host does not refuse it
    rows = np.broadcast_to(H4[:n_meas], (2, n_meas, 7)).copy()
    sg = np.full((2, n_meas), SIG_M)
    rows[0, 1], sg[0, 1] = 0.0, 0.0
    gl, pf, sm, nom, cov, ncov, jac, njac = _device_calls(P, blob, nt, g, n_meas, 4, 1, meas_sigma=sg, meas_rows=rows)
    ok = _device_calls(P, blob, nt, g, n_meas, 4, 1)
    assert sm[0, 0] == 2 and sm[1, 0] == 4 and sm[0, 1] == 0 and sm[1, 1] == 0 and sm[2, 0] == 4
    assert np.isnan(gl[:, :, 3:, 0]).all() and np.isnan(pf[:, 3:, 0]).all() and np.all(gl[:, :, :3, 0] == 0.0) and np.isfinite(pf[:, :3, 0]).all()
    assert np.isnan(cov[..., 0]).all() and np.isnan(ncov[..., 0]).all()
    for a, w in zip((gl, pf, cov, ncov, jac, njac), (ok[0], ok[1], ok[4], ok[5], ok[6], ok[7])):
        assert np.array_equal(a[..., 1], w[..., 1])


def test_a_bad_initial_knowledge_freezes_the_design_without_a_measurement():
    """Device pointers, so the host does not refuse it: a NaN in sigma_nav of problem 0 with meas_stride = K + 1 -- no measurement
    node, so no innovation variance is ever formed -- still gives status 2, first_bad 1 and NaN rows of pfilt_out and gain_l_out
    from the first node, and NaN rows of the corridor; the other problem keeps its bits."""
    nt, K, n_meas = 18, 17, 2
    P, blob = _case(nt, 0, 0)
    g = _gains(nt, 0, 0, "guided", 1e6)
    sn = np.full((7, 2), SIG_NAV)
    sn[2, 0] = np.nan
    gl, pf, sm, nom, cov, ncov, jac, njac = _device_calls(P, blob, nt, g, n_meas, K + 1, 1, nav_sigma=sn)
    ok = _device_calls(P, blob, nt, g, n_meas, K + 1, 1)
    assert sm[0, 0] == 2 and sm[1, 0] == 1 and sm[2, 0] == 0 and sm[0, 1] == 0 and sm[1, 1] == 0
    assert np.isnan(gl[..., 0]).all() and np.isnan(pf[..., 0]).all() and np.isnan(cov[..., 0]).all() and np.isnan(ncov[..., 0]).all()
    assert np.all(ok[0] == 0.0) and np.isfinite(ok[1]).all()
    for a, w in zip((gl, pf, cov, ncov, jac, njac), (ok[0], ok[1], ok[4], ok[5], ok[6], ok[7])):
        assert np.array_equal(a[..., 1], w[..., 1])


def test_the_example_prints_the_filter():
    """examples/apollo11.py --guide --lincov --filter --no-plots: the lines of the filter, every number finite, the filter's own
    1-sigma not above the true one (the truth carries a thrust dispersion the design does not model)."""
    import importlib.util
    import io
    import os
    import re
    from contextlib import redirect_stdout
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("apollo11_example_navfilter", os.path.join(root, "examples", "apollo11.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    m, _, _ = ex.build()
    out = io.StringIO()
    with redirect_stdout(out):
        m.solve(disp=False)
        ex.guide(m, 0, samples=64, lincov=True, navfilter=True)
    text = out.getvalue()
    print(text)
    assert "navigation filter: status 0" in text
    rows = re.findall(r"^(x \(m\)|y \(m\)|xdot \(cm/s\)|ydot \(cm/s\))\s+([\d.eE+-]+)\s+([\d.eE+-]+)$", text, re.M)
    assert len(rows) == 4, text
    for _, true, own in rows:
        assert np.isfinite(float(true)) and np.isfinite(float(own)) and 0.0 < float(own) <= float(true) * (1 + 1e-9), rows
    with_f, without = re.search(r"with the filter \+-([\d.]+) m; with the frozen navigation bias \+-([\d.]+) m", text).groups()
    assert np.isfinite(float(with_f)) and np.isfinite(float(without)) and float(with_f) > 0 and float(without) > 0
