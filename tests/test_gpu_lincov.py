"""The linear covariance corridor on the GPU (ascent_covariance_history_batch; linear_corridor): the per-node Jacobian and
covariance against the CPU reference (tests/lincov_reference.py) on the device's own gains, the forward sweep against the adjoint
sweeps of the flight Jacobian and the guidance gains at the last node, against central differences of the flight kernel's own
samples, the bitwise promises of the header, bounded garbage, the example, and the second-order residual of the Monte Carlo
variance.

The cases are gpu_cases.CASES, each open loop, guided and navigated at q = 1e6 and 1e12 with the device's own gains,
substeps = 2, two problems.  Every entry is compared in the scale of its row -- scaled units for the state, r_peri for the
altitude, max(1, |K_j|_1 + |f_j|) for the control and the correction, products of those for the covariance -- and, for the
Jacobian, per relative step of its column (the field's own size for a parameter column, the thrust for the error of theta-hat,
scaled units elsewhere).  Bounds that depend on the conditioning of the case are computed here from the reference alone -- its
float64 run against its longdouble run -- never from the device.  The differences seen are collected in PARITY; with
ASCENT_LINCOV_PARITY_OUT=<file> they are written there as JSON when the module is done (profiles/lincov_parity.json is such a file)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import guidance_reference as gr
import history_reference as hr
import lincov_reference as lr
from gpu_cases import (CASES, FD_STEPS, FLOOR, M, case as _case, col_scales as _col_scales, gains as _gains,
                       norm_cov as _norm_cov, norm_jac as _norm_jac, parity_writer, sigmas as _sigmas, weights as _weights,
                       xi as _xi)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = {"corridor_vs_reference": {}, "forward_vs_adjoint": {}, "corridor_vs_flight_kernel": {}, "second_order_residual": {}}
KINDS = [("open", 0.0), ("guided", 1e6), ("guided", 1e12), ("navigated", 1e6), ("navigated", 1e12)]
LD = np.longdouble
_write_parity = parity_writer("ASCENT_LINCOV_PARITY_OUT", PARITY)


def _unit_sigmas(P, kind, rel=1.0):
    """keyword arguments of linear_corridor: every sigma `rel` of its column's scale.  The model is linear, so the sigmas only weigh
    the columns; at rel = 1 an entry of cov is of the order of the squared normalised Jacobian and the absolute floor bites."""
    cs = np.array([_col_scales(p) for p in P]) * rel
    kw = dict(z0_sigma=cs[:, :7], param_sigma=cs[:, lr.C_P:lr.C_TF], tf_sigma=cs[:, lr.C_TF], control_sigma=rel)
    if kind == "navigated":
        kw.update(nav_sigma=cs[:, lr.C_NU:lr.C_E], knowledge_sigma=cs[:, lr.C_E])
    return kw


def _law(g, j, kind):
    """keyword arguments of lincov_reference.corridor for problem j flown under the device's gains g"""
    if kind == "open":
        return {}
    kw = dict(gain_u=g.gain_u[j], gain_t=g.gain_t[j], smax=float(g.stretch_max[j]))
    if kind == "navigated":
        kw.update(ff_u=g.ff_u[j], ff_t=float(g.ff_t[j]), know=g.ff_know[j])
    return kw


def _corridor(P, blob, nt, scheme, form, g, **kw):
    from lunar_module_ascent_trajectory_optimiser_amd import linear_corridor
    kw.setdefault("substeps", M)
    return linear_corridor(P, blob, nt, guidance=g, scheme=scheme, formulation=form, **kw)


def _all(lc):
    """everything a LinearCorridor holds, as one array per problem and node"""
    B, NJ = lc.nominal.shape[:2]
    parts = [lc.nominal, lc.cov.reshape(B, NJ, -1)] + ([] if lc.jacobian is None else [lc.jacobian.reshape(B, NJ, -1)])
    return np.concatenate(parts, axis=2)


@functools.lru_cache(maxsize=None)
def _compared(nt, scheme, form, kind, q):
    """The stride-1 corridor of a case at unit relative sigmas against the longdouble reference.  -> per problem dict(jacobian /
    covariance / noise: dict(device_error, reference_gap, bound)); noise is the covariance with only the execution errors on."""
    P, blob = _case(nt, scheme, form)
    K = nt - 1
    g = _gains(nt, scheme, form, kind, q)
    kw = _unit_sigmas(P, kind)
    dev = _corridor(P, blob, nt, scheme, form, g, **kw)
    only_u = _corridor(P, blob, nt, scheme, form, g, control_sigma=1.0, want_jacobian=False)
    assert dev.jacobian.shape == (P.shape[0], K, 10, 32) and dev.cov.shape == (P.shape[0], K, 10, 10) and np.array_equal(dev.nodes, np.arange(1, K + 1))
    assert np.array_equal(dev.cov, dev.cov.transpose(0, 1, 3, 2)) and only_u.jacobian is None
    fig = {}
    for j in range(P.shape[0]):
        law = _law(g, j, kind)
        cs = _col_scales(P[j])
        sn = cs[lr.C_NU:] if kind == "navigated" else None
        ref = {dt: lr.corridor(P[j], blob[:, j], nt, cs[:24], np.ones(K), formulation=form, substeps=M, dtype=dt, sigma_nav=sn, **law)
               for dt in (np.float64, LD)}
        rows = lr.row_scales(P[j], law.get("gain_u"), law.get("ff_u"), K)
        out = {}
        for name, of_ref, of_dev, norm in (("jacobian", "S", dev.jacobian[j], lambda a: _norm_jac(a, rows, cs)),
                                           ("covariance", "cov", dev.cov[j], lambda a: _norm_cov(a, rows)),
                                           ("noise", "noise", only_u.cov[j], lambda a: _norm_cov(a, rows))):
            want = norm(ref[LD][of_ref])
            gap = float(np.abs(norm(ref[np.float64][of_ref]) - want).max())
            err = float(np.abs(norm(of_dev) - want).max())
            assert np.isfinite(of_dev).all()
            out[name] = dict(device_error=err, reference_gap=gap, bound=max(FLOOR, 100.0 * gap), largest_entry=float(np.abs(want).max()))
        # the nominal rows: f_fly's flight against the reference's, test_gpu_flight's bound
        nom = np.abs(dev.nominal[j] - ref[np.float64]["nominal"].astype(np.float64)) / rows
        out["nominal"] = dict(device_error=float(nom[:, :8].max()), reference_gap=0.0, bound=FLOOR)
        assert np.array_equal(dev.nominal[j][:, 8], blob[7 * K:8 * K, j]) and np.all(dev.nominal[j][:, 9] == 0.0)
        fig[f"problem{j}"] = out
        print(nt, scheme, form, kind, q, "problem", j, out)
    PARITY["corridor_vs_reference"][f"nt{nt}_scheme{scheme}_form{form}_{kind}_q{q:g}"] = fig
    return dev, only_u, fig


@pytest.mark.parametrize("kind,q", KINDS)
@pytest.mark.parametrize("nt,scheme,form", CASES)
def test_jacobian_and_covariance_match_reference(nt, scheme, form, kind, q):
    """jac_hist_out and cov_out at stride 1, every node, against the longdouble reference flown with the device's own gains and
    feed-forward; every sigma one unit of its column's scale (see _unit_sigmas), sigma_u = 1.  Bound, the project's convention
    (tests/test_gpu_guidance.py, tests/test_gpu_history.py): the larger of 1e-10 and 100 x the reference's own
    float64-against-longdouble difference of the same quantity on the same blob, in the scales of the module docstring.  Where
    1e-10 does not hold -- at q = 1e12 the gains reach 1e5 and the closed-loop step maps cancel to a few digits -- the bound is
    wider by exactly what the reference's own gap gives, never by what the device shows; both are recorded."""
    _, _, fig = _compared(nt, scheme, form, kind, q)
    for k, v in fig.items():
        for name, f in v.items():
            assert f["device_error"] <= f["bound"], (k, name, f)


@pytest.mark.parametrize("kind,q", KINDS)
@pytest.mark.parametrize("nt,scheme,form", CASES)
def test_forward_sweep_equals_the_adjoint_sweeps_at_the_last_node(nt, scheme, form, kind, q):
    """At node K rows 0..6 of jac_hist_out are rows 0..6 of ascent_flight_jacobian (open loop) or of jac_cl | jac_nav of the gains
    call (guided: jac_cl alone), and Q_K -- the state block of cov_out with only sigma_u = 1 on -- is sum_k (column k of jac_u_cl)
    (column k)'.  Two kernels, two sweeps in opposite directions; each side is within the reference bound of the same reference,
    so they differ by at most twice that bound."""
    from lunar_module_ascent_trajectory_optimiser_amd import flight_jacobian
    P, blob = _case(nt, scheme, form)
    K = nt - 1
    dev, only_u, fig = _compared(nt, scheme, form, kind, q)
    if kind == "open":
        J, nav = flight_jacobian(P, blob, nt, scheme=scheme, formulation=form, substeps=M), None
    else:
        g = _gains(nt, scheme, form, kind, q, jacobian=True)
        g0 = _gains(nt, scheme, form, kind, q)
        assert np.array_equal(g.gain_u, g0.gain_u) and np.array_equal(g.gain_t, g0.gain_t)
        J, nav = g.jacobian, g.jacobian_nav
    adj = np.concatenate([J.dz0, J.dparams, J.dtf[:, :, None]] + ([] if nav is None else [nav]), axis=2)[:, :7]
    out = {}
    for j in range(P.shape[0]):
        cs = _col_scales(P[j])[:adj.shape[2]]
        e_jac = float(np.abs((dev.jacobian[j, -1, :7, :adj.shape[2]] - adj[j]) * cs[None, :]).max())
        Q = np.einsum("ak,bk->ab", J.dcontrols[j, :7], J.dcontrols[j, :7])
        e_q = float(np.abs(only_u.cov[j, -1, :7, :7] - Q).max())
        b_jac, b_q = 2.0 * fig[f"problem{j}"]["jacobian"]["bound"], 2.0 * fig[f"problem{j}"]["noise"]["bound"]
        out[f"problem{j}"] = dict(jacobian_difference=e_jac, jacobian_tolerance=b_jac, Q_difference=e_q, Q_tolerance=b_q)
        print(nt, scheme, form, kind, q, "problem", j, out[f"problem{j}"])
    PARITY["forward_vs_adjoint"][f"nt{nt}_scheme{scheme}_form{form}_{kind}_q{q:g}"] = out
    for k, v in out.items():
        assert v["jacobian_difference"] <= v["jacobian_tolerance"] and v["Q_difference"] <= v["Q_tolerance"], (k, v)


def _reference_flight_difference(p16, rec, nodes, law, cs, form, h):
    """central differences of history_reference.fly_history in float64 at the relative step h: -> (K, 10, 32 + K) per unit of
    the column (the last K columns: the execution errors)"""
    K = len(rec["us"])
    know = law.get("know")
    out = np.zeros((K, lr.NQ, lr.NC + K))

    def fly(c, noise):
        th = c[lr.C_E] + (0.0 if know is None else float(np.dot(know, c[lr.C_P:lr.C_TF])))
        return hr.fly_history(p16 + c[lr.C_P:lr.C_TF], c[:7], rec["us"], noise, rec["tf"] + c[lr.C_TF], rec["m"], nodes, law.get("gain_u"),
                              law.get("gain_t"), law.get("smax", 0.0), law.get("ff_u"), law.get("ff_t"), th, c[lr.C_NU:lr.C_E],
                              np.ones(7, dtype=bool), form)[0]
    for c in range(lr.NC + K):
        e, n = np.zeros(lr.NC), np.zeros(K)
        if c < lr.NC:
            e[c] = h * cs[c]
        else:
            n[c - lr.NC] = h
        out[:, :, c] = (fly(e, n) - fly(-e, -n)) / (2.0 * h * (cs[c] if c < lr.NC else 1.0))
    return out


@pytest.mark.parametrize("kind", ["open", "navigated"])
def test_jacobian_is_the_central_difference_of_the_flight_kernel(kind):
    """nt = 18, q = 1e6: jac_hist_out against central differences of hist_samples_out of ascent_disperse_history_batch -- 2 (32 + K)
    samples, one-hot xi / xi_nav of +-1, every sigma h of its column's scale --, and the noise part of cov_out against the sum over
    the K execution-error columns of the same differences.  Row 51 is zero everywhere: no command clipped.  h is chosen on the CPU:
    of FD_STEPS the step at which the reference's own float64 central difference (history_reference.fly_history) is closest to
    its complex-step derivative (lincov_reference); the bound is 10 x that closest distance, for the noise part propagated through
    N = sum_k s_k s_k' (|dN_ab| <= b (sum_k |s_ka| + |s_kb|) + K b^2).  Both are recorded.  The only test a misconception shared by
    the kernel and the reference cannot pass: the flight kernel knows nothing of either."""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch
    nt, scheme, form, q = 18, 0, 0, 1e6
    K = nt - 1
    P, blob = _case(nt, scheme, form)
    B = P.shape[0]
    g = _gains(nt, scheme, form, kind, q)
    # h and the bound, from the reference alone (problem 0; the two problems are neighbours of one sweep)
    law0, cs0 = _law(g, 0, kind), _col_scales(P[0])
    rec = gr.records(P[0], blob[:, 0], nt, form, M)
    ref = lr.corridor(P[0], blob[:, 0], nt, np.zeros(24), np.ones(K), formulation=form, substeps=M, rec=rec, **law0)
    nodes = gr.nominal_nodes(P[0], rec["us"], rec["tf"], rec["m"], form)
    rows0 = lr.row_scales(P[0], law0.get("gain_u"), law0.get("ff_u"), K)
    tried = {}
    for h in FD_STEPS:
        fd = _reference_flight_difference(P[0], rec, nodes, law0, cs0, form, h)
        tried[h] = float(np.abs(_norm_jac(fd[:, :, :lr.NC], rows0, cs0) - _norm_jac(ref["S"], rows0, cs0)).max())
    h = min(tried, key=tried.get)
    bound = 10.0 * tried[h]
    print(kind, "reference central difference against its complex step, by h:", tried, "-> h", h, "bound", bound)
    # the flight kernel: sample 2c carries +1 on constant c, sample 2c + 1 carries -1
    S = 2 * (lr.NC + K)
    xi, xn = np.zeros((24 + K, S)), np.zeros((8, S))
    for c in range(lr.NC + K):
        tab, r = (xi, c) if c < 24 else (xn, c - 24) if c < lr.NC else (xi, 24 + c - lr.NC)
        tab[r, 2 * c], tab[r, 2 * c + 1] = 1.0, -1.0
    kw = _unit_sigmas(P, kind, h)
    d = disperse_batch(P, blob, nt, xi=xi, scheme=scheme, formulation=form, substeps=M, guidance=g, history=True, keep_history_samples=True,
                       **(dict(xi_nav=xn) if kind == "navigated" else {}), **kw)
    assert (d.history.clipped == 0).all() and (d.history.n_valid == S).all()
    dev = _corridor(P, blob, nt, scheme, form, g, **kw)
    only_u = _corridor(P, blob, nt, scheme, form, g, control_sigma=1.0, want_jacobian=False)
    out = dict(h=h, bound=bound, reference_by_h={str(k): v for k, v in tried.items()})
    for j in range(B):
        law, cs = _law(g, j, kind), _col_scales(P[j])
        rows = lr.row_scales(P[j], law.get("gain_u"), law.get("ff_u"), K)
        smp = d.history.samples[j]                              # (S, K, 10)
        fd = (smp[0::2] - smp[1::2]).transpose(1, 2, 0) / (2.0 * h)          # (K, 10, 32 + K) per relative step
        e_jac = float(np.abs(fd[:, :, :lr.NC] / rows[:, :, None] - _norm_jac(dev.jacobian[j], rows, cs)).max())
        s = fd[:, :, lr.NC:] / rows[:, :, None]                 # (K, 10, K): d y_j / d eps_k
        N = np.einsum("jak,jbk->jab", s, s)
        a1 = np.abs(s).sum(axis=2)
        tol = bound * (a1[:, :, None] + a1[:, None, :]) + K * bound * bound
        dN = np.abs(N - _norm_cov(only_u.cov[j], rows))
        out[f"problem{j}"] = dict(jacobian_difference=e_jac, noise_difference_over_tolerance=float((dN / tol).max()))
        print(kind, "problem", j, out[f"problem{j}"])
    PARITY["corridor_vs_flight_kernel"][kind] = out
    for j in range(B):
        assert out[f"problem{j}"]["jacobian_difference"] <= bound and out[f"problem{j}"]["noise_difference_over_tolerance"] <= 1.0, out


@pytest.mark.parametrize("kind", ["open", "guided", "navigated"])
def test_nominal_rows_are_the_history_calls_bits_and_zero_gains_the_open_loops(kind):
    """nominal_out is rows 1..10 of hist_out on the same blob, bit for bit, substeps 0 and 2, every case's blob at nt = 18 and the
    three-chunk one; all-zero gains without stretch give the bits of gain_u null."""
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult, disperse_batch
    for nt, scheme, form in ((18, 0, 0), (18, 2, 0), (18, 0, 1), (34, 0, 0), (3, 0, 1)):
        P, blob = _case(nt, scheme, form)
        K = nt - 1
        g = _gains(nt, scheme, form, kind, 1e6)
        for m in (0, M):
            h = disperse_batch(P, blob, nt, samples=3, scheme=scheme, formulation=form, substeps=m, history=True, **_sigmas(P)).history
            lc = _corridor(P, blob, nt, scheme, form, g, substeps=m, **_unit_sigmas(P, kind, 1e-3))
            assert np.array_equal(lc.nominal, h.nominal)
    P, blob = _case(18, 0, 0)
    kw = _unit_sigmas(P, "open", 1e-3)
    zero = GuidanceResult(np.zeros((P.shape[0], 17, 7)), None, None, None, None)
    assert np.array_equal(_all(_corridor(P, blob, 18, 0, 0, zero, **kw)), _all(_corridor(P, blob, 18, 0, 0, None, **kw)))
    zero = GuidanceResult(np.zeros((P.shape[0], 17, 7)), np.zeros((P.shape[0], 7)), None, np.zeros(P.shape[0]), None)
    assert np.array_equal(_all(_corridor(P, blob, 18, 0, 0, zero, **kw)), _all(_corridor(P, blob, 18, 0, 0, None, **kw)))


@pytest.mark.parametrize("kind", ["open", "navigated"])
def test_a_nodes_rows_do_not_depend_on_the_stride_or_the_jacobian_output(kind):
    """K = 17: stride 5 reports nodes 5, 10, 15, 17 and stride K node K only, each with the bits of the same node at stride 1;
    without jac_hist_out the other outputs are the same bits.  q = 1e12."""
    nt, K = 18, 17
    P, blob = _case(nt, 0, 0)
    g = _gains(nt, 0, 0, kind, 1e12)
    kw = _unit_sigmas(P, kind, 1e-3)
    full = _corridor(P, blob, nt, 0, 0, g, **kw)
    for stride, nodes in ((5, [5, 10, 15, 17]), (K, [K]), (True, list(range(1, K + 1))), (4, [4, 8, 12, 16, 17])):
        lc = _corridor(P, blob, nt, 0, 0, g, history=stride, **kw)
        assert np.array_equal(lc.nodes, nodes)
        assert np.array_equal(_all(lc), _all(full)[:, np.searchsorted(full.nodes, nodes)])
        bare = _corridor(P, blob, nt, 0, 0, g, history=stride, want_jacobian=False, **kw)
        assert bare.jacobian is None and np.array_equal(bare.cov, lc.cov) and np.array_equal(bare.nominal, lc.nominal)


def test_batch_independence_and_pointers():
    """Each of 5 problems alone and repeated through a batch of 70 gives the same bits; host pointers and device pointers on
    torch's stream give the same bits.  nt = 34, stride 4 (the last node is not a multiple), navigated at q = 1e6, automatic
    substeps."""
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult, _lib, guidance_gains
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    nt, K, B, stride = 34, 33, 5, 4
    P, blob = _case(nt, 0, 0, 5)
    g = guidance_gains(P, blob, nt, want_jacobian=False, feedforward="Ft", **_weights(1e6))
    assert (g.status == 0).all()
    sub = lambda idx: GuidanceResult(g.gain_u[idx], g.gain_t[idx], g.summary[idx], g.stretch_max[idx], None, g.ff_u[idx], g.ff_t[idx],
                                     g.ff_dir[idx], g.ff_know[idx])
    kw = _unit_sigmas(P, "navigated", 1e-3)
    take = lambda idx: {k: v[idx] if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    host = _corridor(P, blob, nt, 0, 0, g, history=stride, substeps=0, **kw)
    NJ = len(host.nodes)
    assert host.nodes[-1] == K and NJ == 9 and np.isfinite(_all(host)).all()
    for q in range(B):
        one = _corridor(P[q:q + 1], blob[:, q:q + 1], nt, 0, 0, sub(slice(q, q + 1)), history=stride, substeps=0, **take(slice(q, q + 1)))
        assert np.array_equal(_all(one)[0], _all(host)[q])
    idx = np.arange(70) % B
    big = _corridor(P[idx], np.ascontiguousarray(blob[:, idx]), nt, 0, 0, sub(idx), history=stride, substeps=0, **take(idx))
    assert np.array_equal(_all(big), _all(host)[idx])
    # device pointers on torch's stream
    L = _lib.load()
    _lib.require_single_hip_runtime()
    o = _opts(nt, 0, 1.0, 0, 0.0)
    stream = torch.cuda.current_stream().cuda_stream
    sig = np.ascontiguousarray(np.concatenate([kw["z0_sigma"], kw["param_sigma"], kw["tf_sigma"][:, None]], axis=1).T)
    sig_u = np.full((K, B), kw["control_sigma"])
    sn = np.ascontiguousarray(np.concatenate([kw["nav_sigma"], kw["knowledge_sigma"][:, None]], axis=1).T)
    arrays = (P, blob, sig, sig_u, np.ascontiguousarray(g.gain_u.transpose(2, 1, 0)), np.ascontiguousarray(g.gain_t.T), g.stretch_max,
              np.ascontiguousarray(g.ff_u.T), g.ff_t, np.ascontiguousarray(g.ff_know.T), sn)
    pt, bt, *law = (torch.from_numpy(np.array(a)).cuda() for a in arrays)
    new = lambda *shape: torch.full(shape, 7.25, dtype=torch.float64, device="cuda")
    nom, cov, jac = new(10, NJ, B), new(55, NJ, B), new(10, 32, NJ, B)
    _lib.check(L.ascent_covariance_history_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), 0, *[a.data_ptr() for a in law], stride,
                                                 nom.data_ptr(), cov.data_ptr(), jac.data_ptr(), 0, C.c_void_p(stream), 1))
    torch.cuda.synchronize()
    assert np.array_equal(nom.cpu().numpy().transpose(2, 1, 0), host.nominal)
    assert np.array_equal(jac.cpu().numpy().transpose(3, 2, 0, 1), host.jacobian)
    iu = np.triu_indices(10)
    assert np.array_equal(cov.cpu().numpy().transpose(2, 1, 0), host.cov[:, :, iu[0], iu[1]])


def test_bounded_garbage():
    """Nothing here provokes a fault; every case is bounded work that ends in NaN rows.  A t_f of NaN gives NaN rows at every node
    (the blob's own control, row 8 of the nominal, stays) and leaves the neighbour's bits untouched; a NaN gain at one step gives
    NaN rows from that step's node on, leaves the nodes before it as they were and the other problem's bits unchanged."""
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult
    nt, K = 18, 17
    P, blob = _case(nt, 0, 0)
    for kind in ("open", "guided"):
        g = _gains(nt, 0, 0, kind, 1e6)
        kw = _unit_sigmas(P, kind, 1e-3)
        good = _corridor(P, blob, nt, 0, 0, g, **kw)
        assert np.isfinite(_all(good)).all()
        b = np.array(blob)
        b[21 * K, 0] = np.nan
        lc = _corridor(P, b, nt, 0, 0, g, **kw)
        assert np.isnan(lc.cov[0]).all() and np.isnan(lc.jacobian[0]).all() and np.isnan(lc.nominal[0, :, :8]).all()
        assert np.array_equal(_all(lc)[1], _all(good)[1])
    step = 6                                # 0-based: the command of step 7, which ends at node 7
    gu = g.gain_u.copy()
    gu[0, step, 2] = np.nan
    lc = _corridor(P, blob, nt, 0, 0, GuidanceResult(gu, g.gain_t, g.summary, g.stretch_max, None), **kw)
    assert np.array_equal(_all(lc)[0, :step], _all(good)[0, :step]) and np.array_equal(_all(lc)[1], _all(good)[1])
    live = np.any(good.jacobian[0] != 0.0, axis=(0, 1))          # (a column no flight depends on, r_apo for one, is exactly 0 and stays)
    assert np.isnan(lc.cov[0, step:]).all() and np.isnan(lc.jacobian[0, step:][:, :, live]).all() and live.sum() >= 24
    assert np.array_equal(lc.nominal, good.nominal)


def test_the_example_shows_both_bands():
    """examples/apollo11.py --guide --lincov --no-plots: the lines of the open and of the closed loop, the linear band within a
    third of the sampled one at its widest node (1024 samples: the sampling noise of a standard deviation is 2 %)."""
    import importlib.util
    import io
    import re
    from contextlib import redirect_stdout
    spec = importlib.util.spec_from_file_location("apollo11_example_lincov", os.path.join(ROOT, "examples", "apollo11.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    m, _, _ = ex.build()
    out = io.StringIO()
    with redirect_stdout(out):
        m.solve(disp=False)
        ex.guide(m, 0, lincov=True)
    text = out.getvalue()
    print(text)
    for line in ("linear 1-sigma altitude band", "largest gap between the two bands"):
        assert text.count(line) == 2, line
    for lin, mc in re.findall(r"linear 1-sigma altitude band at node \d+ \(t = [\d.]+ s\): \+-([\d.]+) m; Monte Carlo \+-([\d.]+) m", text):
        assert abs(float(lin) - float(mc)) <= float(mc) / 3.0, (lin, mc)


RESIDUAL_SIGMAS = (1e-3, 1e-4, 1e-5, 1e-6)


def test_monte_carlo_variance_approaches_the_linear_one_at_second_order():
    """The trimmed nt = 18 blob, 257 samples, guided at q = 1e6, control_sigma = None (no white noise: its part is exact and is taken
    out by not flying it).  history.var against S D C_xi D S' from the same draws -- no sampling noise between the two -- at a
    relative sigma and at a tenth of it: what is left is of second order, so the relative gap (per row, largest over the nodes, in
    units of the row's largest linear variance) falls tenfold; it must fall below a third.  The sigma is picked on the CPU: the
    first of RESIDUAL_SIGMAS at which the reference alone (history_reference + lincov_reference on the same blob, the device's
    gains) flies without a clipped command and shows a ratio between 5 and 20.  That is 1e-4 (at 1e-3 a command clips): the
    reference's gap falls from 2.6e-3 to 1.8e-4, a ratio of 15; the device showed 2.6e-3 -> 1.8e-4 and 2.1e-3 -> 2.0e-4."""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch
    nt, K, S, q = 18, 17, 257, 1e6
    P, blob = _case(nt, 0, 0)
    g = _gains(nt, 0, 0, "guided", q)
    xi = _xi(K, S)
    Cx = np.cov(xi[:24])
    law = _law(g, 0, "guided")
    rec = gr.records(P[0], blob[:, 0], nt, 0, M)
    S_ref = lr.corridor(P[0], blob[:, 0], nt, np.zeros(24), formulation=0, substeps=M, rec=rec, **law)["S"][:, :, :24]

    def gap(var, jac, sigma):
        A = jac * sigma[None, None, :]
        lin = np.einsum("jqc,cd,jqd->jq", A, Cx, A)
        on = lin.max(axis=0) > 0
        return float((np.abs(var - lin).max(axis=0)[on] / lin.max(axis=0)[on]).max())

    def reference_gap(rel):
        sigma = _sigma24(P, rel)[0]
        h = hr.history(P[0], blob[:, 0], nt, xi, sigma, None, law["gain_u"], law["gain_t"], law["smax"], substeps=M)
        return math.inf if h["clipped"].any() else gap(h["stats"][:, 21:31], S_ref, sigma)          # a clipped command is not of second order

    ref_gaps, rel = {}, None
    for r in RESIDUAL_SIGMAS:
        for s in (r, r / 10):
            if s not in ref_gaps:
                ref_gaps[s] = reference_gap(s)
        if 5.0 <= ref_gaps[r] / ref_gaps[r / 10] <= 20.0:
            rel = r
            break
    print("reference gaps by relative sigma", ref_gaps, "-> sigma", rel)
    assert rel is not None, ref_gaps
    gaps = {}
    for s in (rel, rel / 10):
        kw = _sigmas(P, s)
        kw.pop("control_sigma")
        d = disperse_batch(P, blob, nt, xi=xi, scheme=0, formulation=0, substeps=M, guidance=g, history=True, **kw)
        lc = _corridor(P, blob, nt, 0, 0, g, **kw)
        assert (d.history.clipped == 0).all() and (d.history.n_valid == S).all()
        gaps[s] = [gap(d.history.var[j], lc.jacobian[j][:, :, :24], _sigma24(P, s)[j]) for j in range(P.shape[0])]
    PARITY["second_order_residual"] = dict(sigma=rel, reference={str(k): v if math.isfinite(v) else "a command clipped" for k, v in ref_gaps.items()},
                                           device={str(k): v for k, v in gaps.items()})
    print("device gaps", gaps)
    for j in range(P.shape[0]):
        assert gaps[rel / 10][j] < gaps[rel][j] / 3.0, gaps


def _sigma24(P, rel):
    kw = _sigmas(P, rel)
    return np.concatenate([kw["z0_sigma"], kw["param_sigma"], kw["tf_sigma"][:, None]], axis=1)
