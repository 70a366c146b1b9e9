"""The per-node Monte Carlo history on the GPU (ascent_disperse_history_batch; disperse_batch(history=...)): every sample's ten
quantities at every node against the CPU reference (tests/history_reference.py) flown with the device's own gains, the
reduction against numpy on the device's own samples, the bitwise promises of the header -- against the three existing
dispersion calls, against stats_out at the last node, across strides, batches, pointers and optional outputs --, bounded
garbage and the example.

Bounds that depend on the conditioning of the case are computed here from the reference alone -- its float64 run against its
longdouble run -- never from the device.  The differences seen are collected in PARITY; with ASCENT_HISTORY_PARITY_OUT=<file>
they are written there as JSON when the module is done (profiles/history_parity.json is such a file)."""
import ctypes as C
import os

import numpy as np
import pytest

import feedforward_reference as ffr
import history_reference as hr
from gpu_cases import (CASES, M, SAMPLE_BOUND, case as _case, gains as _gains, parity_writer, scaled_error as _scaled_error,
                       sigmas as _sigmas, stats as _stats, weights as _weights, xi as _xi)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = {"history_samples_vs_reference": {}}
CLIPPED = {}               # case -> the largest row 51 seen where the flags were compared with the reference
# open loop; guided at q = 1e6 and 1e12; navigated (feed-forward of the thrust, navigation and knowledge errors) at the same two
KINDS = [("open", 0.0), ("guided", 1e6), ("guided", 1e12), ("navigated", 1e6), ("navigated", 1e12)]
_write_parity = parity_writer("ASCENT_HISTORY_PARITY_OUT", PARITY)


def _nav_kw(P, samples):
    """navigation sigmas 1e-6 (scaled), a knowledge sigma of 1e-3 of the thrust, and their draws"""
    return dict(nav_sigma=np.full(7, 1e-6), knowledge_sigma=1e-3 * P[:, 3], xi_nav=np.random.default_rng(13).standard_normal((8, samples)))


def _fly(P, blob, nt, scheme, form, kind, g, xi, kw, substeps=M, history=True, keep=True, keep_hist=True):
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch
    if kind == "navigated":
        kw = dict(_nav_kw(P, xi.shape[1]), **kw)
    return disperse_batch(P, blob, nt, xi=xi, keep_samples=keep, scheme=scheme, formulation=form, substeps=substeps, guidance=g,
                          history=history, keep_history_samples=keep_hist and history is not False, **kw)


def _hist(h, nodes=None):
    """(batch, NJ, 52) as hist_out holds it, optionally only the named (1-based) nodes"""
    a = np.concatenate([h.n_valid[:, :, None], h.nominal, h.mean, h.var, h.min, h.max, h.clipped[:, :, None]], axis=2)
    return a if nodes is None else a[:, np.searchsorted(h.nodes, nodes)]


def _check_history_statistics(d, j):
    """problem j of a DispersionHistory against numpy on its own samples: means within 1e-11 range, variances within 1e-11
    range^2 (gpu_cases.check_statistics' bounds); count and extrema exact.  -> the worst error in units of the bound"""
    h = d.history
    worst = 0.0
    for i in range(len(h.nodes)):
        s = h.samples[j, :, i]
        v = s[np.isfinite(s).all(axis=1)]
        n = len(v)
        assert h.n_valid[j, i] == n
        if n == 0:
            assert np.isnan(h.mean[j, i]).all() and np.isnan(h.var[j, i]).all() and np.isnan(h.min[j, i]).all() and np.isnan(h.max[j, i]).all()
            continue
        lo, hi = v.min(axis=0), v.max(axis=0)
        assert np.array_equal(h.min[j, i], lo) and np.array_equal(h.max[j, i], hi)
        rng = hi - lo
        em = np.abs(h.mean[j, i] - v.mean(axis=0))
        assert np.all(em <= 1e-11 * rng), (i, em, rng)
        worst = max(worst, float(np.max(np.divide(em, rng, out=np.zeros(10), where=rng > 0))))
        if n < 2:
            assert np.isnan(h.var[j, i]).all()
            continue
        ev = np.abs(h.var[j, i] - v.var(axis=0, ddof=1))
        assert np.all(ev <= 1e-11 * rng * rng), (i, ev, rng)
        worst = max(worst, float(np.max(np.divide(ev, rng * rng, out=np.zeros(10), where=rng > 0))))
    return worst / 1e-11


def _samples_against_reference(nt, scheme, form, samples, kind, q):
    P, blob = _case(nt, scheme, form)
    K = nt - 1
    g = _gains(nt, scheme, form, kind, q)
    xi, kw = _xi(K, samples), _sigmas(P)
    d = _fly(P, blob, nt, scheme, form, kind, g, xi, kw)
    h = d.history
    assert h.samples.shape == (P.shape[0], samples, K, 10) and np.array_equal(h.nodes, np.arange(1, K + 1)) and h.mean.shape == (P.shape[0], K, 10)
    name = f"nt{nt}_scheme{scheme}_form{form}_samples{samples}_{kind}_q{q:g}"
    fig, nonzero = {}, 0
    for j in range(P.shape[0]):
        sigma = np.concatenate([kw["z0_sigma"][j], kw["param_sigma"][j], [kw["tf_sigma"][j]]])
        args = [P[j], blob[:, j], nt, xi, sigma, np.full(K, kw["control_sigma"])]
        th = 0.0
        if kind == "guided":
            args += [g.gain_u[j], g.gain_t[j], 0.5]
        elif kind == "navigated":
            args += [g.gain_u[j], g.gain_t[j], 0.5, g.ff_u[j], g.ff_t[j], g.ff_know[j], d.xi_nav, d.nav_sigma[j]]
            th = np.abs(ffr.beliefs(xi, sigma, g.ff_know[j], d.xi_nav, d.nav_sigma[j])[0]).max()
        ref = hr.history(*args, formulation=form, substeps=M)
        n = samples if j == 0 else min(samples, 65)          # the longdouble flight is slow: fewer samples can only lower the bound
        argl = list(args)
        argl[3] = xi[:, :n]
        if kind == "navigated":
            argl[12] = d.xi_nav[:, :n]
        refl = hr.history(*argl, formulation=form, substeps=M, dtype=np.longdouble)
        # the scale of the control and the correction per step: max(1, |K_j|_1 + |f_j| |theta-hat|)
        k1 = np.zeros(K) if kind == "open" else np.abs(g.gain_u[j]).sum(axis=1) + (np.abs(g.ff_u[j]) * th if kind == "navigated" else 0.0)
        s89 = np.maximum(1.0, k1)
        gap = _scaled_error(ref["samples"][:n], refl["samples"].astype(np.float64), P[j, 9], s89)
        bound = max(SAMPLE_BOUND, 100.0 * gap)
        err = max(_scaled_error(h.samples[j], ref["samples"], P[j, 9], s89), _scaled_error(h.nominal[j][None], ref["nominal"][None], P[j, 9], s89))
        # the clipped flags, per (sample, step), where the reference's command is farther from the clip than the bound
        # (the device reports the flags as row 51, a count per node: the pairs left out are the slack of their node's count)
        far = ref["margin"] > bound * s89[None, :]
        valid = np.isfinite(h.samples[j]).all(axis=2)
        assert valid.all() and np.isfinite(ref["samples"]).all()
        near = (~far).sum(axis=0)
        assert np.all(np.abs(h.clipped[j] - (ref["clipped"] & far).sum(axis=0)) <= near), (name, j, h.clipped[j], ref["clipped"].sum(axis=0), near)
        compared = h.clipped[j][near == 0]
        nonzero = max(nonzero, int(compared.max()) if compared.size else 0)
        left_out = 1.0 - far.mean()
        fig[f"problem{j}"] = dict(device_error=err, reference_gap=gap, bound=bound, pairs_left_out=float(left_out),
                                  clipped_pairs_reference=int(ref["clipped"].sum()), row51_max_compared=int(compared.max()) if compared.size else 0,
                                  statistics_error_over_bound=_check_history_statistics(d, j))
        print(name, "problem", j, fig[f"problem{j}"])
        assert left_out <= 0.02
        # row 51 against the device's own effort row (the same comparison, summed the other way), where every sample is valid throughout
        if kind != "open" and valid.all():
            assert h.clipped[j].sum() == d.effort[j, :, 0].sum()
        if kind == "open":
            assert np.all(h.clipped[j] == 0) and np.all(h.samples[j][:, :, 9] == 0.0)
    PARITY["history_samples_vs_reference"][name] = fig
    CLIPPED[name] = nonzero
    for k, v in fig.items():
        assert v["device_error"] <= v["bound"], (name, k, v)


@pytest.mark.parametrize("kind,q", KINDS)
@pytest.mark.parametrize("nt,scheme,form,samples", [c + (65,) for c in CASES] + [(3, 0, 0, 1), (18, 0, 0, 257)])
def test_history_samples_match_reference_and_the_reduction_matches_numpy(nt, scheme, form, samples, kind, q):
    """Every entry of hist_samples_out at stride 1 against the CPU reference flying the device's own gains and feed-forward: all
    four sigma groups at 1e-3 as in tests/test_gpu_dispersion.py, substeps = 2; navigated: navigation sigmas 1e-6, knowledge sigma
    1e-3 of the thrust.  Bound, as tests/test_gpu_guidance.py: the larger of SAMPLE_BOUND and 100 x the float64-against-longdouble
    difference of the reference's history on the case (on the first 65 samples for the second problem of the 257-sample case), in
    scaled units for the state, times r_peri for the altitude, times max(1, |K_j|_1 + |f_j| |theta-hat|) for the control and the
    correction.  The clipped flags reach the caller as row 51, a count per node: it is the reference's count over the (sample,
    step) pairs whose command stays farther from the clip than that bound, give or take the node's pairs that do not (at most 2 %
    of all pairs may be that close), and its sum over the nodes is the sum of the device's own effort row.  Then the reduction against numpy on the device's own samples."""
    _samples_against_reference(nt, scheme, form, samples, kind, q)


def test_some_compared_case_clips():
    """Row 51 is exercised: at least one case whose flags were compared with the reference has a node where a command clipped."""
    if not any(CLIPPED.values()):          # run alone: the cases at q = 1e12, where the recorded guided runs clip
        for kind in ("guided", "navigated"):
            _samples_against_reference(18, 0, 0, 65, kind, 1e12)
            _samples_against_reference(34, 0, 0, 65, kind, 1e12)
    print({k: v for k, v in CLIPPED.items() if v})
    assert any(CLIPPED.values())


@pytest.mark.parametrize("kind", ["open", "guided", "navigated"])
@pytest.mark.parametrize("nt,scheme,form", [(3, 0, 1), (18, 0, 0), (18, 2, 0), (18, 0, 1), (34, 0, 0)])
def test_bits_of_the_existing_call_and_of_stats_out_at_the_last_node(nt, scheme, form, kind):
    """300 samples (a second workgroup of one partial wavefront), substeps 0 and 2: stats_out and samples_out are the existing
    call's bits (the open-loop flight's rows 9..11 exactly 0, and not returned as effort); with n = samples in both, rows 0, 11..17,
    21..27, 31..37 and 41..47 of the last node are rows 0, 10..16, the state's variances, 64..70 and 73..79 of stats_out."""
    P, blob = _case(nt, scheme, form)
    K, S = nt - 1, 300
    xi, kw = _xi(K, S, 3), _sigmas(P)
    for m in (0, 2):
        g = _gains(nt, scheme, form, kind, 1e6, substeps=m)
        plain = _fly(P, blob, nt, scheme, form, kind, g, xi, kw, m, history=False)
        d = _fly(P, blob, nt, scheme, form, kind, g, xi, kw, m)
        assert plain.history is None and d.history is not None
        assert np.array_equal(_stats(d), _stats(plain), equal_nan=True) and np.array_equal(d.samples, plain.samples, equal_nan=True)
        assert (d.effort is None and plain.effort is None) if kind == "open" else np.array_equal(d.effort, plain.effort)
        h = d.history
        assert (d.n_valid == S).all() and (h.n_valid[:, -1] == S).all() and h.nodes[-1] == K
        st = _stats(d)
        cov = d.cov[:, np.arange(7), np.arange(7)]
        assert np.array_equal(h.mean[:, -1, :7], d.mean[:, :7]) and np.array_equal(h.var[:, -1, :7], cov)
        assert np.array_equal(h.min[:, -1, :7], d.min[:, :7]) and np.array_equal(h.max[:, -1, :7], d.max[:, :7])
        assert np.array_equal(h.nominal[:, -1, :7], d.nominal[:, :7]) and st.shape[1] == 1 + 9 * 4 + 81
        assert np.array_equal(h.samples[:, :, -1, :7], d.samples[:, :, :7])


def test_open_loop_sample_rows_9_to_11_are_zero():
    """samples_out of the history call is always 12 rows; through ctypes, the open-loop flight's last three are exactly 0."""
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    nt, K, S = 18, 17, 65
    P, blob = _case(nt, 0, 0)
    B = P.shape[0]
    kw = _sigmas(P)
    xi = _xi(K, S)
    sig = np.ascontiguousarray(np.concatenate([kw["z0_sigma"], kw["param_sigma"], kw["tf_sigma"][:, None]], axis=1).T)
    L = _lib.load()
    o = _opts(nt, 0, 1.0, 0, 0.0)
    stats, smp, hist = np.empty((82, B)), np.full((12, S, B), 7.25), np.empty((52, K, B))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _lib.check(L.ascent_disperse_history_batch(p(np.ascontiguousarray(P)), B, C.byref(o), p(np.ascontiguousarray(blob)), M, S, p(xi), p(sig), None,
                                               *[None] * 8, 1, p(stats), p(smp), p(hist), None, 0, None, 0))
    assert np.all(smp[9:] == 0.0) and np.isfinite(smp[:9]).all() and np.all(hist[0] == S) and np.all(hist[51] == 0.0)


@pytest.mark.parametrize("kind", ["open", "navigated"])
def test_a_nodes_rows_do_not_depend_on_the_stride(kind):
    """K = 17: stride 5 reports nodes 5, 10, 15, 17 and stride K node K only; the rows and the samples of each node are those of
    the stride-1 run, and everything else of the result is the same bits.  65 and 300 samples."""
    nt, K = 18, 17
    P, blob = _case(nt, 0, 0)
    kw = _sigmas(P)
    g = _gains(nt, 0, 0, kind, 1e12)
    for S in (65, 300):
        xi = _xi(K, S, 5)
        full = _fly(P, blob, nt, 0, 0, kind, g, xi, kw)
        for stride, nodes in ((5, [5, 10, 15, 17]), (K, [K]), (True, list(range(1, K + 1)))):
            d = _fly(P, blob, nt, 0, 0, kind, g, xi, kw, history=stride)
            assert np.array_equal(d.history.nodes, nodes)
            assert np.array_equal(_hist(d.history), _hist(full.history, nodes), equal_nan=True)
            assert np.array_equal(d.history.samples, full.history.samples[:, :, np.searchsorted(full.history.nodes, nodes)])
            assert np.array_equal(_stats(d), _stats(full)) and np.array_equal(d.samples, full.samples)


def test_batch_independence_pointers_and_optional_outputs():
    """Each of 5 problems alone and repeated through a batch of 70 gives the same bits; host pointers and device pointers on
    torch's stream give the same bits; with and without samples_out and hist_samples_out the other outputs are the same bits.
    nt = 34, 300 samples, stride 4 (the last node is not a multiple), guided at q = 1e9, automatic substeps."""
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult, _lib, guidance_gains
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    nt, K, B, S, stride = 34, 33, 5, 300, 4
    P, blob = _case(nt, 0, 0, 5)
    xi, kw = _xi(K, S, 8), _sigmas(P)
    g = guidance_gains(P, blob, nt, want_jacobian=False, **_weights(1e9))
    assert (g.status == 0).all()
    sub = lambda idx: GuidanceResult(g.gain_u[idx], g.gain_t[idx], g.summary[idx], g.stretch_max[idx], None)
    take = lambda idx: {k: v[idx] if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    host = _fly(P, blob, nt, 0, 0, "guided", g, xi, kw, 0, history=stride)
    NJ = len(host.history.nodes)
    assert host.history.nodes[-1] == K and NJ == 9 and (host.history.n_valid == S).all()
    without = _fly(P, blob, nt, 0, 0, "guided", g, xi, kw, 0, history=stride, keep=False, keep_hist=False)
    assert without.samples is None and without.history.samples is None
    assert np.array_equal(_stats(without), _stats(host)) and np.array_equal(_hist(without.history), _hist(host.history))
    for q in range(B):
        one = _fly(P[q:q + 1], blob[:, q:q + 1], nt, 0, 0, "guided", sub(slice(q, q + 1)), xi, take(slice(q, q + 1)), 0, history=stride)
        assert np.array_equal(_hist(one.history)[0], _hist(host.history)[q]) and np.array_equal(one.history.samples[0], host.history.samples[q])
        assert np.array_equal(_stats(one)[0], _stats(host)[q])
    idx = np.arange(70) % B
    big = _fly(P[idx], np.ascontiguousarray(blob[:, idx]), nt, 0, 0, "guided", sub(idx), xi, take(idx), 0, history=stride)
    assert np.array_equal(_hist(big.history), _hist(host.history)[idx]) and np.array_equal(big.history.samples, host.history.samples[idx])
    assert np.array_equal(_stats(big), _stats(host)[idx])
    # device pointers on torch's stream
    L = _lib.load()
    _lib.require_single_hip_runtime()
    o = _opts(nt, 0, 1.0, 0, 0.0)
    stream = torch.cuda.current_stream().cuda_stream
    sig = np.ascontiguousarray(np.concatenate([kw["z0_sigma"], kw["param_sigma"], kw["tf_sigma"][:, None]], axis=1).T)
    sig_u = np.full((K, B), kw["control_sigma"])
    gu, gt = np.ascontiguousarray(g.gain_u.transpose(2, 1, 0)), np.ascontiguousarray(g.gain_t.T)
    pt, bt, xt, st, ut, gut, gtt, smt = (torch.from_numpy(np.array(a)).cuda() for a in (P, blob, xi, sig, sig_u, gu, gt, g.stretch_max))
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    out, smp, hist, hsmp = new(82, B), new(12, S, B), new(52, NJ, B), new(10, NJ, S, B)
    _lib.check(L.ascent_disperse_history_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), 0, S, xt.data_ptr(), st.data_ptr(), ut.data_ptr(),
                                               gut.data_ptr(), gtt.data_ptr(), smt.data_ptr(), None, None, None, None, None, stride,
                                               out.data_ptr(), smp.data_ptr(), hist.data_ptr(), hsmp.data_ptr(), 0, C.c_void_p(stream), 1))
    torch.cuda.synchronize()
    assert np.array_equal(hist.cpu().numpy().transpose(2, 1, 0), _hist(host.history))
    assert np.array_equal(hsmp.cpu().numpy().transpose(3, 2, 1, 0), host.history.samples)
    s = out.cpu().numpy().T
    assert np.array_equal(s[:, 0], host.n_valid) and np.array_equal(s[:, 10:19], host.mean) and np.array_equal(s[:, 73:82], host.max)
    a = smp.cpu().numpy()
    assert np.array_equal(a[:9].transpose(2, 1, 0), host.samples) and np.array_equal(a[9:].transpose(2, 1, 0), host.effort)


def test_bounded_garbage():
    """Nothing here provokes a fault; every case is bounded work that ends in NaN rows.  A t_f of NaN gives n = 0 and NaN rows at
    every node and leaves the neighbour's bits untouched; a NaN gain at one step makes every sample invalid from that step's node
    on and leaves the nodes before it as they were; one escaping sample is counted in the history at node K and left out of
    stats_out."""
    from lunar_module_ascent_trajectory_optimiser_amd import GuidanceResult
    nt, K, S = 18, 17, 65
    P, blob = _case(nt, 0, 0)
    kw = _sigmas(P)
    xi = _xi(K, S, 10)
    g = _gains(nt, 0, 0, "guided", 1e6)
    for kind, gg in (("open", None), ("guided", g)):
        good = _fly(P, blob, nt, 0, 0, kind, gg, xi, kw)
        assert (good.history.n_valid == S).all()
        b = np.array(blob)
        b[21 * K, 0] = np.nan
        d = _fly(P, b, nt, 0, 0, kind, gg, xi, kw)
        h = d.history
        assert (h.n_valid[0] == 0).all() and (h.clipped[0] == 0).all() and d.n_valid[0] == 0
        for f in (h.mean, h.var, h.min, h.max):
            assert np.isnan(f[0]).all()
        assert np.array_equal(_hist(h)[1], _hist(good.history)[1]) and np.array_equal(h.samples[1], good.history.samples[1])
        assert np.array_equal(_stats(d)[1], _stats(good)[1])
    good = _fly(P, blob, nt, 0, 0, "guided", g, xi, kw)
    step = 6                                # 0-based: the command of step 7, which ends at node 7
    gu = g.gain_u.copy()
    gu[0, step, 2] = np.nan
    d = _fly(P, blob, nt, 0, 0, "guided", GuidanceResult(gu, g.gain_t, g.summary, g.stretch_max, None), xi, kw)
    h = d.history
    assert (h.n_valid[0, :step] == S).all() and (h.n_valid[0, step:] == 0).all() and d.n_valid[0] == 0
    assert np.array_equal(_hist(h)[0, :step], _hist(good.history)[0, :step]) and np.isnan(h.mean[0, step:]).all()
    assert np.array_equal(_hist(h)[1], _hist(good.history)[1])
    # one sample alone is given ten times the thrust (a draw of 9000 under the 1e-3 relative sigma): it escapes
    x2 = xi.copy()
    x2[7 + 3, 4] = 9000.0
    d = _fly(P, blob, nt, 0, 0, "open", None, x2, kw)
    assert np.isinf(d.samples[0, 4, 8]) and np.isfinite(d.samples[0, 4, :8]).all()
    assert d.n_valid[0] == S - 1 and d.history.n_valid[0, -1] == S and (d.history.n_valid[0] == S).all()
    assert d.history.max[0, -1, 7] == d.history.samples[0, 4, -1, 7]


def test_the_example_shows_the_corridor():
    """examples/apollo11.py --guide --corridor --no-plots: the guided flights with their history, and the four corridor lines per
    flight flown."""
    import importlib.util
    import io
    from contextlib import redirect_stdout
    spec = importlib.util.spec_from_file_location("apollo11_example_corridor", os.path.join(ROOT, "examples", "apollo11.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    m, _, _ = ex.build()
    out = io.StringIO()
    with redirect_stdout(out):
        m.solve(disp=False)
        op, cl, g = ex.guide(m, 0, corridor=True)
    text = out.getvalue()
    print(text)
    assert op.history is not None and cl.history is not None and cl.history.n_valid[0, -1] == 1024
    for line in ("widest 1-sigma altitude band", "lowest altitude", "angle beyond", "most clipped commands"):
        assert text.count(line) == 2, line
