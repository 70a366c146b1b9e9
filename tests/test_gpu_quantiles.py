"""Quantiles and limit counts on the GPU (include/ascent.h: ascent_sample_quantiles, ascent_disperse_quantiles_batch): order
statistics are exact, so every comparison here is bit for bit (np.array_equal with equal_nan, under which -0 equals +0) against
tests/quantile_reference.py -- on crafted data through the selection call itself, on the samples of flown dispersions through
disperse_batch, and across batch sizes and workspace chunks."""
import ctypes as C
import functools

import numpy as np
import pytest

import quantile_reference as qr
from gpu_cases import M, points as _points, ptr as _ptr, same as _same, sigmas as _sigmas, solved as _solved, stats as _stats, weights as _weights, xi as _xi

pytestmark = pytest.mark.gpu

PROBS = np.array([0.0, 0.00135, 0.25, 0.5, 0.75, 0.99865, 1.0])
Q, V = 3, 2
# the issue's shapes, and the sizes at which the code changes its path: 16384 is the last sample count sorted in LDS (one
# problem per workgroup), 16385 the first selected by radix passes from memory, 65536 the largest the library takes
SAMPLES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4099)
BATCHES = (1, 3, 65, 130)
KINDS = ("normal", "ties", "equal", "ascending", "descending", "zeros", "magnitudes", "validity", "specials")


def _crafted(kind, G, S, B, seed):
    """values (Q, G, S, B) and limits (4, Q, B): a value present in the data, -inf, +inf, NaN"""
    rng = np.random.default_rng(seed)
    shape = (Q, G, S, B)
    if kind == "normal":
        v = rng.standard_normal(shape)
    elif kind == "ties":
        v = rng.integers(0, 4, shape).astype(np.float64)
    elif kind == "equal":
        v = np.full(shape, 2.5)
    elif kind in ("ascending", "descending"):
        ramp = np.arange(S, dtype=np.float64) if kind == "ascending" else np.arange(S, 0, -1, dtype=np.float64)
        v = np.broadcast_to(ramp[None, None, :, None], shape) + rng.integers(0, 3, (Q, G, 1, B))
    elif kind == "zeros":
        v = rng.choice([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], shape)
    elif kind == "magnitudes":
        v = 10.0 ** rng.uniform(-310, 300, shape) * np.where(rng.random(shape) < 0.5, 1.0, -1.0)      # denormals below 1e-308
    elif kind == "validity":
        v = rng.standard_normal(shape)
        bad = rng.random((V, G, S, B)) < 0.2
        v[:V][bad] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
        v[0, 0, :, 0] = np.nan                                      # a (group, problem) with no valid sample
        if G * B > 1:                                               # and one with exactly one
            v[:V, G - 1, :, B - 1] = np.inf
            v[:V, G - 1, S // 2, B - 1] = 1.0
    else:                                                           # +-inf and NaN in row 2 of valid samples
        v = rng.standard_normal(shape)
        hit = rng.random((G, S, B)) < 0.3
        v[2][hit] = rng.choice([np.nan, np.inf, -np.inf, -np.nan], int(hit.sum()))
    v = np.ascontiguousarray(v, dtype=np.float64)
    lim = np.empty((4, Q, B))
    lim[0] = v[:, 0, S // 2, :]
    lim[1], lim[2], lim[3] = -np.inf, np.inf, np.nan
    return v, lim


def _device_call(lib, v, lim, device_pointers):
    """ascent_sample_quantiles -> count (G, B), quant, below as float64 arrays"""
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    _, G, S, B = v.shape
    if not device_pointers:
        count, quant, below = np.empty((G, B)), np.empty((len(PROBS), Q, G, B)), np.empty((len(lim), Q, G, B))
        _lib.check(lib.ascent_sample_quantiles(_ptr(v), Q, G, V, S, B, _ptr(PROBS), len(PROBS), _ptr(lim), len(lim), _ptr(count), _ptr(quant),
                                               _ptr(below), 0, None, 0))
        return count, quant, below
    import torch
    _lib.require_single_hip_runtime()
    tv, tl = torch.from_numpy(v).cuda(), torch.from_numpy(lim).cuda()
    count, quant = torch.full((G, B), -1.0, dtype=torch.float64, device="cuda"), torch.full((len(PROBS), Q, G, B), -1.0, dtype=torch.float64, device="cuda")
    below = torch.full((len(lim), Q, G, B), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.ascent_sample_quantiles(tv.data_ptr(), Q, G, V, S, B, _ptr(PROBS), len(PROBS), tl.data_ptr(), len(lim), count.data_ptr(),
                                           quant.data_ptr(), below.data_ptr(), 0, None, 1))
    torch.cuda.synchronize()
    return count.cpu().numpy(), quant.cpu().numpy(), below.cpu().numpy()


def _check_crafted(lib, kind, G, S, B, seed):
    v, lim = _crafted(kind, G, S, B, seed)
    rc, rq, rb = qr.sample_quantiles(v, PROBS, V, lim)
    for dev in (False, True):
        count, quant, below = _device_call(lib, v, lim, dev)
        where = (kind, G, S, B, "device pointers" if dev else "host pointers")
        assert np.array_equal(count, rc), where
        assert np.array_equal(quant, rq, equal_nan=True), where
        assert np.array_equal(below, rb), where


@pytest.fixture(scope="module")
def lib():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_crafted_data_bit_for_bit(lib, kind, G):
    for S in SAMPLES:
        for B in BATCHES:
            _check_crafted(lib, kind, G, S, B, seed=1000 * S + 10 * B + G)


@pytest.mark.parametrize("kind", ["normal", "ties", "validity", "specials", "magnitudes"])
def test_crafted_data_where_the_kernel_changes(lib, kind):
    for S, B, G in ((16384, 1, 1), (16384, 3, 1), (16385, 1, 1), (16385, 3, 2), (65536, 1, 1)):
        _check_crafted(lib, kind, G, S, B, seed=S + B)


def test_sample_quantiles_wrapper(lib):
    from lunar_module_ascent_trajectory_optimiser_amd import sample_quantiles
    v, lim = _crafted("validity", 4, 257, 3, 5)
    rc, rq, rb = qr.sample_quantiles(v, PROBS, V, lim)
    count, quant, below = sample_quantiles(v, PROBS, V, limits=lim)
    assert np.array_equal(count, rc) and np.array_equal(quant, rq, equal_nan=True) and np.array_equal(below, rb)
    count, quant, below = sample_quantiles(v[:, 1], PROBS, V)
    assert below is None and np.array_equal(count, rc[1]) and np.array_equal(quant, rq[:, :, 1], equal_nan=True)
    count, quant, below = sample_quantiles(v[:, 2], (0.5,), 0, limits=lim[:2, :, 0])
    r0 = qr.sample_quantiles(v[:, 2:3], (0.5,), 0, np.repeat(lim[:2, :, :1], 3, axis=2))
    assert (count == 257).all() and np.array_equal(quant, r0[1][:, :, 0], equal_nan=True) and np.array_equal(below, r0[2][:, :, 0])


# ---- through disperse_batch ----
NT, K = 18, 17
TAU = np.array([60.0, 10.0, np.inf, 60.0, 1e-300, 30.0, np.inf])


@functools.lru_cache(maxsize=None)
def _law(form, feedforward):
    from lunar_module_ascent_trajectory_optimiser_amd import guidance_gains
    P, blob = _solved(NT, 0, form)
    return guidance_gains(P, blob, NT, formulation=form, substeps=M, want_jacobian=False, **(dict(feedforward="Ft") if feedforward else {}),
                          **_weights(1e6))


def _flight(name, form=0):
    P, _ = _solved(NT, 0, form)
    kw = dict(formulation=form, substeps=M, **_sigmas(P))
    if name == "guided":
        kw.update(guidance=_law(form, False))
    elif name in ("navigated", "drifting"):
        kw.update(guidance=_law(form, True), nav_sigma=np.full(7, 1e-6), knowledge_sigma=1e-3 * P[:, 3])
        if name == "drifting":
            kw.update(nav_tau=TAU, knowledge_tau=5.0)
    return kw


def _limits(res):
    """(2, 12) and (2, 10): a limit inside each quantity's sampled range, and NaN / +inf"""
    end = np.concatenate([0.5 * (res.min[0] + res.max[0]), [1.0, 1e-3, 0.0]])
    return np.stack([end, np.where(np.arange(12) % 2 == 0, np.nan, np.inf)])


def _check_flown(P, blob, kw, S, history, xi=None, expect_n=None):
    """quantiles / limits with every sample kept: against the reference on the returned samples, and everything else against the
    call without the new keywords"""
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch
    xi = _xi(K, S, 21) if xi is None else xi
    keep = dict(keep_samples=True, keep_history_samples=bool(history), history=history)
    plain = disperse_batch(P, blob, NT, xi=xi, **keep, **kw)
    lim = _limits(plain)
    hlim = None
    if history:
        with np.errstate(invalid="ignore"):
            hlim = np.stack([0.5 * (plain.history.min[:, -1] + plain.history.max[:, -1]), np.full((len(P), 10), np.inf)], axis=1)      # (batch, 2, 10)
    d = disperse_batch(P, blob, NT, xi=xi, quantiles=PROBS, limits=lim, history_limits=hlim, **keep, **kw)
    fused = disperse_batch(P, blob, NT, xi=xi, quantiles=PROBS, limits=lim, history_limits=hlim, history=history, **kw)
    guided = kw.get("guidance") is not None
    B = len(P)
    for r in (d, fused):
        assert np.array_equal(_stats(r), _stats(plain), equal_nan=True)
        assert np.array_equal(r.quantile_probs, PROBS)
    assert np.array_equal(d.samples, plain.samples, equal_nan=True) and _same(d.effort, plain.effort)
    assert fused.samples is None and fused.effort is None
    rows = plain.samples if not guided else np.concatenate([plain.samples, plain.effort], axis=2)      # (batch, S, 9 | 12)
    NQ = rows.shape[2]
    values = np.ascontiguousarray(rows.transpose(2, 1, 0))[:, None]                                    # (NQ, 1, S, batch)
    L = np.ascontiguousarray(np.broadcast_to(lim[:, :NQ, None], (2, NQ, B)))
    count, quant, below = qr.sample_quantiles(values, PROBS, 9, L)
    assert np.array_equal(count[0], plain.n_valid)
    if expect_n is not None:
        assert plain.n_valid.tolist() == expect_n
    for r in (d, fused):
        assert np.array_equal(r.quantiles, quant[:, :9, 0].transpose(2, 0, 1), equal_nan=True)
        assert np.array_equal(r.below, below[:, :9, 0].transpose(2, 0, 1))
        if guided:
            assert np.array_equal(r.effort_quantiles, quant[:, 9:, 0].transpose(2, 0, 1), equal_nan=True)
            assert np.array_equal(r.effort_below, below[:, 9:, 0].transpose(2, 0, 1))
        else:
            assert r.effort_quantiles is None and r.effort_below is None
        # pi = 0 and pi = 1: the extrema the reduction reports, as values
        assert np.array_equal(r.quantiles[:, 0], plain.min, equal_nan=True) and np.array_equal(r.quantiles[:, -1], plain.max, equal_nan=True)
        # the +inf limit counts every valid sample, the NaN limit none
        assert np.array_equal(r.below[:, 1], np.where(np.arange(9) % 2 == 0, 0, plain.n_valid[:, None]))
    if not history:
        assert d.history is None and fused.history is None
        return d
    h = plain.history
    hv = np.ascontiguousarray(h.samples.transpose(3, 2, 1, 0))                                         # (10, NJ, S, batch)
    hcount, hquant, hbelow = qr.sample_quantiles(hv, PROBS, 10, np.ascontiguousarray(hlim.transpose(1, 2, 0)))
    assert np.array_equal(hcount.T, h.n_valid)
    for r in (d, fused):
        for a in ("nodes", "n_valid", "nominal", "mean", "var", "min", "max", "clipped"):
            assert np.array_equal(getattr(r.history, a), getattr(h, a), equal_nan=True), a
        assert np.array_equal(r.history.quantiles, hquant.transpose(3, 2, 0, 1), equal_nan=True)
        assert np.array_equal(r.history.below, hbelow.transpose(3, 2, 0, 1))
        assert np.array_equal(r.history.quantiles[:, :, 0], h.min, equal_nan=True) and np.array_equal(r.history.quantiles[:, :, -1], h.max, equal_nan=True)
        assert np.array_equal(r.history.below[:, :, 1], np.broadcast_to(h.n_valid[:, :, None], hbelow.shape[3:1:-1] + (10,)))
    assert np.array_equal(d.history.samples, h.samples, equal_nan=True) and fused.history.samples is None
    return d


@pytest.mark.parametrize("history", [False, 4])
@pytest.mark.parametrize("S", [65, 300])
@pytest.mark.parametrize("name", ["open", "guided", "navigated", "drifting"])
def test_flown_quantiles_bit_for_bit(name, S, history):
    P, blob = _solved(NT, 0, 0)
    d = _check_flown(P, blob, _flight(name), S, history, expect_n=[S, S])
    assert np.all(np.diff(d.quantiles, axis=1) >= 0)
    if name == "open" and history:      # the history call's open loop: three zero rows behind the nine, not reported as an effort
        assert d.effort_quantiles is None


def test_flown_quantiles_formulation_one():
    P, blob = _solved(NT, 0, 1)
    _check_flown(P, blob, _flight("navigated", form=1), 65, 4, expect_n=[65, 65])


def test_flown_quantiles_with_invalid_samples():
    """a NaN in xi's thrust row for one sample (tests/test_gpu_dispersion.py): the problem with sigma_Ft != 0 loses it, the other
    does not"""
    P, blob = _solved(NT, 0, 0)
    kw = _flight("guided")
    kw["param_sigma"][1, 3] = 0.0
    xi = _xi(K, 300, 9)
    xi[7 + 3, 131] = np.nan
    _check_flown(P, blob, kw, 300, 4, xi=xi, expect_n=[299, 300])


def test_flown_quantiles_with_no_valid_sample():
    """t_f = NaN in one blob of two: NaN quantiles and zero counts there"""
    P, blob = _solved(NT, 0, 0)
    b = np.array(blob)
    b[21 * K, 0] = np.nan
    d = _check_flown(P, b, _flight("open"), 65, 4, expect_n=[0, 65])
    assert np.isnan(d.quantiles[0]).all() and (d.below[0] == 0).all() and np.isfinite(d.quantiles[1]).all()
    assert np.isnan(d.history.quantiles[0]).all() and (d.history.below[0] == 0).all()


# ---- batch independence and chunking ----
def test_batch_independence_and_chunks(lib):
    from lunar_module_ascent_trajectory_optimiser_amd import disperse_batch, guidance_gains, solve_batch
    P = _points(5)
    r = solve_batch(P, NT, tol=1e-10, max_iter=500, want_blob=True)
    assert (r.status == 0).all()
    g = guidance_gains(P, r.blob, NT, substeps=M, want_jacobian=False, **_weights(1e6))
    S = 65
    xi = _xi(K, S, 33)
    sg = _sigmas(P)
    lim = np.full((1, 12), np.inf)
    lim[0, 7] = 15000.0

    def run(idx, **more):
        law = type("Law", (), dict(gain_u=g.gain_u[idx], gain_t=g.gain_t[idx], stretch_max=np.asarray(g.stretch_max)[idx] if np.ndim(g.stretch_max) else g.stretch_max))
        return disperse_batch(P[idx], r.blob[:, idx], NT, xi=xi, substeps=M, guidance=law, history=4, quantiles=PROBS, limits=lim,
                              history_limits=np.full((1, 10), 0.0), **{k: (v[idx] if np.ndim(v) else v) for k, v in sg.items()}, **more)
    full = run(np.arange(5))
    parts = dict(quantiles=full.quantiles, effort_quantiles=full.effort_quantiles, below=full.below, effort_below=full.effort_below,
                 hq=full.history.quantiles, hb=full.history.below, stats=_stats(full), hmean=full.history.mean)

    def parts_of(d):
        return dict(quantiles=d.quantiles, effort_quantiles=d.effort_quantiles, below=d.below, effort_below=d.effort_below, hq=d.history.quantiles,
                    hb=d.history.below, stats=_stats(d), hmean=d.history.mean)
    for j in (0, 3):
        alone = parts_of(run(np.array([j])))
        assert all(np.array_equal(alone[k][0], parts[k][j], equal_nan=True) for k in parts), j
    for n in (1, 2):      # runs of one and of two problems
        cap = lib.ascent_disperse_quantiles_bytes(n, NT, S, 4)
        assert lib.ascent_disperse_quantiles_bytes(n + 1, NT, S, 4) > cap
        assert _same(parts_of(run(np.arange(5), max_workspace_bytes=cap)), parts), n


def test_device_pointers_on_a_stream_only_enqueue_and_give_the_same_bits(lib):
    """ascent_disperse_quantiles_batch with torch tensors on a stream of its own against the same call with host pointers: every
    output bit for bit, navigated with history and limits."""
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts, history_nodes
    _lib.require_single_hip_runtime()
    P, blob = _solved(NT, 0, 0)
    g = _law(0, True)
    B, S, stride, NL = len(P), 300, 4, 2
    NJ = len(history_nodes(K, stride))
    o = _opts(NT, 0, 1.0, 0, 0.0)
    sg = _sigmas(P)
    rng = np.random.default_rng(77)
    ins = dict(p=np.array(P), blob=np.array(blob), xi=_xi(K, S, 41),      # (copies: the shared case is read-only)
               sigma=np.ascontiguousarray(np.concatenate([sg["z0_sigma"], sg["param_sigma"], sg["tf_sigma"][:, None]], axis=1).T),
               sigma_u=np.full((K, B), 1e-3), gain_u=np.ascontiguousarray(g.gain_u.transpose(2, 1, 0)), gain_t=np.ascontiguousarray(g.gain_t.T),
               stretch_max=np.full(B, 0.5), ff_u=np.ascontiguousarray(g.ff_u.T), ff_t=np.ascontiguousarray(g.ff_t),
               ff_know=np.ascontiguousarray(g.ff_know.T), xi_nav=rng.standard_normal((8, S)), sigma_nav=np.full((8, B), 1e-6),
               limits=rng.standard_normal((NL, 12, B)), hist_limits=rng.standard_normal((NL, 10, B)))
    shapes = dict(stats=(82, B), hist=(52, NJ, B), quant=(len(PROBS), 12, B), below=(NL, 12, B), hquant=(len(PROBS), 10, NJ, B), hbelow=(NL, 10, NJ, B))

    def call(a, out, stream, dev):
        pt = (lambda x: x.data_ptr()) if dev else _ptr
        _lib.check(lib.ascent_disperse_quantiles_batch(
            pt(a["p"]), B, C.byref(o), pt(a["blob"]), M, S, pt(a["xi"]), pt(a["sigma"]), pt(a["sigma_u"]), pt(a["gain_u"]), pt(a["gain_t"]),
            pt(a["stretch_max"]), pt(a["ff_u"]), pt(a["ff_t"]), pt(a["ff_know"]), pt(a["xi_nav"]), pt(a["sigma_nav"]), None, None, None, stride,
            pt(out["stats"]), pt(out["hist"]), _ptr(PROBS), len(PROBS), pt(a["limits"]), pt(a["hist_limits"]), NL, pt(out["quant"]), pt(out["below"]),
            pt(out["hquant"]), pt(out["hbelow"]), 0, stream, dev))
    host = {k: np.full(v, -1.0) for k, v in shapes.items()}
    call(ins, host, None, 0)
    assert (host["stats"][0] == S).all() and np.isfinite(host["quant"]).all()
    tin = {k: torch.from_numpy(np.array(v)).cuda() for k, v in ins.items()}
    tout = {k: torch.full(v, -1.0, dtype=torch.float64, device="cuda") for k, v in shapes.items()}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        call(tin, tout, C.c_void_p(stream.cuda_stream), 1)
    stream.synchronize()
    for k in shapes:
        assert np.array_equal(tout[k].cpu().numpy(), host[k], equal_nan=True), k
