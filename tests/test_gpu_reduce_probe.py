"""The lane reductions and the 16-lane scan of the persistent kernels (csrc/ascent_persist_dev.hpp) on DPP moves against the
shuffle butterflies they replaced, through the test hook ascent_reduce_probe: the two versions of every quantity must agree bit
for bit on every lane -- the kernels' results may not move by a rounding -- and be NaN together."""
import ctypes as C

import numpy as np
import pytest

from lunar_module_ascent_trajectory_optimiser_amd import _lib

pytestmark = pytest.mark.gpu
ROWS = ("sum16", "max16", "min16", "sumW", "maxW", "minW", "scan16")
PAIRS = ((0, 3), (1, 4), (2, 5), (6, 9), (7, 10), (8, 11), (12, 13))      # (DPP helpers, shuffles) rows of a record


def _inputs():
    rng = np.random.default_rng(20)
    v = rng.choice([-1.0, 1.0], (256, 64)) * 10.0 ** rng.uniform(-15.0, 15.0, (256, 64))      # 30 decades, mixed signs
    tiny = 4.9406564584124654e-324
    special = []
    pz = np.zeros(64)
    special.append(pz)                                                       # +0 everywhere
    special.append(-pz)                                                      # -0 everywhere
    a = np.zeros(64); a[::2] = -0.0; special.append(a)                       # +0 and -0 alternating: sums and max / min of signed zeros
    a = np.zeros(64); a[1::4] = -0.0; a[2::8] = -0.0; special.append(a)
    a = v[0].copy(); a[5] = np.inf; a[40] = np.inf; special.append(a)        # +inf
    a = v[1].copy(); a[9] = -np.inf; a[63] = -np.inf; special.append(a)      # -inf
    a = v[2].copy(); a[3] = np.inf; a[12] = -np.inf; special.append(a)       # both in one row of 16: the sum is NaN there
    special.append(rng.integers(-2000, 2000, 64) * tiny)                     # denormals
    a = rng.integers(1, 2000, 64) * tiny; a[::3] *= -1.0; a[7] = 1e-300; special.append(a)
    a = v[3].copy(); a[1::2] = -a[0::2]; special.append(a)                   # equal magnitudes of opposite sign, neighbours
    a = v[4].copy(); a[8:16] = -a[0:8]; a[48:64] = -a[32:48]; special.append(a)      # ... across the halves of a row, across rows
    a = np.full(64, 1e308); a[::2] = -1e308; special.append(a)
    a = v[5].copy(); a[22] = np.nan; special.append(a)                       # a NaN in one lane
    a = v[6].copy(); a[0] = np.nan; special.append(a)
    return np.ascontiguousarray(np.concatenate([v, np.stack(special)]))


@pytest.fixture(scope="module")
def probe():
    L = _lib.load()
    x = _inputs()
    out = np.full((len(x), _lib.REDUCE_PROBE_ROWS, 64), -7.0)
    _lib.check(L.ascent_reduce_probe(x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p), 0))
    return x, out


@pytest.mark.parametrize("q", range(len(PAIRS)), ids=ROWS)
def test_dpp_equals_shuffle_bit_for_bit(probe, q):
    x, out = probe
    a, b = out[:, PAIRS[q][0], :], out[:, PAIRS[q][1], :]
    nan = np.isnan(a) | np.isnan(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))                          # NaN in both where in either
    assert np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])
    assert not nan[:256].any()
    if ROWS[q][:3] in ("sum", "sca"):                                        # (fmax / fmin drop a NaN operand; the sums must carry it)
        assert nan[256:].any()


def test_probe_computes_the_reductions(probe):
    """The hook reports what it says: exact quantities (max, min, the first lanes of the scan) against numpy, sums to rounding."""
    x, out = probe
    r = x[:256].reshape(256, 4, 16)
    rep = lambda a: np.repeat(a, 16, axis=1)
    assert np.array_equal(out[:256, 1], rep(r.max(axis=2))) and np.array_equal(out[:256, 2], rep(r.min(axis=2)))
    assert np.array_equal(out[:256, 7], np.repeat(x[:256].max(axis=1, keepdims=True), 64, axis=1))
    assert np.array_equal(out[:256, 8], np.repeat(x[:256].min(axis=1, keepdims=True), 64, axis=1))
    scale = rep(np.abs(r).sum(axis=2))
    assert np.all(np.abs(out[:256, 0] - rep(r.sum(axis=2))) <= 16 * 2.3e-16 * scale)
    assert np.all(np.abs(out[:256, 6] - x[:256].sum(axis=1, keepdims=True)) <= 64 * 2.3e-16 * np.abs(x[:256]).sum(axis=1, keepdims=True))
    scan = np.cumsum(r, axis=2).reshape(256, 64)
    assert np.array_equal(out[:256, 12].reshape(256, 4, 16)[:, :, 0], r[:, :, 0])
    assert np.array_equal(out[:256, 12].reshape(256, 4, 16)[:, :, 1], r[:, :, 0] + r[:, :, 1])
    assert np.all(np.abs(out[:256, 12] - scan) <= 16 * 2.3e-16 * np.cumsum(np.abs(r), axis=2).reshape(256, 64))
    # signed zeros: the sum of -0s is -0, max(+0, -0) = +0, min = -0 -- on every lane, in either version
    z = 256 + 1
    assert np.all(np.signbit(out[z, 0])) and np.all(np.signbit(out[z, 12]))
    assert not np.signbit(out[z + 1, 1]).any() and np.signbit(out[z + 1, 2]).all()


def test_probe_refuses_bad_arguments():
    L = _lib.load()
    x = np.zeros(64)
    assert L.ascent_reduce_probe(None, 1, x.ctypes.data_as(C.c_void_p), 0) == -1
    assert L.ascent_reduce_probe(x.ctypes.data_as(C.c_void_p), 0, x.ctypes.data_as(C.c_void_p), 0) == -1
