"""The numpy reference of the order statistics (tests/quantile_reference.py) against numpy itself.  No GPU."""
import numpy as np
import pytest

import quantile_reference as qr

EPS = np.finfo(np.float64).eps
PROBS = (0.0, 0.00135, 0.25, 0.5, 0.75, 0.99865, 1.0)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 257, 1000])
def test_reference_against_np_quantile(n):
    """Both sides evaluate x_(lo) + g (x_(hi) - x_(lo)) or an equivalent of it in three roundings of quantities no larger than
    twice max(|x_(lo)|, |x_(hi)|), so they agree within 8 eps of that maximum: derived, not tuned."""
    rng = np.random.default_rng(n)
    for x in (rng.standard_normal(n), 1e6 + rng.standard_normal(n), rng.integers(0, 4, n).astype(np.float64)):
        s = np.sort(x)
        for pi in PROBS + tuple(rng.random(5)):
            got, want = qr.quantile_of_sorted(s, pi), np.quantile(x, pi)
            h = pi * (n - 1)
            lo = int(np.floor(h))
            hi = min(lo + 1, n - 1)
            assert abs(got - want) <= 8 * EPS * max(abs(s[lo]), abs(s[hi])), (n, pi, got, want)


def test_the_ends_are_the_extrema():
    x = np.sort(np.random.default_rng(3).standard_normal(300))
    assert qr.quantile_of_sorted(x, 0.0) == x[0] and qr.quantile_of_sorted(x, 1.0) == x[-1]


def test_no_one_and_two_samples():
    assert np.isnan(qr.quantile_of_sorted(np.array([]), 0.5))
    assert qr.quantile_of_sorted(np.array([3.5]), 0.3) == 3.5
    two = np.array([1.0, 3.0])
    assert [qr.quantile_of_sorted(two, p) for p in (0.0, 0.25, 0.5, 1.0)] == [1.0, 1.5, 2.0, 3.0]


def test_validity_counts_and_limits():
    """values (Q = 3, G = 1, S = 5, B = 2), V = 2: a sample with a NaN or an infinity in rows 0 .. 1 is left out of every row; row 2
    may hold anything.  A limit equal to a sample counts it; a NaN limit counts nothing, +inf everything but NaN."""
    v = np.zeros((3, 1, 5, 2))
    v[0, 0, :, 0] = [4.0, 1.0, np.nan, 2.0, 3.0]
    v[1, 0, :, 0] = [0.0, 0.0, 0.0, np.inf, 0.0]
    v[2, 0, :, 0] = [np.nan, 5.0, 6.0, 7.0, -8.0]
    v[:, 0, :, 1] = np.arange(15.0).reshape(3, 5)
    lim = np.empty((4, 3, 2))
    lim[0], lim[1], lim[2], lim[3] = 3.0, -np.inf, np.inf, np.nan
    count, quant, below = qr.sample_quantiles(v, (0.0, 0.5, 1.0), 2, lim)
    assert count.tolist() == [[3, 5]]
    assert quant[:, 0, 0, 0].tolist() == [1.0, 3.0, 4.0]              # samples 0, 1, 4 are valid
    assert quant[0, 2, 0, 0] == -8.0 and np.isnan(quant[2, 2, 0, 0])         # row 2 of them: nan, 5, -8; NaN sorts last
    assert below[0, 0, 0, 0] == 2 and below[0, 0, 0, 1] == 4          # 1 and 3 (the limit itself); 0 .. 3
    assert below[1, 0, 0, 0] == 0 and below[1, 2, 0, 0] == 0          # -inf: nothing finite
    assert below[2, 0, 0, 0] == 3 and below[2, 2, 0, 0] == 2          # +inf: not the NaN
    assert (below[3] == 0).all()
    count0, _, _ = qr.sample_quantiles(v, (0.5,), 0)
    assert count0.tolist() == [[5, 5]]
