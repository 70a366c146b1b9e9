"""numpy reference of ascent_sample_quantiles (include/ascent.h): per (quantity, group, problem) np.sort over the valid samples,
the quantile x_(lo) + g (x_(hi) - x_(lo)) written with the library's three operations -- float64 scalars, each rounded once --
and the limit counts.  Shared by test_quantile_reference.py, test_quantile_host.py and test_gpu_quantiles.py."""
import numpy as np


def valid_mask(values, valid_quantities):
    """values (Q, G, S, B) -> (G, S, B): the rows q < valid_quantities all finite"""
    Q, G, S, B = values.shape
    if valid_quantities == 0:
        return np.ones((G, S, B), dtype=bool)
    return np.isfinite(values[:valid_quantities]).all(axis=0)


def quantile_of_sorted(x, pi):
    """x: the valid values in ascending order (1-D float64).  NaN where there is none."""
    n = x.size
    if n == 0:
        return np.float64(np.nan)
    h = np.float64(pi) * np.float64(n - 1)
    lo = int(np.floor(h))
    g = h - np.float64(lo)
    hi = min(lo + 1, n - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float64(x[hi]) - np.float64(x[lo])
        m = g * d
        return np.float64(x[lo]) + m


def sample_quantiles(values, probs, valid_quantities, limits=None):
    """values (Q, G, S, B), probs (n_probs,), limits (n_limits, Q, B) or None -> count (G, B) int64, quant (n_probs, Q, G, B),
    below (n_limits, Q, G, B) int64 or None"""
    values = np.asarray(values, dtype=np.float64)
    Q, G, S, B = values.shape
    ok = valid_mask(values, valid_quantities)
    count = ok.sum(axis=1).astype(np.int64)
    quant = np.empty((len(probs), Q, G, B))
    below = None if limits is None else np.zeros((len(limits), Q, G, B), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(Q):
            for i in range(G):
                for p in range(B):
                    x = np.sort(values[q, i, ok[i, :, p], p])
                    for j, pi in enumerate(probs):
                        quant[j, q, i, p] = quantile_of_sorted(x, pi)
                    if limits is not None:
                        for l in range(len(limits)):
                            below[l, q, i, p] = int(np.count_nonzero(x <= limits[l][q][p]))
    return count, quant, below
