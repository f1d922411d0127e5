"""``count_pairs`` and ``threshold_for`` stated in NumPy on a dense float64 matrix: counts over the off-diagonal mask,
``threshold_for`` by sorting.  ``skip``: a boolean mask of the entries that are no pairs (default: the diagonal of a
square matrix)."""
import math

import numpy as np


def off_diagonal(S, skip=None):
    """float64 1-D: the entries that count as pairs."""
    S = np.asarray(S, dtype=np.float64)
    if skip is None:
        assert S.shape[0] == S.shape[1]
        skip = np.eye(S.shape[0], dtype=bool)
    return S[~np.asarray(skip, dtype=bool)]


def count_pairs(S, thresholds, skip=None):
    """int64 [len(thresholds)]: #{pairs : S >= t} per threshold, in the order given (NaN >= t is False)."""
    v = off_diagonal(S, skip)
    with np.errstate(invalid="ignore"):
        return np.array([int(np.count_nonzero(v >= float(t))) for t in thresholds], dtype=np.int64)


def threshold_for(S, max_pairs, skip=None):
    """(t, n): the smallest value t among the pairs with n = #{pairs : S >= t} <= max_pairs; (inf, 0) when there is
    none.  -0.0 and +0.0 are one value, +0.0; NaN is ignored."""
    v = off_diagonal(S, skip)
    v = np.sort(v[~np.isnan(v)])[::-1]                       # descending
    best = (math.inf, 0)
    i = 0
    while i < v.size:
        j = i
        while j < v.size and v[j] == v[i]:                   # (the run of equal values: -0.0 == +0.0)
            j += 1
        if j > max_pairs:
            break
        best = (float(v[i]) + 0.0, j)                        # (-0.0 + 0.0 = +0.0)
        i = j
    return best
