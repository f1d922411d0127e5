"""Plain NumPy statements of include/simrank_exemplars.h and of ``exemplars``: the term, the ordered sum of a gain (the
header's order, restated), the exact sum, the cover rule and plain greedy on a dense float64 matrix.  Written for
reading, not for speed; no device."""
import math
from fractions import Fraction

import numpy as np

T = 256                  # SIMRANK_EXEMPLARS_THREADS


def terms(row, cover):
    """term(m, a) for every column: ``v - cover`` where ``v > cover`` (one float64 subtraction), +0.0 elsewhere; the
    comparison is false for a NaN element."""
    row, cover = np.asarray(row, dtype=np.float64), np.asarray(cover, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        up = row > cover
    out = np.zeros(row.shape, dtype=np.float64)
    out[up] = row[up] - cover[up]
    return out


def ordered_sum(t):
    """The float64 sum of the terms ``t`` [n_cols] in the header's order, which depends on n_cols alone:

    1. with the columns padded by +0.0 to whole passes of 4 T, thread ``q mod T`` of quad ``q = c // 4`` adds column
       ``4 (t + T j) + i`` into its running sum i, in the order j = 0, 1, ...;
    2. ``x_t = (s_t[0] + s_t[1]) + (s_t[2] + s_t[3])``;
    3. in every wave of 64 consecutive threads, for d = 32, 16, 8, 4, 2, 1: ``x_l = x_l + x_(l xor d)``;
    4. ``(w_0 + w_1) + (w_2 + w_3)`` over the four waves."""
    t = np.asarray(t, dtype=np.float64)
    passes = max(1, -(-t.size // (4 * T)))
    padded = np.zeros(passes * 4 * T, dtype=np.float64)
    padded[:t.size] = t
    padded = padded.reshape(passes, T, 4)
    s = np.zeros((T, 4), dtype=np.float64)
    for j in range(passes):
        s = s + padded[j]
    x = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
    lanes = np.arange(T)
    for d in (32, 16, 8, 4, 2, 1):
        x = x + x[lanes ^ d]                                   # (l xor d stays inside l's wave of 64)
    w = x[::64]
    return float((w[0] + w[1]) + (w[2] + w[3]))


def gain(row, cover):
    return ordered_sum(terms(row, cover))


def exact_sum(t):
    """The exact sum of the terms, correctly rounded."""
    return math.fsum(np.asarray(t, dtype=np.float64).tolist())


def bound(t):
    """``(n_cols + 1) * 2^-52 * (the exact sum of the terms)``: how far a float64 sum of n_cols non-negative terms in any
    order lies from the exact one (each of at most n_cols - 1 additions errs by 2^-53 of a partial sum that is at most
    the total; the factor leaves room for the second-order terms and for the rounding of the exact sum itself)."""
    t = np.asarray(t, dtype=np.float64)
    return (t.size + 1) * 2.0 ** -52 * exact_sum(t)


def exact_fraction(t):
    return sum((Fraction(float(x)) for x in np.asarray(t, dtype=np.float64) if x != 0), Fraction(0))


def apply(row, cover):
    """The cover rule on ``cover`` in place: ``cover[a] = v`` iff ``v > cover[a]`` -> the number of columns raised."""
    row = np.asarray(row, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        up = row > cover
    cover[up] = row[up]
    return int(up.sum())


def block_gains(A, rows, cover, total=ordered_sum):
    """simrank_exemplars_gains on the logical matrix A: NaN for a row outside the block.  ``total``: how a row's terms are
    added (``ordered_sum``, or ``exact_sum`` where every sum is exact)."""
    rows = range(A.shape[0]) if rows is None else rows
    return np.array([total(terms(A[r], cover)) if 0 <= r < A.shape[0] else np.nan for r in rows], dtype=np.float64)


def block_cover(A, rows, cover, raised):
    """simrank_exemplars_cover: (the cover after the listed rows were applied in order, the counters after it)."""
    cover, raised = np.array(cover, dtype=np.float64), np.array(raised, dtype=np.int64)
    for i, r in enumerate(rows):
        if 0 <= r < A.shape[0]:
            raised[i] += apply(A[r], cover)
    return cover, raised


def coverage(rows):
    """The final cover from the rows [m, n] of the given and the picked nodes: ``np.maximum.reduce`` with the +0.0 start
    and the NaN rule (a NaN never covers)."""
    rows = np.asarray(rows, dtype=np.float64)
    start = np.zeros((1, rows.shape[1]))
    return np.maximum.reduce(np.concatenate([start, np.where(np.isnan(rows), 0.0, rows)]), axis=0)


class DenseEvaluator:
    """The evaluator interface of ``_exemplars.greedy`` on a dense float64 matrix, with the ordered sum."""

    def __init__(self, S, total=ordered_sum):
        self.S, self.total = np.asarray(S, dtype=np.float64), total
        self.cover = np.zeros(self.S.shape[1], dtype=np.float64)
        self.calls = []                                        # the rows of every gains call (None: a sweep)

    def gains(self, rows):
        self.calls.append(None if rows is None else np.array(rows))
        return block_gains(self.S, None if rows is None else np.asarray(rows).tolist(), self.cover, self.total)

    def apply(self, row):
        return apply(self.S[row], self.cover)


def greedy(S, k, given=(), total=ordered_sum):
    """Plain greedy on the dense matrix S -> (picks, gains, raised, cover): ``given`` rows applied first and never
    picked; k times the candidate first in the order (gain descending, position ascending), then its row applied."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    cover = np.zeros(S.shape[1], dtype=np.float64)
    for g in given:
        apply(S[g], cover)
    out = set(int(g) for g in given)
    picks, gains, raised = [], [], []
    for _ in range(k):
        best, best_gain = -1, 0.0
        for m in range(n):
            if m in out:
                continue
            g = total(terms(S[m], cover))
            if best < 0 or g > best_gain:                      # (positions ascend: the first of a tie stays)
                best, best_gain = m, g
        picks.append(best)
        gains.append(best_gain)
        raised.append(apply(S[best], cover))
        out.add(best)
    return np.array(picks, dtype=np.int64), np.array(gains, dtype=np.float64), np.array(raised, dtype=np.int64), cover
