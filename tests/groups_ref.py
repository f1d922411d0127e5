"""``cluster_quality`` & co in plain NumPy loops, on a float64 matrix ``S`` and a vector of integer cluster values: every
definition of include/simrank_groups.h and ``_KeptModel.cluster_quality``, written for reading.  Sums are ``math.fsum``
(the exact sum, rounded once); the order and the tie rules are written out; ``bound`` is what a float64 sum in any order
may differ from it by.

    M_g(a)       {b : labels[b] = g, b != a}
    sum(a, g)    the sum of S[a, b] over M_g(a)            (row a; a sum of zeros of either sign is +0.0)
    mean(a, g)   sum / |M_g(a)|, NaN when M_g(a) is empty
    own          mean(a, labels[a])
    other        the first mean(a, g), g != labels[a], in the order (mean descending, cluster value ascending); NaN is
                 never chosen; nearest = that g.  No candidate: nearest = labels[a], other = NaN
"""
import math

import numpy as np

NAN = float("nan")


def clusters_of(labels):
    """The distinct cluster values, ascending."""
    return sorted(set(int(x) for x in labels))


def members(labels, g, a):
    return [b for b in range(len(labels)) if int(labels[b]) == g and b != a]


def mean_of(S, a, m):
    """mean of S[a, b] over the list m; NaN when it is empty."""
    if not m:
        return NAN
    return (math.fsum(float(S[a, b]) for b in m) + 0.0) / len(m)          # (+ 0.0: -0.0 counts as zero)


def mean(S, labels, a, g):
    return mean_of(S, a, members(labels, g, a))


def means(S, labels):
    """float64 [N, K]: mean(a, g), the clusters ascending."""
    cl = clusters_of(labels)
    of = {g: [b for b in range(len(labels)) if int(labels[b]) == g] for g in cl}
    out = np.empty((len(labels), len(cl)), dtype=np.float64)
    for a in range(len(labels)):
        for k, g in enumerate(cl):
            out[a, k] = mean_of(S, a, [b for b in of[g] if b != a] if int(labels[a]) == g else of[g])
    return out


def quality(S, labels, table=None):
    """(own float64 [N], nearest int64 [N], other float64 [N]) from the table of means (``means(S, labels)``)."""
    cl = clusters_of(labels)
    table = means(S, labels) if table is None else table
    n = len(labels)
    own, other, nearest = np.full(n, NAN), np.full(n, NAN), np.zeros(n, dtype=np.int64)
    for a in range(n):
        mine = int(labels[a])
        own[a] = table[a, cl.index(mine)]
        best = None
        for k, g in enumerate(cl):                                         # ascending: the first of equal means stays
            v = table[a, k]
            if g == mine or math.isnan(v):
                continue
            if best is None or v > best[0]:
                best = (v, g)
        nearest[a], other[a] = (mine, NAN) if best is None else (best[1], best[0])
    return own, nearest, other


def silhouette(own, other, singleton):
    """One node's, checked in this order."""
    if singleton:
        return 0.0
    if math.isnan(own) or math.isnan(other):
        return NAN
    top = max(own, other)
    return (own - other) / top if top > 0 else 0.0


def silhouettes(labels, own, other):
    size = {g: sum(1 for x in labels if int(x) == g) for g in clusters_of(labels)}
    return np.array([silhouette(float(own[a]), float(other[a]), size[int(labels[a])] == 1) for a in range(len(labels))])


def medoids(labels, own):
    """cluster -> the position of its medoid: the largest ``own``, the first member of a tie, NaN skipped; all NaN: the
    first member."""
    out = {}
    for g in clusters_of(labels):
        m = [a for a in range(len(labels)) if int(labels[a]) == g]
        best = None
        for a in m:
            if not math.isnan(own[a]) and (best is None or own[a] > own[best]):
                best = a
        out[g] = m[0] if best is None else best
    return out


def summary(labels, own, other, sil):
    """cluster -> (size, cohesion, separation, silhouette): fsum over the members / size; NaN propagates."""
    out = {}
    for g in clusters_of(labels):
        m = [a for a in range(len(labels)) if int(labels[a]) == g]
        out[g] = (len(m),) + tuple(math.fsum(float(x[a]) for a in m) / len(m) for x in (own, other, sil))
    return out


# ---- the bound ---------------------------------------------------------------------------------------------------------------
def bound(S, labels):
    """float64 [N, K]: how far a float64 MEAN computed in any order of additions may lie from ``means``.  The sum of m
    values in any order is within (m - 1) u sum|x| / (1 - (m - 1) u) of the exact one (u = 2^-53), which
    m * 2^-52 * sum|x| covers twice over; dividing by m divides the error, and the quotient's own rounding and the
    reference's two roundings (the fsum and its division) add at most 3 u |mean| <= 2^-51 |mean|:
        |got - mean| <= 2^-52 * sum|S[a, b]| + 2^-51 * |mean|                     (sum over M_g(a))"""
    cl = clusters_of(labels)
    of = {g: [b for b in range(len(labels)) if int(labels[b]) == g] for g in cl}
    out = np.zeros((len(labels), len(cl)))
    for a in range(len(labels)):
        for k, g in enumerate(cl):
            m = [b for b in of[g] if b != a]
            if m:
                out[a, k] = mean_bound([abs(float(S[a, b])) for b in m])
    return out


def mean_bound(magnitudes):
    """The bound above for one mean, from the magnitudes of its terms (0 where a term is NaN: nothing is compared)."""
    total = math.fsum(magnitudes)
    return 0.0 if math.isnan(total) else 2.0 ** -52 * total + 2.0 ** -51 * total / len(magnitudes)


# ---- the C entry on a block ----------------------------------------------------------------------------------------------------
def block_means(A, row_group, row_col, col_pos, group_ptr):
    """simrank_groups_means on the logical matrix ``A`` [n_rows, n_cols] of a block: (own [n_rows], other [n_rows], nearest
    int32 [n_rows], means [n_rows, K], bound [n_rows, K]).  A list position outside the columns reads NaN; the position
    row_col[r] is left out; the rows with row_group[r] < 0 hold NaN / -2 here: the call leaves them untouched."""
    n_rows, n_cols = A.shape
    k = len(group_ptr) - 1
    lists = [[int(c) for c in col_pos[group_ptr[g]:group_ptr[g + 1]]] for g in range(k)]
    own, other = np.full(n_rows, NAN), np.full(n_rows, NAN)
    nearest = np.full(n_rows, -2, dtype=np.int32)
    table, tol = np.full((n_rows, k), NAN), np.zeros((n_rows, k))
    for r in range(n_rows):
        mine = int(row_group[r])
        if mine < 0:
            continue
        row = [float(x) for x in A[r]]
        best = None
        for g in range(k):
            v = [row[c] if 0 <= c < n_cols else NAN for c in lists[g] if c != row_col[r]]
            if v:
                table[r, g] = (v[0] if len(v) == 1 else math.fsum(v)) + 0.0
                table[r, g] /= len(v)
                tol[r, g] = mean_bound([abs(x) for x in v])
            if g != mine and not math.isnan(table[r, g]) and (best is None or table[r, g] > best[0]):
                best = (table[r, g], g)
        own[r] = table[r, mine]
        nearest[r], other[r] = (-1, NAN) if best is None else (best[1], best[0])
    return own, other, nearest, table, tol


# ---- a vectorised twin (tools/bench_groups.py: the route the device call replaces) -----------------------------------------------
def quality_fast(S, labels):
    """(own, nearest, other) with NumPy group-bys: one matrix product's worth of additions per cluster, float64 in NumPy's
    order.  Equal to ``quality`` within ``bound``; ties in ``nearest`` go to the smaller cluster value, as there."""
    labels = np.asarray(labels, dtype=np.int64)
    cl, gidx = np.unique(labels, return_inverse=True)
    gidx = gidx.reshape(-1)
    n, k = labels.size, cl.size
    order = np.argsort(gidx, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(gidx, minlength=k))[:-1]])
    G = np.asarray(S, dtype=np.float64)[:, order]                           # a copy, the columns cluster-major
    where = np.empty(n, dtype=np.int64)
    where[order] = np.arange(n)
    G[np.arange(n), where] = 0.0                                           # a node is no member of its own M_g(a)
    sums = np.add.reduceat(G, starts, axis=1) + 0.0
    counts = np.broadcast_to(np.bincount(gidx, minlength=k), (n, k)).astype(np.float64).copy()
    counts[np.arange(n), gidx] -= 1
    with np.errstate(invalid="ignore", divide="ignore"):
        table = np.where(counts > 0, sums / counts, np.nan)
    own = table[np.arange(n), gidx]
    cand = table.copy()
    cand[np.arange(n), gidx] = np.nan
    none = np.isnan(cand).all(axis=1)
    best = np.argmax(np.where(np.isnan(cand), -np.inf, cand), axis=1)      # (the first of equal maxima: the smaller cluster)
    other = np.where(none, np.nan, cand[np.arange(n), best])
    nearest = np.where(none, labels, cl[best])
    return own, nearest, other
