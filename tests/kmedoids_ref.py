"""``assign`` and ``kmedoids`` in plain NumPy loops: every definition of include/simrank_kmedoids.h and of
``_KeptModel.assign`` / ``kmedoids``, written for reading.  Nothing is added in the two steps themselves: they compare
and copy, so they are exact on any values; the sums are in ``own``, which a caller supplies (``own_of``).

    v(j, a)      S[m_j, a]: row m_j, the j-th medoid's
    order        (v descending, j ascending); a NaN is never chosen; -0.0 equals +0.0 (Python's ``>`` on floats)
    assign       node a -> the first j in that order; no candidate: cluster 0.  With a current cluster c: a moves to the
                 best j* iff v(j*, a) > v(c, a), or v(c, a) is NaN and a candidate exists.  A medoid is in its own cluster
    pick         cluster j keeps its medoid unless a member has a strictly larger own (NaN never is; a NaN incumbent loses
                 to any non-NaN); the new medoid is the member with the largest own, the first in order on a tie
"""
import math

import numpy as np

NAN = float("nan")


# ---- the C entries on a block ------------------------------------------------------------------------------------------------
def block_assign(A, med_row, med_col, current=None):
    """simrank_kmedoids_assign on the logical matrix ``A`` [n_rows, n_cols] of a block -> (cluster int32 [n_cols], value
    float64 [n_cols], the number added to *moved).  A medoid row outside the block reads NaN; an entry of ``current``
    outside 0 .. K - 1 is no current cluster; column med_col[j] is cluster j (the first such j)."""
    n_rows, n_cols = A.shape
    k = len(med_row)
    cluster, value, moved = np.zeros(n_cols, dtype=np.int32), np.full(n_cols, NAN), 0
    V = np.full((k, n_cols), NAN)                                          # v(j, c)
    for j, r in enumerate(med_row):
        if 0 <= r < n_rows:
            V[j] = A[r]
    owner = {}                                                             # column -> the first medoid whose own node it is
    for j in range(k - 1, -1, -1):
        owner[int(med_col[j])] = j
    for c in range(n_cols):
        v = V[:, c]
        candidates = np.flatnonzero(~np.isnan(v))
        best = int(candidates[np.argmax(v[candidates])]) if candidates.size else None     # (argmax: the first of equal values)
        cur = None if current is None or not 0 <= current[c] < k else int(current[c])
        if c in owner:
            at = owner[c]
        elif cur is None:
            at = 0 if best is None else best
        elif best is not None and (v[best] > v[cur] or math.isnan(v[cur])):
            at = best
        else:
            at = cur
        cluster[c], value[c] = at, v[at]
        moved += current is None or at != current[c]
    return cluster, value, int(moved)


def block_pick(own, col_pos, group_ptr, med_row):
    """simrank_kmedoids_pick -> (med_row int32 [K] after the call, cohesion float64 [K], the number added to *changed).  A
    position outside 0 .. len(own) - 1 is skipped (as a member) or reads NaN (as the incumbent); an empty list leaves its
    medoid and has the cohesion NaN."""
    n = len(own)
    at = lambda p: float(own[p]) if 0 <= p < n else NAN
    med, cohesion, changed = np.array(med_row, dtype=np.int32), np.full(len(med_row), NAN), 0
    for j in range(len(med_row)):
        members = [int(p) for p in col_pos[group_ptr[j]:group_ptr[j + 1]]]
        if not members:
            continue
        best = None
        for p in members:                                                  # list order: the first of equal values stays
            if 0 <= p < n and not math.isnan(at(p)) and (best is None or at(p) > at(best)):
                best = p
        mine = at(med[j])
        if best is not None and (at(best) > mine or math.isnan(mine)):
            med[j], cohesion[j], changed = best, at(best), changed + 1
        else:
            cohesion[j] = mine
    return med, cohesion, changed


# ---- on a square matrix --------------------------------------------------------------------------------------------------------
def assign(S, medoids, current=None, rows_only=False):
    """(cluster int64 [N], value float64 [N], moved) for the medoids (node positions) on the matrix ``S`` [N, N]; with
    ``rows_only`` ``S`` holds the medoids' rows [K, N] alone."""
    S = np.asarray(S, dtype=np.float64)
    rows = np.arange(len(medoids)) if rows_only else medoids
    cluster, value, moved = block_assign(S, list(rows), list(medoids), current)
    return cluster.astype(np.int64), value, moved


def pick(own, labels, medoids):
    """(medoids int64 [K], cohesion float64 [K], changed): a cluster's members in ascending order (the frame's)."""
    k = len(medoids)
    lists = [np.flatnonzero(np.asarray(labels) == j) for j in range(k)]
    ptr = np.zeros(k + 1, dtype=np.int64)
    np.cumsum([l.size for l in lists], out=ptr[1:])
    med, cohesion, changed = block_pick(own, np.concatenate(lists), ptr, medoids)
    return med.astype(np.int64), cohesion, changed


def objective(cohesion, sizes):
    return math.fsum(float(c) * (int(s) - 1) for c, s in zip(cohesion, sizes) if s > 1)


def kmedoids(S, seeds, max_iter, own_of):
    """The alternation -> (cluster int64 [N], medoids int64 [K], similarity float64 [N], sizes int64 [K], cohesion float64
    [K], history [(moved, changed, objective)]).  ``S``: the matrix [N, N], or a function from K medoid positions to their
    rows [K, N] (``model.rows``); ``own_of(labels)``: float64 [N], ``own`` of ``cluster_quality`` for the labelling (from
    ``groups_ref.quality``, or from a model).  ``similarity[a]`` is the element of a's FINAL medoid's row."""
    rows_of = S if callable(S) else (lambda m: np.asarray(S, dtype=np.float64)[m])
    medoids, k = np.array(seeds, dtype=np.int64), len(seeds)
    cluster, history = None, []
    for _ in range(max_iter):
        cluster, _, moved = assign(rows_of(medoids), medoids, cluster, rows_only=True)
        sizes = np.bincount(cluster, minlength=k).astype(np.int64)
        medoids, cohesion, changed = pick(own_of(cluster), cluster, medoids)
        history.append((moved, changed, objective(cohesion, sizes)))
        if changed == 0:
            break
    V = np.asarray(rows_of(medoids), dtype=np.float64)
    return cluster, medoids, V[cluster, np.arange(V.shape[1])], sizes, cohesion, history
