"""A float64 NumPy statement of ``score_sets(diversity=d)`` and ``recommend(diversity=d)`` on a dense matrix: greedy
maximal-marginal-relevance picks.

    pen = +0.0;  k times:  value = (rel_w * score) - (d * pen);  pick the live candidate with the greatest value that is
    not NaN, ties by position (-0.0 and +0.0 tie);  pen = where(S[pick] > pen, S[pick], pen)

``rel_w = 1.0 - d`` once; NumPy's elementwise ``*`` and ``-`` never fuse, so every value is three IEEE double
operations.  ROW ``pick`` of S is read.  Built on ``sets_ref.scores`` and its exclusions.  tests/test_diverse_cpu.py
checks it on a hand-made case; the GPU tests hold the device to it bit for bit."""
import numpy as np
import pandas as pd

from tests import sets_ref


def picks(score, row_of, k, d):
    """One basket: ``score`` float64 [n] (excluded candidates at -inf), ``row_of(b)`` the float64 [n] row of the matrix for
    pick b (entry c = S[b, c]) -> (positions int64, score, penalty, value float64) of at most k picks, in picking order."""
    score = np.asarray(score, dtype=np.float64)
    rel_w, d = 1.0 - float(d), float(d)
    pen = np.zeros(score.size, dtype=np.float64)
    live = ~np.isnan(score) & (score != -np.inf)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(k):
            value = (rel_w * score) - (d * pen)
            cand = np.flatnonzero(live & ~np.isnan(value))
            if not cand.size:
                break
            key = value[cand] + 0.0                                        # (-0.0 + 0.0 = +0.0: the two zeros tie)
            b = int(cand[np.argsort(-key, kind="stable")[0]])
            out.append((b, score[b], pen[b], value[b]))
            live[b] = False
            x = np.asarray(row_of(b), dtype=np.float64)
            pen = np.where(x > pen, x, pen)
    pos = np.array([o[0] for o in out], dtype=np.int64)
    return (pos,) + tuple(np.array([o[i] for o in out], dtype=np.float64) for i in (1, 2, 3))


def band_picks(band, row_of, k, d):
    """The library's four outputs for a band [n_sets, n_out]: (idx int32 [n_sets, k], score, pen, value float64), slots
    past the last pick at -1 / 0."""
    n_sets = len(band)
    idx = np.full((n_sets, k), -1, dtype=np.int32)
    score, pen, val = (np.zeros((n_sets, k), dtype=np.float64) for _ in range(3))
    for q, row in enumerate(band):
        p, s, pn, v = picks(row, row_of, k, d)
        idx[q, :p.size], score[q, :p.size], pen[q, :p.size], val[q, :p.size] = p, s, pn, v
    return idx, score, pen, val


def dense_p(ids, vals, diag):
    """The matrix P of a pruned model's tables: the kept entries of each row, the diagonal, +0.0 everywhere else (an id
    outside 0 .. n - 1 is an empty slot)."""
    n = len(diag)
    P = np.zeros((n, n), dtype=np.float64)
    for a in range(n):
        ok = (ids[a] >= 0) & (ids[a] < n)
        P[a, ids[a][ok]] = vals[a][ok]
        P[a, a] = diag[a]
    return P


def long_frame(first, who, labels, dense, S, k, d, excluded, keep=None):
    """The long frame (``first``, rank, neighbor, score, penalty, value) of the k picks per row of ``dense``."""
    S = np.asarray(S, dtype=np.float64)
    qs, ranks, ps, cols = [], [], [], ([], [], [])
    for q, row in enumerate(dense):
        if keep is not None and not keep[q]:
            continue
        row = np.array(row, dtype=np.float64)
        if excluded is not None:
            row[np.asarray(list(excluded[q]), dtype=np.int64)] = -np.inf
        pos, *three = picks(row, lambda b: S[b], k, d)
        qs += [q] * len(pos)
        ranks += list(range(1, len(pos) + 1))
        ps += list(pos)
        for c, v in zip(cols, three):
            c += list(v)
    return pd.DataFrame({first: who.take(np.asarray(qs, dtype=np.int64)), "rank": np.asarray(ranks, dtype=np.int64),
                         "neighbor": pd.Index(labels).take(np.asarray(ps, dtype=np.int64)),
                         "score": np.asarray(cols[0], dtype=np.float64), "penalty": np.asarray(cols[1], dtype=np.float64),
                         "value": np.asarray(cols[2], dtype=np.float64)})


def score_sets_ref(frame, sets, weights=None, names=None, top_k=None, exclude="members", diversity=0.0):
    """``model.score_sets(..., top_k=k, diversity=d)`` restated on the dense ``frame`` of that group."""
    labels = list(frame.index)
    at = {lab: i for i, lab in enumerate(labels)}
    lists = [[at[x] for x in one] for one in sets]
    dense = sets_ref.scores(frame.values, lists, weights)
    who = pd.RangeIndex(len(sets)) if names is None else pd.Index(list(names))
    if exclude is None:
        excluded = None
    elif isinstance(exclude, str):
        excluded = lists
    else:
        excluded = [[at[x] for x in one] for one in exclude]
    return long_frame("set", who, labels, dense, frame.values, min(top_k, len(labels)), diversity, excluded)


def recommend_ref(read_frame, node_labels, rowptr, col, rowscale, nodes, k, exclude_seen=True, also_self=False,
                  diversity=0.0):
    """``model.recommend(nodes, k, diversity=d)`` restated; the arguments of ``sets_ref.recommend_ref``."""
    at = {lab: i for i, lab in enumerate(node_labels)}
    us = [at[x] for x in nodes]
    lists = [list(col[rowptr[u]:rowptr[u + 1]]) for u in us]
    weights = [np.full(len(l), rowscale[u], dtype=np.float64) for l, u in zip(lists, us)]
    dense = sets_ref.scores(read_frame.values, lists, weights)
    excluded = [l + ([u] if also_self else []) for l, u in zip(lists, us)] if exclude_seen else None
    labels = list(read_frame.index)
    return long_frame("node", pd.Index(node_labels).take(np.asarray(us, dtype=np.int64)), labels, dense, read_frame.values,
                      min(k, len(labels)), diversity, excluded, keep=[len(l) > 0 for l in lists])
