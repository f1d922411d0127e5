"""A float64 NumPy statement of ``score_sets`` and ``recommend`` on a dense matrix.

    score(q, b) = sum_{e in basket q} w_e * S[e, b]:     acc = 0.0; for e in list order: acc = acc + (w_e * S[e])

every product and every sum one IEEE double operation (NumPy's elementwise ``*`` and ``+`` never fuse), then the
exclusion and a stable sort on (-score, position).  tests/test_sets_cpu.py checks it on a hand-made case and against the
reference's ``W @ S``; tests/test_gpu_sets.py holds the device to it bit for bit."""
import numpy as np
import pandas as pd


def scores(S, lists, weights=None):
    """float64 [len(lists), N]: ``lists`` integer positions (rows of ``S``) per basket, ``weights`` one array per basket
    (default ones)."""
    S = np.asarray(S, dtype=np.float64)
    out = np.zeros((len(lists), S.shape[1]), dtype=np.float64)
    for q, members in enumerate(lists):
        acc = np.zeros(S.shape[1], dtype=np.float64)
        w = np.ones(len(members)) if weights is None else np.asarray(weights[q], dtype=np.float64)
        for e, i in enumerate(members):
            acc = acc + (w[e] * S[int(i)])
        out[q] = acc
    return out


def best(row, k, excluded=()):
    """(positions, values) of the k best candidates of one score row: score descending, position ascending; excluded
    positions, -inf and NaN are no candidates."""
    row = np.asarray(row, dtype=np.float64)
    ok = np.isfinite(row) | (row == np.inf)
    ok[np.asarray(list(excluded), dtype=np.int64)] = False
    cand = np.flatnonzero(ok)
    order = cand[np.argsort(-row[cand], kind="stable")][:k]
    return order, row[order]


def long_frame(first, who, labels, dense, k, excluded, keep=None):
    """The long frame (``first``, rank, neighbor, score) of the k best per row of ``dense``; ``who``: pandas Index with
    one label per row."""
    qs, ranks, ps, vals = [], [], [], []
    for q, row in enumerate(dense):
        if keep is not None and not keep[q]:
            continue
        pos, val = best(row, k, excluded[q] if excluded is not None else ())
        qs += [q] * len(pos)
        ranks += list(range(1, len(pos) + 1))
        ps += list(pos)
        vals += list(val)
    return pd.DataFrame({first: who.take(np.asarray(qs, dtype=np.int64)), "rank": np.asarray(ranks, dtype=np.int64),
                         "neighbor": pd.Index(labels).take(np.asarray(ps, dtype=np.int64)),
                         "score": np.asarray(vals, dtype=np.float64)})


def score_sets_ref(frame, sets, weights=None, names=None, top_k=None, exclude="members"):
    """``model.score_sets(...)`` restated on the dense ``frame`` of that group."""
    labels = list(frame.index)
    at = {lab: i for i, lab in enumerate(labels)}
    lists = [[at[x] for x in one] for one in sets]
    dense = scores(frame.values, lists, weights)
    who = pd.RangeIndex(len(sets)) if names is None else pd.Index(list(names))
    if top_k is None:
        return pd.DataFrame(dense, index=who, columns=frame.columns.copy())
    if exclude is None:
        excluded = None
    elif isinstance(exclude, str):
        excluded = lists
    else:
        excluded = [[at[x] for x in one] for one in exclude]
    return long_frame("set", who, labels, dense, min(top_k, len(labels)), excluded)


def recommend_ref(read_frame, node_labels, rowptr, col, rowscale, nodes, k, exclude_seen=True, also_self=False):
    """``model.recommend(nodes, k)`` restated: ``read_frame`` the dense frame of the group the baskets live in,
    ``node_labels`` the labels of the group ``nodes`` belong to, (``rowptr``, ``col``, ``rowscale``) that group's CSR over
    the other one (positions in the frames' orders); ``also_self``: the directed classes, where u is no candidate."""
    at = {lab: i for i, lab in enumerate(node_labels)}
    us = [at[x] for x in nodes]
    lists = [list(col[rowptr[u]:rowptr[u + 1]]) for u in us]
    weights = [np.full(len(l), rowscale[u], dtype=np.float64) for l, u in zip(lists, us)]
    dense = scores(read_frame.values, lists, weights)
    excluded = [l + ([u] if also_self else []) for l, u in zip(lists, us)] if exclude_seen else None
    labels = list(read_frame.index)
    return long_frame("node", pd.Index(node_labels).take(np.asarray(us, dtype=np.int64)), labels, dense, min(k, len(labels)), excluded, keep=[len(l) > 0 for l in lists])
