"""A float64 NumPy statement of ``rank_sets``, ``rank_recommended`` and ``evaluate`` on a dense matrix, built on
tests/sets_ref.py: the score rows (``scores``), the exclusion as -inf, and per target

    before     = #{columns c: v_c > -inf and (v_c > s, or v_c == s and id(c) < t)}     s the target's score, t its id
    candidates = #{columns c: v_c > -inf}
    rank       = 1 + before where s > -inf, 0 elsewhere (an excluded target, or one scored NaN)

every comparison one IEEE double comparison (NaN compares false, -0.0 == +0.0).  tests/test_rank_cpu.py checks it on a
hand-made case against ``sets_ref.best``; the GPU tests hold the device to it for equality."""
import numpy as np
import pandas as pd

from tests import sets_ref as R


def count(row, ids, s, t):
    """(before, candidates) of one band row: ``ids`` the ids of its columns, (``s``, ``t``) the target's score and id."""
    row = np.asarray(row, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        cand = row > -np.inf
        precedes = cand & ((row > s) | ((row == s) & (np.asarray(ids) < t)))
    return int(precedes.sum()), int(cand.sum())


def rank_of(s, before):
    return 1 + before if s > -np.inf else 0


def excluded_rows(dense, excluded):
    """``dense`` with every basket's excluded positions set to -inf (a copy)."""
    out = np.array(dense, dtype=np.float64, copy=True)
    if excluded is not None:
        for q, x in enumerate(excluded):
            out[q, np.asarray(list(x), dtype=np.int64)] = -np.inf
    return out


def long_frame(first, who, labels, band, target_lists, live=None):
    """The long frame (``first``, target, score, rank, candidates): one row per listed target (positions), from the
    marked band; ``live``: per basket whether it ranks anything at all."""
    ids = np.arange(band.shape[1])
    qs, ts, ss, rs, cs = [], [], [], [], []
    for q, targets in enumerate(target_lists):
        for t in targets:
            s = band[q, t]
            before, cand = count(band[q], ids, s, t)
            dead = live is not None and not live[q]
            qs.append(q), ts.append(t), ss.append(s)
            rs.append(0 if dead else rank_of(s, before)), cs.append(0 if dead else cand)
    return pd.DataFrame({first: who.take(np.asarray(qs, dtype=np.int64)),
                         "target": pd.Index(labels).take(np.asarray(ts, dtype=np.int64)),
                         "score": np.asarray(ss, dtype=np.float64), "rank": np.asarray(rs, dtype=np.int64),
                         "candidates": np.asarray(cs, dtype=np.int64)})


def rank_sets_ref(frame, sets, targets, weights=None, names=None, exclude="members"):
    """``model.rank_sets(...)`` restated on the dense ``frame`` of that group."""
    labels = list(frame.index)
    at = {lab: i for i, lab in enumerate(labels)}
    lists = [[at[x] for x in one] for one in sets]
    dense = R.scores(frame.values, lists, weights)
    if exclude is None:
        excluded = None
    elif isinstance(exclude, str):
        excluded = lists
    else:
        excluded = [[at[x] for x in one] for one in exclude]
    who = pd.RangeIndex(len(sets)) if names is None else pd.Index(list(names))
    return long_frame("set", who, labels, excluded_rows(dense, excluded), [[at[x] for x in one] for one in targets])


def rank_recommended_ref(read_frame, node_labels, rowptr, col, rowscale, nodes, targets, exclude_seen=True, also_self=False):
    """``model.rank_recommended(nodes, targets)`` restated from ``sets_ref.recommend_ref``'s inputs."""
    at = {lab: i for i, lab in enumerate(node_labels)}
    us = [at[x] for x in nodes]
    lists = [list(col[rowptr[u]:rowptr[u + 1]]) for u in us]
    weights = [np.full(len(l), rowscale[u], dtype=np.float64) for l, u in zip(lists, us)]
    dense = R.scores(read_frame.values, lists, weights)
    excluded = [l + ([u] if also_self else []) for l, u in zip(lists, us)] if exclude_seen else None
    labels = list(read_frame.index)
    to = {lab: i for i, lab in enumerate(labels)}
    return long_frame("node", pd.Index(node_labels).take(np.asarray(us, dtype=np.int64)), labels,
                      excluded_rows(dense, excluded), [[to[x] for x in one] for one in targets],
                      live=[len(l) > 0 for l in lists])


def evaluate_ref(long, nodes, targets, ks):
    """``model.evaluate(nodes, targets, ks)`` restated on ``rank_recommended``'s long frame, node by node."""
    rows, at = [], 0
    for node, one in zip(nodes, targets):
        ranks = long["rank"].to_numpy()[at:at + len(one)]
        at += len(one)
        good = ranks[ranks > 0]
        best = int(good.min()) if good.size else 0
        row = {"node": node, "targets": len(one), "not_candidates": int((ranks == 0).sum()), "best_rank": best,
               "reciprocal_rank": 1.0 / best if best else 0.0}
        for k in ks:
            row[f"hits@{k}"] = int(((ranks >= 1) & (ranks <= k)).sum())
        rows.append(row)
    return pd.DataFrame(rows, columns=["node", "targets", "not_candidates", "best_rank", "reciprocal_rank"]
                        + [f"hits@{k}" for k in ks])
