"""A plain NumPy statement of the candidate filter, written for reading: ``ref_topk`` is the contract of
``simrank_candidates_topk`` (include/simrank_candidates.h), ``ref_most_similar`` what ``most_similar(nodes, k, among=,
exclude=)`` returns, stated on the dense frame."""
import numpy as np
import pandas as pd


def ref_topk(A, row_pos, row_ids, cand_pos, cand_ids, k):
    """(ids int32 [n_q, k], values float64 [n_q, k]): for each query the k best of row ``row_pos[q]`` of ``A`` among the
    listed columns.  Candidate i is column ``cand_pos[i]`` with the id ``cand_ids[i]`` (``cand_pos[i]`` without
    ``cand_ids``); value descending, ties by LIST INDEX ascending.  No candidate: the one whose id is ``row_ids[q]``, a
    NaN, a position outside the columns; a row outside the block has none.  -0.0 and +0.0 tie and keep their bits.
    Slots past the candidates hold -1 / 0.0."""
    n_rows, n_cols = A.shape
    cand_pos = np.asarray(cand_pos, dtype=np.int64).reshape(-1)
    ids = cand_pos if cand_ids is None else np.asarray(cand_ids, dtype=np.int64)
    idx = np.full((len(row_pos), k), -1, dtype=np.int32)
    val = np.zeros((len(row_pos), k), dtype=np.float64)
    inside = (cand_pos >= 0) & (cand_pos < n_cols)
    for q, (r, own) in enumerate(zip(row_pos, row_ids)):
        if not 0 <= r < n_rows:
            continue
        values = np.full(cand_pos.size, np.nan)
        values[inside] = A[r, cand_pos[inside]]                # (a position outside is not read)
        i = np.flatnonzero(inside & (ids != own) & ~np.isnan(values))         # list indices of the candidates
        i = i[np.lexsort((i, -values[i]))][:k]                 # (-(-0.0) == -(+0.0): the zeros tie; then the list index)
        idx[q, :i.size], val[q, :i.size] = ids[i], values[i]
    return idx, val


def ref_most_similar(dense, nodes, k, among=None, exclude=None):
    """The long frame (node, rank, neighbor, similarity) of ``most_similar(nodes, k, among=, exclude=)`` from the dense
    frame ``dense``: per node its candidates ``(among or every label) - exclude - {node}`` sorted by (-value, label
    position), NaN dropped, cut at k."""
    labels = list(dense.index)
    at = {lab: i for i, lab in enumerate(labels)}
    allowed = set(labels if among is None else among) - set(() if exclude is None else exclude)
    cand = sorted(at[x] for x in allowed)
    V = dense.to_numpy()
    rows = {"node": [], "rank": [], "neighbor": [], "similarity": []}
    for a in nodes:
        r = at[a]
        ranked = sorted((-V[r, c], c) for c in cand if c != r and not np.isnan(V[r, c]))
        for j, (_, c) in enumerate(ranked[:k]):
            rows["node"].append(a)
            rows["rank"].append(j + 1)
            rows["neighbor"].append(labels[c])
            rows["similarity"].append(V[r, c])
    as_labels = lambda xs: pd.Index(xs, dtype=dense.index.dtype) if xs else dense.index[:0]
    return pd.DataFrame({"node": as_labels(rows["node"]), "rank": np.asarray(rows["rank"], dtype=np.int64),
                         "neighbor": as_labels(rows["neighbor"]),
                         "similarity": np.asarray(rows["similarity"], dtype=np.float64)})
