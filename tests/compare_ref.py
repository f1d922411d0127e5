"""The NumPy statement of include/simrank_compare.h and of ``model.compare``: the definitions on widened float64 arrays,
vectorised, written for reading.  ``np.argmax`` returns the first occurrence of a maximum: the smallest column attaining
it.  Nothing here is a floating-point sum, so the device's outputs equal these bit for bit."""
import numpy as np

BINS = 2048


def distance(A, B):
    """d of every pair of elements: +0.0 where a == b or both are NaN, +inf where exactly one is NaN, else |a - b|."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    na, nb = np.isnan(A), np.isnan(B)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(A - B)
    d[(A == B) | (na & nb)] = 0.0
    d[na ^ nb] = np.inf
    assert not np.isnan(d).any() and not np.signbit(d).any()
    return d


def relative(A, B, d, floor):
    """rel of every pair, the first rule that applies: +0.0 where d == 0 or max(|a|, |b|) < floor (a NaN operand makes the
    maximum NaN, which is below nothing), +inf where d == inf, else d / max(|a|, |b|)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    m = np.maximum(np.abs(A), np.abs(B))                   # (np.maximum propagates NaN)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rel = d / m
        small = (d == 0) | (m < floor)
    rel[d == np.inf] = np.inf
    rel[small] = 0.0
    assert not np.isnan(rel).any() and not np.signbit(rel).any()
    return rel


def sweep(A, B, tol=(), floor=0.0):
    """simrank_compare_sweep on the widened matrices -> (max_abs float64 [rows], arg_abs int32, max_rel, arg_rel, over
    uint32 [rows, len(tol)], hist uint64 [2048]: what the call ADDS)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    assert A.shape == B.shape and A.ndim == 2
    rows, cols = A.shape
    d = distance(A, B)
    rel = relative(A, B, d, floor)
    if cols:
        max_abs, arg_abs = d.max(axis=1), d.argmax(axis=1).astype(np.int32)
        max_rel, arg_rel = rel.max(axis=1), rel.argmax(axis=1).astype(np.int32)
    else:
        max_abs, max_rel = np.zeros(rows), np.zeros(rows)
        arg_abs, arg_rel = np.full(rows, -1, dtype=np.int32), np.full(rows, -1, dtype=np.int32)
    over = np.stack([(d > t).sum(axis=1) for t in tol], axis=1).astype(np.uint32) if len(tol) else \
        np.zeros((rows, 0), dtype=np.uint32)
    hist = np.bincount((np.ascontiguousarray(d).view(np.uint64) >> np.uint64(52)).ravel().astype(np.int64),
                       minlength=BINS).astype(np.uint64)
    return max_abs, arg_abs, max_rel, arg_rel, over, hist


def lists_agreement(ids_a, ids_b):
    """Two id tables [n, k] (-1: an empty slot) -> (overlap, same_prefix) int64 [n], by plain set logic."""
    overlap, prefix = [], []
    for la, lb in zip(np.asarray(ids_a).tolist(), np.asarray(ids_b).tolist()):
        overlap.append(len({x for x in la if x >= 0} & {x for x in lb if x >= 0}))
        p = 0
        for x, y in zip(la, lb):
            if x < 0 or x != y:
                break
            p += 1
        prefix.append(p)
    return np.array(overlap, dtype=np.int64), np.array(prefix, dtype=np.int64)


def id_table(long, index, k):
    """A ``most_similar(all nodes, k)`` long frame -> int64 [n, k] of positions in ``index``, -1 in the empty slots."""
    n = len(index)
    out = np.full((n, k), -1, dtype=np.int64)
    rows = index.get_indexer(long["node"])
    out[rows, long["rank"].to_numpy() - 1] = index.get_indexer(long["neighbor"])
    return out


def model(SA, SB, index, tolerances, floor, lists=None):
    """``model.compare`` of one group from the two dense frames' values -> (summary dict, nodes dict of columns, hist
    int64 [2048]).  ``lists``: (ids_a, ids_b, k) for the neighbour lists' agreement."""
    n = len(index)
    tol = tuple(sorted(set(tolerances) | {0.0}))
    max_abs, arg_abs, max_rel, arg_rel, over, hist = sweep(SA, SB, tol, floor)
    over = over.astype(np.int64)
    nodes = {"max_abs": max_abs, "at": index.take(arg_abs).to_numpy(), "max_rel": max_rel,
             "at_rel": index.take(arg_rel).to_numpy(), "differing": over[:, tol.index(0.0)]}
    for t in tolerances:
        nodes[f"over@{float(t)!r}"] = over[:, tol.index(float(t))]
    d = distance(SA, SB)
    rel = relative(SA, SB, d, floor)
    r, c = np.unravel_index(int(np.argmax(d)), d.shape)    # (the first pair in row-major order)
    r2, c2 = np.unravel_index(int(np.argmax(rel)), rel.shape)
    summary = {"entries": n * n, "differing": int((d > 0).sum()), "max_abs": d[r, c], "node": index[r], "neighbor": index[c],
               "max_rel": rel[r2, c2], "node_rel": index[r2], "neighbor_rel": index[c2]}
    for t in tolerances:
        summary[f"over@{float(t)!r}"] = int((d > t).sum())
    if lists is not None:
        ids_a, ids_b, k = lists
        nodes["overlap"], nodes["same_prefix"] = lists_agreement(ids_a, ids_b)
        summary["mean_overlap"] = float(nodes["overlap"].sum()) / n
        summary["identical_lists"] = int((nodes["same_prefix"] == k).sum())
    return summary, nodes, hist.astype(np.int64)
