"""The contract of ``components`` (single-linkage clusters at a threshold), stated independently of the package: a boolean
graph, a plain Python union-find, components numbered by first member.

Two different nodes a, b are joined at t iff ``S[a, b] >= t`` or ``S[b, a] >= t`` in float64 (NaN joins nothing; -0.0 >=
0.0 does).  Written for reading, not for speed."""
import numpy as np


def labels_of_edges(n, edges):
    """int64 [n]: the components of the graph on nodes 0 .. n - 1 with the given (a, b) edges, numbered 0, 1, 2, ... in
    the order of each component's first member."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in edges:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    number, out = {}, np.empty(n, dtype=np.int64)
    for x in range(n):
        out[x] = number.setdefault(find(x), len(number))
    return out


def graph(S, t):
    """bool [n, n]: the OR-symmetrised graph of a square float64 matrix at threshold t, nothing on the diagonal."""
    S = np.asarray(S, dtype=np.float64)
    assert S.ndim == 2 and S.shape[0] == S.shape[1]
    with np.errstate(invalid="ignore"):
        hit = S >= t
    adj = hit | hit.T
    np.fill_diagonal(adj, False)
    return adj


def components(S, ts):
    """int64 [len(ts), n]: per threshold the labels of every node of the square matrix S."""
    n = len(S)
    return np.array([labels_of_edges(n, np.argwhere(np.triu(graph(S, t)))) for t in ts], dtype=np.int64).reshape(len(ts), n)


def block_edges(A, row_ids, col_ids, n, t):
    """The (a, b) edges a block A [n_rows, n_cols] of a larger matrix contributes at t: row r is node row_ids[r], column c
    node col_ids[c] (None: the positions); an id outside 0 .. n - 1 is padding; an entry between a node and itself is none."""
    A = np.asarray(A, dtype=np.float64)
    rid = np.arange(A.shape[0]) if row_ids is None else np.asarray(row_ids, dtype=np.int64)
    cid = np.arange(A.shape[1]) if col_ids is None else np.asarray(col_ids, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        hit = A >= t
    hit &= ((rid >= 0) & (rid < n))[:, None] & ((cid >= 0) & (cid < n))[None, :] & (rid[:, None] != cid[None, :])
    r, c = np.nonzero(hit)
    return list(zip(rid[r].tolist(), cid[c].tolist()))


def matrix_of_lists(ids, vals):
    """float64 [n, n]: the matrix P of a pruned model's lists: ``vals[i, j]`` at (i, ids[i, j]) where ids[i, j] >= 0, +0.0
    elsewhere (the diagonal too: it joins nothing)."""
    n = len(ids)
    P = np.zeros((n, n))
    for i in range(n):
        for j, v in zip(ids[i], vals[i]):
            if j >= 0:
                P[i, j] = v
    return P
