"""The contract of ``linkage`` and ``cut`` (the single-linkage dendrogram in its canonical order), stated independently of
the package in plain NumPy on float64, on top of ``cluster_ref``'s union-find.

Two different nodes a, b have the weight ``w(a, b) = max(S[a, b], S[b, a])``: a NaN entry is no entry (one NaN: the other
direction decides; two: no edge), -0.0 and +0.0 are one height, +0.0.  With h1 > h2 > ... the distinct heights and P(h) the
partition ``cluster_ref.components`` gives at h: going from P(h_(j-1)) to P(h_j), every class that unites m >= 2 earlier
classes c1 .. cm (in the order of their smallest member) gives the rows (c1, c2) -> x1, (x1, c3) -> x2, ...; the new classes
of one height come in the order of their smallest member.  Leaves are 0 .. n - 1; row i forms cluster n + i.

P(h_j) is P(h_(j-1)) with the classes joined that an entry of height exactly h_j lies between, so ``rows_of_edges`` walks
the heights downwards and looks, per height, only at its own entries.  Written for reading, not for speed."""
import numpy as np

from tests import cluster_ref as CR


def weights(S):
    """float64 [n, n]: w(a, b) of a square matrix, NaN on the diagonal and where there is no edge."""
    S = np.asarray(S, dtype=np.float64)
    assert S.ndim == 2 and S.shape[0] == S.shape[1]
    with np.errstate(invalid="ignore"):
        W = np.fmax(S, S.T) + 0.0                            # (fmax passes a NaN over; -0.0 + 0.0 = +0.0)
    np.fill_diagonal(W, np.nan)
    return W


def heights(S):
    """The distinct heights of a square matrix, descending."""
    W = weights(S)
    return np.unique(W[~np.isnan(W)])[::-1]


def matrix_edges(S):
    """(a, b, w) over the pairs a < b of a square matrix that have an edge."""
    W = weights(S)
    a, b = np.triu_indices(len(W), 1)
    w = W[a, b]
    ok = ~np.isnan(w)
    return a[ok], b[ok], w[ok]


def block_edges(A, row_ids, col_ids, n):
    """(a, b, v): the entries a block A [n_rows, n_cols] of a larger matrix contributes, ``cluster_ref.block_edges``
    without a threshold: row r is node row_ids[r], column c node col_ids[c] (None: the positions); an id outside 0 ..
    n - 1 is padding; an entry between a node and itself and a NaN entry are none.  A pair met twice has the larger
    value as its weight: ``rows_of_edges`` sees to that by taking the larger first."""
    A = np.asarray(A, dtype=np.float64)
    rid = np.arange(A.shape[0]) if row_ids is None else np.asarray(row_ids, dtype=np.int64)
    cid = np.arange(A.shape[1]) if col_ids is None else np.asarray(col_ids, dtype=np.int64)
    ok = ~np.isnan(A) & ((rid >= 0) & (rid < n))[:, None] & ((cid >= 0) & (cid < n))[None, :] & (rid[:, None] != cid[None, :])
    r, c = np.nonzero(ok)
    return rid[r], cid[c], A[r, c] + 0.0


def rows_of_edges(n, a, b, v, floor=None):
    """(left, right, similarity, size) as int64 / int64 / float64 / int64 arrays: the canonical rows of the graph on nodes
    0 .. n - 1 with an edge (a[i], b[i]) of weight v[i] (no NaN); edges with v < floor are not used."""
    a, b, v = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(v, dtype=np.float64) + 0.0
    if floor is not None:
        use = v >= floor
        a, b, v = a[use], b[use], v[use]
    order = np.argsort(-v, kind="stable")
    a, b, v = a[order], b[order], v[order]
    bounds = np.flatnonzero(np.r_[True, v[1:] != v[:-1], True]) if v.size else np.zeros(1, dtype=np.int64)
    name = np.arange(n)                                      # per node: the smallest member of its class
    cluster, members = np.arange(n), np.ones(n, dtype=np.int64)          # per class name: cluster id, size
    out = []
    BATCH = 4096                                             # heights looked at together: most of them join nothing
    g = 0
    while g < len(bounds) - 1:
        g_hi = g + 1
        while g_hi < len(bounds) - 1 and bounds[g_hi] - bounds[g] < BATCH:
            g_hi += 1
        lo, hi = bounds[g], bounds[g_hi]
        open_ = name[a[lo:hi]] != name[b[lo:hi]]
        # a height none of whose entries lies between two classes now will have none later either
        todo = [k for k in range(g, g_hi) if open_[bounds[k] - lo:bounds[k + 1] - lo].any()] if open_.any() else []
        for k in todo:
            s = slice(bounds[k], bounds[k + 1])
            ca, cb = name[a[s]], name[b[s]]
            between = ca != cb
            if not between.any():
                continue
            ca, cb = ca[between], cb[between]
            old = np.unique(np.concatenate([ca, cb]))        # the earlier classes this height touches, by smallest member
            joined = CR.labels_of_edges(old.size, zip(np.searchsorted(old, ca), np.searchsorted(old, cb)))
            for c in range(int(joined.max()) + 1):           # (numbered by first member: the order of the new classes)
                parts = old[joined == c]
                acc, total = cluster[parts[0]], members[parts[0]]
                for p in parts[1:]:
                    total += members[p]
                    out.append((acc, cluster[p], float(v[bounds[k]]), total))
                    acc = n + len(out) - 1
                name[np.isin(name, parts)] = parts[0]
                cluster[parts[0]], members[parts[0]] = acc, total
        g = g_hi
    cols = list(zip(*out)) if out else [[], [], [], []]
    return (np.array(cols[0], dtype=np.int64), np.array(cols[1], dtype=np.int64), np.array(cols[2], dtype=np.float64),
            np.array(cols[3], dtype=np.int64))


def linkage(S, floor=None):
    """The canonical rows of a square matrix."""
    return rows_of_edges(len(S), *matrix_edges(S), floor=floor)


def linkage_by_partitions(S, floor=None):
    """The same rows, read off the definition: ``cluster_ref.components`` at every distinct height.  For small matrices;
    tests/test_linkage_cpu.py holds ``linkage`` against it."""
    S = np.asarray(S, dtype=np.float64)
    n = len(S)
    hs = [h for h in heights(S) if floor is None or h >= floor]
    prev = np.arange(n)
    cluster, members = {i: i for i in range(n)}, {i: 1 for i in range(n)}          # per class label of `prev`
    out = []
    for h in hs:
        now = CR.components(S, [h])[0]
        new_cluster, new_members = {}, {}
        for c in range(int(now.max()) + 1):
            parts = sorted(set(prev[now == c].tolist()))     # labels are numbered by first member
            acc, total = cluster[parts[0]], members[parts[0]]
            for p in parts[1:]:
                total += members[p]
                out.append((acc, cluster[p], float(h) + 0.0, total))
                acc = n + len(out) - 1
            new_cluster[c], new_members[c] = acc, total
        prev, cluster, members = now, new_cluster, new_members
    cols = list(zip(*out)) if out else [[], [], [], []]
    return (np.array(cols[0], dtype=np.int64), np.array(cols[1], dtype=np.int64), np.array(cols[2], dtype=np.float64),
            np.array(cols[3], dtype=np.int64))


def cut(n, rows, t=None, n_clusters=None):
    """int64 [n]: labels numbered by first member after the rows with similarity >= t, or the first n - n_clusters rows."""
    left, right, sim, _ = rows
    m = int((sim >= t).sum()) if t is not None else n - n_clusters
    assert 0 <= m <= len(left)
    leaves = {i: [i] for i in range(n)}
    for i in range(m):
        leaves[n + i] = leaves.pop(int(left[i])) + leaves.pop(int(right[i]))
    label = np.empty(n, dtype=np.int64)
    for k, group in enumerate(sorted(leaves.values(), key=min)):
        label[group] = k
    return label


def stats(n, rows):
    """(distinct heights, the largest m of a merge of m classes into one) of a table of n leaves: what the tests ask of a
    case that is to count.  Row i continues the merge of row i - 1 when its ``left`` is the cluster that row formed."""
    left, _, sim, _ = rows
    widest = run = 2 if len(left) else 0
    for i in range(1, len(left)):
        run = run + 1 if left[i] == n + i - 1 and sim[i] == sim[i - 1] else 2
        widest = max(widest, run)
    return int(np.unique(sim).size), widest
