"""The contract of ``degrees`` and ``dbscan`` (density clusters at a threshold), stated independently of the package: a
boolean graph, a plain Python union-find over the core nodes, border nodes by first core neighbour, clusters numbered by
first member.

Two different nodes a, b are neighbours at t iff ``S[a, b] >= t`` or ``S[b, a] >= t`` in float64 (NaN passes nothing;
-0.0 >= 0.0 does); a pair that passes both ways is one neighbour.  A node is core iff ``neighbours + 1 >= min_samples``
(it counts itself, as scikit-learn counts it).  Written for reading, not for speed."""
import numpy as np

from tests.cluster_ref import graph


def degrees(S, ts):
    """int64 [len(ts), n]: per threshold the number of neighbours of every node of the square matrix S."""
    return np.array([graph(S, t).sum(axis=1) for t in ts], dtype=np.int64).reshape(len(ts), len(S))


def dbscan_of_graph(W, min_samples):
    """(cluster int64 [n], core bool [n], neighbours int64 [n], root int64 [n]) of the symmetric boolean graph W without
    a diagonal.  ``root``: per node the smallest CORE node of its cluster, -1 for noise: what the device hands back
    before the numbering."""
    W = np.asarray(W, dtype=bool)
    n = len(W)
    assert W.shape == (n, n) and not W.diagonal().any() and np.array_equal(W, W.T)
    deg = W.sum(axis=1).astype(np.int64)
    core = deg + 1 >= min_samples
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in np.argwhere(np.triu(W & core[:, None] & core[None, :])):       # clusters grow through core nodes only
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.full(n, -1, dtype=np.int64)
    for x in range(n):
        if core[x]:
            root[x] = find(x)
        elif (W[x] & core).any():
            root[x] = find(int(np.flatnonzero(W[x] & core)[0]))                 # a border node: its FIRST core neighbour
    number, cluster = {}, np.full(n, -1, dtype=np.int64)
    for x in range(n):                                                          # numbered by first member, core or border
        if root[x] >= 0:
            cluster[x] = number.setdefault(int(root[x]), len(number))
    return cluster, core, deg, root


def dbscan(S, t, min_samples):
    """(cluster, core, neighbours, root) of the square float64 matrix S at threshold t."""
    return dbscan_of_graph(graph(S, t), min_samples)


def counts(cluster, core):
    """(clusters, border nodes, noise nodes) of a result."""
    return int(cluster.max()) + 1, int(((cluster >= 0) & ~core).sum()), int((cluster < 0).sum())


def block_graph(A, ids, n, t):
    """bool [n, n] over the node ids: the graph a square block A contributes at t when position p is node ids[p] (None:
    the positions); an id outside 0 .. n - 1 is padding and its row and column are skipped."""
    A = np.asarray(A, dtype=np.float64)
    pid = np.arange(len(A)) if ids is None else np.asarray(ids, dtype=np.int64)
    ok = np.flatnonzero((pid >= 0) & (pid < n))
    W = np.zeros((n, n), dtype=bool)
    W[np.ix_(pid[ok], pid[ok])] = graph(A, t)[np.ix_(ok, ok)]
    return W
