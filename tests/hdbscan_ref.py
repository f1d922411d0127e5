"""The contract of ``core_similarity``, ``linkage(min_samples=)`` and ``hdbscan``, stated independently of the package on a
dense float64 matrix, on top of ``linkage_ref`` (pair heights, the canonical table) and ``cluster_ref`` (components).

``w(a, b) = max(S[a, b], S[b, a])`` as ``linkage_ref.weights`` has it.  ``core_m(a)`` is the (m - 1)-th largest existing
``w(a, b)``, b != a: +inf at m = 1, -inf when fewer exist.  ``mr_m(a, b) = min(w(a, b), core_m(a), core_m(b))``, and a
pair at -inf is no entry.  The table is ``linkage_ref.linkage`` of the matrix of mr.

The hierarchy is read off the definition: a CLASS is a component of ``cluster_ref.components(mr, h)`` at some distinct
height h that is no component at the next higher one; its children are the components of the next higher level inside
it (single nodes above every height).  Condensing, stability and selection follow the words of ``hdbscan``'s docstring,
one node at a time.  Written for reading, not for speed."""
import math

import numpy as np

from tests import cluster_ref as CR
from tests import linkage_ref as LR


def core(S, m):
    """float64 [n]: core_m of every node of the square matrix S."""
    W = LR.weights(S)
    out = np.empty(len(W))
    for a, row in enumerate(W):
        have = np.sort(row[~np.isnan(row)])[::-1]
        out[a] = np.inf if m == 1 else have[m - 2] if have.size >= m - 1 else -np.inf
    return out


def mutual(S, m):
    """float64 [n, n], symmetric: mr_m, NaN on the diagonal and where there is no entry."""
    W, c = LR.weights(S), core(S, m)
    M = np.minimum(W, np.minimum(c[:, None], c[None, :]))    # (a NaN of W stays)
    M[np.isneginf(M)] = np.nan
    return M


def linkage(S, m, floor=None):
    """The canonical rows of ``linkage(min_samples=m, min_similarity=floor)``."""
    return LR.linkage(mutual(S, m), floor)


class Class:
    def __init__(self, members, height, children):
        self.members, self.height, self.children = frozenset(members), height, children      # children: Class or int (a leaf)

    def size(self):
        return len(self.members)


def size_of(x):
    return 1 if isinstance(x, int) else x.size()


def members_of(x):
    return frozenset([x]) if isinstance(x, int) else x.members


def roots(M, floor=None):
    """The roots of the hierarchy of the symmetric matrix M of heights (NaN: no entry): Class objects, and the single
    nodes that never join anything as ints.  The partition at a height is the one above it with the components joined
    that an entry of exactly this height lies between (``linkage_ref.rows_of_edges`` walks the same way), so every height
    looks at its own entries only; tests/test_hdbscan_cpu.py holds this against ``roots_by_partitions``."""
    n = len(M)
    a, b, w = LR.matrix_edges(M)
    if floor is not None:
        a, b, w = a[w >= floor], b[w >= floor], w[w >= floor]
    order = np.argsort(-w, kind="stable")
    a, b, w = a[order], b[order], w[order]
    bounds = np.flatnonzero(np.r_[True, w[1:] != w[:-1], True]) if w.size else np.zeros(1, dtype=np.int64)
    name = np.arange(n)                                      # per node: the smallest member of its component
    top = {i: i for i in range(n)}                           # per component name: the Class, or the leaf
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ca, cb = name[a[lo:hi]], name[b[lo:hi]]
        between = ca != cb
        if not between.any():
            continue
        ca, cb = ca[between], cb[between]
        old = np.unique(np.concatenate([ca, cb]))
        joined = CR.labels_of_edges(old.size, zip(np.searchsorted(old, ca), np.searchsorted(old, cb)))
        for c in range(int(joined.max()) + 1):
            parts = old[joined == c]                         # ascending: the children in the order of their smallest member
            kids = [top.pop(int(p)) for p in parts]
            top[int(parts[0])] = Class(frozenset().union(*(members_of(x) for x in kids)), float(w[lo]), kids)
            name[np.isin(name, parts)] = parts[0]
    return [top[k] for k in sorted(top)]


def roots_by_partitions(M, floor=None):
    """The same roots, read off the definition: ``cluster_ref.components`` at every distinct height.  For small
    matrices."""
    n = len(M)
    now = {frozenset([i]): i for i in range(n)}              # the components above the current height -> Class or leaf
    for h in LR.heights(M):
        if floor is not None and h < floor:
            break
        labels = CR.components(M, [h])[0]
        nxt = {}
        for c in range(int(labels.max()) + 1):
            comp = frozenset(np.flatnonzero(labels == c).tolist())
            inside = sorted((x for s, x in now.items() if s <= comp), key=lambda x: min(members_of(x)))
            nxt[comp] = inside[0] if len(inside) == 1 else Class(comp, float(h) + 0.0, inside)
        now = nxt
    return sorted(now.values(), key=lambda x: min(members_of(x)))


class Cluster:
    def __init__(self, parent, birth, members):
        self.parent, self.birth, self.members = parent, birth, frozenset(members)
        self.leave, self.children = {}, []
        self.selected, self.score = False, 0.0

    def stability(self):
        return math.fsum(self.leave[p] - self.birth for p in sorted(self.members))


def condensed(M, min_cluster_size, floor=None):
    """Every cluster of the condensed tree, parents before children."""
    out = []

    def walk(X, C):
        h = X.height
        big = [x for x in X.children if size_of(x) >= min_cluster_size]
        for x in X.children:
            if x not in big or len(big) >= 2:
                for p in members_of(x):
                    C.leave[p] = h
        if len(big) >= 2:
            for x in big:
                child = Cluster(C, h, x.members)
                C.children.append(child)
                out.append(child)
                walk(x, child)
        elif len(big) == 1:
            walk(big[0], C)

    for root in roots(M, floor):
        if size_of(root) >= min_cluster_size:
            C = Cluster(None, root.height, root.members)
            out.append(C)
            walk(root, C)
    for C in out:
        assert set(C.leave) == set(C.members)
    return out


def unselect_below(C):
    for x in C.children:
        x.selected = False
        unselect_below(x)


def select(clusters, selection, allow_single_cluster):
    if selection == "leaf":
        for C in clusters:
            C.selected = not C.children and (C.parent is not None or allow_single_cluster)
        return
    assert selection == "eom"
    for C in reversed(clusters):                             # children before parents
        if not C.children:
            C.selected, C.score = True, C.stability()
            continue
        child_sum = math.fsum(x.score for x in C.children)
        if C.stability() >= child_sum and (C.parent is not None or allow_single_cluster):
            C.selected, C.score = True, C.stability()
            unselect_below(C)
        else:
            C.score = child_sum


def hdbscan(S, min_cluster_size, min_samples=None, floor=None, selection="eom", allow_single_cluster=False):
    """(labels int64 [n], core float64 [n], clusters): ``clusters`` a dict of arrays parent, birth, size, stability,
    selected, cluster, ordered by (smallest member, size descending)."""
    m = min_cluster_size if min_samples is None else min_samples
    n = len(S)
    tree = condensed(mutual(S, m), min_cluster_size, floor)
    select(tree, selection, allow_single_cluster)
    rows = sorted(tree, key=lambda C: (min(C.members), -len(C.members)))
    chosen = sorted((C for C in tree if C.selected), key=lambda C: min(C.members))
    labels = np.full(n, -1, dtype=np.int64)
    for i, C in enumerate(chosen):
        assert (labels[sorted(C.members)] == -1).all()       # the selected clusters are disjoint
        labels[sorted(C.members)] = i
    number = {id(C): i for i, C in enumerate(chosen)}
    row_of = {id(C): r for r, C in enumerate(rows)}
    clusters = {
        "parent": np.array([-1 if C.parent is None else row_of[id(C.parent)] for C in rows], dtype=np.int64),
        "birth": np.array([C.birth for C in rows], dtype=np.float64),
        "size": np.array([len(C.members) for C in rows], dtype=np.int64),
        "stability": np.array([C.stability() for C in rows], dtype=np.float64),
        "selected": np.array([C.selected for C in rows], dtype=bool),
        "cluster": np.array([number.get(id(C), -1) for C in rows], dtype=np.int64),
    }
    return labels, core(S, m), clusters


def block_core(A, ids, n, rank):
    """float64 [n] over the node ids: what the select gives on a square block A when position p is node ids[p] (None:
    the positions); an id outside 0 .. n - 1 is padding and its row and column are skipped; a node no position names has
    no pair.  ``rank`` = m - 1."""
    A = np.asarray(A, dtype=np.float64)
    pid = np.arange(len(A)) if ids is None else np.asarray(ids, dtype=np.int64)
    ok = np.flatnonzero((pid >= 0) & (pid < n))
    S = np.full((n, n), np.nan)
    S[np.ix_(pid[ok], pid[ok])] = A[np.ix_(ok, ok)]
    return core(S, rank + 1)
