"""ctypes binding of libsimrank_hdbscan.so (include/simrank_hdbscan.h), and HDBSCAN* of a kept model on top of it.

Two different nodes a, b have the pair height ``w(a, b) = max(S[a, b], S[b, a])`` (``linkage``'s: NaN is no entry, both
zeros are +0.0).  ``core_similarity(m)`` is every node's (m - 1)-th largest pair height, the node counting itself as
``dbscan`` counts: +inf at m = 1, -inf when fewer pairs exist.  ``linkage(min_samples=m)`` is single linkage on the mutual
reachability ``min(w(a, b), core(a), core(b))``, and ``hdbscan`` reads clusters of different density off that table.

The device does the two steps that read the matrix: a radix select over both directions of every pair (the count sweeps
pair each 64 x 64 tile with its transposed partner, as ``degrees`` does) and the Boruvka rounds of ``_linkage`` with a pick
that clamps every entry by two core similarities.  Everything after the table is host arithmetic here (``condense``).
The sweeps read the one square block of a side in place (``SolverQueries.one_block``).  A pruned model (a solver with
``lists``) is answered on the host for its matrix P.  No CPU fallback for the matrices: a missing library or device is
an error.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _linkage
from ._checks import is_int
from ._companion import PANEL_F16, PANEL_F32, ROWMAJOR_F32, ROWMAJOR_F64, Companion  # noqa: F401 (a block's layouts)
from ._driver import Scratch, stage

VERSION = 1              # SIMRANK_HDBSCAN_VERSION of include/simrank_hdbscan.h
TILE = 64                # SIMRANK_HDBSCAN_TILE
DIGIT_BITS, BINS = 4, 16                # SIMRANK_HDBSCAN_DIGIT_BITS, SIMRANK_HDBSCAN_BINS
BAD_COMPONENT = 1        # bit of the pick's device status word
SELECTIONS = ("eom", "leaf")

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_hdbscan_version": [],
    "simrank_hdbscan_last_error": [],
    "simrank_hdbscan_select_passes": [_i32],
    "simrank_hdbscan_select_init": [_vp, _vp, _vp, _i64, _i64, _vp],
    "simrank_hdbscan_select_count": [_vp, _i32, _i64, _i64, _vp, _i32, _vp, _vp, _vp],
    "simrank_hdbscan_select_step": [_i32, _i32, _vp, _vp, _vp, _i64, _vp],
    "simrank_hdbscan_select_finish": [_i32, _vp, _vp, _i64, _vp, _vp, _vp],
    "simrank_hdbscan_select": [_vp, _i32, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    "simrank_hdbscan_pick": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp],
}
_RESTYPES = {"simrank_hdbscan_last_error": C.c_char_p}


class HdbscanError(RuntimeError):
    """A call into libsimrank_hdbscan.so failed."""


_c = Companion("hdbscan", VERSION, PROTOTYPES, _RESTYPES, HdbscanError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- argument checks: nothing touches a device ---------------------------------------------------------------------------
def check_min_samples(min_samples) -> int:
    """``min_samples``: an int >= 1 -> the rank m - 1 of the pair height that is the core similarity (the node counts
    itself), capped at what an int32 holds.  ValueError otherwise."""
    if not is_int(min_samples) or min_samples < 1:
        raise ValueError(f"min_samples must be an int >= 1, not {min_samples!r}")
    return int(min(int(min_samples) - 1, 2 ** 31 - 1))


def check_hdbscan(min_cluster_size, min_samples, min_similarity, selection):
    """The arguments of ``hdbscan`` -> (min_cluster_size, rank, floor).  ValueError otherwise."""
    if not is_int(min_cluster_size) or min_cluster_size < 2:
        raise ValueError(f"min_cluster_size must be an int >= 2, not {min_cluster_size!r}")
    rank = check_min_samples(min_cluster_size if min_samples is None else min_samples)
    if selection not in SELECTIONS:
        raise ValueError(f"selection must be one of {', '.join(map(repr, SELECTIONS))}, not {selection!r}")
    return int(min_cluster_size), rank, _linkage.check_floor(min_similarity)


# ---- the device path -----------------------------------------------------------------------------------------------------
def _square(b, n):
    assert b["rows"] == n and b["cols"] == n and b.get("col_lo", 0) == 0, "the select takes one square block"
    return b["ptr"], b["layout"], b["stride"]


def cmp_bytes(layout) -> int:
    """Bytes of a value in the type the block is compared in: float, or double for float64."""
    return 8 if layout == ROWMAJOR_F64 else 4


def select_passes(layout) -> int:
    return 16 if layout == ROWMAJOR_F64 else 4 if layout == PANEL_F16 else 8


def _select(lib, ops, scratch, b, n, rank, timing):
    """Queue the select of the square block ``b`` -> (device core float64 [n], device core in the compare type [n])."""
    S, layout, stride = _square(b, n)
    prefix, remaining, hist = scratch.malloc(8 * n), scratch.malloc(4 * n), scratch.malloc(4 * BINS * n)
    core64, core_cmp = scratch.malloc(8 * n), scratch.malloc(cmp_bytes(layout) * n)
    stage(ops, timing, "select_ms", lambda: check(lib.simrank_hdbscan_select(
        S, layout, stride, n, b.get("row_ids"), rank, prefix, remaining, hist, core64, core_cmp, ops.stream),
        "simrank_hdbscan_select"))
    return core64, core_cmp


def core_block(ops, b, n: int, rank: int, timing=None) -> np.ndarray:
    """float64 [n]: every node's ``rank``-th largest pair height in the square block ``b`` (a dict with ptr, layout,
    stride, rows = cols = n and optional device row_ids naming ids 0 .. n - 1 for its positions)."""
    assert n >= 1 and rank >= 0
    lib = load()
    got = np.empty(n, dtype=np.float64)
    with Scratch(ops) as scratch:
        core64, _ = _select(lib, ops, scratch, b, n, rank, timing)
        ops.d2h(got, core64)
        ops.synchronize()
    return got


def forest_blocks(ops, b, blocks, n: int, rank: int, floor, timing=None):
    """(core float64 [n], a, b, value, rounds): the core similarities of the square block ``b``, then
    ``_linkage.forest_blocks`` over ``blocks`` (the same block, or column blocks of the same matrix) with
    ``simrank_hdbscan_pick``: a maximum spanning forest of the mutual reachability."""
    assert n >= 1 and rank >= 0
    lib = load()
    core = np.empty(n, dtype=np.float64)
    with Scratch(ops) as scratch:
        core64, core_cmp = _select(lib, ops, scratch, b, n, rank, timing)
        ops.d2h(core, core64)

        def pick(u, floor_ref, phase, comp, best, n_, status, stream):
            check(lib.simrank_hdbscan_pick(u["ptr"], u["layout"], u["stride"], u["rows"], u["cols"], u.get("row_ids"),
                                           u.get("col_ids"), floor_ref, phase, core_cmp, comp, best, n_, status, stream),
                  "simrank_hdbscan_pick")
        a, c, value, rounds = _linkage.forest_blocks(ops, blocks, n, floor, timing, pick=pick)
    return core, a, c, value, rounds


# ---- the host path of a pruned model ---------------------------------------------------------------------------------------
def core_of_lists(ids, vals, rank: int) -> np.ndarray:
    """float64 [n]: the core similarities of the matrix P of a pruned model: ``ids`` int [n, k] (-1: an empty slot),
    ``vals`` float64 [n, k] the kept off-diagonal entries of each row, every other entry +0.0.  A pair with a kept entry
    in either direction has the height fmax of its two directions (an absent one is +0.0); the other pairs of a node
    are +0.0 and are counted by arithmetic, not listed."""
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64)
    n = len(ids)
    if rank == 0:
        return np.full(n, np.inf)
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], ids.shape)
    kept = (ids >= 0) & (ids != rows)
    a, b, v = rows[kept], ids[kept].astype(np.int64), vals[kept]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.lexsort((hi, lo))
    lo, hi, v, forward = lo[order], hi[order], v[order], (a < b)[order]
    new = np.r_[True, (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])] if lo.size else np.zeros(0, dtype=bool)
    pair = np.cumsum(new) - 1
    n_pairs = int(new.sum())
    # per pair and direction the kept value (a list names a column once), +0.0 where absent; fmax passes a NaN over
    up, down = np.zeros(n_pairs), np.zeros(n_pairs)
    up[pair[forward]], down[pair[~forward]] = v[forward], v[~forward]
    w = np.fmax(up, down) + 0.0
    plo, phi = lo[new], hi[new]
    out = np.empty(n, dtype=np.float64)
    node = np.concatenate([plo, phi])
    height = np.concatenate([w, w])
    by_node = np.argsort(node, kind="stable")
    node, height = node[by_node], height[by_node]
    starts = np.searchsorted(node, np.arange(n + 1))
    for x in range(n):
        h = height[starts[x]:starts[x + 1]]
        exists = h[~np.isnan(h)]
        rest = (n - 1) - h.size                               # the pairs no list names: +0.0 each
        pos, neg = np.sort(exists[exists > 0])[::-1], np.sort(exists[exists < 0])[::-1]
        zeros = int((exists == 0).sum()) + rest
        if rank <= pos.size:
            out[x] = pos[rank - 1]
        elif rank <= pos.size + zeros:
            out[x] = 0.0
        elif rank <= pos.size + zeros + neg.size:
            out[x] = neg[rank - pos.size - zeros - 1]
        else:
            out[x] = -np.inf
    return out


def clamp_lists(ids, vals, core):
    """float64 [n, k]: every kept entry clamped by the core similarities of its two nodes (NaN stays NaN)."""
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64)
    col = core[np.where(ids >= 0, ids, 0)]
    return np.where(np.isnan(vals), np.nan, np.minimum(np.minimum(vals, core[:, None]), col))


# ---- a solver's side ---------------------------------------------------------------------------------------------------------
def core_similarity(solver, j, rank: int) -> np.ndarray:
    """float64 [n] of side j over the caller's ids."""
    lists = solver.lists(j)
    if lists is not None:
        return core_of_lists(lists[0], lists[1], rank)
    if solver.n[j] == 0:
        return np.empty(0, dtype=np.float64)
    with solver.one_block(j) as reader:
        return core_block(reader.ops, reader.blocks[0], reader.n, rank)


def table(solver, j, rank: int, floor):
    """(n, core float64 [n], left, right, similarity, size) of side j: ``_linkage.table`` of the mutual reachability."""
    lists = solver.lists(j)
    if lists is not None:
        ids, vals, _ = lists
        core = core_of_lists(ids, vals, rank)
        forest = _linkage.forest_of_lists(ids, clamp_lists(ids, vals, core), floor)
        return (len(ids), core) + _linkage.canonical(len(ids), *forest)
    if solver.n[j] == 0:
        return (0, np.empty(0, dtype=np.float64)) + _linkage.canonical(0, [], [], [])
    with solver.one_block(j) as reader:
        b = reader.blocks[0]
        core, a, c, value, _ = forest_blocks(reader.ops, b, [b], reader.n, rank, floor)
    return (reader.n, core) + _linkage.canonical(reader.n, a, c, value)


# ---- the condensed tree: host arithmetic on a table --------------------------------------------------------------------------
def classes_of_table(n: int, left, right, sim, size):
    """The multi-way hierarchy a canonical table encodes -> (height, members, children, parent) per class, lists indexed
    by class; a child is a leaf id below n or n + a class index.  Rows of one height that chain (c1, c2) -> x1,
    (x1, c3) -> x2 are ONE class with the children c1, c2, c3: in a canonical table the ``left`` of a row is the cluster
    the row before it formed exactly when the two rows belong to one merge."""
    height, members, children = [], [], []
    klass_of_row = {}                                        # the LAST row of a class -> the class
    for i in range(len(left)):
        lf, rt = int(left[i]), int(right[i])
        if i > 0 and lf == n + i - 1 and sim[i] == sim[i - 1]:
            k = klass_of_row.pop(i - 1)
            children[k].append(rt)
            members[k] = int(size[i])
        else:
            k = len(height)
            height.append(float(sim[i]))
            children.append([lf, rt])
            members.append(int(size[i]))
        klass_of_row[i] = k
    # children named by row -> named by class
    for k in range(len(children)):
        children[k] = [c if c < n else n + klass_of_row[c - n] for c in children[k]]
    parent = [-1] * len(height)
    for k, ch in enumerate(children):
        for c in ch:
            if c >= n:
                parent[c - n] = k
    return height, members, children, parent


def _exact_sum(terms):
    """The float64 nearest to the exact sum of count x difference over ``terms`` [(count, difference)]: what
    ``math.fsum`` gives over every node's own term, without listing them."""
    if not all(math.isfinite(d) for _, d in terms):
        return float(sum(k * d for k, d in terms))
    # a float64 is an integer over a power of two: the sum in integers over the largest of them, divided once (the
    # division of two Python ints rounds correctly)
    ratios = [(k,) + float(d).as_integer_ratio() for k, d in terms]
    over = max((den for _, _, den in ratios), default=1)
    return sum(k * num * (over // den) for k, num, den in ratios) / over


def condense(n: int, left, right, sim, size, min_cluster_size: int, selection="eom", allow_single_cluster=False):
    """HDBSCAN*'s condensed tree, stabilities and selection from a canonical table of n leaves, with the similarity as
    the density level -> (labels int64 [n], clusters): ``clusters`` a dict of equal-length arrays parent, birth, size,
    stability, selected, cluster, ordered by (smallest member ascending, size descending).  ``_kept.hdbscan`` says what
    each means."""
    mcs = int(min_cluster_size)
    height, members, children, parent = classes_of_table(n, left, right, sim, size)
    K = len(height)
    size_of = lambda c: 1 if c < n else members[c - n]

    # leaves of every class as a range of one order of the leaves, and every class' smallest member
    first, last, smallest = [0] * K, [0] * K, [0] * K
    order = []
    for root in (k for k in range(K) if parent[k] < 0):
        stack = [(n + root, False)]
        while stack:
            c, done = stack.pop()
            if c < n:
                order.append(c)
            elif done:
                k = c - n
                last[k] = len(order)
                smallest[k] = min(x if x < n else smallest[x - n] for x in children[k])
            else:
                first[c - n] = len(order)
                stack.append((c, True))
                stack.extend((x, False) for x in reversed(children[c - n]))
    order = np.array(order, dtype=np.int64)

    # the condensed tree, top-down
    c_parent, c_birth, c_class, c_terms, c_children = [], [], [], [], []

    def new_cluster(par, birth, klass):
        c_parent.append(par)
        c_birth.append(birth)
        c_class.append(klass)
        c_terms.append([])
        c_children.append([])
        if par >= 0:
            c_children[par].append(len(c_parent) - 1)
        return len(c_parent) - 1

    stack = [(k, new_cluster(-1, height[k], k)) for k in range(K) if parent[k] < 0 and members[k] >= mcs]
    while stack:
        k, c = stack.pop()
        h = height[k]
        big = [x for x in children[k] if size_of(x) >= mcs]
        gone = h - c_birth[c]                                # (one float64 subtraction: every leaving node's term)
        if len(big) >= 2:
            c_terms[c].append((members[k], gone))            # C ends: everybody still in it leaves at h
            stack.extend((x - n, new_cluster(c, h, x - n)) for x in big)
        elif len(big) == 1:
            c_terms[c].append((members[k] - size_of(big[0]), gone))
            stack.append((big[0] - n, c))
        else:
            c_terms[c].append((members[k], gone))
    C_ = len(c_parent)
    stability = [_exact_sum(t) for t in c_terms]

    # selection, bottom-up (a child cluster has a larger index than its parent)
    selected = [False] * C_
    if selection == "leaf":
        for c in range(C_):
            selected[c] = not c_children[c] and (c_parent[c] >= 0 or allow_single_cluster)
    else:
        score = [0.0] * C_
        for c in range(C_ - 1, -1, -1):
            may = c_parent[c] >= 0 or allow_single_cluster
            if not c_children[c]:
                selected[c], score[c] = True, stability[c]
                continue
            child_sum = math.fsum(score[x] for x in c_children[c])
            if stability[c] >= child_sum and may:
                selected[c], score[c] = True, stability[c]
                todo = list(c_children[c])
                while todo:
                    x = todo.pop()
                    selected[x] = False
                    todo.extend(c_children[x])
            else:
                score[c] = child_sum

    # the table of clusters in its order, and the labels
    c_small = [smallest[k] for k in c_class]
    c_size = [members[k] for k in c_class]
    rows = sorted(range(C_), key=lambda c: (c_small[c], -c_size[c]))
    row_of = {c: r for r, c in enumerate(rows)}
    labels = np.full(n, -1, dtype=np.int64)
    chosen = sorted((c for c in range(C_) if selected[c]), key=lambda c: c_small[c])
    number = {c: i for i, c in enumerate(chosen)}
    for c in chosen:
        labels[order[first[c_class[c]]:last[c_class[c]]]] = number[c]
    clusters = {
        "parent": np.array([row_of.get(c_parent[c], -1) for c in rows], dtype=np.int64),
        "birth": np.array([c_birth[c] for c in rows], dtype=np.float64),
        "size": np.array([c_size[c] for c in rows], dtype=np.int64),
        "stability": np.array([stability[c] for c in rows], dtype=np.float64),
        "selected": np.array([selected[c] for c in rows], dtype=bool),
        "cluster": np.array([number.get(c, -1) for c in rows], dtype=np.int64),
    }
    return labels, clusters
