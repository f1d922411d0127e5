"""ctypes binding of libsimrank_groups.so (include/simrank_groups.h): a clustering of a kept model scored on the device.

``cluster_quality(labels)`` answers "which clusters are tight, which node stands for each, which nodes sit between two?"
for any labelling of the fitted nodes: per node the mean similarity to the other members of its own cluster, the best
mean similarity to another cluster and that cluster.  One sweep of the iterate in place (the block a solver's
``_query.Reader`` describes, in solver order with its column map); three numbers per node cross PCIe, or with
``cluster_means`` the N x K means.  A side held in several column blocks (``LocalWorld(P)``) is first packed into one
temporary block (the solver's ``one_block`` scope), as ``_neighbors.prune`` does.  A pruned model (a solver with
``lists``) is answered on the host from its lists, for its matrix P.  No CPU fallback for the matrices: a missing library
or device is an error.

The definitions (include/simrank_groups.h states them for a block; here for a model).  For node a and cluster g,
``M_g(a) = {b : labels[b] = g, b != a}``; ``sum(a, g)`` is the float64 sum of ``S[a, b]`` over it (row a: the element
``similarity(a, b)`` reads), ``mean(a, g) = sum / |M_g(a)|`` and NaN when the set is empty; ``own = mean(a, labels[a])``;
``other`` is the first ``mean(a, g)``, g != labels[a], in the order (mean descending, cluster value ascending), a NaN
mean never chosen, and ``nearest`` that cluster (no candidate: ``labels[a]`` and NaN).  The rest is host arithmetic,
written down at ``silhouette``, ``medoid_positions`` and ``summary``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._checks import is_int
from ._companion import PANEL_F16, PANEL_F32, ROWMAJOR_F32, ROWMAJOR_F64, Companion  # noqa: F401 (a block's layouts)
from ._driver import Scratch, stage

VERSION = 1              # SIMRANK_GROUPS_VERSION of include/simrank_groups.h
LANE_MAX = 8             # SIMRANK_GROUPS_LANE_MAX: a list this long or shorter is summed by one lane
WAVE_MAX = 1023          # SIMRANK_GROUPS_WAVE_MAX: a longer one up to here by one wave, beyond by the workgroup

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_groups_version": [],
    "simrank_groups_last_error": [],
    "simrank_groups_means": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _vp],
}
_RESTYPES = {"simrank_groups_last_error": C.c_char_p}


class GroupsError(RuntimeError):
    """A call into libsimrank_groups.so failed."""


_c = Companion("groups", VERSION, PROTOTYPES, _RESTYPES, GroupsError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- argument checks: nothing touches a device ---------------------------------------------------------------------------
def _integers(values) -> np.ndarray:
    """A 1-D array of cluster values -> int64; ValueError for anything but integers (bool, float, NaN, None, str)."""
    a = np.asarray(values)
    if a.ndim != 1:
        raise ValueError(f"labels must be one-dimensional, not of shape {a.shape}")
    if a.dtype == object:
        for x in a:
            if not is_int(x):
                raise ValueError(f"a cluster label must be an integer, not {x!r}")
        try:
            return np.array([int(x) for x in a], dtype=np.int64)
        except OverflowError:
            raise ValueError("a cluster label does not fit 64 bits") from None
    if a.dtype.kind not in "iu":
        raise ValueError(f"cluster labels must be integers, not {a.dtype} (bool, floats, NaN and None are refused)")
    if a.dtype.kind == "u" and a.size and int(a.max()) > np.iinfo(np.int64).max:
        raise ValueError("a cluster label does not fit 64 bits")
    return a.astype(np.int64)


def check_labels(labels, index) -> np.ndarray:
    """The ``labels`` argument of ``cluster_quality`` & co -> int64 [N], the cluster of every node in the order of
    ``index`` (a pandas Index: the dense frame's labels).  A pandas Series indexed by the fitted labels, in any order,
    holding every node exactly once (KeyError for an unknown node; ValueError for a repeated or a missing one), or a 1-D
    sequence of length N in the frame's order.  Values: integers of any sign."""
    import pandas as pd
    n = len(index)
    if isinstance(labels, pd.DataFrame) or isinstance(labels, (str, bytes, dict)) or labels is None:
        raise ValueError("labels must be a pandas Series indexed by the fitted labels or a 1-D sequence of integers, not "
                         f"{type(labels).__name__}")
    if isinstance(labels, pd.Series):
        given = labels.index
        at = index.get_indexer(pd.Index(list(given), dtype=object) if index.dtype == object else given) if len(given) else \
            np.empty(0, dtype=np.int64)
        if (at < 0).any():
            raise KeyError(given[int(np.argmax(at < 0))])
        if np.unique(at).size != at.size:
            raise ValueError("labels names a node more than once: every fitted node must appear exactly once")
        if at.size != n:
            raise ValueError(f"labels holds {at.size} of the {n} fitted nodes: every fitted node must appear exactly once")
        values = _integers(labels.to_numpy())
        out = np.empty(n, dtype=np.int64)
        out[at] = values
        return out
    if not hasattr(labels, "__len__") and not hasattr(labels, "__iter__"):
        raise ValueError(f"labels must be a pandas Series or a 1-D sequence of integers, not {labels!r}")
    # (a list is judged element by element: NumPy would turn [0, 1, True] into integers)
    values = _integers(labels if isinstance(labels, np.ndarray) else np.array(list(labels) + [None], dtype=object)[:-1])
    if values.size != n:
        raise ValueError(f"labels has {values.size} entries for {n} fitted nodes")
    return values


def check_max_bytes(max_bytes) -> int:
    if not is_int(max_bytes) or max_bytes < 1:
        raise ValueError(f"max_bytes must be a positive integer, not {max_bytes!r}")
    return int(max_bytes)


def check_means_bytes(n: int, k: int, max_bytes: int):
    if n * k * 8 > max_bytes:
        raise ValueError(f"cluster_means of {n} nodes and {k} clusters is {n * k * 8} bytes, above max_bytes = {max_bytes}: "
                         "raise max_bytes, or read own / other / nearest from cluster_quality")


def groups_of(lab):
    """int64 [N] cluster values -> (clusters int64 [K] ascending, gidx int64 [N]: the cluster's rank, sizes int64 [K])."""
    clusters, gidx = np.unique(lab, return_inverse=True)
    gidx = gidx.reshape(-1).astype(np.int64)
    return clusters.astype(np.int64), gidx, np.bincount(gidx, minlength=clusters.size).astype(np.int64)


# ---- the device path -----------------------------------------------------------------------------------------------------
def means_block(ops, block, row_group, row_col, col_pos, group_ptr, want_means=False, timing=None):
    """One ``simrank_groups_means`` on ``block`` (a dict with ptr, layout, stride, rows, cols): host arrays in, (own
    float64 [rows], other float64 [rows], nearest int32 [rows], means float64 [rows, K] or None) out, in block row order.
    ``timing``: a list that receives the kernel's milliseconds (HIP events)."""
    rows, k = int(block["rows"]), int(group_ptr.size - 1)
    lib = load()
    own, other, nearest = np.empty(rows, dtype=np.float64), np.empty(rows, dtype=np.float64), np.empty(rows, dtype=np.int32)
    means = np.empty((rows, k), dtype=np.float64) if want_means else None
    with Scratch(ops) as scratch:
        rg, rc = scratch.put(row_group.astype(np.int32)), scratch.put(row_col.astype(np.int32))
        cp = scratch.put(col_pos.astype(np.int32)) if col_pos.size else scratch.malloc(16)
        gp = scratch.put(group_ptr.astype(np.int64))
        own_dev, other_dev, near_dev = scratch.malloc(8 * rows), scratch.malloc(8 * rows), scratch.malloc(4 * rows)
        means_dev = scratch.malloc(8 * rows * k) if want_means else None
        stage(ops, timing, "means_ms", lambda: check(lib.simrank_groups_means(
            block["ptr"], block["layout"], block["stride"], rows, block["cols"], rg, rc, cp, gp, k, own_dev, other_dev,
            near_dev, means_dev, k, ops.stream), "simrank_groups_means"))
        ops.d2h(own, own_dev)
        ops.d2h(other, other_dev)
        ops.d2h(nearest, near_dev)
        if want_means:
            ops.d2h(means, means_dev)
        ops.synchronize()
    return own, other, nearest, means


def compose(reader, gidx, sizes):
    """The arrays ``simrank_groups_means`` takes for a reader's one block: the nodes sorted by cluster (stable: a
    cluster's members in the frame's order) and mapped to block positions through the reader's ``inv``; block row r holds
    the node ``order[r]``, whose own column is r."""
    n = reader.n
    members = np.argsort(gidx, kind="stable")                 # caller ids, cluster-major
    col_pos = reader.inv[members].astype(np.int32)
    group_ptr = np.zeros(sizes.size + 1, dtype=np.int64)
    np.cumsum(sizes, out=group_ptr[1:])
    row_group = gidx[reader.order].astype(np.int32)
    row_col = np.arange(n, dtype=np.int32)
    return row_group, row_col, col_pos, group_ptr


def scores_reader(reader, gidx, sizes, want_means=False, timing=None):
    """(own, other, nearest rank or -1, means or None) in the caller's order, of a reader whose one block holds every
    column."""
    (b,) = reader.blocks
    own_p, other_p, near_p, means_p = means_block(reader.ops, b, *compose(reader, gidx, sizes), want_means, timing)
    n = reader.n
    own, other, nearest = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64), np.empty(n, dtype=np.int64)
    own[reader.order], other[reader.order], nearest[reader.order] = own_p, other_p, near_p
    means = None
    if want_means:
        means = np.empty_like(means_p)
        means[reader.order] = means_p
    return own, other, nearest, means


# ---- the host path of a pruned model ---------------------------------------------------------------------------------------
def scores_of_lists(ids, vals, gidx, sizes, want_means=False):
    """The same four for the matrix P of a pruned model: ``ids`` int [n, k] (-1: an empty slot), ``vals`` float64 [n, k]
    the kept off-diagonal entries of each row; every other off-diagonal entry is +0.0: it counts in ``|M_g(a)|`` and adds
    nothing, so a cluster none of whose members a node keeps has the mean +0.0.  A node's kept entries are added per
    cluster in list order."""
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64)
    n, k_groups = ids.shape[0], int(sizes.size)
    own, other = np.full(n, np.nan), np.full(n, np.nan)
    nearest = np.full(n, -1, dtype=np.int64)
    means = None
    if want_means:
        means = np.zeros((n, k_groups), dtype=np.float64)
    for a in range(n):
        mine = int(gidx[a])
        keep = (ids[a] >= 0) & (ids[a] != a)
        g = gidx[ids[a][keep]]
        seen, slot = np.unique(g, return_inverse=True)
        sums = np.bincount(slot.reshape(-1), weights=vals[a][keep], minlength=seen.size) + 0.0
        counts = sizes[seen] - (seen == mine)
        kept_means = sums / counts                           # (a kept entry is a member: its count is at least 1)
        if want_means:
            means[a, seen] = kept_means
            if sizes[mine] == 1:
                means[a, mine] = np.nan
        hit = np.flatnonzero(seen == mine)
        if hit.size:
            own[a] = kept_means[hit[0]]
        elif sizes[mine] > 1:
            own[a] = 0.0
        # the candidates: the kept clusters but the node's own, and the first cluster with no kept entry (mean +0.0)
        best_v, best_g = 0.0, -1
        taken = set(seen.tolist()) | {mine}
        for absent in range(len(taken) + 1):
            if absent not in taken:
                if absent < k_groups:
                    best_v, best_g = 0.0, absent
                break
        for v, gg in zip(kept_means.tolist(), seen.tolist()):
            if gg != mine and not math.isnan(v) and (best_g < 0 or v > best_v or (v == best_v and gg < best_g)):
                best_v, best_g = v, gg
        if best_g >= 0:
            other[a], nearest[a] = best_v, best_g
    return own, other, nearest, means


# ---- a solver's side ---------------------------------------------------------------------------------------------------------
def scores(solver, j, gidx, sizes, want_means=False):
    """(own, other, nearest rank or -1, means or None) of side j, in the caller's order."""
    lists = solver.lists(j)
    if lists is not None:
        return scores_of_lists(lists[0], lists[1], gidx, sizes, want_means)
    with solver.one_block(j) as reader:
        return scores_reader(reader, gidx, sizes, want_means)


# ---- host arithmetic on the three numbers ------------------------------------------------------------------------------------
def silhouette(own, other, own_size) -> np.ndarray:
    """float64 [N], checked in this order: 0.0 for a singleton; NaN if ``own`` or ``other`` is NaN; otherwise
    ``(own - other) / max(own, other)`` when that maximum is > 0, else 0.0."""
    own, other = np.asarray(own, dtype=np.float64), np.asarray(other, dtype=np.float64)
    out = np.zeros(own.size, dtype=np.float64)
    for i in range(own.size):
        if own_size[i] == 1:
            out[i] = 0.0
        elif math.isnan(own[i]) or math.isnan(other[i]):
            out[i] = np.nan
        else:
            top = max(own[i], other[i])
            out[i] = (own[i] - other[i]) / top if top > 0 else 0.0
    return out


def medoid_positions(gidx, n_groups, own) -> np.ndarray:
    """int64 [K]: per cluster the position of the member with the largest ``own``; ties go to the first member in the
    frame's order, NaN is skipped; every member NaN: the first member."""
    best = np.full(n_groups, -1, dtype=np.int64)
    first = np.full(n_groups, -1, dtype=np.int64)
    for i, g in enumerate(np.asarray(gidx).tolist()):
        if first[g] < 0:
            first[g] = i
        if not math.isnan(own[i]) and (best[g] < 0 or own[i] > own[best[g]]):
            best[g] = i
    return np.where(best >= 0, best, first)


def summary(gidx, n_groups, own, other, sil):
    """(cohesion, separation, silhouette) float64 [K]: ``math.fsum`` of the members' ``own``, ``other`` and silhouette over
    the cluster's size; NaN propagates."""
    members = [[] for _ in range(n_groups)]
    for i, g in enumerate(np.asarray(gidx).tolist()):
        members[g].append(i)
    mean = lambda x, m: math.fsum(x[i] for i in m) / len(m)
    return tuple(np.array([mean(x, m) for m in members], dtype=np.float64) for x in (own, other, sil))
