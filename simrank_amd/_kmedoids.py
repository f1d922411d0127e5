"""ctypes binding of libsimrank_kmedoids.so (include/simrank_kmedoids.h): clusters around medoids on a kept model.

``assign(seeds)`` gives every fitted node to the seed whose row likes it best; ``kmedoids(seeds)`` alternates that
assignment with the move of every cluster's medoid to the member with the largest ``own`` of ``cluster_quality``, until
no medoid moves.  Both steps read the iterate in place (the block a solver's ``_query.Reader`` describes): the assignment
is K medoid rows against all N columns (``simrank_kmedoids_assign``), the update is the sweep of ``_groups``
(``simrank_groups_means``, the same call with the same lists: the same bits as ``cluster_quality``) followed by
``simrank_kmedoids_pick``.  Per iteration N int32 labels come to the host, which regroups them as ``_groups.compose`` does
and sends the lists back, and two 4-byte counters come down; ``own``, the medoid rows and the per-node values stay on the
device.  A side held in several column blocks (``LocalWorld(P)``) is packed into one temporary block once per call
(the solver's ``one_block`` scope).  A pruned model (a solver with ``lists``) is answered on the host from its lists, for
its matrix P.  No CPU fallback for the matrices: a missing library or device is an error.

The definitions (include/simrank_kmedoids.h states them for a block; here for a model).  ``v(j, a) = S[m_j, a]``: row
m_j, the element ``similarity(m_j, a)`` reads, compared in float64; candidates in the order (v descending, j ascending),
a NaN never chosen, -0.0 equal to +0.0.  With strict-improvement rules on both steps every change raises
``F = sum over the non-medoids a of S[m(a), a]`` in exact arithmetic, so no configuration repeats.
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np

from . import _groups
from ._checks import is_int
from ._companion import Companion
from ._driver import Scratch, stage

VERSION = 1              # SIMRANK_KMEDOIDS_VERSION of include/simrank_kmedoids.h
CHUNK = 1024             # SIMRANK_KMEDOIDS_CHUNK: block columns of one workgroup of the assignment
HISTORY_ROWS = 32        # iterations whose cohesions wait on the device for one copy

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_kmedoids_version": [],
    "simrank_kmedoids_last_error": [],
    "simrank_kmedoids_assign": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp],
    "simrank_kmedoids_pick": [_vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp],
}
_RESTYPES = {"simrank_kmedoids_last_error": C.c_char_p}


class KMedoidsError(RuntimeError):
    """A call into libsimrank_kmedoids.so failed."""


_c = Companion("kmedoids", VERSION, PROTOTYPES, _RESTYPES, KMedoidsError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- argument checks: nothing touches a device ---------------------------------------------------------------------------
def check_seeds(seeds, index) -> np.ndarray:
    """The ``seeds`` argument of ``assign`` and ``kmedoids`` -> int64 [K], K >= 1: the positions in ``index`` (a pandas
    Index: the dense frame's labels) of distinct fitted labels, in the order given.  A sequence of labels; of a pandas
    Series (``medoids(labels)``) the values are taken.  ValueError for anything that is no sequence, an empty one and a
    repeated label; KeyError for an unknown label."""
    import pandas as pd
    if isinstance(seeds, pd.Series):
        seeds = seeds.tolist()
    if isinstance(seeds, (str, bytes, dict, set, frozenset, pd.DataFrame)) or not hasattr(seeds, "__len__") or not hasattr(seeds, "__iter__"):
        raise ValueError(f"seeds must be a sequence of fitted labels or a pandas Series of them, not {type(seeds).__name__}")
    if getattr(seeds, "ndim", 1) != 1:
        raise ValueError(f"seeds must be one-dimensional, not of shape {seeds.shape}")
    seeds = list(seeds)
    if not seeds:
        raise ValueError("seeds is empty: at least one medoid is needed")
    try:
        at = index.get_indexer(pd.Index(seeds, dtype=object) if index.dtype == object else pd.Index(seeds))
    except TypeError:
        raise ValueError("seeds must hold labels (hashable values)") from None
    if (at < 0).any():
        raise KeyError(seeds[int(np.argmax(at < 0))])
    if np.unique(at).size != at.size:
        raise ValueError("seeds repeats a label: the medoids must be distinct nodes")
    return at.astype(np.int64)


def check_max_iter(max_iter) -> int:
    if not is_int(max_iter) or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, not {max_iter!r}")
    return int(max_iter)


def objective(cohesion, sizes) -> float:
    """``math.fsum(cohesion_j * (size_j - 1))`` over the clusters of two members or more."""
    return math.fsum(float(c) * (int(s) - 1) for c, s in zip(cohesion, sizes) if s > 1)


# ---- the device path -----------------------------------------------------------------------------------------------------
def _clock(timing, name, t0):
    if timing is not None:
        timing[name] = timing.get(name, 0.0) + (time.perf_counter() - t0) * 1e3


def _assign(lib, ops, b, med, k, current, cluster, value, moved, timing):
    """Queue one assignment.  ``med`` serves as med_row and med_col: in a one-block reader a node's row is its column."""
    stage(ops, timing, "assign_ms", lambda: check(lib.simrank_kmedoids_assign(
        b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], med, med, k, current, cluster, value, moved, ops.stream),
        "simrank_kmedoids_assign"))


def assign_reader(reader, seeds, timing=None):
    """(cluster int64 [N], value float64 [N]) in the caller's order: the first assignment to the seeds (caller ids)."""
    (b,), ops, n, k = reader.blocks, reader.ops, reader.n, int(seeds.size)
    lab, val = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64)
    with Scratch(ops) as scratch:
        med = scratch.put(reader.inv[seeds].astype(np.int32))
        lab_dev, val_dev = scratch.malloc(4 * n), scratch.malloc(8 * n)
        _assign(load(), ops, b, med, k, None, lab_dev, val_dev, None, timing)
        ops.d2h(lab, lab_dev)
        ops.d2h(val, val_dev)
        ops.synchronize()
    return lab[reader.inv].astype(np.int64), val[reader.inv]


def loop_reader(reader, seeds, max_iter, timing=None):
    """The alternation on a reader whose one block holds every column -> (cluster int64 [N] in the caller's order, medoids
    int64 [K] caller ids, value float64 [N] or None, sizes int64 [K], cohesion float64 [K], history [(moved, changed,
    objective)]).  ``value`` is what the last assignment read; None when the medoids moved after it (``max_iter`` ran
    out).  ``timing``: a dict that receives the milliseconds of the stages, added up over the iterations (HIP events for
    the kernels, which serialises them; the host clock for the regroup and its copies)."""
    (b,), ops, n, k = reader.blocks, reader.ops, reader.n, int(seeds.size)
    lib, groups = load(), _groups.load()
    hist_rows = min(max_iter, HISTORY_ROWS)
    zero, got = np.zeros(2, dtype=np.uint32), np.empty(2, dtype=np.uint32)
    lab, val, med_host = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64), np.empty(k, dtype=np.int32)
    coh_host = np.empty((hist_rows, k), dtype=np.float64)
    group_ptr = np.zeros(k + 1, dtype=np.int64)
    steps, cohesions = [], []
    with Scratch(ops) as scratch:
        med = scratch.put(reader.inv[seeds].astype(np.int32))
        labs = [scratch.malloc(4 * n), scratch.malloc(4 * n)]
        val_dev, own, other, near = scratch.malloc(8 * n), scratch.malloc(8 * n), scratch.malloc(8 * n), scratch.malloc(4 * n)
        row_col = scratch.put(np.arange(n, dtype=np.int32))
        col_pos, ptr_dev = scratch.malloc(4 * n), scratch.malloc(8 * (k + 1))
        coh, counters = scratch.malloc(8 * k * hist_rows), scratch.malloc(8)
        for i in range(max_iter):
            current, new = (None if i == 0 else labs[(i - 1) % 2]), labs[i % 2]
            ops.h2d(counters, zero)
            _assign(lib, ops, b, med, k, current, new, val_dev, counters, timing)
            t0 = time.perf_counter()
            ops.d2h(lab, new)
            ops.synchronize()
            _clock(timing, "labels_d2h_ms", t0)
            # the regroup of _groups.compose: a cluster's members in the frame's order, as block positions.  The labels
            # are in block order, which is what the sweep takes as row_group: they never go back
            t0 = time.perf_counter()
            gidx = lab[reader.inv]
            sizes = np.bincount(gidx, minlength=k).astype(np.int64)
            assert sizes.size == k and sizes.min() >= 1               # (a medoid stays in its cluster)
            members = np.ascontiguousarray(reader.inv[np.argsort(gidx, kind="stable")], dtype=np.int32)
            np.cumsum(sizes, out=group_ptr[1:])
            _clock(timing, "regroup_ms", t0)
            t0 = time.perf_counter()
            ops.h2d(col_pos, members)
            ops.h2d(ptr_dev, group_ptr)
            if timing is not None:
                ops.synchronize()
            _clock(timing, "lists_h2d_ms", t0)
            stage(ops, timing, "means_ms", lambda: _groups.check(groups.simrank_groups_means(
                b["ptr"], b["layout"], b["stride"], n, n, new, row_col, col_pos, ptr_dev, k, own, other, near, None, 0,
                ops.stream), "simrank_groups_means"))
            slot = i % hist_rows
            stage(ops, timing, "pick_ms", lambda: check(lib.simrank_kmedoids_pick(
                own, n, col_pos, ptr_dev, k, med, coh + 8 * k * slot, counters + 4, ops.stream), "simrank_kmedoids_pick"))
            ops.d2h(got, counters)
            ops.synchronize()
            steps.append((int(got[0]), int(got[1]), sizes))
            done = got[1] == 0 or i + 1 == max_iter
            if done or slot + 1 == hist_rows:
                ops.d2h(coh_host, coh)
                ops.synchronize()
                cohesions.extend(coh_host[:slot + 1].copy())
            if done:
                break
        ops.d2h(med_host, med)
        ops.d2h(val, val_dev)
        ops.synchronize()
    moved_last, changed_last, sizes = steps[-1]
    history = [(m, c, objective(co, s)) for (m, c, s), co in zip(steps, cohesions)]
    cluster = lab[reader.inv].astype(np.int64)
    return (cluster, reader.order[med_host].astype(np.int64), val[reader.inv] if changed_last == 0 else None, sizes,
            cohesions[-1], history)


# ---- the host path of a pruned model ---------------------------------------------------------------------------------------
def rows_of_lists(ids, vals, diag, medoids) -> np.ndarray:
    """float64 [K, n]: the medoids' rows of the matrix P of a pruned model: a row's kept entries, its stored diagonal
    element, +0.0 everywhere else."""
    V = np.zeros((len(medoids), ids.shape[0]), dtype=np.float64)
    for j, m in enumerate(np.asarray(medoids).tolist()):
        kept = ids[m] >= 0
        V[j, ids[m][kept]] = vals[m][kept]
        V[j, m] = diag[m]
    return V


def _first_best(W, candidate):
    """Per column of W [K, n] the first row in the order (value descending, row ascending) among the candidates, and
    whether there is one."""
    best = np.argmax(np.where(candidate, W, -np.inf), axis=0)
    cols = np.arange(W.shape[1])
    best = np.where(candidate[best, cols], best, np.argmax(candidate, axis=0))     # (a best of -inf: the first candidate)
    return best, candidate.any(axis=0)


def assign_rows(V, medoids, current=None):
    """The assignment of include/simrank_kmedoids.h on the medoids' rows ``V`` [K, n] (row j: medoid j, the node
    ``medoids[j]``) -> (cluster int64 [n], value float64 [n], moved)."""
    k, n = V.shape
    cols = np.arange(n)
    best, any_ = _first_best(V, ~np.isnan(V))
    best_v = V[best, cols]
    if current is None:
        cluster, value = np.where(any_, best, 0), np.where(any_, best_v, np.nan)
    else:
        cur_v = V[current, cols]
        with np.errstate(invalid="ignore"):
            move = any_ & ((best_v > cur_v) | np.isnan(cur_v))
        cluster, value = np.where(move, best, current), np.where(move, best_v, cur_v)
    cluster = cluster.astype(np.int64)
    medoids = np.asarray(medoids, dtype=np.int64)
    cluster[medoids], value[medoids] = np.arange(k), V[np.arange(k), medoids]
    return cluster, value, n if current is None else int((cluster != current).sum())


def pick_members(own, cluster, medoids):
    """The update of include/simrank_kmedoids.h with every cluster's members in ascending order -> (medoids int64 [K],
    cohesion float64 [K], changed)."""
    medoids = np.array(medoids, dtype=np.int64)
    k = medoids.size
    members = np.argsort(cluster, kind="stable")
    ends = np.cumsum(np.bincount(cluster, minlength=k))
    cohesion, changed = np.full(k, np.nan), 0
    for j in range(k):
        m = members[ends[j - 1] if j else 0:ends[j]]
        if not m.size:
            continue
        o = own[m]
        candidate = ~np.isnan(o)
        mine = own[medoids[j]]
        cohesion[j] = mine
        if candidate.any():
            at = int(np.argmax(np.where(candidate, o, -np.inf)))
            if not candidate[at]:
                at = int(np.argmax(candidate))
            if o[at] > mine or math.isnan(mine):
                medoids[j], cohesion[j], changed = m[at], o[at], changed + 1
    return medoids, cohesion, changed


def loop_lists(ids, vals, diag, seeds, max_iter):
    """``loop_reader`` for the matrix P of a pruned model, on the host."""
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64)
    medoids, k = np.array(seeds, dtype=np.int64), int(seeds.size)
    cluster, history = None, []
    for _ in range(max_iter):
        cluster, value, moved = assign_rows(rows_of_lists(ids, vals, diag, medoids), medoids, cluster)
        sizes = np.bincount(cluster, minlength=k).astype(np.int64)
        own = _groups.scores_of_lists(ids, vals, cluster, sizes)[0]
        medoids, cohesion, changed = pick_members(own, cluster, medoids)
        history.append((moved, changed, objective(cohesion, sizes)))
        if changed == 0:
            break
    return cluster, medoids, value if history[-1][1] == 0 else None, sizes, cohesion, history


# ---- a solver's side ---------------------------------------------------------------------------------------------------------
def assign(solver, j, seeds):
    """(cluster int64 [N], value float64 [N]) of side j, in the caller's order."""
    lists = solver.lists(j)
    if lists is not None:
        return assign_rows(rows_of_lists(*lists, seeds), seeds)[:2]
    with solver.one_block(j) as reader:
        return assign_reader(reader, seeds)


def kmedoids(solver, j, seeds, max_iter):
    """(cluster, medoids, value, sizes, cohesion, history) of side j as ``loop_reader`` returns them, ``value`` read again
    for the final medoids where the loop left it open."""
    lists = solver.lists(j)
    if lists is not None:
        out = loop_lists(*lists, seeds, max_iter)
        if out[2] is None:
            V = rows_of_lists(*lists, out[1])
            out = out[:2] + (V[out[0], np.arange(V.shape[1])],) + out[3:]
        return out
    with solver.one_block(j) as reader:
        out = loop_reader(reader, seeds, max_iter)
        if out[2] is None:                                   # max_iter ran out: every node's element of its final medoid's row
            out = out[:2] + (reader.pair_values(out[1][out[0]], np.arange(reader.n)),) + out[3:]
        return out
