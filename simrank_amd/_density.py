"""ctypes binding of libsimrank_density.so (include/simrank_density.h): density clusters (DBSCAN) of a kept model, found on
the device.

Two different nodes a, b are neighbours at t iff ``S[a, b] >= t`` or ``S[b, a] >= t``: the relation of ``components``,
``pairs`` and ``count_pairs``.  ``degrees(t)`` counts every node's neighbours, for up to ``MAX_LEVELS`` thresholds in one
sweep that reads every element once; ``dbscan(t, min_samples)`` grows clusters through the core nodes (those with
``neighbors + 1 >= min_samples``), hands every border node to its first core neighbour and leaves the rest as noise.  The
sweeps read the one square block of a side in place (``SolverQueries.one_block``: a side held in several column blocks
is packed first); 4 N bytes per level, or 8 N for ``dbscan``, cross PCIe.  A pruned model (a solver with ``lists``) is
answered on the host from its lists, for its matrix P, at t > 0.  No CPU fallback for the matrices: a missing library or
device is an error.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._checks import is_int
from ._cluster import check_thresholds, roots_of_edges
from ._companion import PANEL_F16, PANEL_F32, ROWMAJOR_F32, ROWMAJOR_F64, Companion  # noqa: F401 (a block's layouts)
from ._driver import Scratch, stage
from ._profile import edges_f32

VERSION = 1              # SIMRANK_DENSITY_VERSION of include/simrank_density.h
MAX_LEVELS = 8           # SIMRANK_DENSITY_MAX_LEVELS: thresholds of one degrees sweep
TILE = 64                # SIMRANK_DENSITY_TILE
NONE = 0x7fffffff        # SIMRANK_DENSITY_NONE: attach[x] of a node no core node has claimed
BAD_PARENT, CAP_REACHED = 1, 2      # bits of the device status word

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_density_version": [],
    "simrank_density_last_error": [],
    "simrank_density_init": [_vp, _vp, _vp, _i64, _i32, _vp, _vp],
    "simrank_density_degrees": [_vp, _i32, _i64, _i64, _vp, _vp, _i32, _vp, _vp],
    "simrank_density_union": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _vp, _vp],
    "simrank_density_labels": [_vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp],
}
_RESTYPES = {"simrank_density_last_error": C.c_char_p}


class DensityError(RuntimeError):
    """A call into libsimrank_density.so failed, or its kernels reported a forest out of order."""


_c = Companion("density", VERSION, PROTOTYPES, _RESTYPES, DensityError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- argument checks: nothing touches a device ---------------------------------------------------------------------------
def check_min_samples(min_samples) -> int:
    """``dbscan(t, min_samples)``: an int >= 1 -> the number of OTHER nodes a core node needs (the node counts itself),
    capped at what an int32 holds.  ValueError otherwise."""
    if not is_int(min_samples) or min_samples < 1:
        raise ValueError(f"min_samples must be an int >= 1, not {min_samples!r}")
    return int(min(int(min_samples) - 1, 2 ** 31 - 1))


def check_solver(solver, ts):
    """What ``degrees`` and ``dbscan`` refuse of a model before any work: a pruned model at a threshold <= 0."""
    if getattr(solver, "kept_k", None) is not None and not (np.asarray(ts) > 0).all():
        raise ValueError("degrees and dbscan of a pruned model need a threshold t > 0: the entries a pruned model does not "
                         "keep are +0.0 and would make every node every node's neighbour")


# ---- the device path -----------------------------------------------------------------------------------------------------
def _edges(layout, ts) -> np.ndarray:
    ts = np.asarray(ts, dtype=np.float64)
    return np.ascontiguousarray(ts if layout == ROWMAJOR_F64 else edges_f32(ts))


def _square(b, n):
    assert b["rows"] == n and b["cols"] == n and b.get("col_lo", 0) == 0, "the degrees sweep takes one square block"
    return b["ptr"], b["layout"], b["stride"]


def degrees_block(ops, b, n: int, ts, timing=None) -> np.ndarray:
    """int32 [len(ts), n]: per threshold every node's number of neighbours in the square block ``b`` (a dict with ptr,
    layout, stride, rows = cols = n and optional device row_ids naming ids 0 .. n - 1 for its positions).  ``timing``: a
    list or dict that receives the milliseconds of the sweep (HIP events)."""
    ts = np.asarray(ts, dtype=np.float64)
    m = int(ts.size)
    assert 1 <= m <= MAX_LEVELS and n >= 1
    S, layout, stride = _square(b, n)
    lib = load()
    got = np.empty(m * n + 1, dtype=np.int32)                # the counts, then the status word
    with Scratch(ops) as scratch:
        edges_dev = scratch.put(_edges(layout, ts))
        deg = scratch.malloc(4 * (m * n + 1))
        status = deg + 4 * m * n
        check(lib.simrank_density_init(deg, None, None, n, m, status, ops.stream), "simrank_density_init")
        stage(ops, timing, "degrees_ms", lambda: check(lib.simrank_density_degrees(
            S, layout, stride, n, b.get("row_ids"), edges_dev, m, deg, ops.stream), "simrank_density_degrees"))
        ops.d2h(got, deg)
        ops.synchronize()
    return got[:-1].reshape(m, n)


def dbscan_blocks(ops, b, blocks, n: int, t: float, min_neighbors: int, timing=None):
    """(neighbours int32 [n], labels int32 [n]): the counts of the square block ``b``, then one
    ``simrank_density_union`` per block of ``blocks`` (the same block, or column blocks of the same matrix) into one
    forest; a label is the smallest core node of the node's cluster, or -1 for noise.  DensityError when the device
    status word is not 0."""
    assert n >= 1 and 0 <= min_neighbors < 2 ** 31
    S, layout, stride = _square(b, n)
    lib = load()
    got = np.empty(2 * n + 1, dtype=np.int32)                # the counts, the labels, then the status word
    with Scratch(ops) as scratch:
        edge_dev = scratch.put(_edges(layout, [t]))
        out, parent, attach = scratch.malloc(4 * (2 * n + 1)), scratch.malloc(4 * n), scratch.malloc(4 * n)
        deg, labels, status = out, out + 4 * n, out + 8 * n
        check(lib.simrank_density_init(deg, parent, attach, n, 1, status, ops.stream), "simrank_density_init")
        stage(ops, timing, "degrees_ms", lambda: check(lib.simrank_density_degrees(
            S, layout, stride, n, b.get("row_ids"), edge_dev, 1, deg, ops.stream), "simrank_density_degrees"))
        for u in blocks:
            stage(ops, timing, "union_ms", lambda: check(lib.simrank_density_union(
                u["ptr"], u["layout"], u["stride"], u["rows"], u["cols"], u.get("row_ids"), u.get("col_ids"), edge_dev, deg,
                min_neighbors, parent, attach, n, status, ops.stream), "simrank_density_union"))
        stage(ops, timing, "labels_ms", lambda: check(lib.simrank_density_labels(
            parent, attach, deg, min_neighbors, n, labels, status, ops.stream), "simrank_density_labels"))
        ops.d2h(got, out)
        ops.synchronize()
    if got[-1] != 0:
        raise DensityError(f"the union-find kernels reported status {int(got[-1])} (1: a parent out of order, 2: an "
                           "iteration cap reached): the labels are not to be trusted")
    return got[:n], got[n:2 * n]


# ---- the host path of a pruned model ---------------------------------------------------------------------------------------
def neighbour_pairs(ids, vals, t):
    """(lo, hi) int64: every unordered pair of different nodes with a kept entry >= t in either direction, once.  ``ids``
    int [n, k] (-1: an empty slot), ``vals`` float64 [n, k]: the lists of a pruned model; t > 0 (an absent entry is +0.0)."""
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64)
    assert t > 0
    n = len(ids)
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], ids.shape)
    with np.errstate(invalid="ignore"):
        passes = (ids >= 0) & (ids != rows) & (vals >= t)    # (NaN passes nothing)
    a, b = rows[passes], ids[passes].astype(np.int64)
    key = np.unique(np.minimum(a, b) * n + np.maximum(a, b))
    return key // max(n, 1), key % max(n, 1)


def dbscan_of_pairs(n: int, lo, hi, min_neighbors):
    """(neighbours int64 [n], labels int64 [n]) of the graph of the unordered pairs (lo[i], hi[i]), each once: what the
    device path returns.  ``min_neighbors`` None: the counts alone, labels None."""
    deg = np.bincount(lo, minlength=n).astype(np.int64) + np.bincount(hi, minlength=n)
    if min_neighbors is None:
        return deg, None
    core = deg >= min_neighbors
    both = core[lo] & core[hi]
    roots = roots_of_edges(n, lo[both], hi[both])
    attach = np.full(n, NONE, dtype=np.int64)
    for x, y in ((lo, hi), (hi, lo)):                        # x core, y not: y is claimed by its smallest core neighbour
        one = core[x] & ~core[y]
        np.minimum.at(attach, y[one], x[one])
    claimed = ~core & (attach != NONE)
    labels = np.where(core, roots, -1)
    labels[claimed] = roots[attach[claimed]]
    return deg, labels


# ---- a solver's side ---------------------------------------------------------------------------------------------------------
def degrees(solver, j, ts) -> np.ndarray:
    """int64 [len(ts), n] of side j: per threshold every node's number of neighbours, over the caller's ids."""
    lists = solver.lists(j)
    if lists is not None:
        n = len(lists[0])
        return np.array([dbscan_of_pairs(n, *neighbour_pairs(lists[0], lists[1], t), None)[0] for t in ts],
                        dtype=np.int64).reshape(len(ts), n)
    if solver.n[j] == 0:
        return np.empty((len(ts), 0), dtype=np.int64)
    with solver.one_block(j) as reader:
        return degrees_block(reader.ops, reader.blocks[0], reader.n, ts).astype(np.int64)


def dbscan(solver, j, t: float, min_neighbors: int):
    """(neighbours int64 [n], labels int64 [n]) of side j over the caller's ids: a label is the smallest core node of the
    node's cluster, -1 for noise."""
    lists = solver.lists(j)
    if lists is not None:
        return dbscan_of_pairs(len(lists[0]), *neighbour_pairs(lists[0], lists[1], t), min_neighbors)
    if solver.n[j] == 0:
        return np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64)
    with solver.one_block(j) as reader:
        b = reader.blocks[0]
        deg, labels = dbscan_blocks(reader.ops, b, [b], reader.n, t, min_neighbors)
    return deg.astype(np.int64), labels.astype(np.int64)


def number(labels) -> np.ndarray:
    """int64 [n]: the clusters numbered 0, 1, 2, ... in the order of their first member, core or border; noise stays -1."""
    labels = np.asarray(labels, dtype=np.int64)
    out = np.full(labels.shape, -1, dtype=np.int64)
    at = np.flatnonzero(labels >= 0)
    if at.size:
        _, first, inverse = np.unique(labels[at], return_index=True, return_inverse=True)
        rank = np.empty(first.size, dtype=np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(first.size)
        out[at] = rank[inverse.reshape(-1)]
    return out
