"""ctypes binding of libsimrank_cluster.so (include/simrank_cluster.h): single-linkage clusters of a kept model, found on
the device.

``components(t)`` answers "which nodes belong together at threshold t?": the connected components of the graph that joins
two different nodes a, b iff ``S[a, b] >= t`` or ``S[b, a] >= t`` (iff (a, b) or (b, a) is a row of ``pairs(t)``).  One
sweep of the iterate serves up to ``MAX_LEVELS`` thresholds; it reads the blocks a solver's ``_query.Reader`` describes in
place and unites over them (one block on one GPU, one per virtual rank of a ``LocalWorld(P)``); N labels per threshold
cross PCIe.  A pruned model (a solver with ``lists``) is answered on the host from its lists, for its matrix P.  No
CPU fallback for the matrices: a missing library or device is an error.
"""
from __future__ import annotations

import ctypes as C
import numbers

import numpy as np

from ._checks import finite
from ._companion import PANEL_F16, PANEL_F32, ROWMAJOR_F32, ROWMAJOR_F64, Companion  # noqa: F401 (a block's layouts)
from ._driver import Scratch, stage
from ._profile import edges_f32

VERSION = 1              # SIMRANK_CLUSTER_VERSION of include/simrank_cluster.h
MAX_LEVELS = 8           # SIMRANK_CLUSTER_MAX_LEVELS: thresholds of one sweep
BAD_PARENT, CAP_REACHED = 1, 2      # bits of the device status word

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_cluster_version": [],
    "simrank_cluster_last_error": [],
    "simrank_cluster_init": [_vp, _i64, _i32, _vp, _vp],
    "simrank_cluster_union": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp],
    "simrank_cluster_labels": [_vp, _i64, _i32, _vp, _vp, _vp],
}
_RESTYPES = {"simrank_cluster_last_error": C.c_char_p}


class ClusterError(RuntimeError):
    """A call into libsimrank_cluster.so failed, or its kernels reported a forest out of order."""


_c = Companion("cluster", VERSION, PROTOTYPES, _RESTYPES, ClusterError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- argument checks: nothing touches a device ---------------------------------------------------------------------------
def check_thresholds(t):
    """``components(t)``: one finite real number -> (float64 [1], True); a sequence of 1 to ``MAX_LEVELS`` of them ->
    (float64 array, False).  ValueError otherwise."""
    if isinstance(t, np.ndarray) and t.ndim == 0:
        t = t[()]                                            # a 0-d array holds one number
    if isinstance(t, numbers.Real) and not isinstance(t, (bool, np.bool_)):
        return np.array([finite(t, "a threshold")], dtype=np.float64), True
    if isinstance(t, (str, bytes, bool, np.bool_)):
        raise ValueError(f"a threshold must be a finite number or a sequence of them, not {t!r}")
    try:
        items = list(t)
    except TypeError:
        raise ValueError(f"a threshold must be a finite number or a sequence of them, not {t!r}") from None
    if not 1 <= len(items) <= MAX_LEVELS:
        raise ValueError(f"components takes 1 to {MAX_LEVELS} thresholds, not {len(items)}")
    return np.array([finite(x, "a threshold") for x in items], dtype=np.float64), False


# ---- the device path -----------------------------------------------------------------------------------------------------
def roots_blocks(ops, blocks, n: int, ts, timing=None) -> np.ndarray:
    """int32 [len(ts), n]: per threshold the smallest id of every node's component over ``blocks`` (dicts with ptr,
    layout, stride, rows, cols and optional device row_ids / col_ids naming ids 0 .. n - 1), one
    ``simrank_cluster_union`` per block into one forest.  ``timing``: a list that receives the milliseconds of each
    union sweep and of the labels call (HIP events).  ClusterError when the device status word is not 0."""
    ts = np.asarray(ts, dtype=np.float64)
    m = int(ts.size)
    assert 1 <= m <= MAX_LEVELS and n >= 1
    layouts = {b["layout"] for b in blocks}
    assert len({lay == ROWMAJOR_F64 for lay in layouts}) == 1, "the blocks of one iterate hold one type"
    edges = ts if ROWMAJOR_F64 in layouts else edges_f32(ts)
    lib = load()
    got = np.empty(m * n + 1, dtype=np.int32)                # the labels, then the status word
    with Scratch(ops) as scratch:
        edges_dev = scratch.put(edges)
        parent, out = scratch.malloc(4 * m * n), scratch.malloc(4 * (m * n + 1))
        status = out + 4 * m * n
        check(lib.simrank_cluster_init(parent, n, m, status, ops.stream), "simrank_cluster_init")
        for b in blocks:
            stage(ops, timing, "union_ms", lambda: check(lib.simrank_cluster_union(
                b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], b.get("row_ids"), b.get("col_ids"), edges_dev, m,
                parent, n, status, ops.stream), "simrank_cluster_union"))
        stage(ops, timing, "labels_ms", lambda: check(lib.simrank_cluster_labels(parent, n, m, out, status, ops.stream),
                                                      "simrank_cluster_labels"))
        ops.d2h(got, out)
        ops.synchronize()
    if got[-1] != 0:
        raise ClusterError(f"the union-find kernels reported status {int(got[-1])} (1: a parent out of order, 2: an "
                           "iteration cap reached): the labels are not to be trusted")
    return got[:-1].reshape(m, n)


# ---- the host path of a pruned model ---------------------------------------------------------------------------------------
def roots_of_edges(n: int, a, b) -> np.ndarray:
    """int64 [n]: the smallest id of every node's component in the graph of the edges (a[i], b[i]): every node takes the
    smallest label among itself and its neighbours, then labels jump to their own labels, until nothing moves."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, a, label[b])
        np.minimum.at(new, b, label[a])
        while True:                                          # (label[x] <= x and in x's component: so is label[label[x]])
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            return label
        label = new


def roots_of_lists(ids, vals, ts) -> np.ndarray:
    """int64 [len(ts), n] for the matrix P of a pruned model: ``ids`` int [n, k] (-1: an empty slot), ``vals`` float64
    [n, k] the kept off-diagonal entries of each row; every other off-diagonal entry is +0.0."""
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64)
    n, k = ids.shape
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], ids.shape)
    kept = (ids >= 0) & (ids != rows)
    out = np.empty((len(ts), n), dtype=np.int64)
    for i, t in enumerate(ts):
        with np.errstate(invalid="ignore"):
            passes = kept & (vals >= t)                      # (NaN passes nothing; -0.0 >= 0.0 does)
        if t > 0:
            out[i] = roots_of_edges(n, rows[passes], ids[passes])
            continue
        # t <= 0: an absent entry joins its pair.  Two nodes stay apart only when BOTH directions are kept and neither
        # passes; a node has at most k such partners.
        if n > 2 * k:
            # any node v is joined to the n - 1 - k or more nodes it is not barred from, and every other node is barred
            # from at most k < n - k of those: one component
            out[i] = 0
            continue
        barred = np.zeros((n, n), dtype=bool)                # (n <= 2 k <= 8192)
        fails = kept & ~passes
        barred[rows[fails], ids[fails]] = True
        barred &= barred.T
        a, b = np.nonzero(np.triu(~barred, 1))
        out[i] = roots_of_edges(n, a, b)
    return out


# ---- a solver's side ---------------------------------------------------------------------------------------------------------
def roots(solver, j, ts) -> np.ndarray:
    """[len(ts), n] of side j: per threshold every node's component as its smallest caller id."""
    lists = solver.lists(j)
    if lists is not None:
        return roots_of_lists(lists[0], lists[1], ts)
    reader = solver._reader(j)
    if reader.n == 0:
        return np.empty((len(ts), 0), dtype=np.int64)
    return roots_blocks(reader.ops, reader.blocks, reader.n, ts)


def number(roots) -> np.ndarray:
    """int64, the shape of ``roots``: per row the components numbered 0, 1, 2, ... in the order of their first member (a
    root is its component's smallest id, so the sorted roots are in that order)."""
    out = np.empty(np.shape(roots), dtype=np.int64)
    for i, row in enumerate(roots):
        out[i] = np.unique(row, return_inverse=True)[1].reshape(-1)
    return out
