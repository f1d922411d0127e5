"""ctypes binding of libsimrank_sets.so (include/simrank_sets.h): basket queries on a model that stays on the device.

    score(q, b) = sum_{e in basket q} w_e * S[e, b]       float64, in list order, product and sum rounded separately

A companion of libsimrank_hip.so with its own header, version and binding, as ``_query.py`` is.  ``prepare`` checks and
normalises the arguments of ``score_sets`` on the host (no device); ``run`` scores the baskets over the column blocks of
the kept iterate a ``_query.Reader`` describes, in bands of at most ``_query.SLAB_BYTES`` on the device, and hands back
the dense rows or the k best of each.  No CPU fallback: a missing library or device is an error.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from ._companion import Companion
from . import _driver
from ._driver import Scratch, bands, id_lists, join, scatter_blocks

VERSION = 1              # SIMRANK_SETS_VERSION of include/simrank_sets.h
CHUNK = 1024             # SIMRANK_SETS_CHUNK: output columns of one workgroup
MAX_BLOCKS = 1 << 24     # SIMRANK_SETS_MAX_BLOCKS: workgroups of one call
BASKET_MAJOR, CHUNK_LABEL = 0, 1     # SIMRANK_SETS_GRID_*: how the workgroups are numbered
GRID_ORDER = BASKET_MAJOR            # the one ``run`` uses (measured both ways)

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_sets_version": [],
    "simrank_sets_last_error": [],
    "simrank_sets_blocks": [_i64, _i64, _i32],
    "simrank_sets_score": [_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp],
    "simrank_sets_topk": [_vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _vp],
}
_RESTYPES = {"simrank_sets_last_error": C.c_char_p, "simrank_sets_blocks": C.c_int64}


class SetsError(RuntimeError):
    """A call into libsimrank_sets.so failed."""


_c = Companion("sets", VERSION, PROTOTYPES, _RESTYPES, SetsError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- the host half: arguments ----------------------------------------------------------------------------------------
def _id_lists(what, seqs, index):
    """``seqs``: one sequence of labels per basket -> (offsets int64 [n + 1], ids int32): positions in ``index``, in the
    order given, repeats kept.  KeyError for an unknown label."""
    return join(id_lists(what, seqs, index))


def check_top_k(top_k, n: int):
    """None, or k checked by ``_query.check_k`` and clamped to the ``n`` candidates there can be.  The selection kernel
    has no limit of its own on k (its cost is k passes over a row)."""
    from ._query import check_k
    return None if top_k is None else min(check_k(top_k), max(1, int(n)))


def prepare(sets, index, *, weights=None, names=None, top_k=None, exclude="members"):
    """The arguments of ``score_sets`` checked and normalised on the host, before any device work.  ``index``: pandas
    Index of the group's labels in the dense frame's order.  -> (ptr int64 [n_sets + 1], ids int32, w float64, names:
    list or None, k or None, excl: None or (ptr, ids) of the excluded candidates per basket)."""
    ptr, ids = _id_lists("sets", sets, index)
    n_sets = ptr.size - 1
    if weights is None:
        w = np.ones(ids.size, dtype=np.float64)
    else:
        if isinstance(weights, (str, bytes)) or not hasattr(weights, "__len__") or len(weights) != n_sets:
            raise ValueError(f"weights must have one sequence per basket ({n_sets})")
        parts = []
        for q, one in enumerate(weights):
            try:
                a = np.asarray(one, dtype=np.float64).ravel()
            except (TypeError, ValueError) as e:
                raise ValueError(f"weights[{q}] must be a sequence of floats") from e
            if a.size != ptr[q + 1] - ptr[q]:
                raise ValueError(f"weights[{q}] has {a.size} entries for {int(ptr[q + 1] - ptr[q])} members")
            if not np.isfinite(a).all():
                raise ValueError(f"weights[{q}] holds a value that is not finite")
            parts.append(a)
        w = np.ascontiguousarray(np.concatenate(parts) if parts else np.empty(0), dtype=np.float64)
    if names is not None:
        names = list(names)
        if len(names) != n_sets:
            raise ValueError(f"names must have one entry per basket ({n_sets}), not {len(names)}")
    k = check_top_k(top_k, len(index))
    if exclude is None:
        excl = None
    elif isinstance(exclude, str):
        if exclude != "members":
            raise ValueError(f"exclude must be 'members', None or one sequence of labels per basket, not {exclude!r}")
        excl = (ptr, ids)
    else:
        if not hasattr(exclude, "__len__") or len(exclude) != n_sets:
            raise ValueError(f"exclude must be 'members', None or one sequence of labels per basket ({n_sets})")
        excl = _id_lists("exclude", exclude, index)
    return ptr, ids, w, names, k, (excl if k is not None else None)


def csr_baskets(csr, rowscale, nodes, also_self: bool, exclude_seen: bool):
    """``recommend``'s baskets from one side's CSR: per node u of ``nodes`` (row ids) the row's columns in its order, every
    weight ``rowscale[u]``; the excluded candidates (the row itself, and u when ``also_self``) or None.
    -> (ptr, ids, w, excl)"""
    rowptr = np.asarray(csr.rowptr, dtype=np.int64)
    col = np.asarray(csr.col, dtype=np.int32)
    nodes = np.asarray(nodes, dtype=np.int64)
    lists = [col[rowptr[u]:rowptr[u + 1]] for u in nodes]
    ptr, ids = join(lists)
    w = np.repeat(np.asarray(rowscale, dtype=np.float64)[nodes], np.diff(ptr))
    excl = None
    if exclude_seen:
        excl = join([np.append(l, np.int32(u)) for l, u in zip(lists, nodes)]) if also_self else (ptr, ids)
    return ptr, ids, np.ascontiguousarray(w), excl


# ---- the device half -------------------------------------------------------------------------------------------------
def _block_exclusions(excl, ids_sorted, whole):
    """The excluded candidates (caller ids per basket) as OUTPUT columns of one block: ``ids_sorted`` are the caller ids
    of the block's output columns, ascending.  -> (ptr int64, cols int32)"""
    ptr, ids = excl
    if whole:
        return ptr, ids
    at = np.minimum(np.searchsorted(ids_sorted, ids), max(0, ids_sorted.size - 1))
    hit = ids_sorted[at] == ids if ids_sorted.size else np.zeros(ids.size, dtype=bool)
    basket = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    out = np.zeros(ptr.size, dtype=np.int64)
    np.cumsum(np.bincount(basket[hit], minlength=ptr.size - 1), out=out[1:])
    return out, np.ascontiguousarray(at[hit], dtype=np.int32)


def _outside(excl, among, n, n_sets):
    """``excl`` (or None) with every caller id outside ``among`` added to every basket: what marks the band of a reader
    that writes all n columns (a pruned model's ``score_band``) so that only the candidates remain."""
    rest = np.setdiff1d(np.arange(n, dtype=np.int32), among, assume_unique=True).astype(np.int32)
    if excl is None:
        return np.arange(n_sets + 1, dtype=np.int64) * rest.size, np.tile(rest, n_sets)
    ptr, ids = excl
    return join([np.concatenate([ids[ptr[q]:ptr[q + 1]], rest]) for q in range(n_sets)])


def run(reader, ptr, ids, w, k=None, excl=None, timing=None, grid_order=None, consumer=None, among=None):
    """Score the baskets (``ptr`` int64 [n_sets + 1], ``ids`` int32 caller ids, ``w`` float64) on ``reader``'s iterate
    (``_query.Reader``, or the ``_neighbors.NeighborReader`` of a pruned model, whose ``score_band`` fills the band from
    the neighbour lists instead) -> float64 [n_sets, n] in the caller's column order, or with ``k`` (ids int32 [n_sets, k], values
    float64 [n_sets, k]): the k best per basket (score descending, id ascending; id -1 / value 0 past the candidates),
    ``excl`` = (ptr, ids) of the caller ids that are no candidates.  With ``consumer`` nothing of the band is handed back
    (-> None): ``excl`` marks the band as it does for a selection, and after the kernels of each band are queued the
    band stays on the device for ``consumer(q0, m, pieces, stage)``: baskets q0 .. q0 + m - 1, ``pieces`` one (block
    index, device pointer of the block's [m, cols] float64 piece, cols, device caller ids of its columns or None where
    they are 0 .. cols - 1) per block with columns, ``stage(name, launch)`` the timing hook; what it queues on the
    reader's stream is done before the next band overwrites the slab (``_rank.run``).  One band of baskets holds at most
    ``_query.SLAB_BYTES`` on the device; per band one score kernel per column block, then one copy of the band or one
    selection per block with the pieces merged on the host.  ``timing``: a dict that receives the milliseconds of the
    stages (HIP events; serialises them).  ``among`` (with ``k`` or a ``consumer``): the caller ids (int32, sorted, each
    once) of the only candidates.  A block then scores its candidates' columns alone: ``col_pos`` their positions, ``n_out``
    their number, so the band is |among| wide and a piece's columns are the block's candidates in id order (a consumer
    always gets their device ids); a score depends on its own column only and keeps its bits.  A pruned model's
    ``score_band`` writes every column: there the columns outside ``among`` are marked as ``excl`` marks them."""
    from . import _query, hostpool
    lib, ops, n = load(), reader.ops, reader.n
    order = GRID_ORDER if grid_order is None else int(grid_order)
    n_sets = int(ptr.size - 1)
    marked = k is not None or consumer is not None         # the band carries the exclusions and the blocks their ids
    score_band = getattr(reader, "score_band", None)
    if among is not None:
        if not marked:
            raise ValueError("among narrows a selection: give k or a consumer")
        among = np.ascontiguousarray(among, dtype=np.int32)
        if score_band is not None:                           # (every column is written: mark, do not narrow)
            excl, among = (_outside(excl, among, n, n_sets) if n_sets and n else excl), None
    width = n if among is None else int(among.size)        # columns of the band
    if consumer is not None:
        if k is not None:
            raise ValueError("a consumer takes the band instead of a selection: k must be None")
        result = None
    elif k is None:
        result = hostpool.empty_f64(n_sets, n)
    else:
        k = int(min(k, max(1, width)))
        result = (np.full((n_sets, k), -1, dtype=np.int32), np.zeros((n_sets, k), dtype=np.float64))
    if n_sets == 0 or width == 0:
        return result
    # a band's workgroups on one block, in either grid order: at most band * max(8, chunks + 7)
    per_basket = max(8, -(-max(b["cols"] for b in reader.blocks) // CHUNK) + 7)
    walk = bands(n_sets, 8 * width, MAX_BLOCKS // per_basket)
    whole = len(reader.blocks) == 1 and among is None
    stage = functools.partial(_driver.stage, ops, timing)
    with Scratch(ops) as scratch:
        slab, put = scratch.malloc(8 * walk.size * width), scratch.put
        ptr_dev = put(ptr.astype(np.int64, copy=False))
        pos_dev = put(reader.inv[ids]) if ids.size else None
        w_dev = put(np.asarray(w, dtype=np.float64)) if ids.size else None
        per_block = []
        for i, b in enumerate(reader.blocks):
            if among is None:
                cmap, ids_sorted = reader._col_map(i)
            else:                                            # (the block's candidates, in id order, and where they lie)
                at = reader.inv[among].astype(np.int64) - b.get("col_lo", 0)
                mine = (at >= 0) & (at < b["cols"])
                ids_sorted = np.ascontiguousarray(among[mine])
                cmap = put(at[mine].astype(np.int32)) if ids_sorted.size else None
            xp = xc = cid = None
            if marked and ids_sorted.size:
                if excl is not None:
                    bp, bc = _block_exclusions(excl, ids_sorted, whole)
                    xp, xc = put(bp), put(bc if bc.size else np.zeros(1, dtype=np.int32))
                if not whole:
                    cid = put(np.ascontiguousarray(ids_sorted, dtype=np.int32))
            per_block.append((b, cmap, ids_sorted, xp, xc, cid))
        if k is not None:
            kks = [int(min(k, p[2].size)) for p in per_block]
            idx_dev = [scratch.malloc(4 * walk.size * max(1, kk)) for kk in kks]
            val_dev = [scratch.malloc(8 * walk.size * max(1, kk)) for kk in kks]
        stitch = None if whole or marked else np.empty((walk.size, n), dtype=np.float64)
        for q0, m in walk:
            off, pieces = 0, []
            for i, (b, cmap, ids_sorted, xp, xc, cid) in enumerate(per_block):
                cols = int(ids_sorted.size)                  # (output columns; without among the block's own)
                if not cols:
                    continue
                piece = slab + 8 * off
                if score_band is not None:               # (a pruned model: the same band from its neighbour lists)
                    stage("score_ms", lambda: score_band(ptr_dev + 8 * q0, pos_dev, w_dev, m,
                                                         None if xp is None else xp + 8 * q0, xc, piece, cols))
                else:
                    stage("score_ms", lambda: check(lib.simrank_sets_score(
                        b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], cmap, cols, ptr_dev + 8 * q0, pos_dev,
                        w_dev, m, None if xp is None else xp + 8 * q0, xc, piece, cols, order, ops.stream),
                        "simrank_sets_score"))
                if k is not None:
                    kk = kks[i]
                    stage("topk_ms", lambda: check(lib.simrank_sets_topk(
                        piece, cols, m, cols, cid, kk, idx_dev[i], val_dev[i], ops.stream), "simrank_sets_topk"))
                    idx, val = np.empty((m, kk), dtype=np.int32), np.empty((m, kk), dtype=np.float64)
                    ops.d2h(idx, idx_dev[i])
                    ops.d2h(val, val_dev[i])
                    pieces.append((idx, val))
                elif consumer is not None:
                    pieces.append((i, piece, cols, cid))
                off += m * cols
            if consumer is not None:
                consumer(q0, m, pieces, stage)
            elif k is not None:
                ops.synchronize()
                result[0][q0:q0 + m], result[1][q0:q0 + m] = _query.merge_topk(pieces, k)
            elif whole:
                ops.d2h(result[q0:q0 + m], slab, 8 * m * n)
            else:
                ops.d2h(stitch, slab, 8 * m * n)
                ops.synchronize()
                scatter_blocks(result[q0:q0 + m], stitch, m, reader.blocks, lambda i: per_block[i][2])
        ops.synchronize()
    return result
