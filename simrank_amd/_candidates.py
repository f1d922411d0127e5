"""ctypes binding of libsimrank_candidates.so (include/simrank_candidates.h): the k best of chosen rows of a kept model
among a LIST of candidate nodes, the same for every query of a call (the items in stock, of a category, not yet shown).

A companion of libsimrank_hip.so with its own header, version and binding, as ``_neighbors.py`` is.  ``prepare`` turns the
``among=`` / ``exclude=`` keywords of ``most_similar``, ``score_sets`` and ``recommend`` into the sorted caller ids of the
candidate set on the host (no device); ``topk_of`` selects among them over the column blocks of the kept iterate a
``_query.Reader`` describes, one call per block that holds candidates, merged on the host; ``topk_of_lists`` is the same
statement on the matrix P of a pruned model, on the host.  No CPU fallback: a missing library or device is an error.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._companion import Companion
from ._driver import Scratch

VERSION = 1              # SIMRANK_CANDIDATES_VERSION of include/simrank_candidates.h
MAX_K = 4096             # SIMRANK_CANDIDATES_MAX_K: the most picks per query
MAX_BLOCKS = 1 << 16     # SIMRANK_CANDIDATES_MAX_BLOCKS: workgroups of one call

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_candidates_version": [],
    "simrank_candidates_last_error": [],
    "simrank_candidates_topk": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _vp],
    "simrank_candidates_staged": [_i32],
}
_RESTYPES = {"simrank_candidates_last_error": C.c_char_p, "simrank_candidates_staged": C.c_int64}


class CandidatesError(RuntimeError):
    """A call into libsimrank_candidates.so failed."""


_c = Companion("candidates", VERSION, PROTOTYPES, _RESTYPES, CandidatesError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- the host half: arguments ----------------------------------------------------------------------------------------
def _label_ids(what, labels, index):
    """``labels``: a non-string iterable of labels of ``index`` -> their positions (int64, as given).  ValueError for a
    str, bytes or a scalar; KeyError for an unknown label."""
    if isinstance(labels, (str, bytes)) or not hasattr(labels, "__iter__"):
        raise ValueError(f"{what} must be None or an iterable of labels, not {labels!r}")
    import pandas as pd
    labels = list(labels)
    if not labels:
        return np.empty(0, dtype=np.int64)
    ids = index.get_indexer(pd.Index(labels, dtype=object) if index.dtype == object else pd.Index(labels))
    if (ids < 0).any():
        raise KeyError(labels[int(np.argmax(ids < 0))])
    return ids.astype(np.int64)


def prepare(among, exclude, index):
    """``among=`` / ``exclude=`` checked on the host, before any device work.  ``index``: pandas Index of the group's labels
    in the dense frame's order.  -> None when both are None, else the caller ids (int32, sorted, each once) of ``(among or
    every node) - exclude``; duplicates collapse and the order given does not matter."""
    if among is None and exclude is None:
        return None
    cand = np.arange(len(index), dtype=np.int64) if among is None else np.unique(_label_ids("among", among, index))
    if exclude is not None:
        cand = np.setdiff1d(cand, _label_ids("exclude", exclude, index), assume_unique=True)
    return np.ascontiguousarray(cand, dtype=np.int32)


def clamp_k(k, n_cand: int) -> int:
    """k of a filtered query: ``_query.check_k``, no more than the candidates there are, at least 1; ValueError when that
    is more than the selection holds."""
    from ._query import check_k
    k = min(check_k(k), max(1, int(n_cand)))
    if k > MAX_K:
        raise ValueError(f"a query among candidates picks at most {MAX_K} per node (the selection sorts the picks in the "
                         f"workgroup's local memory); k = {k} is more")
    return k


def staged(layout: int) -> int:
    """``simrank_candidates_staged``: the longest list whose keys a workgroup keeps in local memory (host only)."""
    return int(load().simrank_candidates_staged(int(layout)))


# ---- the device half -------------------------------------------------------------------------------------------------
def topk_of(reader, node_ids, cand_ids, k):
    """(ids int32 [len(node_ids), k], values float64): of each node the k best of the candidates ``cand_ids`` (caller ids,
    int32, sorted, each once) other than itself, in the order (value descending, id ascending); id -1 / value 0 past the
    candidates.  The candidates are dealt to ``reader.blocks`` by their position in the solver's order; one
    ``simrank_candidates_topk`` per block that holds any, with min(k, candidates of the block) picks, merged on the host
    as ``Reader.topk_of`` merges the blocks of a ``LocalWorld(P)``."""
    from ._query import check_k, merge_topk
    lib, ops = load(), reader.ops
    node_ids = np.ascontiguousarray(node_ids, dtype=np.int32)
    cand_ids = np.ascontiguousarray(cand_ids, dtype=np.int32)
    n_q, k = int(node_ids.size), check_k(k)
    empty = np.full((n_q, k), -1, dtype=np.int32), np.zeros((n_q, k), dtype=np.float64)
    if n_q == 0 or cand_ids.size == 0:
        return empty
    pos = reader.inv[cand_ids]
    pieces = []
    with Scratch(ops) as scratch:
        pos_dev = scratch.put(reader.inv[node_ids])
        ids_dev = scratch.put(node_ids)
        for b in reader.blocks:
            lo = b.get("col_lo", 0)
            mine = np.flatnonzero((pos >= lo) & (pos < lo + b["cols"]))
            if not mine.size:
                continue
            kk = int(min(k, mine.size))
            cpos_dev = scratch.put(np.ascontiguousarray(pos[mine] - lo, dtype=np.int32))
            cids_dev = scratch.put(np.ascontiguousarray(cand_ids[mine]))
            idx, val = np.empty((n_q, kk), dtype=np.int32), np.empty((n_q, kk), dtype=np.float64)
            idx_dev, val_dev = scratch.malloc(4 * n_q * kk), scratch.malloc(8 * n_q * kk)
            check(lib.simrank_candidates_topk(b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], pos_dev, ids_dev,
                                              n_q, cpos_dev, cids_dev, mine.size, kk, idx_dev, val_dev, ops.stream),
                  "simrank_candidates_topk")
            ops.d2h(idx, idx_dev)
            ops.d2h(val, val_dev)
            ops.synchronize()
            pieces.append((idx, val))
    return merge_topk(pieces, k) if pieces else empty


def topk_of_lists(lists, node_ids, cand_ids, k):
    """``topk_of`` for the matrix P of a pruned model, on the host: ``lists`` = (ids, values, diag) of the side.  A
    candidate counts with its listed value where it is in the node's list and with +0.0 where it is absent; the node
    itself is no candidate, NaN is none either."""
    from ._query import check_k
    ids, vals, _ = lists
    node_ids = np.asarray(node_ids, dtype=np.int64)
    cand_ids = np.asarray(cand_ids, dtype=np.int64)
    k = check_k(k)
    idx = np.full((node_ids.size, k), -1, dtype=np.int32)
    val = np.zeros((node_ids.size, k), dtype=np.float64)
    for q, a in enumerate(node_ids.tolist()):
        row = np.zeros(cand_ids.size, dtype=np.float64)
        listed = ids[a] >= 0
        at = np.searchsorted(cand_ids, ids[a][listed])
        hit = at < cand_ids.size
        hit[hit] = cand_ids[at[hit]] == ids[a][listed][hit]
        row[at[hit]] = vals[a][listed][hit]
        ok = (cand_ids != a) & ~np.isnan(row)
        best = np.flatnonzero(ok)
        best = best[np.lexsort((cand_ids[best], -row[best]))][:k]
        idx[q, :best.size], val[q, :best.size] = cand_ids[best], row[best]
    return idx, val
