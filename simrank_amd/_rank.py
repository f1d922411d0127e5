"""ctypes binding of libsimrank_rank.so (include/simrank_rank.h): held-out ranks on a model that stays on the device.

    rank(q, t) = 1 + #{candidates c of basket q: score(q, c) > score(q, t), or equal with c before t in the frame's order}

the position of target t in what ``score_sets(top_k=N)`` returns for basket q, counted on the score band where
``_sets.run`` leaves it.  A companion of libsimrank_hip.so with its own header, version and binding, as ``_sets.py`` is.
``prepare`` checks the targets on the host (no device); ``run`` is ``_sets.run``'s band loop with a consumer that gathers
the targets' scores and counts what precedes them, block by block.  Per target 8 + 8 bytes cross to the host, per basket
8.  No CPU fallback: a missing library or device is an error.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._companion import Companion
from ._driver import Scratch, id_lists, join

VERSION = 1              # SIMRANK_RANK_VERSION of include/simrank_rank.h
CHUNK = 1024             # SIMRANK_RANK_CHUNK: band columns of one workgroup
TILE = 256               # SIMRANK_RANK_TILE: targets staged together
MAX_BLOCKS = 1 << 24     # SIMRANK_RANK_MAX_BLOCKS: workgroups of one call

_vp, _i64 = C.c_void_p, C.c_int64

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_rank_version": [],
    "simrank_rank_last_error": [],
    "simrank_rank_blocks": [_i64, _i64],
    "simrank_rank_gather": [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    "simrank_rank_count": [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
}
_RESTYPES = {"simrank_rank_last_error": C.c_char_p, "simrank_rank_blocks": C.c_int64}


class RankError(RuntimeError):
    """A call into libsimrank_rank.so failed."""


_c = Companion("rank", VERSION, PROTOTYPES, _RESTYPES, RankError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- the host half: arguments ----------------------------------------------------------------------------------------
def prepare(targets, index, n_sets: int):
    """The targets of ``rank_sets`` checked on the host, before any device work: one sequence of labels of fitted nodes
    per basket (``n_sets`` of them), repeats kept, empty lists allowed.  ``index``: pandas Index of the group's labels in
    the dense frame's order.  -> (tptr int64 [n_sets + 1], tids int32: positions in ``index``).  KeyError for an unknown
    label, ValueError for anything else."""
    tptr, tids = join(id_lists("targets", targets, index))
    if tptr.size - 1 != n_sets:
        raise ValueError(f"targets must have one sequence of labels per basket ({n_sets}), not {tptr.size - 1}")
    return tptr, tids


def check_ks(ks):
    """``evaluate``'s ``ks``: a non-empty sequence of positive ints -> list of int (ValueError otherwise)."""
    from ._query import check_k
    if isinstance(ks, (str, bytes)) or not hasattr(ks, "__iter__"):
        raise ValueError(f"ks must be a non-empty sequence of positive integers, not {ks!r}")
    ks = list(ks)
    if not ks:
        raise ValueError("ks must be a non-empty sequence of positive integers, not an empty one")
    return [check_k(k) for k in ks]


def ranks_of(score, before):
    """int64: 1 + before where the target is a candidate (its score is neither -inf nor NaN), 0 elsewhere."""
    return np.where(score > -np.inf, before + 1, 0).astype(np.int64)


def block_columns(tids, ids_sorted, whole):
    """The targets (caller ids) as columns of one block whose output columns hold the caller ids ``ids_sorted``
    (ascending): int32, -1 where the target's column is not in the block."""
    if whole:
        return np.ascontiguousarray(tids, dtype=np.int32)
    if not ids_sorted.size:
        return np.full(tids.size, -1, dtype=np.int32)
    at = np.minimum(np.searchsorted(ids_sorted, tids), ids_sorted.size - 1)
    return np.ascontiguousarray(np.where(ids_sorted[at] == tids, at, -1), dtype=np.int32)


# ---- the device half -------------------------------------------------------------------------------------------------
def run(reader, ptr, ids, w, excl, tptr, tids, timing=None):
    """The baskets (``ptr``, ``ids``, ``w``, ``excl`` as ``_sets.run`` takes them) scored on ``reader``'s iterate, and of
    each basket's targets (``tptr`` int64 [n_sets + 1], ``tids`` int32 caller ids) -> (score float64 [T]: the band's
    value, -inf for an excluded target; before int64 [T]: the candidates that precede it; candidates int64 [n_sets]: the
    basket's candidates, 0 for a basket without targets).  Per band of ``_sets.run``: the score kernels, then per column
    block one gather and one count (libsimrank_rank.so), which add over the blocks.  ``timing`` also receives
    ``gather_ms`` and ``count_ms``."""
    from . import _sets
    lib, ops = load(), reader.ops
    n_sets, n_t = int(ptr.size - 1), int(tids.size)
    score = np.full(n_t, np.nan, dtype=np.float64)
    before = np.zeros(n_t, dtype=np.int64)
    candidates = np.zeros(n_sets, dtype=np.int64)
    if n_t == 0 or reader.n == 0:
        return score, before, candidates
    whole = len(reader.blocks) == 1
    with Scratch(ops) as scratch:
        put = scratch.put
        tptr_dev = put(tptr.astype(np.int64, copy=False))
        tid_dev = put(tids.astype(np.int32, copy=False))
        score_dev, before_dev, cand_dev = put(score), put(before), put(candidates)
        cols_dev = {i: put(block_columns(tids, reader._col_map(i)[1], whole))
                    for i, b in enumerate(reader.blocks) if b["cols"]}

        def consume(q0, m, pieces, stage):
            tp = tptr_dev + 8 * q0
            for i, piece, cols, _ in pieces:
                stage("gather_ms", lambda: check(lib.simrank_rank_gather(
                    piece, cols, m, cols, tp, cols_dev[i], score_dev, ops.stream), "simrank_rank_gather"))
            for i, piece, cols, cid in pieces:
                stage("count_ms", lambda: check(lib.simrank_rank_count(
                    piece, cols, m, cols, cid, tp, score_dev, tid_dev, before_dev, cand_dev + 8 * q0, ops.stream),
                    "simrank_rank_count"))

        _sets.run(reader, ptr, ids, w, None, excl, timing, consumer=consume)
        ops.d2h(score, score_dev)
        ops.d2h(before, before_dev)
        ops.d2h(candidates, cand_dev)
        ops.synchronize()
    return score, before, candidates
