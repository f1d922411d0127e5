"""What the companion drivers (``_query``, ``_sets``, ``_rank``, ``_foldin``, ``_neighbors``, ``_profile``, ``_cluster``,
``_linkage``, ``_groups``, ``_kmedoids``, ``_explain``, ``_compare``, ``_diverse``, ``_density``, ``_model``, ``_exemplars``) share on the host: the lifetime of a call's device scratch, the timed stage, the band walk, the stitch of
column blocks and the label lists.  ``ops`` is the engine's ``HipOps`` (or a double with its methods); nothing here
calls a library.
"""
from __future__ import annotations

import numpy as np


class Scratch:
    """The transient device blocks of one driver call, as a context manager.  ``simrank_free`` hands a block to a pool
    that every stream of the device allocates from, so no block goes back while a kernel that reads it may be queued:
    the exit first synchronises ``ops``' stream, then frees what was handed out, last first, with or without an
    exception in flight (every call that holds scratch therefore ends synchronised).  A synchronise that fails while
    another exception is pending still frees everything and leaves that exception the one that propagates."""

    def __init__(self, ops):
        self.ops, self._held = ops, []

    def malloc(self, nbytes) -> int:
        self._held.append(self.ops._malloc(nbytes))
        return self._held[-1]

    def put(self, host) -> int:
        """A block holding a copy of the host array (made C-contiguous here)."""
        self._held.append(self.ops.put(np.ascontiguousarray(host)))
        return self._held[-1]

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            self.ops.synchronize()
        except Exception:
            if exc_type is None:
                raise
        finally:
            while self._held:
                self.ops._free(self._held.pop())
        return False


def stage(ops, timing, name, launch):
    """Run ``launch()``; with ``timing`` between two HIP events (``ops.timed``: serialises the stages), the
    milliseconds appended to a list or added under ``name`` in a dict."""
    if timing is None:
        launch()
    elif isinstance(timing, dict):
        timing[name] = timing.get(name, 0.0) + ops.timed(launch)
    else:
        timing.append(ops.timed(launch))


class bands:
    """The walk over ``n_items`` rows of ``row_bytes`` device bytes each in bands that fit ``_query.SLAB_BYTES`` (read
    at the call: tests cut it down) and stay within ``caps``: ``size`` rows, whole multiples of ``unit`` and at least
    one; iterating yields (first row, rows) of every band."""

    def __init__(self, n_items, row_bytes, *caps, unit=1):
        from . import _query
        self.n_items = int(n_items)
        self.size = int(max(unit, min(-(-self.n_items // unit) * unit, _query.SLAB_BYTES // row_bytes // unit * unit,
                                      *caps)))

    def __iter__(self):
        for q0 in range(0, self.n_items, self.size):
            yield q0, min(self.size, self.n_items - q0)


def scatter_blocks(out_rows, staged, m, blocks, col_ids_of):
    """A band of m rows as it lies in the slab, every block's [m, cols] piece after the other (``staged``: its host
    copy, which may be longer) -> ``out_rows`` [m, n]: block i's columns go to their caller ids ``col_ids_of(i)``."""
    flat, off = staged.reshape(-1), 0
    for i, b in enumerate(blocks):
        out_rows[:, col_ids_of(i)] = flat[off:off + m * b["cols"]].reshape(m, b["cols"])
        off += m * b["cols"]


def id_lists(what, seqs, index, unique=False, each="basket"):
    """``seqs``: one sequence of labels per ``each`` -> one int32 array per sequence: positions in ``index`` (a pandas
    Index), in the order given; repeats kept, or with ``unique`` a ValueError.  KeyError for the first unknown label."""
    import pandas as pd
    if isinstance(seqs, (str, bytes)) or not hasattr(seqs, "__len__"):
        raise ValueError(f"{what} must be a sequence with one sequence of labels per {each}")
    lists = []
    for q, one in enumerate(seqs):
        if isinstance(one, (str, bytes)) or not hasattr(one, "__iter__"):
            raise ValueError(f"{what}[{q}] must be a sequence of labels, not {one!r}")
        one = list(one)
        if not one:
            lists.append(np.empty(0, dtype=np.int32))
            continue
        ids = index.get_indexer(pd.Index(one, dtype=object) if index.dtype == object else pd.Index(one))
        if (ids < 0).any():
            raise KeyError(one[int(np.argmax(ids < 0))])
        if unique and np.unique(ids).size != ids.size:
            raise ValueError(f"{what}[{q}] repeats a label: a node has one edge per neighbour (duplicate entries)")
        lists.append(np.ascontiguousarray(ids, dtype=np.int32))
    return lists


def join(lists):
    """Arrays of ids -> (offsets int64 [n + 1], ids int32)."""
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([a.size for a in lists], out=ptr[1:])
    ids = np.concatenate(lists).astype(np.int32, copy=False) if ptr[-1] else np.empty(0, dtype=np.int32)
    return ptr, np.ascontiguousarray(ids)
