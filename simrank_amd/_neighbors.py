"""ctypes binding of libsimrank_neighbors.so (include/simrank_neighbors.h): a kept model pruned to the k most similar
OTHER nodes of every node, and the solver that answers the queries of a kept model from those lists.

The pruned form of a side of n nodes is two tables [n][k] (int32 ids in the caller's order, float64 values; id -1 / value 0
past the candidates) and the diagonal [n].  They stand for the matrix P that holds the kept entries, the diagonal and +0.0
everywhere else; every query of ``NeighborSolver`` is the same query of a dense model on P, bit for bit.  ``select`` builds
the tables from the block(s) of a kept iterate with ``simrank_neighbors_select``, whose cost does not grow with k.  The
queries with a host path of their own (``components``, ``linkage``, ``count_pairs``, ``cluster_quality``, ``kmedoids``,
``explain``) ask any solver for ``lists(j)``: ``NeighborSolver`` alone answers with its tables, so nothing outside this
module tests for the class.  No CPU fallback: a missing library or device is an error.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._companion import Companion
from ._driver import Scratch, bands, stage
from ._query import SolverQueries, check_k

VERSION = 1              # SIMRANK_NEIGHBORS_VERSION of include/simrank_neighbors.h
MAX_K = 4096             # SIMRANK_NEIGHBORS_MAX_K: the longest list
CHUNK = 2048             # SIMRANK_NEIGHBORS_CHUNK: output columns of one workgroup of rows / score
MAX_BLOCKS = 1 << 24     # SIMRANK_NEIGHBORS_MAX_BLOCKS: workgroups of one call of rows / score

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_neighbors_version": [],
    "simrank_neighbors_last_error": [],
    "simrank_neighbors_select": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp],
    "simrank_neighbors_rows": [_vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp],
    "simrank_neighbors_pairs": [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp],
    "simrank_neighbors_score": [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp],
}
_RESTYPES = {"simrank_neighbors_last_error": C.c_char_p}


class NeighborsError(RuntimeError):
    """A call into libsimrank_neighbors.so failed."""


_c = Companion("neighbors", VERSION, PROTOTYPES, _RESTYPES, NeighborsError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


def clamp_k(k: int, n: int) -> int:
    """k as ``topk_of`` clamps it: at most the n - 1 other nodes, at least 1."""
    return int(min(int(k), max(1, int(n) - 1)))


def check_prune_k(k, ns):
    """``prune(k)``: k a positive integer whose clamped value the selection can hold for every side (ValueError otherwise;
    nothing touches a device).  -> k"""
    k = check_k(k)
    for n in ns:
        if clamp_k(k, n) > MAX_K:
            raise ValueError(f"prune(k) keeps at most {MAX_K} neighbours per node (the selection sorts a node's list in "
                             f"the workgroup's local memory); k = {k} on {n} nodes is more")
    return k


def table_bytes(n: int, k: int) -> int:
    """Device bytes of one side's pruned form: 12 per kept entry, 8 per diagonal element."""
    return int(n) * int(k) * 12 + int(n) * 8


class Tables:
    """One side's pruned form on the device (the engine's pooled allocator): ``ids`` int32 [n][k], ``vals`` float64
    [n][k], ``diag`` float64 [n]."""

    def __init__(self, ops, n: int, k: int):
        self.ops, self.n, self.k = ops, int(n), int(k)
        self.ids = self.vals = self.diag = None
        try:
            self.ids = ops._malloc(4 * self.n * self.k)
            self.vals = ops._malloc(8 * self.n * self.k)
            self.diag = ops._malloc(8 * self.n)
        except Exception:
            self.free()
            raise

    @classmethod
    def from_host(cls, ops, ids, vals, diag):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        diag = np.ascontiguousarray(diag, dtype=np.float64)
        t = cls(ops, ids.shape[0], ids.shape[1])
        try:
            for ptr, host in ((t.ids, ids), (t.vals, vals), (t.diag, diag)):
                if host.size:
                    ops.h2d(ptr, host)
            ops.synchronize()
        except Exception:
            t.free()
            raise
        return t

    @property
    def nbytes(self) -> int:
        return table_bytes(self.n, self.k)

    def host(self):
        """(ids int32 [n, k], values float64 [n, k], diag float64 [n]) copied from the device."""
        ids, vals = np.empty((self.n, self.k), dtype=np.int32), np.empty((self.n, self.k), dtype=np.float64)
        diag = np.empty(self.n, dtype=np.float64)
        for host, ptr in ((ids, self.ids), (vals, self.vals), (diag, self.diag)):
            if host.size:
                self.ops.d2h(host, ptr)
        self.ops.synchronize()
        return ids, vals, diag

    def free(self):
        for name in ("ids", "vals", "diag"):
            p = getattr(self, name, None)
            if p:
                self.ops._free(p)
            setattr(self, name, None)


def select(reader, k: int, timing=None) -> Tables:
    """The pruned form of the iterate ``reader`` (``_query.Reader`` over ONE block holding every column) describes: every
    node's k best other nodes through ``simrank_neighbors_select``, written straight into the tables in the caller's
    order, and the diagonal through the reader's pair query.  ``timing``: a list that receives the selection's
    milliseconds (HIP events)."""
    ops, n = reader.ops, reader.n
    (b,) = reader.blocks
    assert b["cols"] == n and b.get("col_lo", 0) == 0
    k = clamp_k(k, n)
    t = Tables(ops, n, k)
    try:
        if n:
            nodes = np.arange(n, dtype=np.int32)
            with Scratch(ops) as scratch:
                pos_dev, ids_dev = scratch.put(reader.inv[nodes]), scratch.put(nodes)
                stage(ops, timing, "select_ms", lambda: check(load().simrank_neighbors_select(
                    b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], pos_dev, ids_dev, n, b.get("col_ids"), k,
                    t.ids, t.vals, ops.stream), "simrank_neighbors_select"))
                ops.synchronize()
                ops.h2d(t.diag, np.ascontiguousarray(reader.pair_values(nodes, nodes)))
    except Exception:
        t.free()
        raise
    return t


class NeighborReader:
    """The queries of one side's tables; node ids in, values in the caller's order out, every call ends synchronised.
    ``blocks`` / ``inv`` / ``_col_map`` / ``score_band`` are what ``_sets.run`` asks of a reader: one block that holds every
    column in the caller's order, whose score band comes from ``simrank_neighbors_score``."""

    def __init__(self, ops, tables: Tables):
        self.ops, self.t, self.n = ops, tables, tables.n
        self.q = load()
        self.order = self.inv = np.arange(self.n, dtype=np.int32)
        self.blocks = [dict(cols=self.n, col_lo=0)]

    def _col_map(self, i):
        return None, self.order

    def close(self):
        pass

    def _tables(self):
        t = self.t
        if t.ids is None:
            raise ValueError("the model's tables were released")
        return t.ids, t.vals, t.diag, t.n, t.k

    def rows(self, node_ids, out=None, timing=None):
        """float64 [len(node_ids), n]: those rows of P, in bands of at most ``_query.SLAB_BYTES`` on the device."""
        from . import hostpool
        ops, n = self.ops, self.n
        node_ids = np.ascontiguousarray(node_ids, dtype=np.int32)
        n_q = int(node_ids.size)
        if out is None:
            out = hostpool.empty_f64(n_q, n)
        if n_q == 0 or n == 0:
            return out
        tables = self._tables()
        walk = bands(n_q, 8 * n, MAX_BLOCKS // -(-n // CHUNK))
        with Scratch(ops) as scratch:
            pos_dev = scratch.put(node_ids)
            slab = scratch.malloc(8 * walk.size * n)
            for q0, m in walk:
                stage(ops, timing, "rows_ms", lambda: check(self.q.simrank_neighbors_rows(
                    *tables, pos_dev + 4 * q0, m, slab, n, ops.stream), "simrank_neighbors_rows"))
                ops.d2h(out[q0:q0 + m], slab, 8 * m * n)
            ops.synchronize()
        return out

    def pair_values(self, a_ids, b_ids):
        """float64 [len(a_ids)]: P[a][b] per pair of node ids (a's list is read)."""
        ops = self.ops
        a = np.ascontiguousarray(a_ids, dtype=np.int32)
        b = np.ascontiguousarray(b_ids, dtype=np.int32)
        out = np.empty(a.size, dtype=np.float64)
        if a.size == 0:
            return out
        tables = self._tables()
        with Scratch(ops) as scratch:
            a_dev, b_dev, val_dev = scratch.put(a), scratch.put(b), scratch.malloc(8 * a.size)
            check(self.q.simrank_neighbors_pairs(*tables, a_dev, b_dev, a.size, val_dev, ops.stream),
                  "simrank_neighbors_pairs")
            ops.d2h(out, val_dev)
            ops.synchronize()
        return out

    def topk_of(self, node_ids, k):
        """(ids int32 [len(node_ids), k], values float64): the first k entries of those nodes' lists (k at most the kept
        number).  The tables are small: a few nodes are copied row by row, many through one copy of the tables."""
        ops, t = self.ops, self.t
        node_ids = np.ascontiguousarray(node_ids, dtype=np.int32)
        n_q, k = int(node_ids.size), check_k(k)
        if k > t.k:
            raise ValueError(f"the model keeps kept_neighbors = {t.k} neighbours per node; k = {k} asks for more")
        self._tables()
        if n_q * 8 >= t.n:
            ids, vals, _ = t.host()
            return np.ascontiguousarray(ids[node_ids, :k]), np.ascontiguousarray(vals[node_ids, :k])
        ids, vals = np.empty((n_q, t.k), dtype=np.int32), np.empty((n_q, t.k), dtype=np.float64)
        for q, a in enumerate(node_ids.tolist()):
            ops.d2h(ids[q], t.ids + 4 * a * t.k)
            ops.d2h(vals[q], t.vals + 8 * a * t.k)
        ops.synchronize()
        return np.ascontiguousarray(ids[:, :k]), np.ascontiguousarray(vals[:, :k])

    def score_band(self, ptr_dev, pos_dev, w_dev, m, excl_ptr_dev, excl_cols_dev, out_dev, ld_out):
        """Queue the score band of m baskets (``_sets.run``'s device arrays) into ``out_dev``."""
        check(self.q.simrank_neighbors_score(*self._tables(), ptr_dev, pos_dev, w_dev, m, excl_ptr_dev, excl_cols_dev,
                                             out_dev, ld_out, self.ops.stream), "simrank_neighbors_score")


class NeighborSolver(SolverQueries):
    """The queries of a kept model over the pruned form of every side: no plan, no matrix.  ``specs`` and ``fitted`` as
    ``_model.DetachedSolver`` holds them (``recommend`` reads the CSR and the row scales, the lazy ``Evidence`` attributes
    the counts of the released solver)."""

    def __init__(self, ops, specs, tables, mode="sparse", fitted=None, storage=None):
        self.ops = {0: ops}
        self.specs = list(specs)
        self.tables = list(tables)
        self.n = [t.n for t in self.tables]
        self.kept_k = [t.k for t in self.tables]      # per side: the lists' length
        self.bipartite = len(self.tables) == 2
        self.storage = storage or self.specs[0].storage
        self.mode = mode
        self.fitted = fitted

    @property
    def device_bytes(self) -> int:
        return sum(t.nbytes for t in self.tables)

    def _make_reader(self, j):
        if j >= len(self.tables) or self.tables[j].ids is None:
            raise ValueError("the model's tables were released")
        return NeighborReader(self.ops[0], self.tables[j])

    def topk_of(self, j, node_ids, k):
        return self._reader(j).topk_of(node_ids, clamp_k(k, self.n[j]))

    def topk_among(self, j, node_ids, cand_ids, k):
        """``SolverQueries.topk_among`` for the matrix P, on the host after one copy of the tables: a candidate counts
        with its listed value, or with the +0.0 of an absent entry."""
        from . import _candidates
        return _candidates.topk_of_lists(self.lists(j), node_ids, cand_ids, k)

    def result(self, j=0):
        return self.rows(j, np.arange(self.n[j], dtype=np.int32))

    def topk(self, j, k, exclude_diag=True):
        if not exclude_diag:
            raise ValueError("a pruned model holds the k most similar OTHER nodes")
        return self.topk_of(j, np.arange(self.n[j], dtype=np.int32), k)

    def lists(self, j):
        """Side j's tables on the host, (ids, values, diag): what answers a query of a pruned model."""
        self._reader(j)                                      # (raises when the tables were released)
        return self.tables[j].host()

    def score_diverse(self, j, ptr, ids, w, k, excl, d, timing=None, among=None):
        """``SolverQueries.score_diverse`` for the matrix P, on the device: the band from ``score_band``, the picks from
        ``simrank_diverse_pick_lists`` on the tables."""
        from . import _diverse
        return _diverse.run(self._reader(j), ptr, ids, w, k, excl, d, timing, among=among)

    def pairs(self, j, t, max_pairs):
        """Side j's kept off-diagonal entries at least ``t``: (offsets [n + 1], neighbour ids ascending within a node,
        values), on the host after one copy of the tables."""
        from ._select import too_many
        ids, vals, _ = self.lists(j)
        hit = (ids >= 0) & (vals >= float(t))
        counts = hit.sum(axis=1)
        total = int(counts.sum())
        if max_pairs is not None and total > max_pairs:
            raise too_many(total, max_pairs)
        offsets = np.zeros(self.n[j] + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        rr, cc = np.nonzero(hit)
        got_ids, got_vals = ids[rr, cc], vals[rr, cc]
        order = np.lexsort((got_ids, rr))                    # (within a node: ascending by id)
        return offsets, np.ascontiguousarray(got_ids[order]), np.ascontiguousarray(got_vals[order])

    def fold_in(self, *args, **kw):
        raise ValueError("fold_in needs whole rows of the iterate, which a pruned model no longer holds: fold in before "
                         "prune()")

    def truncated(self, k):
        """A ``NeighborSolver`` on copies of the lists cut to their first ``k`` entries (clamped per side); this one is left
        as it is."""
        ops, tables = self.ops[0], []
        try:
            for t in self.tables:
                ids, vals, diag = t.host()
                kk = clamp_k(k, t.n)
                tables.append(Tables.from_host(ops, ids[:, :kk], vals[:, :kk], diag))
        except Exception:
            for t in tables:
                t.free()
            raise
        return NeighborSolver(ops, self.specs, tables, mode=self.mode, fitted=self.fitted, storage=self.storage)

    def evidence(self, j=0):
        """Evidence matrix of side j from the counts the released solver still keeps."""
        if self.fitted is None or not hasattr(self.fitted, "evidence"):
            raise AttributeError("this model was loaded from a file, not fitted: it holds no evidence counts")
        return self.fitted.evidence(j)

    def release(self):
        self._close_readers()
        for t in self.tables:
            t.free()


def prune(solver, k) -> NeighborSolver:
    """A ``NeighborSolver`` holding the k best neighbours of every node of every side of ``solver`` (a kept plan solver
    or a ``_model.DetachedSolver``); ``solver`` is left as it is.  Sides held in several column blocks are first packed
    into one temporary block each, once for the model (``one_block``): the selection reads one block that holds every
    column."""
    from . import _model
    tables = []
    try:
        with solver.one_block() as readers:
            for reader in readers:
                tables.append(select(reader, k))
    except Exception:
        for t in tables:
            t.free()
        raise
    if isinstance(solver, _model.DetachedSolver):
        specs, fitted = solver.specs, solver.fitted
    else:
        import dataclasses
        specs = [dataclasses.replace(s, apriori=None if s.apriori is None else _model._HAS_PRIOR) for s in solver.specs]
        fitted = solver
    ops = next(iter(solver.ops.values()))
    return NeighborSolver(ops, specs, tables, mode=getattr(solver, "mode", "sparse"), fitted=fitted,
                          storage=_model.storage_of(solver))
