"""ctypes binding of libsimrank_query.so (include/simrank_query.h): node queries on a model that stays on the device.

A companion of libsimrank_hip.so with its own header, version and binding, so that the main library's C ABI stays as it
is; it reads the iterate a plan reports through ``simrank_plan_get`` & co in place.  ``Reader`` runs the three queries over
the column blocks of one kept iterate (one block on one GPU, one per virtual rank of a ``LocalWorld(P)``).  No CPU
fallback: a missing library or device is an error.
"""
from __future__ import annotations

import contextlib
import ctypes as C

from ._checks import is_int
from ._companion import PANEL_F16, PANEL_F32, ROWMAJOR_F32, ROWMAJOR_F64, Companion  # noqa: F401 (a block's layouts)
from ._driver import Scratch, bands, scatter_blocks, stage

VERSION = 1              # SIMRANK_QUERY_VERSION of include/simrank_query.h

SLAB_BYTES = 256 << 20   # device block of one band of ``rows`` (a larger request is cut into bands of query rows)

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_query_version": [],
    "simrank_query_last_error": [],
    "simrank_query_rows": [_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp],
    "simrank_query_pairs": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp],
    "simrank_query_topk": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp],
    "simrank_query_merge_topk": [_i32, _vp, _vp, _vp, _i64, _i32, _vp, _vp],
}
_RESTYPES = {"simrank_query_last_error": C.c_char_p}


class QueryError(RuntimeError):
    """A call into libsimrank_query.so failed."""


_c = Companion("query", VERSION, PROTOTYPES, _RESTYPES, QueryError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


def check_k(k):
    """``most_similar(nodes, k)`` / ``top_k(k)``: k a positive integer (ValueError otherwise; nothing touches a device)."""
    if not is_int(k) or int(k) < 1:
        raise ValueError(f"k must be a positive integer, not {k!r}")
    return int(k)


def merge_topk(pieces, k: int):
    """Host: pieces [(ids int32 [n_q, k_p], values float64 [n_q, k_p])] over the same query rows, one per column block
    (id -1 = empty slot) -> (ids int32 [n_q, k], values float64 [n_q, k]): each row's k best in the order (value
    descending, id ascending), empty slots as id -1 / value 0."""
    import numpy as np
    pieces = [(np.ascontiguousarray(i, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)) for i, v in pieces]
    n_q = pieces[0][0].shape[0] if pieces else 0
    k = check_k(k)
    for i, v in pieces:
        if i.ndim != 2 or i.shape != v.shape or i.shape[0] != n_q:
            raise ValueError("every piece is (ids [n_q, k_p], values [n_q, k_p]) over the same n_q rows")
    if len(pieces) == 1 and pieces[0][0].shape[1] == k:
        return pieces[0]                                       # (one block's k best are in the order already)
    idx = np.empty((n_q, k), dtype=np.int32)
    val = np.empty((n_q, k), dtype=np.float64)
    P = len(pieces)
    ids = (C.c_void_p * max(1, P))(*[i.ctypes.data if i.size else None for i, _ in pieces])
    vals = (C.c_void_p * max(1, P))(*[v.ctypes.data if v.size else None for _, v in pieces])
    ks = (C.c_int32 * max(1, P))(*[i.shape[1] for i, _ in pieces])
    check(load().simrank_query_merge_topk(P, ids, vals, ks, n_q, k, idx.ctypes.data if n_q else None,
                                          val.ctypes.data if n_q else None), "simrank_query_merge_topk")
    return idx, val


def clamp_k(n, k, exclude_diag=True) -> int:
    """The k a top-k of ``n`` nodes is cut to: no more than the candidates of a node, at least one."""
    return int(min(k, max(1, n - (1 if exclude_diag else 0))))


class SolverQueries:
    """What a kept solver (``cplan.PlanSolver``, ``cshard.CShardSolver``, ``cdouble.F64Solver``, ``_model.DetachedSolver``,
    ``_neighbors.NeighborSolver``) answers node queries with: one ``Reader`` per side, made on first use by the solver's
    ``_make_reader(j)`` and closed at ``release``; and the two decisions every query of a side makes first: ``lists``
    (is this a pruned model, answered on the host?) and ``one_block`` (is the side held in several column blocks?)."""

    _readers = None
    _folders = None

    def _reader(self, j):
        if self._readers is None:
            self._readers = {}
        if j not in self._readers:
            self._readers[j] = self._make_reader(j)
        return self._readers[j]

    def lists(self, j):
        """None: side j is held as a matrix.  The solver of a pruned model returns its host lists (ids, values, diag)
        here, and the query is answered from them on the host."""
        return None

    @contextlib.contextmanager
    def one_block(self, j=None):
        """Side j's reader where its one block holds every row and column; a side held in several column blocks
        (``LocalWorld(P)``) is first packed into a temporary ``_model.detach(self)``, every side in the model's own
        storage, which is released at the end of the scope, with or without an exception.  Without ``j``: the readers
        of all sides, packed at most once."""
        from . import _model
        sides = range(len(self.n)) if j is None else [j]
        temp = None
        try:
            if any(len(self._reader(i).blocks) != 1 for i in sides):
                temp = _model.detach(self)
            readers = [(temp or self)._reader(i) for i in sides]
            for r in readers:
                (b,) = r.blocks
                assert b["cols"] == r.n and b["rows"] == r.n and b.get("col_lo", 0) == 0
            yield readers if j is None else readers[0]
        finally:
            if temp is not None:
                temp.release()

    def rows(self, j, node_ids):
        """float64 [len(node_ids), n]: side j's rows of those nodes (caller's ids), columns in the caller's order."""
        return self._reader(j).rows(node_ids)

    def pair_values(self, j, a_ids, b_ids):
        """float64 [len(a_ids)]: side j's S[a][b] per pair of node ids."""
        return self._reader(j).pair_values(a_ids, b_ids)

    def topk_of(self, j, node_ids, k):
        """(ids int32 [len(node_ids), k], values float64): the k most similar OTHER nodes of those nodes, k clamped as
        the solver's ``topk`` clamps it."""
        return self._reader(j).topk_of(node_ids, clamp_k(self.n[j], k))

    def topk_among(self, j, node_ids, cand_ids, k):
        """(ids int32 [len(node_ids), k], values float64): of those nodes the k best among the candidates ``cand_ids``
        (caller ids, int32, sorted, each once) other than the node itself (``_candidates.topk_of``); ``k`` as the caller
        clamped it to the candidates."""
        from . import _candidates
        return _candidates.topk_of(self._reader(j), node_ids, cand_ids, k)

    def fold_in(self, j, lists, w, prior=None, top_k=None, timing=None):
        """Rows of NEW nodes joining side j (``_foldin.Folder.run``): ``lists`` hold ids of the side the update reads
        (the same side for the one-matrix classes, the other one for the bipartite classes).  Side j's CSR goes to the
        device at the first call and stays until ``release``."""
        from . import _foldin
        if self._folders is None:
            self._folders = {}
        if j not in self._folders:
            spec = self.specs[j]
            evidence = spec.evidence_from is not None
            if evidence and spec.evidence_from is not spec.csr:
                _foldin.check_strict_group(len(self.specs), j, True)
                raise ValueError("fold_in needs the evidence of the side's own pattern")
            src = len(self.specs) - 1 - j
            self._folders[j] = _foldin.Folder(self._reader(src), spec.csr, spec.rowscale, spec.coef, spec.lbd, evidence)
        return self._folders[j].run(lists, w, prior, top_k, timing)

    def score_sets(self, j, ptr, ids, w, k=None, excl=None, timing=None, among=None):
        """Basket scores on side j's iterate (``_sets.run``): ``ptr`` / ``ids`` / ``w`` the baskets as offsets, node ids
        of side j and weights; the dense rows, or with ``k`` the k best per basket outside ``excl`` (and, with ``among``,
        among those sorted caller ids only)."""
        from . import _sets
        return _sets.run(self._reader(j), ptr, ids, w, k, excl, timing, among=among)

    def score_ranks(self, j, ptr, ids, w, excl, tptr, tids, timing=None):
        """Held-out ranks on side j's iterate (``_rank.run``): the baskets as ``score_sets`` takes them, ``tptr`` /
        ``tids`` their targets as offsets and node ids of side j -> (score float64, before int64) per target and the
        candidates (int64) per basket; the score band stays on the device."""
        from . import _rank
        return _rank.run(self._reader(j), ptr, ids, w, excl, tptr, tids, timing)

    def score_diverse(self, j, ptr, ids, w, k, excl, d, timing=None, among=None):
        """The k picks per basket at diversity ``d`` on side j's iterate (``_diverse.run``): the baskets as ``score_sets``
        takes them -> (ids int32, score, penalty, value float64), each [n_sets, k]; the score band stays on the device.
        A side held in several column blocks is first packed into one (``one_block``)."""
        from . import _diverse
        with self.one_block(j) as reader:
            return _diverse.run(reader, ptr, ids, w, k, excl, d, timing, among=among)

    def apply_operator(self, j, X, transpose=False, timing=None):
        """Side j's matrix as a linear operator (``_operator.product``): ``S @ X``, or ``S.T @ X``, for the host float64
        [n, d] block ``X`` in the caller's order -> float64 [n, d].  A side held in several column blocks is first packed
        into one (``one_block``); a pruned model is answered on the host for its matrix P (``lists``)."""
        from . import _operator
        lists = self.lists(j)
        if lists is not None:
            return _operator.product_lists(*lists, X, transpose)
        with self.one_block(j) as reader:
            return _operator.product(reader, X, transpose, timing)

    def embed_operator(self, j, dim, p, power_iterations, seed, timing=None):
        """The spectral embedding of the symmetric part of side j's matrix (``_operator.embed``) -> (V float64 [n, dim],
        eigenvalues float64 [dim]); where ``apply_operator`` runs, and as it does."""
        from . import _operator
        lists = self.lists(j)
        if lists is not None:
            sym = lambda Q: 0.5 * _operator.product_lists(*lists, Q) + 0.5 * _operator.product_lists(*lists, Q, True)
            return _operator.embed_host(sym, self.n[j], dim, p, power_iterations, seed)
        with self.one_block(j) as reader:
            return _operator.embed(reader, dim, p, power_iterations, seed, timing)

    def _close_readers(self):
        folders, self._folders = self._folders or {}, None
        for f in folders.values():
            f.close()
        readers, self._readers = self._readers or {}, None
        for r in readers.values():
            r.close()


class Reader:
    """The queries of one kept iterate: ``blocks`` as ``engine._iterate_block`` describes them (dicts with ptr, layout,
    stride, rows, cols, col_lo, col_ids), all over the same rows in the solver's order ``order`` (host int32: caller id of
    position r), on ``ops``' stream.  Node ids in, values in the caller's order out; every call ends synchronised."""

    def __init__(self, ops, blocks, order):
        import numpy as np
        self.ops, self.blocks = ops, blocks
        self.q = load()
        self.n = int(order.size)
        self.order = np.ascontiguousarray(order, dtype=np.int32)
        self.inv = np.empty(self.n, dtype=np.int32)           # caller id -> solver position
        self.inv[self.order] = np.arange(self.n, dtype=np.int32)
        self._maps = {}                                        # block index -> device int32 column map (made on first use)

    def _col_map(self, i):
        """Block i's columns in the caller's order: positions (within the block) sorted by caller id, on the device;
        with them the caller ids they go to (host).  One block holding every column: the inverse of the order."""
        import numpy as np
        got = self._maps.get(i)
        if got is None:
            b = self.blocks[i]
            ids = self.order[b["col_lo"]:b["col_lo"] + b["cols"]]
            if np.array_equal(ids, np.arange(ids.size, dtype=np.int32)):
                got = self._maps[i] = (None, ids)              # (the caller's order already: no map)
            else:
                pos = np.ascontiguousarray(np.argsort(ids, kind="stable").astype(np.int32))
                got = self._maps[i] = (self.ops.put(pos), np.ascontiguousarray(ids[pos]))
                self.ops.synchronize()
        return got

    def close(self):
        for ptr, _ in self._maps.values():
            if ptr is not None:
                self.ops._free(ptr)
        self._maps = {}

    # ---- queries ----------------------------------------------------------------------------------------------------
    def rows(self, node_ids, out=None, timing=None):
        """float64 [len(node_ids), n]: those rows of the iterate, columns in the caller's order.  The device block of a
        band holds at most ``SLAB_BYTES``; each band is one kernel per column block and one copy into ``out``.
        ``timing``: a list that receives the kernels' milliseconds (HIP events; serialises the bands)."""
        import numpy as np
        from . import hostpool
        ops, n = self.ops, self.n
        node_ids = np.ascontiguousarray(node_ids, dtype=np.int32)
        n_q = int(node_ids.size)
        if out is None:
            out = hostpool.empty_f64(n_q, n)
        if n_q == 0 or n == 0:
            return out
        whole = len(self.blocks) == 1
        walk = bands(n_q, 8 * n)
        with Scratch(ops) as scratch:
            pos_dev = scratch.put(self.inv[node_ids])
            slab = scratch.malloc(8 * walk.size * n)
            staged = None if whole else np.empty((walk.size, n), dtype=np.float64)
            for q0, m in walk:
                off = 0
                for i, b in enumerate(self.blocks):
                    cmap, _ = self._col_map(i)
                    stage(ops, timing, "rows_ms", lambda: check(self.q.simrank_query_rows(
                        b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], pos_dev + 4 * q0, m, cmap, b["cols"],
                        slab + 8 * off, b["cols"], ops.stream), "simrank_query_rows"))
                    off += m * b["cols"]
                if whole:
                    ops.d2h(out[q0:q0 + m], slab, 8 * m * n)
                else:
                    ops.d2h(staged, slab, 8 * m * n)
                    ops.synchronize()
                    scatter_blocks(out[q0:q0 + m], staged, m, self.blocks, lambda i: self._col_map(i)[1])
        return out

    def pair_values(self, a_ids, b_ids):
        """float64 [len(a_ids)]: S[a][b] per pair of node ids."""
        import numpy as np
        ops = self.ops
        a = self.inv[np.ascontiguousarray(a_ids, dtype=np.int32)]
        bp = self.inv[np.ascontiguousarray(b_ids, dtype=np.int32)]
        m = int(a.size)
        out = np.empty(m, dtype=np.float64)
        if m == 0:
            return out
        with Scratch(ops) as scratch:
            a_dev = scratch.put(a)
            val_dev = scratch.malloc(8 * m)
            for b in self.blocks:
                lo = b["col_lo"]
                mine = np.nonzero((bp >= lo) & (bp < lo + b["cols"]))[0]
                if not mine.size:
                    continue
                if mine.size == m:
                    rows_dev, got = a_dev, out
                else:
                    rows_dev, got = scratch.put(a[mine]), np.empty(mine.size, dtype=np.float64)
                cols_dev = scratch.put(bp[mine] - lo)
                check(self.q.simrank_query_pairs(b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], rows_dev,
                                                 cols_dev, mine.size, val_dev, ops.stream), "simrank_query_pairs")
                ops.d2h(got, val_dev)
                ops.synchronize()
                if got is not out:
                    out[mine] = got
        return out

    def topk_of(self, node_ids, k):
        """(ids int32 [len(node_ids), k], values float64): the k most similar OTHER nodes of each node, caller's ids, in
        the order (value descending, id ascending); id -1 / value 0 past the candidates.  Several column blocks: each
        block's min(k, columns) candidates, merged on the host."""
        import numpy as np
        ops = self.ops
        node_ids = np.ascontiguousarray(node_ids, dtype=np.int32)
        n_q, k = int(node_ids.size), check_k(k)
        if n_q == 0:
            return np.empty((0, k), dtype=np.int32), np.empty((0, k), dtype=np.float64)
        pieces = []
        with Scratch(ops) as scratch:
            pos_dev = scratch.put(self.inv[node_ids])
            ids_dev = scratch.put(node_ids)
            for b in self.blocks:
                kk = int(min(k, b["cols"]))
                if kk < 1:
                    continue
                idx, val = np.empty((n_q, kk), dtype=np.int32), np.empty((n_q, kk), dtype=np.float64)
                idx_dev, val_dev = scratch.malloc(4 * n_q * kk), scratch.malloc(8 * n_q * kk)
                check(self.q.simrank_query_topk(b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], pos_dev,
                                                ids_dev, n_q, b["col_ids"], kk, idx_dev, val_dev, ops.stream),
                      "simrank_query_topk")
                ops.d2h(idx, idx_dev)
                ops.d2h(val, val_dev)
                ops.synchronize()
                pieces.append((idx, val))
        return merge_topk(pieces, k)
