"""ctypes binding of libsimrank_foldin.so (include/simrank_foldin.h): similarities of nodes that were NOT in the fitted
graph, from a model that stays on the device.

A companion of libsimrank_hip.so with its own header, version and binding, as ``_query.py`` is.  ``prepare`` checks and
normalises the arguments of ``fold_in`` on the host (no device); ``Folder`` holds one side's CSR on the device and runs
the two stages over the column blocks of the kept iterate a ``_query.Reader`` describes.  No CPU fallback: a missing
library or device is an error.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _driver
from ._companion import ROWMAJOR_F64, Companion
from ._driver import bands, id_lists, join

VERSION = 1              # SIMRANK_FOLDIN_VERSION of include/simrank_foldin.h
TILE = 32                # SIMRANK_FOLDIN_TILE: new nodes per gather / apply
KEEP_BYTES = 32 << 20    # a scratch buffer larger than this is freed at the end of the call that needed it
MAX_TOP_K = 1024        # simrank_query_topk's limit on k (include/simrank_query.h)
LONG_ROW = 256           # SIMRANK_FOLDIN_LONG_ROW: CSR rows with more entries are listed for the workgroup-per-row kernel

_vp, _i64, _i32, _f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_foldin_version": [],
    "simrank_foldin_last_error": [],
    "simrank_foldin_t_bytes": [_i32, _i64],
    "simrank_foldin_alloc": [_vp, C.c_size_t],
    "simrank_foldin_free": [_vp],
    "simrank_foldin_gather": [_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _i64, _vp],
    "simrank_foldin_member": [_vp, _vp, _vp, _i32, _vp, _i64, _vp],
    "simrank_foldin_apply": [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _i32, _vp, _f64, _f64, _vp, _i64, _i32, _vp, _i64,
                             _vp],
}
_RESTYPES = {"simrank_foldin_last_error": C.c_char_p, "simrank_foldin_t_bytes": C.c_int64}


class FoldInError(RuntimeError):
    """A call into libsimrank_foldin.so failed."""


_c = Companion("foldin", VERSION, PROTOTYPES, _RESTYPES, FoldInError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- the host half: arguments ----------------------------------------------------------------------------------------
def side_of(n_sides: int, group):
    """Index of the side ``group`` names: None | 1 for the one-matrix classes, 1 | 2 for the bipartite ones."""
    if n_sides == 1:
        if group not in (None, 1):
            raise ValueError(f"this class has one node group: group must be None or 1, not {group!r}")
        return 0
    if group not in (1, 2):
        raise ValueError(f"group must be 1 or 2, not {group!r}")
    return group - 1


def check_strict_group(n_sides: int, side: int, strict_evidence: bool):
    """A bipartite SimRank++ fit with ``strict_reference=True`` gates its group-2 update by ``Evidence_N1`` (the
    reference's quirk), a matrix over group-1 nodes: it has no row for a new group-2 node."""
    if n_sides == 2 and side == 1 and strict_evidence:
        raise ValueError("fold_in(group=2) on a fit with strict_reference=True: that fit gates the group-2 update by "
                         "Evidence_N1, which has no row for a new group-2 node; refit with strict_reference=False")


def row_scales(lengths, weights, weighted: bool) -> np.ndarray:
    """float64 [n_new]: the scale of every entry of a new node's row, with the reference's quirks (``_create_graph``):
    unweighted 1 / len(list); weighted 1 / sum(weights) for EVERY entry (the weight itself is not used); 0 where that is
    not finite (an empty list, a zero sum)."""
    if weighted:
        total = np.array([float(np.sum(np.asarray(w, dtype=np.float64))) if len(w) else 0.0 for w in weights],
                         dtype=np.float64)
    else:
        total = np.asarray(lengths, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 1.0 / total
    r[~np.isfinite(r)] = 0.0
    return r


def prepare(neighbors, index, *, n_out: int, weighted: bool, has_prior: bool, weights=None, prior=None, names=None,
            top_k=None):
    """The arguments of ``fold_in`` checked and normalised on the host, before any device work.  ``index``: pandas Index
    of the SOURCE side's labels in the dense frame's order.  -> (lists: int32 arrays of source ids, w: float64 [n_new],
    prior: float64 [n_new, n_out] C-contiguous or None, names: list or None, k or None)."""
    from ._query import check_k
    lists = id_lists("neighbors", neighbors, index, unique=True, each="new node")
    n_new = len(lists)
    if weighted:
        if weights is None:
            raise ValueError("this model was fitted with weighted=True: fold_in needs weights (one sequence per new node)")
        if not hasattr(weights, "__len__") or len(weights) != n_new:
            raise ValueError(f"weights must have one sequence per new node ({n_new})")
        weights = [np.asarray(w, dtype=np.float64).ravel() for w in weights]
        for q, (w, ids) in enumerate(zip(weights, lists)):
            if w.size != ids.size:
                raise ValueError(f"weights[{q}] has {w.size} entries for {ids.size} neighbours")
    elif weights is not None:
        raise ValueError("this model was fitted with weighted=False: fold_in takes no weights")
    w = row_scales([ids.size for ids in lists], weights, weighted)
    if prior is not None:
        if not has_prior:
            raise ValueError("prior needs a class fitted with a prior (AprioriSimRank / BipartitleAprioriSimRank)")
        prior = np.asarray(prior)
        if prior.shape != (n_new, n_out):
            raise ValueError(f"prior must have shape ({n_new}, {n_out}): one row per new node in the dense frame's column "
                             f"order, not {prior.shape}")
        prior = np.ascontiguousarray(prior, dtype=np.float64)
    if names is not None:
        names = list(names)
        if len(names) != n_new:
            raise ValueError(f"names must have one entry per new node ({n_new}), not {len(names)}")
    k = None if top_k is None else check_k(top_k)
    if k is not None and min(k, max(1, n_out)) > MAX_TOP_K:
        raise ValueError(f"top_k must be at most {MAX_TOP_K} (the device selection's limit; ask for the dense frame "
                         f"instead), not {k}")
    return lists, w, prior, names, k


# ---- the device half -------------------------------------------------------------------------------------------------
class Folder:
    """One side of a kept model as ``fold_in`` needs it: the CSR of the fitted nodes the new ones join (rows = those
    nodes, columns = SOURCE nodes; ids in the dense frame's order), its per-row scale in float64 and the list of its long
    rows, uploaded once; ``run`` reads the source side's iterate in place through ``reader`` (``_query.Reader``)."""

    def __init__(self, reader, csr, scale, coef, lbd, evidence: bool):
        self.f = load()
        self.reader, self.ops = reader, reader.ops
        self.n_out, self.n_src = int(csr.n_rows), int(csr.n_cols)
        if reader.n != self.n_src:
            raise ValueError(f"the iterate has {reader.n} nodes, the pattern {self.n_src} columns")
        self.coef, self.lbd, self.evidence = float(coef), float(lbd), bool(evidence)
        rowptr = np.ascontiguousarray(csr.rowptr, dtype=np.int32)
        col = np.ascontiguousarray(csr.col, dtype=np.int32)
        if col.size and (int(col.min()) < 0 or int(col.max()) >= self.n_src):
            raise ValueError("the pattern names a column outside the source nodes")
        self.nnz = int(col.size)
        long_rows = np.ascontiguousarray(np.nonzero(np.diff(rowptr) > LONG_ROW)[0], dtype=np.int32)
        self.n_long = int(long_rows.size)
        self.layout = reader.blocks[0]["layout"] if reader.blocks else 0
        self._bufs = {}                                   # name -> (device pointer, bytes): grown on demand, kept
        self.rowptr = self._put("rowptr", rowptr)
        self.col = self._put("col", col)
        self.scale = self._put("scale", np.ascontiguousarray(scale, dtype=np.float64))
        self.long_rows = self._put("long_rows", long_rows) if self.n_long else None

    # Device memory of a fold-in is the library's own (simrank_foldin_alloc: hipMalloc), not the main library's block pool:
    # it is held between calls (no allocation on the path of a query) and goes back to the driver at release, so a model
    # that folded in leaves the pool as one that never did.
    def _buf(self, name, nbytes):
        ptr, cap = self._bufs.get(name, (None, 0))
        if cap < nbytes:
            self.ops.synchronize()
            if ptr:
                check(self.f.simrank_foldin_free(ptr), "simrank_foldin_free")
            self._bufs.pop(name, None)
            p = C.c_void_p()
            check(self.f.simrank_foldin_alloc(C.byref(p), max(256, int(nbytes))), "simrank_foldin_alloc")
            ptr = p.value
            self._bufs[name] = (ptr, max(256, int(nbytes)))
        return ptr

    def _put(self, name, host):
        ptr = self._buf(name, host.nbytes)
        self.ops.h2d(ptr, host)
        return ptr

    def _drop(self, keep=()):
        self.ops.synchronize()
        for name in [n for n in self._bufs if n not in keep]:
            check(self.f.simrank_foldin_free(self._bufs.pop(name)[0]), "simrank_foldin_free")

    def close(self):
        self._drop()

    def run(self, lists, w, prior=None, top_k=None, timing=None):
        """``lists``: int32 arrays of source ids, ``w`` float64 [n_new], ``prior`` float64 [n_new, n_out] or None ->
        float64 [n_new, n_out], or with ``top_k`` (ids int32 [n_new, k], values float64 [n_new, k]) selected on the
        device.  ``timing``: a dict that receives the milliseconds of the stages (HIP events; serialises them)."""
        from . import _query, hostpool
        ops, rd, n_out, n_src = self.ops, self.reader, self.n_out, self.n_src
        n_new = len(lists)
        k = None if top_k is None else int(min(top_k, max(1, n_out)))
        if k is None:
            result = hostpool.empty_f64(n_new, n_out)
        else:
            result = (np.full((n_new, k), -1, dtype=np.int32), np.zeros((n_new, k), dtype=np.float64))
        if n_new == 0 or n_out == 0:
            return result
        walk = bands(n_new, 8 * n_out, unit=TILE)             # (bands are whole tiles)
        t_bytes = self.f.simrank_foldin_t_bytes(self.layout, n_src)
        dev, up = self._buf, self._put
        stage = functools.partial(_driver.stage, ops, timing)
        try:
            T = dev("T", t_bytes)
            member = dev("member", 4 * n_src) if self.evidence else None
            slab = dev("slab", 8 * walk.size * n_out)
            # the lists of every new node, once: offsets, source ids, and the iterate's row positions of those ids
            ptr, ids = join(lists)
            ids_dev, pos_dev = up("ids", ids), up("pos", np.ascontiguousarray(rd.inv[ids]))
            w_dev = up("w", np.ascontiguousarray(w, dtype=np.float64))
            # (every tile's offsets from its own first entry, TILE + 1 per tile; bands are whole tiles)
            n_tiles = -(-n_new // TILE)
            rel = np.zeros((n_tiles, TILE + 1), dtype=np.int32)
            for ti in range(n_tiles):
                seg = ptr[ti * TILE:min(n_new, (ti + 1) * TILE) + 1]
                rel[ti, :seg.size] = seg - seg[0]
            rel_dev = up("rel", rel)
            for q0, m in walk:
                prior_dev = up("prior", prior[q0:q0 + m]) if prior is not None else None
                for t0 in range(q0, q0 + m, TILE):
                    nt = min(TILE, q0 + m - t0)
                    lp = rel_dev + 4 * (TILE + 1) * (t0 // TILE)
                    off = 4 * int(ptr[t0])
                    for b in rd.blocks:
                        stage("gather_ms", lambda b=b: check(self.f.simrank_foldin_gather(
                            b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], b["col_ids"], b["col_lo"], lp,
                            pos_dev + off, w_dev + 8 * t0, nt, T, n_src, ops.stream), "simrank_foldin_gather"))
                    if member is not None:
                        stage("member_ms", lambda: check(self.f.simrank_foldin_member(
                            lp, ids_dev + off, w_dev + 8 * t0, nt, member, n_src, ops.stream), "simrank_foldin_member"))
                    stage("apply_ms", lambda: check(self.f.simrank_foldin_apply(
                        self.rowptr, self.col, self.scale, n_out, n_src, self.long_rows, self.n_long, T, self.layout,
                        member, self.coef, self.lbd, None if prior_dev is None else prior_dev + 8 * (t0 - q0) * n_out,
                        n_out, nt, slab + 8 * (t0 - q0) * n_out, n_out, ops.stream), "simrank_foldin_apply"))
                if k is None:
                    ops.d2h(result[q0:q0 + m], slab)
                else:
                    # the k best of each new row on the device: the result as a float64 row-major block, positions = ids,
                    # no node excluded (a new node has no diagonal)
                    rows = up("rows", np.arange(m, dtype=np.int32))
                    nobody = up("nobody", np.full(m, -1, dtype=np.int32))
                    idx_dev, val_dev = dev("idx", 4 * m * k), dev("val", 8 * m * k)
                    stage("topk_ms", lambda: _query.check(rd.q.simrank_query_topk(
                        slab, ROWMAJOR_F64, n_out, m, n_out, rows, nobody, m, None, k, idx_dev, val_dev,
                        ops.stream), "simrank_query_topk"))
                    ops.d2h(result[0][q0:q0 + m], idx_dev)
                    ops.d2h(result[1][q0:q0 + m], val_dev)
                ops.synchronize()
        finally:
            # (what a large request needed does not stay with the model)
            big = [n for n, (_, cap) in self._bufs.items() if cap > KEEP_BYTES and n not in ("rowptr", "col", "scale")]
            if big:
                self._drop(keep=[n for n in self._bufs if n not in big])
            else:
                ops.synchronize()
        return result
