"""ctypes binding of libsimrank_explain.so (include/simrank_explain.h): why two nodes of a kept model are similar.

The update gives a pair (a, b) the double sum of ``S_src[i, j]`` over i in I(a), j in I(b) (``S_src``: the matrix the
update READS, the same side for the directed classes and the other group's for the bipartite ones), times a factor every
term of the pair shares.  ``run`` cuts the pairs into bands whose pieces ``S_src[I(a), I(b)]`` fit the scratch slab and
queues, per band, the three entries: ``simrank_explain_gather`` reads the iterate in place (the block a solver's
``_query.Reader`` describes) into the band, ``simrank_explain_reduce`` adds up the rows, the columns and the whole of
every piece, ``simrank_explain_select`` finds its k largest contributors.  Only the sums, the counts and the k best cross;
the band stays on the device.  A side held in several column blocks (``LocalWorld(P)``) is packed into one temporary block
once per call (the solver's ``one_block`` scope).  A pruned model (a solver with ``lists``) is answered on the host from its
lists, for its matrix P.  No CPU fallback for the matrices: a missing library or device is an error.

The lists go to the device sorted by frame position, so that the position in a list, which is what the selection's order
(value descending, i ascending, j ascending) compares, is the frame's order; ``explain`` hands the marginals back in the
order of the CSR row.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._checks import is_int
from ._companion import Companion
from ._driver import Scratch, join, stage

VERSION = 1              # SIMRANK_EXPLAIN_VERSION of include/simrank_explain.h
MAX_K = 1024             # SIMRANK_EXPLAIN_MAX_K
BIG_TERMS = 1 << 20      # a pair with more terms gets a band (and so a launch shaped for it) of its own

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_explain_version": [],
    "simrank_explain_last_error": [],
    "simrank_explain_gather": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "simrank_explain_reduce": [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    "simrank_explain_select": [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp],
}
_RESTYPES = {"simrank_explain_last_error": C.c_char_p}


class ExplainError(RuntimeError):
    """A call into libsimrank_explain.so failed."""


_c = Companion("explain", VERSION, PROTOTYPES, _RESTYPES, ExplainError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- argument checks: nothing touches a device ---------------------------------------------------------------------------
def check_k(k) -> int:
    if not is_int(k) or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in 1 .. {MAX_K}, not {k!r}")
    return int(k)


def check_max_terms(max_terms) -> int:
    if not is_int(max_terms) or int(max_terms) < 1:
        raise ValueError(f"max_terms must be a positive integer, not {max_terms!r}")
    return int(max_terms)


def check_pairs(a, b):
    """The two label sequences of ``explain`` as lists of equal length."""
    for name, seq in (("a", a), ("b", b)):
        if isinstance(seq, (str, bytes, dict, set, frozenset)) or not hasattr(seq, "__iter__") or not hasattr(seq, "__len__"):
            raise ValueError(f"{name} must be a sequence of fitted labels, not {type(seq).__name__}")
    a, b = list(a), list(b)
    if len(a) != len(b):
        raise ValueError(f"a and b must have the same length ({len(a)} != {len(b)})")
    return a, b


def lists_of(csr, nodes):
    """Row ``u`` of the side's CSR for every u of ``nodes``, in the row's order -> (ptr int64, ids int32)."""
    rowptr, col = np.asarray(csr.rowptr, dtype=np.int64), np.asarray(csr.col, dtype=np.int32)
    return join([col[rowptr[u]:rowptr[u + 1]] for u in np.asarray(nodes, dtype=np.int64)])


def sorted_lists(ptr, ids):
    """Every list sorted ascending (stable) -> (ids sorted, ``back``: sorted[back] is the list in its own order)."""
    seg = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    order = np.lexsort((ids, seg))                            # (stable: equal ids keep their order)
    back = np.empty_like(order)
    back[order] = np.arange(order.size)
    return np.ascontiguousarray(ids[order]), back


def common_of(ptr_a, ids_a, ptr_b, ids_b, alive):
    """int64 [n]: the entries of I(b) that are in I(a) (``simrank_foldin_apply``'s count); 0 where ``alive`` is not."""
    out = np.zeros(ptr_a.size - 1, dtype=np.int64)
    for p in np.flatnonzero(alive):
        out[p] = int(np.isin(ids_b[ptr_b[p]:ptr_b[p + 1]], ids_a[ptr_a[p]:ptr_a[p + 1]]).sum())
    return out


def evidence_of(common):
    """``1 - 2^-min(common, 255)``, as the fold-in's epilogue computes it."""
    return 1.0 - np.ldexp(1.0, -np.minimum(np.asarray(common, dtype=np.int64), 255).astype(np.int64))


def propagated_of(raw, sc_a, sc_b, coef, lbd, evidence):
    """``F * (rowscale[a] * (rowscale[b] * raw))`` in float64 in exactly that association; ``evidence``: float64 [n] or
    None (F = coef)."""
    raw, sc_a, sc_b = (np.asarray(x, dtype=np.float64) for x in (raw, sc_a, sc_b))
    with np.errstate(invalid="ignore", over="ignore"):
        F = np.float64(coef) if evidence is None else ((np.float64(1.0) - np.float64(lbd)) * evidence) * np.float64(coef)
        return F * (sc_a * (sc_b * raw))


def cut_bands(terms, slab_elems):
    """[(first pair, pairs)]: consecutive pairs whose pieces fit ``slab_elems`` doubles together; a pair above
    ``BIG_TERMS`` (or above the slab) stands alone."""
    out, q0, tot = [], 0, 0
    for p, t in enumerate(np.asarray(terms).tolist()):
        alone = t > BIG_TERMS
        if p > q0 and (alone or tot + t > slab_elems):
            out.append((q0, p - q0))
            q0, tot = p, 0
        tot += t
        if alone:
            out.append((p, 1))
            q0, tot = p + 1, 0
    if q0 < len(terms):
        out.append((q0, len(terms) - q0))
    return out


# ---- the host statement: the pruned model's path ------------------------------------------------------------------------------
def reduce_host(piece):
    """(row sums, column sums, raw = the sum of the row sums, contributors) of a float64 piece; every sum from +0.0."""
    with np.errstate(invalid="ignore", over="ignore"):
        rows, cols = piece.sum(axis=1) + 0.0, piece.sum(axis=0) + 0.0
        raw = float(rows.sum() + 0.0)
    return rows, cols, raw, int((~np.isnan(piece) & (piece != 0)).sum())


def best_host(piece, k):
    """(i int32 [k], j int32 [k], value float64 [k]): the k best contributors in the order (value descending, i ascending,
    j ascending); slots past them -1 / -1 / 0.0."""
    flat = piece.ravel()
    cand = np.flatnonzero(~np.isnan(flat) & (flat != 0))
    first = cand[np.lexsort((cand, -flat[cand]))][:k]
    bi, bj, bv = np.full(k, -1, dtype=np.int32), np.full(k, -1, dtype=np.int32), np.zeros(k, dtype=np.float64)
    if first.size:
        bi[:first.size], bj[:first.size] = np.divmod(first, piece.shape[1])
        bv[:first.size] = flat[first]
    return bi, bj, bv


def sub_of_lists(ids, vals, diag, rows, cols):
    """float64 [len(rows), len(cols)] of the matrix P of a pruned model: a row's kept entries, its stored diagonal element,
    +0.0 everywhere else."""
    cols = np.asarray(cols, dtype=np.int64)
    out = np.zeros((len(rows), cols.size), dtype=np.float64)
    for i, r in enumerate(np.asarray(rows).tolist()):
        kept = ids[r] >= 0
        row_ids, row_vals = ids[r][kept].astype(np.int64), vals[r][kept]
        order = np.argsort(row_ids, kind="stable")
        row_ids, row_vals = row_ids[order], row_vals[order]
        if row_ids.size and cols.size:
            at = np.minimum(np.searchsorted(row_ids, cols), row_ids.size - 1)
            hit = row_ids[at] == cols
            out[i, hit] = row_vals[at[hit]]
        out[i, cols == r] = diag[r]
    return out


def run_lists(tables, ptr_a, pos_a, ptr_b, pos_b, k):
    """``run`` for the matrix P of a pruned model (``tables``: ids, vals, diag on the host), on the host."""
    ids, vals, diag = tables
    n = ptr_a.size - 1
    row_sum, col_sum = np.zeros(int(ptr_a[-1])), np.zeros(int(ptr_b[-1]))
    raw, count = np.zeros(n), np.zeros(n, dtype=np.int64)
    bi, bj, bv = np.full((n, k), -1, dtype=np.int32), np.full((n, k), -1, dtype=np.int32), np.zeros((n, k))
    for p in range(n):
        piece = sub_of_lists(ids, vals, diag, pos_a[ptr_a[p]:ptr_a[p + 1]], pos_b[ptr_b[p]:ptr_b[p + 1]])
        row_sum[ptr_a[p]:ptr_a[p + 1]], col_sum[ptr_b[p]:ptr_b[p + 1]], raw[p], count[p] = reduce_host(piece)
        bi[p], bj[p], bv[p] = best_host(piece, k)
    return row_sum, col_sum, raw, count, bi, bj, bv


def pairs_of_lists(tables, ia, ib):
    """float64 [n]: P[a][b] per pair (a's list is read), on the host."""
    ids, vals, diag = tables
    return np.array([sub_of_lists(ids, vals, diag, [a], [b])[0, 0] for a, b in zip(np.asarray(ia).tolist(), np.asarray(ib).tolist())],
                    dtype=np.float64)


# ---- the device path -----------------------------------------------------------------------------------------------------
def run(reader, ptr_a, pos_a, ptr_b, pos_b, k, timing=None):
    """The three entries over every pair, on a reader whose one block holds every column.  ``pos_a`` / ``pos_b``: the lists
    as caller ids of the reader's side (int32, pair after pair, each sorted), ``ptr_a`` / ``ptr_b`` their int64 offsets.
    -> (row_sum float64 [ptr_a[-1]], col_sum float64 [ptr_b[-1]], raw float64 [n], contributors int64 [n], best_i int32
    [n, k], best_j int32 [n, k], best_value float64 [n, k]).  ``timing``: a dict that receives the stages' milliseconds
    (HIP events; serialises them)."""
    from . import _query
    (b,) = reader.blocks
    ops, lib, n = reader.ops, load(), int(ptr_a.size - 1)
    na, nb = np.diff(ptr_a), np.diff(ptr_b)
    terms = na * nb
    row_sum, col_sum = np.zeros(int(ptr_a[-1])), np.zeros(int(ptr_b[-1]))
    raw, count = np.zeros(n), np.zeros(n, dtype=np.int64)
    bi, bj, bv = np.full((n, k), -1, dtype=np.int32), np.full((n, k), -1, dtype=np.int32), np.zeros((n, k))
    if n == 0:
        return row_sum, col_sum, raw, count, bi, bj, bv
    slab_elems = max(_query.SLAB_BYTES // 8, int(terms.max()), 1)
    walk = cut_bands(terms, slab_elems)
    with Scratch(ops) as scratch:
        some = lambda ids: ids if ids.size else np.zeros(1, dtype=np.int32)            # (no block of no bytes)
        a_dev, b_dev = scratch.put(some(reader.inv[pos_a])), scratch.put(some(reader.inv[pos_b]))     # (block positions)
        a_ptr, b_ptr = scratch.put(ptr_a), scratch.put(ptr_b)
        band = scratch.malloc(8 * max(1, max(int(terms[q0:q0 + m].sum()) for q0, m in walk)))
        rs_dev, cs_dev = scratch.malloc(8 * max(1, row_sum.size)), scratch.malloc(8 * max(1, col_sum.size))
        raw_dev, cnt_dev = scratch.malloc(8 * n), scratch.malloc(8 * n)
        bi_dev, bj_dev, bv_dev = scratch.malloc(4 * n * k), scratch.malloc(4 * n * k), scratch.malloc(8 * n * k)
        for q0, m in walk:
            band_ptr = np.zeros(m + 1, dtype=np.int64)
            np.cumsum(terms[q0:q0 + m], out=band_ptr[1:])
            bp = scratch.put(band_ptr)
            ap, bq = a_ptr + 8 * q0, b_ptr + 8 * q0
            stage(ops, timing, "gather_ms", lambda: check(lib.simrank_explain_gather(
                b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], a_dev, ap, b_dev, bq, bp, m,
                int(terms[q0:q0 + m].max()), band, ops.stream), "simrank_explain_gather"))
            stage(ops, timing, "reduce_ms", lambda: check(lib.simrank_explain_reduce(
                band, ap, bq, bp, m, int(na[q0:q0 + m].max()), int(nb[q0:q0 + m].max()), rs_dev, cs_dev, raw_dev + 8 * q0,
                cnt_dev + 8 * q0, ops.stream), "simrank_explain_reduce"))
            stage(ops, timing, "select_ms", lambda: check(lib.simrank_explain_select(
                band, ap, bq, bp, m, k, bi_dev + 4 * q0 * k, bj_dev + 4 * q0 * k, bv_dev + 8 * q0 * k, ops.stream),
                "simrank_explain_select"))
        for host, dev in ((row_sum, rs_dev), (col_sum, cs_dev), (raw, raw_dev), (count, cnt_dev), (bi, bi_dev), (bj, bj_dev),
                          (bv, bv_dev)):
            if host.size:
                ops.d2h(host, dev)
        ops.synchronize()
    return row_sum, col_sum, raw, count, bi, bj, bv


# ---- a solver's side ---------------------------------------------------------------------------------------------------------
def explain(solver, j, src_j, spec, ia, ib, k, max_terms, labels=None, timing=None):
    """What ``_KeptModel.explain`` builds its frames from, for the pairs (``ia``, ``ib``: caller ids of side j) whose
    neighbours (``spec``: side j's ``SideSpec``) live on side ``src_j``: a dict of per-pair arrays (similarity, terms,
    contributors, common, evidence, raw, propagated), the lists (ptr_a, ids_a, ptr_b, ids_b: caller ids of side src_j in
    the CSR rows' order) with their marginals (sum_a, sum_b), and the k best (best_a, best_b: caller ids of side src_j or
    -1, best_value).  ``labels``: names the pair a refusal speaks of."""
    ia, ib = np.asarray(ia, dtype=np.int64), np.asarray(ib, dtype=np.int64)
    n = int(ia.size)
    ptr_a, ids_a = lists_of(spec.csr, ia)
    ptr_b, ids_b = lists_of(spec.csr, ib)
    terms = np.diff(ptr_a) * np.diff(ptr_b)
    over = np.flatnonzero(terms > max_terms)
    if over.size:
        p = int(over[0])
        who = (labels[0][p], labels[1][p]) if labels is not None else (int(ia[p]), int(ib[p]))
        raise ValueError(f"the pair ({who[0]!r}, {who[1]!r}) has {int(np.diff(ptr_a)[p])} x {int(np.diff(ptr_b)[p])} = "
                         f"{int(terms[p])} terms, more than max_terms = {max_terms}")
    sorted_a, back_a = sorted_lists(ptr_a, ids_a)
    sorted_b, back_b = sorted_lists(ptr_b, ids_b)
    tables = solver.lists(src_j)
    if tables is not None:
        out = run_lists(tables, ptr_a, sorted_a, ptr_b, sorted_b, k)
        similarity = pairs_of_lists(tables if src_j == j else solver.lists(j), ia, ib)
    else:
        with solver.one_block(src_j) as reader:
            out = run(reader, ptr_a, sorted_a, ptr_b, sorted_b, k, timing)
        similarity = solver.pair_values(j, ia.astype(np.int32), ib.astype(np.int32))
    row_sum, col_sum, raw, count, bi, bj, bv = out
    scale = np.asarray(spec.rowscale, dtype=np.float64)
    sc_a, sc_b = scale[ia], scale[ib]
    with np.errstate(invalid="ignore"):
        alive = (sc_a > 0) & (sc_b > 0)
    common = common_of(ptr_a, ids_a, ptr_b, ids_b, alive)
    has_evidence = spec.evidence_from is not None
    evidence = evidence_of(common) if has_evidence else np.ones(n, dtype=np.float64)
    propagated = propagated_of(raw, sc_a, sc_b, spec.coef, spec.lbd, evidence if has_evidence else None)
    # the k best: positions in the sorted lists -> caller ids of the source side
    some = bi >= 0
    best_a = np.where(some, sorted_a[np.where(some, ptr_a[:-1][:, None] + bi, 0)] if sorted_a.size else -1, -1)
    best_b = np.where(some, sorted_b[np.where(some, ptr_b[:-1][:, None] + bj, 0)] if sorted_b.size else -1, -1)
    return dict(similarity=similarity, terms=terms.astype(np.int64), contributors=count, common=common, evidence=evidence,
                raw=raw, propagated=propagated, ptr_a=ptr_a, ids_a=ids_a, sum_a=row_sum[back_a], ptr_b=ptr_b, ids_b=ids_b,
                sum_b=col_sum[back_b], best_a=best_a, best_b=best_b, best_value=bv)
