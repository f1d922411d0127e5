"""A NumPy float64 statement of ``explain`` and of the three entries of include/simrank_explain.h, with ``math.fsum`` for
the exact sums.

    next(a, b) = F(a, b) * rowscale[a] * rowscale[b] * sum_{i in I(a)} sum_{j in I(b)} S_src[i, j]      (a != b)

``block_gather`` / ``reduce`` / ``best`` are the entries on one piece; ``explain_ref`` builds what the three frames of
``model.explain`` hold, from a dense matrix or from ``model.rows``.  Written for reading, not for speed."""
import math

import numpy as np


def block_gather(A, a_pos, b_col):
    """float64 [len(a_pos), len(b_col)]: A[a_pos[i], b_col[j]]; NaN where either position is outside the block."""
    n_rows, n_cols = A.shape
    a_pos, b_col = np.asarray(a_pos, dtype=np.int64), np.asarray(b_col, dtype=np.int64)
    out = np.full((a_pos.size, b_col.size), np.nan)
    ok_r, ok_c = (a_pos >= 0) & (a_pos < n_rows), (b_col >= 0) & (b_col < n_cols)
    if ok_r.any() and ok_c.any():
        out[np.ix_(ok_r, ok_c)] = A[np.ix_(a_pos[ok_r], b_col[ok_c])]
    return out


def _fsum(x):
    """The exact sum, rounded once, from +0.0; NaN when a term is."""
    x = np.asarray(x, dtype=np.float64).ravel()
    return float("nan") if np.isnan(x).any() else 0.0 + math.fsum(x.tolist())


def contributors(band):
    band = np.asarray(band, dtype=np.float64)
    return ~np.isnan(band) & (band != 0)


def reduce(band):
    """(row sums [na], column sums [nb], raw, contributor count) of a piece, every sum exact and rounded once."""
    band = np.asarray(band, dtype=np.float64)
    rows = np.array([_fsum(r) for r in band], dtype=np.float64)
    cols = np.array([_fsum(c) for c in band.T], dtype=np.float64)
    return rows, cols, _fsum(band), int(contributors(band).sum())


def bounds(band):
    """(per row, per column, for raw): ``m * 2^-52 * sum |x|`` over the m terms of each sum (NaN where a term is)."""
    mag = np.abs(np.asarray(band, dtype=np.float64))
    na, nb = mag.shape
    return (np.array([nb * 2.0 ** -52 * _fsum(r) for r in mag]), np.array([na * 2.0 ** -52 * _fsum(c) for c in mag.T]),
            na * nb * 2.0 ** -52 * _fsum(mag))


def best(band, k):
    """(i int32 [k], j int32 [k], value float64 [k]): the k largest contributors in the total order (value descending, i
    ascending, j ascending); NaN and both zeros are never listed; slots past them hold -1 / -1 / 0.0."""
    band = np.asarray(band, dtype=np.float64)
    ii, jj = np.nonzero(contributors(band))
    order = np.lexsort((jj, ii, -band[ii, jj]))[:k]
    bi, bj, bv = np.full(k, -1, dtype=np.int32), np.full(k, -1, dtype=np.int32), np.zeros(k, dtype=np.float64)
    bi[:order.size], bj[:order.size], bv[:order.size] = ii[order], jj[order], band[ii[order], jj[order]]
    return bi, bj, bv


def evidence_of(common):
    return 1.0 - 2.0 ** -min(int(common), 255)


def propagated(raw, sc_a, sc_b, coef, lbd, evidence):
    """``F * (rowscale[a] * (rowscale[b] * raw))``: every step one IEEE double operation; ``evidence``: E or None."""
    F = float(coef) if evidence is None else ((1.0 - float(lbd)) * float(evidence)) * float(coef)
    return F * (float(sc_a) * (float(sc_b) * float(raw)))


def explain_ref(read_rows, csr, rowscale, coef, lbd, evidence, pairs, k):
    """``read_rows``: the dense matrix the update READS (float64 [n_src, n_src]), or a function (list of source ids) ->
    their rows; ``csr``: the side's pattern (rowptr, col: source ids); ``evidence``: whether the class gates by common
    neighbours; ``pairs``: [(a, b)] ids of the side.  -> (pairs, terms, neighbors):

        pairs       dict of arrays: terms, contributors, common (int64), evidence, raw, propagated (float64), and
                    raw_bound: the derived bound of raw, abs: the exact sum of the terms' magnitudes
        terms       [(pair, rank, via_a, via_b, similarity)] source ids; share is similarity / raw of the CALLER's raw
        neighbors   [(pair, "a" | "b", neighbor, sum, bound)] in the order of the CSR rows
    """
    rowptr, col = np.asarray(csr.rowptr, dtype=np.int64), np.asarray(csr.col, dtype=np.int64)
    rows_of = (lambda ids: np.asarray(read_rows, dtype=np.float64)[ids]) if not callable(read_rows) else read_rows
    scale = np.asarray(rowscale, dtype=np.float64)
    out = {name: [] for name in ("terms", "contributors", "common", "evidence", "raw", "propagated", "raw_bound", "abs")}
    terms, neighbors = [], []
    for p, (a, b) in enumerate(pairs):
        la, lb = col[rowptr[a]:rowptr[a + 1]], col[rowptr[b]:rowptr[b + 1]]
        piece = np.asarray(rows_of(la), dtype=np.float64).reshape(la.size, -1)[:, lb] if la.size else np.zeros((0, lb.size))
        row_sum, col_sum, raw, count = reduce(piece)
        row_bound, col_bound, raw_bound = bounds(piece)
        common = int(np.isin(lb, la).sum()) if scale[a] > 0 and scale[b] > 0 else 0
        E = evidence_of(common) if evidence else 1.0
        for name, v in (("terms", la.size * lb.size), ("contributors", count), ("common", common), ("evidence", E),
                        ("raw", raw), ("propagated", propagated(raw, scale[a], scale[b], coef, lbd, E if evidence else None)),
                        ("raw_bound", raw_bound), ("abs", _fsum(np.abs(piece)))):
            out[name].append(v)
        # the k best in the order (value descending, via_a's frame position ascending, via_b's ascending): the lists sorted
        sa, sb = np.argsort(la, kind="stable"), np.argsort(lb, kind="stable")
        bi, bj, bv = best(piece[np.ix_(sa, sb)], k)
        terms += [(p, r + 1, int(la[sa[i]]), int(lb[sb[j]]), float(v)) for r, (i, j, v) in enumerate(zip(bi, bj, bv)) if i >= 0]
        neighbors += [(p, "a", int(i), float(s), float(t)) for i, s, t in zip(la, row_sum, row_bound)]
        neighbors += [(p, "b", int(j), float(s), float(t)) for j, s, t in zip(lb, col_sum, col_bound)]
    ints = ("terms", "contributors", "common")
    return {n: np.array(v, dtype=np.int64 if n in ints else np.float64) for n, v in out.items()}, terms, neighbors
