"""A float64 NumPy statement of ``fold_in`` on dense matrices, and the lists the tests feed it.

    s(q, b) = [(1 - lbd)] * E(q, b) * C * sum_{i in I_q} w_q * sum_{j in I(b)} S[i, j] * W[b, j]   [+ lbd * prior(q, b)]

the body of the reference's update (oracle ``update``) for ONE new row g_q = w_q . [j in I_q] of the graph, with S, W and
the pattern of the fitted nodes held fixed.  tests/test_foldin_cpu.py proves it against the reference's own loop."""
import numpy as np


def row_scales(lengths, weights=None):
    """1 / len(list), or 1 / sum(weights) per new node; 0 where that is not finite (the oracle's ``_inv_or_zero``)."""
    total = (np.asarray(lengths, dtype=np.float64) if weights is None
             else np.array([float(np.sum(np.asarray(w, dtype=np.float64))) for w in weights], dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 1.0 / total
    r[~np.isfinite(r)] = 0.0
    return r


def fold_in_ref(lists, S, W, coef, w=None, pattern=None, lbd=None, prior=None):
    """float64 [len(lists), W.shape[0]].  ``lists``: integer positions (rows of ``S``) per new node; ``S`` [n_src, n_src]
    the similarities the update reads; ``W`` [n_out, n_src] the weighted graph of the fitted nodes the new ones join;
    ``w``: row scale per new node (default 1 / len); ``pattern``: the graph whose entries > 0 count as evidence (the
    SimRank++ classes: the oracle's ``G``), or None; ``lbd`` with ``prior`` [n_new, n_out] or None (zeros)."""
    S, W = np.asarray(S, dtype=np.float64), np.asarray(W, dtype=np.float64)
    n_out, n_src = W.shape
    assert S.shape == (n_src, n_src)
    if w is None:
        w = row_scales([len(l) for l in lists])
    out = np.zeros((len(lists), n_out))
    for q, l in enumerate(lists):
        g = np.zeros(n_src)
        g[np.asarray(l, dtype=np.int64)] = w[q]
        prod = g.dot(S).dot(W.T)
        if pattern is not None:
            common = np.rint((g > 0).astype(np.float64) @ (np.asarray(pattern) > 0).astype(np.float64).T)
            E = 1 - 0.5 ** common                                          # the oracle's ``evidence`` for the new row
        if lbd is not None:
            new = (1 - lbd) * E * coef * prod                              # SimRank.py:453
            if prior is not None:
                new = new + lbd * np.asarray(prior, dtype=np.float64)[q]
        elif pattern is not None:
            new = E * coef * prod                                          # :361
        else:
            new = coef * prod                                              # :139
        out[q] = new
    return out


def own_lists(G):
    """(lists, w) of the fitted nodes themselves, from a dense graph of the oracle (``G`` [n_out, n_src]): row a's non-zero
    positions and its (single) entry value.  A row the reference scaled to zero has an empty list and scale 0."""
    lists, w = [], np.zeros(G.shape[0])
    for a in range(G.shape[0]):
        nz = np.nonzero(G[a])[0]
        lists.append(nz)
        if nz.size:
            w[a] = G[a, nz[0]]
            assert np.all(G[a, nz] == w[a])
    return lists, w


def edge_lists(frame, to_col, from_col, weight_col=None):
    """{target label: (list of source labels, list of weights or None)} of an edge list, in the frame's row order."""
    out = {}
    for key, grp in frame.groupby(to_col, sort=False):
        out[key] = (list(grp[from_col]), None if weight_col is None else list(grp[weight_col]))
    return out


def tolerance(lists, W, u):
    """The derived bound of a fold-in summed in any order on non-negative terms: per new node,
    (|I_q| + max_b |I(b)| + 8) * u relative (u: unit roundoff of the sums)."""
    longest = int((np.asarray(W) != 0).sum(axis=1).max()) if np.asarray(W).size else 0
    return np.array([(len(l) + longest + 8) * u for l in lists])


def topk_ref(dense, k):
    """(positions int [n, k'], values) of the k best per row: value descending, position ascending; k' = min(k, N)."""
    dense = np.asarray(dense, dtype=np.float64)
    k = min(k, dense.shape[1])
    idx = np.stack([np.lexsort((np.arange(dense.shape[1]), -row))[:k] for row in dense]) if len(dense) else \
        np.empty((0, k), dtype=np.int64)
    return idx, np.take_along_axis(dense, idx, axis=1) if len(dense) else np.empty((0, k))


def run_oracle(g, **override):
    """The oracle on a golden's inputs (``tests.conftest.Golden``) with some keyword arguments replaced."""
    from oracle import simrank_oracle as O
    kw = dict(g.kwargs, **override)
    strict = kw.pop("strict_reference", True)
    if g.cls == "SimRank":
        return O.fit_simrank(g.frame, **kw)
    if g.cls == "SimRankPP":
        return O.fit_simrank_pp(g.frame, **kw)
    if g.cls == "AprioriSimRank":
        return O.fit_simrank_pp(g.frame, apriori=g.args[0], **kw)
    if g.cls == "BipartiteSimRank":
        return O.fit_bipartite(g.frame, **kw)
    if g.cls == "BipartiteSimRankPP":
        return O.fit_bipartite_pp(g.frame, strict_reference=strict, **kw)
    if g.cls == "BipartitleAprioriSimRank":
        return O.fit_bipartite_pp(g.frame, strict_reference=strict, apriori1=g.args[0], apriori2=g.args[1], **kw)
    raise AssertionError(g.cls)


def sides_of(g, r, kwargs=None):
    """What ``fold_in_ref`` needs per group of an oracle result ``r`` of golden ``g``: a list of dicts (group, S_key of the
    matrix the update READS, W, coef, pattern or None, lbd or None, prior or None, out_key of the matrix it WRITES)."""
    kw = dict(g.kwargs, **(kwargs or {}))
    pp = g.cls not in ("SimRank", "BipartiteSimRank")
    if "S" in r:
        lbd = kw.get("lbd", 0.5) if g.cls == "AprioriSimRank" else None
        return [dict(group=None, reads="S", writes="S", G=r["G"], W=r["W"] if pp else r["G"], coef=kw.get("C", 0.8),
                     pattern=r["G"] if pp else None, lbd=lbd, prior=g.args[0] if lbd is not None else None)]
    ap = g.cls == "BipartitleAprioriSimRank"
    return [dict(group=1, reads="S2", writes="S1", G=r["G12"], W=r["W1"] if pp else r["G12"], coef=kw.get("C1", 0.8),
                 pattern=r["G12"] if pp else None, lbd=kw.get("lbd1", 0.5) if ap else None, prior=g.args[0] if ap else None),
            dict(group=2, reads="S1", writes="S2", G=r["G21"], W=r["W2"] if pp else r["G21"], coef=kw.get("C2", 0.8),
                 pattern=r["G21"] if pp else None, lbd=kw.get("lbd2", 0.5) if ap else None, prior=g.args[1] if ap else None)]
