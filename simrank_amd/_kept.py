"""What ``fit(keep=True)`` leaves on an estimator (``_KeptModel``): the solver with its iterate on the device, and every
query on it, from ``rows`` to ``explain``.  ``estimators`` holds the six classes and ``fit``; this module holds what they
inherit once a model is kept, and the frame helpers the two share.  A query of one side goes to the solver
(``_query.SolverQueries``) or to the side function of its binding (``_cluster.roots``, ``_groups.scores``, ...), which
decide there, once, whether the model is pruned (``lists``) or held in several column blocks (``one_block``).
"""
from __future__ import annotations

import contextlib

import numpy as np
import pandas as pd



def _square_frame(S, labels):
    """``pd.DataFrame(S, index=labels, columns=labels)`` (SimRank.py:141) with the labels converted once instead of twice
    (7 ms for 32768 of them); the two axes are separate Index objects, as the reference's."""
    idx = pd.Index(labels)
    return pd.DataFrame(S, index=idx, columns=idx.copy())


def _long_frame(first, value, who, out_index, idx, val, keep_rows=None):
    """Long frame (``first``, rank, neighbor, ``value``) of a device selection ``idx`` / ``val`` [n, k] (id -1: an empty
    slot, dropped): ``who`` the label of every row of ``idx``, ``out_index`` the labels the ids stand for; ``keep_rows``:
    per row whether it is listed at all."""
    n, kk = idx.shape
    keep = idx.ravel() >= 0
    if keep_rows is not None:
        keep &= np.repeat(np.asarray(keep_rows, dtype=bool), kk)
    return pd.DataFrame({
        first: who.take(np.repeat(np.arange(n), kk)[keep]),
        "rank": np.tile(np.arange(1, kk + 1), n)[keep],
        "neighbor": out_index.take(idx.ravel()[keep]),
        value: val.ravel()[keep]})


def _diverse_frame(first, who, out_index, idx, score, pen, val, keep_rows=None):
    """``_long_frame`` of a diversified selection: (``first``, rank, neighbor, score) and the two float64 columns
    ``penalty`` and ``value`` of every pick; ``rank`` is the order of picking."""
    n, kk = idx.shape
    keep = idx.ravel() >= 0
    if keep_rows is not None:
        keep &= np.repeat(np.asarray(keep_rows, dtype=bool), kk)
    frame = _long_frame(first, "score", who, out_index, idx, score, keep_rows)
    frame["penalty"] = pen.ravel()[keep]
    frame["value"] = val.ravel()[keep]
    return frame


def _topk_frame(solver, j, k, labels):
    """Long-format hand-back: one row per (node, rank) with the k most similar OTHER nodes."""
    lab = pd.Index(labels)
    return _long_frame("node", "similarity", lab, lab, *solver.topk(j, k))


def _check_pairs_args(min_similarity, max_pairs):
    """``min_similarity`` / ``max_pairs`` checked before any device work (ValueError)."""
    if min_similarity is not None:
        from ._select import check_threshold
        check_threshold(min_similarity, max_pairs)


def _pairs_frame(solver, j, t, max_pairs, labels):
    """Long-format hand-back: one row per (node, neighbor) pair of different nodes with similarity >= t."""
    if not hasattr(solver, "pairs"):
        raise ValueError("min_similarity needs a solver behind the C ABI (fit on one GPU, LocalWorld(P) or an RCCL "
                         "TorchWorld)")
    got = solver.pairs(j, t, max_pairs)
    if got is None:                       # multi-process world, root-only hand-back: not the root
        return None
    offsets, ids, vals = got
    lab = pd.Index(labels)
    return pd.DataFrame({
        "node": lab.take(np.repeat(np.arange(len(lab)), np.diff(offsets))),
        "neighbor": lab.take(ids.astype(np.intp)),
        "similarity": vals.astype(np.float64)})



class _KeptModel:
    """What ``fit(keep=True)`` leaves on an estimator: the solver with its iterate on the device, and the queries on it.
    ``nodes`` are the caller's labels, in any order, repeats allowed (KeyError for an unknown one); bipartite classes take
    ``group=1 | 2`` and label as their ``fit`` did.  Every value is bit-identical to the same element of what the same
    ``fit`` without ``keep`` returns.  The model holds its whole plan (three N x N matrices per side plus prior and
    counts) until ``release()``, the end of a ``with`` block, a second ``fit`` or the estimator's collection."""

    _model = None              # (solver, [(side j, labels)]) of a kept fit
    _model_released = False

    def _keep(self, solver, sides):
        self._model = (solver, [(j, list(lab) if not isinstance(lab, list) else lab) for j, lab in sides])
        self._model_released = False
        self._indexes = {}
        return self

    def _solver_sides(self):
        """(solver, [(side j, labels)]) of the kept model; the RuntimeError that says why there is none."""
        if self._model is None:
            if self._model_released:
                raise RuntimeError("the kept model was released (release(), the end of a with block, or a second fit): "
                                   "fit(keep=True) again")
            raise RuntimeError("there is no kept model: call fit(..., keep=True) first")
        return self._model

    def _kept(self, group=None):
        solver, sides = self._solver_sides()
        if len(sides) == 1:
            if group not in (None, 1):
                raise ValueError(f"this class has one node group: group must be None or 1, not {group!r}")
            s = 0
        else:
            if group not in (1, 2):
                raise ValueError(f"group must be 1 or 2, not {group!r}")
            s = group - 1
        j, labels = sides[s]
        return solver, j, labels

    def _ids(self, s, labels, nodes):
        """The caller ids (positions in the dense frame's label order) of ``nodes``."""
        index = self._indexes.get(s)
        if index is None:
            index = self._indexes[s] = pd.Index(labels)
        nodes = list(nodes)
        if not nodes:
            return index, np.empty(0, dtype=np.int32)
        ids = index.get_indexer(pd.Index(nodes, dtype=object) if index.dtype == object else pd.Index(nodes))
        if (ids < 0).any():
            raise KeyError(nodes[int(np.argmax(ids < 0))])
        return index, ids.astype(np.int32)

    @staticmethod
    def _strict(solver) -> bool:
        """A bipartite fit with ``strict_reference=True``: its group-2 update is gated by group 1's evidence."""
        specs = getattr(solver, "specs", None)
        return bool(specs and len(specs) == 2 and specs[1].evidence_from is not None
                    and specs[1].evidence_from is specs[0].csr)

    def _across(self, group, gate=False):
        """The lookup of the queries that read the matrix of the side a node's neighbours live on (the same side for the
        one-matrix classes, the other group's for the bipartite ones) -> (solver, side, j, the side's pandas Index, src_j,
        the source side's Index).  ``gate``: refuse group 2 of a strict fit, as ``fold_in`` does."""
        from . import _foldin
        solver, sides = self._solver_sides()
        side = _foldin.side_of(len(sides), group)
        if gate:
            _foldin.check_strict_group(len(sides), side, self._strict(solver))
        j, labels = sides[side]
        src_j, src_labels = sides[len(sides) - 1 - side]
        return solver, side, j, self._ids(j, labels, [])[0], src_j, self._ids(src_j, src_labels, [])[0]

    def rows(self, nodes, group=None):
        """DataFrame, index = ``nodes`` as given, columns = the dense frame's: ``dense.loc[nodes]``, read on the device."""
        solver, j, labels = self._kept(group)
        index, ids = self._ids(j, labels, nodes)
        return pd.DataFrame(solver.rows(j, ids), index=index.take(ids), columns=index.copy())

    def similarity(self, a, b, group=None):
        """float64 ndarray: element i is ``dense.at[a[i], b[i]]`` (``a`` and ``b`` label sequences of equal length)."""
        a, b = list(a), list(b)
        if len(a) != len(b):
            raise ValueError(f"a and b must have the same length ({len(a)} != {len(b)})")
        solver, j, labels = self._kept(group)
        _, ia = self._ids(j, labels, a)
        _, ib = self._ids(j, labels, b)
        return solver.pair_values(j, ia, ib)

    def most_similar(self, nodes, k, group=None, among=None, exclude=None):
        """Long frame (node, rank, neighbor, similarity): the rows of the ``fit(top_k=k)`` frame of the nodes in ``nodes``,
        blocks in the order of ``nodes``.

        ``among`` / ``exclude``: None, or a non-string iterable of fitted labels of the group, shared by all queries
        (duplicates collapse, the order does not matter, empty is allowed; a str, bytes or a scalar is a ValueError, an
        unknown label a KeyError).  The candidates of node a are then ``(among or every node) - exclude - {a}``, ranked
        in the same order (similarity descending, label position ascending; NaN never listed); a node with fewer than
        k candidates gets fewer rows, an empty candidate set a frame of zero rows.  ``k`` is clamped to ``max(1, |among -
        exclude|)`` and may then be at most 4096 (ValueError); every refusal comes before any device work.  The
        selection reads the candidates' elements in place on the device, once per query (libsimrank_candidates.so), per
        column block with a merge on the host under ``LocalWorld(P)``; a pruned model is answered on the host for its
        matrix P: a candidate counts with its listed value, or with the +0.0 of an absent entry.  With both None the
        call is what it was without the keywords.  ``fold_in(top_k=)``, ``rank_sets``, ``rank_recommended``,
        ``evaluate``, ``top_k()`` and ``pairs()`` take no candidate filter, and a ``TorchWorld`` model answers none."""
        from . import _candidates
        from ._query import check_k
        k = check_k(k)
        solver, j, labels = self._kept(group)
        lab, _ = self._ids(j, labels, [])
        cand = _candidates.prepare(among, exclude, lab)
        if cand is None:
            self._check_kept_neighbors(solver, [j], k)
            lab, ids = self._ids(j, labels, nodes)
            return _long_frame("node", "similarity", lab.take(ids), lab, *solver.topk_of(j, ids, k))
        k = _candidates.clamp_k(k, cand.size)
        self._check_kept_neighbors(solver, [j], k)
        if not hasattr(solver, "topk_among"):
            raise ValueError("among= / exclude= need a solver behind the C ABI (fit on one GPU or LocalWorld(P))")
        lab, ids = self._ids(j, labels, nodes)
        return _long_frame("node", "similarity", lab.take(ids), lab, *solver.topk_among(j, ids, cand, k))

    def fold_in(self, neighbors, weights=None, prior=None, names=None, group=None, top_k=None):
        """Similarities of nodes that were NOT in the fitted graph: for each new node, the row the NEXT update would
        compute for a node with that neighbour list, with every existing similarity and every existing normalisation
        held fixed (a new group-1 node does NOT change the normalisation of its items: that is what makes the answer one
        update and not a refit):

            s(q, b) = [(1 - lbd)] * E(q, b) * C * sum_{i in I_q} w_q * sum_{j in I(b)} S[i, j] * W[b, j]  [+ lbd * prior(q, b)]

        ``neighbors``: one sequence of labels of FITTED nodes per new node: its in-neighbours (the ``from`` nodes of its
        edges) for the directed classes; for the bipartite classes ``group=1`` is a new group-1 node given by its group-2
        neighbours, ``group=2`` the other way round.  ``weights`` (exactly when the fit had ``weighted=True``): one
        sequence per new node; every entry of the new row is 1 / sum(weights), as the reference scales a row (0 where that
        is not finite); unweighted 1 / len(list); an empty list gives a row of zeros.  ``prior`` (classes fitted with a
        prior): array [n_new, N] in the dense frame's column order (default zeros).  ``names``: the index of the result.
        SimRank++ classes count the evidence |I_q ∩ I(b)| on the device from the new list.

        -> DataFrame [n_new x N] float64, columns as the dense frame's; with ``top_k=k`` the long frame (node, rank,
        neighbor, similarity) of the k best per new node (value descending, label position ascending; no node is
        excluded: a new node has no diagonal), selected on the device; k is clamped to N and may then be at most 1024
        (the selection kernel's limit: ValueError before any device work)."""
        from . import _foldin
        self._solver_sides()
        if self.kept_neighbors is not None:
            raise ValueError("fold_in needs whole rows of the iterate, which a pruned model no longer holds: fold in "
                             "before prune()")
        solver, side, j, out_index, _, src_index = self._across(group, gate=True)
        specs = getattr(solver, "specs", None)
        lists, w, prior, names, k = _foldin.prepare(
            neighbors, src_index, n_out=len(out_index), weighted=bool(getattr(self, "_weighted", False)),
            has_prior=bool(specs and specs[side].apriori is not None), weights=weights, prior=prior, names=names,
            top_k=top_k)
        new_index = pd.RangeIndex(len(lists)) if names is None else pd.Index(names)
        if k is None:
            return pd.DataFrame(solver.fold_in(j, lists, w, prior), index=new_index, columns=out_index.copy())
        return _long_frame("node", "similarity", new_index, out_index, *solver.fold_in(j, lists, w, prior, top_k=k))

    def score_sets(self, sets, weights=None, names=None, group=None, top_k=None, exclude="members", diversity=None,
                   among=None):
        """Basket queries: for each basket (a sequence of labels of FITTED nodes of ``group``, repeats counting as often
        as they occur) the row

            score(b) = sum_{i in basket} w_i * S[i, b]

        of that group's matrix, summed on the device in float64 in the order given, every product and every sum rounded
        separately: bit for bit what ``(w[:, None] * model.rows(basket).values)`` accumulated row by row gives.
        ``weights``: one sequence of finite floats per basket (default 1.0 each); ``names``: the index of the result.  An
        empty basket scores 0 everywhere.

        -> DataFrame [n_sets x N] float64, columns as the dense frame's; with ``top_k=k`` the long frame (set, rank,
        neighbor, score) of the k best per basket (score descending, label position ascending), selected on the device,
        k clamped to N.  ``exclude``: "members" (the basket's own members are no candidates), None, or one sequence of
        labels per basket that are no candidates instead; a basket with fewer than k candidates gets fewer rows.

        ``diversity=d`` (with ``top_k``; a real number in [0, 1]): the k are picked one by one on the device by maximal
        marginal relevance instead.  Every remaining candidate b carries ``penalty(b)``, the largest ``S[p, b]`` over
        the picks p made so far (row p of the group's matrix; +0.0 before the first pick and never below it), and the
        next pick is the candidate with the greatest ``value = ((1 - d) * score) - (d * penalty)``, three float64
        operations, ties by label position.  -> the long frame (set, rank, neighbor, score, penalty, value), ``rank`` the
        order of picking.  ``d = 0`` picks what ``top_k`` alone does.

        ``among`` (with ``top_k``; as ``most_similar`` takes it: None or a non-string iterable of fitted labels of the
        group, shared by all baskets): the candidates of a basket are ``among`` minus its exclusions, with or without
        ``diversity``.  Only the candidates' columns are scored, so the band on the device is |among| wide; a score
        depends on its own column alone and keeps its bits.  ``among`` without ``top_k`` is a ValueError."""
        from . import _diverse, _sets
        solver, j, labels = self._kept(group)
        d = _diverse.check_diversity(diversity, top_k)
        index, _ = self._ids(j, labels, [])
        cand = self._among(among, top_k, index)
        ptr, ids, w, names, k, excl = _sets.prepare(sets, index, weights=weights, names=names, top_k=top_k,
                                                    exclude=exclude)
        who = pd.RangeIndex(ptr.size - 1) if names is None else pd.Index(names)
        more = {} if cand is None else {"among": cand}
        if d is not None:
            return _diverse_frame("set", who, index, *solver.score_diverse(j, ptr, ids, w, k, excl, d, **more))
        if k is None:
            return pd.DataFrame(solver.score_sets(j, ptr, ids, w), index=who, columns=index.copy())
        return _long_frame("set", "score", who, index, *solver.score_sets(j, ptr, ids, w, k, excl, **more))

    @staticmethod
    def _among(among, top_k, index):
        """``among=`` of the band queries, checked before any device work: None, or the sorted caller ids of the
        candidates (``_candidates.prepare``); ValueError without ``top_k``."""
        from . import _candidates
        if among is None:
            return None
        if top_k is None:
            raise ValueError("among narrows a selection: give top_k as well")
        return _candidates.prepare(among, None, index)

    def matmul(self, X, transpose=False, group=None):
        """The model as a linear operator: ``S @ X`` of the group's matrix (``transpose=True``: ``S.T @ X``; the matrices
        are not symmetric in general), every element widened as ``rows`` widens it, products and sums in float64.

        ``X``: a DataFrame or Series indexed by the group's fitted labels, in any order, every node exactly once (as
        ``cluster_quality`` takes ``labels``), or an array-like of shape [N] or [N, d] in the dense frame's order; real
        floating or integer data, finite or not (bool, object and complex dtypes are a ValueError, an unknown label a
        KeyError), checked before any device work.

        -> DataFrame [N x d] float64, indexed by the dense frame's labels in its order, with ``X``'s columns (a
        ``RangeIndex`` for an array); a Series or a 1-D array in gives a Series.

        The matrix is read in place on the device (libsimrank_operator.so), once per band of 64 columns; ``X`` and the
        result cross PCIe once.  The order of a sum's additions depends on the shape alone and there are no
        floating-point atomics: two calls give the same bits, and every element lies within ``N * 2^-52 * sum |S| |X|``
        of the exact one.  A model held in several column blocks (``LocalWorld(P)``) is packed into one temporary block
        first; a pruned model is answered on the host for its matrix P, whose absent entries are +0.0 and add nothing.
        The model is left unchanged."""
        from . import _operator
        solver, j, labels = self._kept(group)
        if not isinstance(transpose, (bool, np.bool_)):
            raise ValueError(f"transpose must be True or False, not {transpose!r}")
        index, _ = self._ids(j, labels, [])
        dense, columns, kind, name = _operator.check_operand(X, index)
        out = solver.apply_operator(j, dense, bool(transpose))
        if kind in ("series", "vector"):
            return pd.Series(out[:, 0], index=index.copy(), name=name)
        return pd.DataFrame(out, index=index.copy(), columns=columns)

    def embed(self, dim, oversample=8, power_iterations=2, seed=0, group=None):
        """Vectors for the nodes: the spectral embedding of the symmetric part ``M = (S + S.T) / 2`` of the group's
        matrix by a randomized subspace iteration.  With ``p = min(dim + oversample, N)``:

            Q = qr(default_rng(seed).standard_normal((N, p)))[0]
            repeat power_iterations times:  Q = qr(M @ Q)[0]
            Y = M @ Q;  B = Q.T @ Y;  B = (B + B.T) / 2;  w, Z = eigh(B)
            the dim largest w, descending;  V = Q @ Z[:, those]

        and every column of V gets the sign that makes its entry of largest magnitude (the first on a tie) positive.
        ``dim``: an int in 1 .. N; ``oversample``: an int >= 0; ``power_iterations``: an int in 0 .. 16; ``seed``: a
        non-negative int (each a ValueError before any device work).

        -> ``(vectors, eigenvalues)``: a DataFrame [N x dim] float64 indexed by the dense frame's labels in its order,
        orthonormal columns; a float64 Series of length ``dim``, ``eigenvalues[i] = v_i.T M v_i``.

        ``M @ Q`` is two products of ``matmul``'s kernel on the device, ``0.5 S Q`` and ``+ 0.5 S.T Q`` where the first
        result lies; per product Q goes up and Y (N x p x 8 bytes) comes down for the host's QR.  The same call gives
        the same bits twice.  Where ``matmul`` runs, and as it does.  The model is left unchanged."""
        from . import _operator
        solver, j, labels = self._kept(group)
        index, _ = self._ids(j, labels, [])
        dim, p, iters, seed = _operator.check_embed_args(dim, oversample, power_iterations, seed, len(index))
        V, w = solver.embed_operator(j, dim, p, iters, seed)
        cols = pd.RangeIndex(dim)
        return (pd.DataFrame(V, index=index.copy(), columns=cols),
                pd.Series(w, index=cols.copy(), name="eigenvalue", dtype=np.float64))

    def recommend(self, nodes, k, group=None, exclude_seen=True, diversity=None, among=None):
        """Leg 1 of the update for chosen rows: for each fitted node u of ``group`` the k best of ``(W . S)[u, :]``, the
        scores of u's neighbours' rows (its in-neighbours for the directed classes; for the bipartite classes the
        group-2 neighbours of a group-1 node, read from group 2's matrix, and the other way round), every weight
        ``W[u, .]`` as the fit scaled that row.  The same sum as ``score_sets`` of that basket with those weights.
        ``exclude_seen``: u's neighbours (and, for the directed classes, u itself) are no candidates.

        -> long frame (node, rank, neighbor, score), blocks in the order of ``nodes``; ``neighbor`` is a node of the
        group the basket lives in.  A node without neighbours gets no rows.  ``diversity=d``: the k picked by maximal
        marginal relevance as ``score_sets(diversity=d)`` picks them, the penalties read from the matrix the baskets live
        in -> (node, rank, neighbor, score, penalty, value).  ``among``: as ``score_sets`` takes it, labels of the group
        the ``neighbor`` column lives in; the candidates of a node are ``among`` minus what ``exclude_seen`` removes."""
        from . import _diverse, _sets
        solver, side, j, index, src_j, src_index = self._across(group)
        if not isinstance(exclude_seen, bool):
            raise ValueError(f"exclude_seen must be True or False, not {exclude_seen!r}")
        d = _diverse.check_diversity(diversity, k)
        k = _sets.check_top_k(k, len(src_index))
        cand = self._among(among, k, src_index)
        more = {} if cand is None else {"among": cand}
        _, ids = self._ids(j, index, nodes)
        spec = solver.specs[side]
        ptr, members, w, excl = _sets.csr_baskets(spec.csr, spec.rowscale, ids, src_j == j, exclude_seen)
        if d is not None:
            return _diverse_frame("node", index.take(ids), src_index,
                                  *solver.score_diverse(src_j, ptr, members, w, k, excl, d, **more),
                                  keep_rows=np.diff(ptr) > 0)
        idx, val = solver.score_sets(src_j, ptr, members, w, k, excl, **more)
        return _long_frame("node", "score", index.take(ids), src_index, idx, val, keep_rows=np.diff(ptr) > 0)

    def explain(self, a, b, k=10, group=None, max_terms=2 ** 27):
        """WHY are a and b similar: the update gives a pair of fitted nodes of ``group`` a sum over the pairs of their
        neighbours (their in-neighbours for the directed classes; for the bipartite classes the group-2 neighbours of
        group-1 nodes, read from group 2's matrix, and the other way round, as ``recommend`` reads them),

            next(a, b) = F(a, b) * rowscale[a] * rowscale[b] * sum_{i in I(a)} sum_{j in I(b)} S_src[i, j]     (a != b)

        with ``F = coef`` for SimRank and BipartiteSimRank and ``F = (1 - lbd) * E(a, b) * coef``, ``E = 1 - 2^-|I(a) ∩
        I(b)|``, for the ++ and prior classes.  Every term of a pair carries the same scale, so the pairs that contribute
        most are the largest elements of the sub-matrix ``S_src[I(a), I(b)]`` and a neighbour's part is its row or column
        sum.  ``a``, ``b``: label sequences of equal length, repeats allowed; KeyError for an unknown label.  A ValueError,
        before any device work, for unequal lengths, ``a[i] == b[i]`` (the update SETS the diagonal, it does not sum it),
        ``k`` not an int in 1 .. 1024, a bad ``group``, ``group=2`` on a bipartite ``strict_reference=True`` fit (as
        ``fold_in``), and a pair whose ``|I(a)| * |I(b)|`` exceeds ``max_terms``.

        -> ``(pairs, terms, neighbors)``.  ``pairs`` has one row per pair in the order given: ``a``, ``b``,
        ``similarity`` (the stored ``S[a, b]``: the bits ``similarity`` returns), ``terms`` (int64) = ``|I(a)| * |I(b)|``,
        ``contributors`` (int64: the terms that are neither NaN nor a zero of either sign), ``common`` (int64) = ``|I(a) ∩
        I(b)|``, 0 when either row scale is not > 0, ``evidence`` (float64) = ``1 - 2^-min(common, 255)`` for the classes
        with evidence and 1.0 otherwise, ``raw`` (float64: the double sum) and ``propagated`` (float64) = ``F *
        (rowscale[a] * (rowscale[b] * raw))``, host arithmetic in float64 in exactly that association, ``F = ((1 - lbd)
        * evidence) * coef`` with evidence.  For the classes fitted with a prior the next update's value is ``propagated
        + lbd * prior[a, b]``: the caller holds the prior and can add it.

        ``terms`` is the long frame (pair, rank, via_a, via_b, similarity, share): ``pair`` the position in the input,
        the k largest contributors of each pair in the total order (value descending, then ``via_a``'s position in the
        source group's frame ascending, then ``via_b``'s); NaN and ±0.0 are never listed, so a pair with fewer than k
        contributors gets fewer rows; ``similarity = S_src[via_a, via_b]`` widened as ``rows`` widens it, ``share =
        similarity / raw``.  ``neighbors`` is the long frame (pair, of, neighbor, sum, share): per pair one row per
        neighbour of a (``of = "a"``, ``sum = sum_{j in I(b)} S_src[i, j]``), then one per neighbour of b (``of = "b"``,
        ``sum = sum_{i in I(a)} S_src[i, j]``), in the order of the side's CSR row; ``share = sum / raw``.

        The sums are float64 with no floating-point atomics, in an order that depends on the two lists' lengths alone: the
        same call gives the same bits twice, and a sum of m terms lies within ``m * 2^-52 * sum |x|`` of the exact one;
        ``raw`` is the sum of a's marginals; NaN propagates.  The sub-matrices are gathered from the iterate in place on
        the device (libsimrank_explain.so) in bands that fit the scratch slab; only the sums, the counts and the k best
        cross.  A model held in several column blocks (``LocalWorld(P)``) is packed into one temporary block first; a
        pruned model is answered on the host for its matrix P, whose absent entries are +0.0.  The model is unchanged."""
        from . import _explain
        a, b = _explain.check_pairs(a, b)
        k, max_terms = _explain.check_k(k), _explain.check_max_terms(max_terms)
        solver, side, j, index, src_j, src_index = self._across(group, gate=True)
        _, ia = self._ids(j, index, a)
        _, ib = self._ids(j, index, b)
        same = np.flatnonzero(ia == ib)
        if same.size:
            raise ValueError(f"a[{int(same[0])}] == b[{int(same[0])}] == {a[int(same[0])]!r}: the update sets the diagonal "
                             "to 1, it does not sum it; there is nothing to explain")
        r = _explain.explain(solver, j, src_j, solver.specs[side], ia, ib, k, max_terms, labels=(a, b))
        n = len(a)
        pairs = pd.DataFrame({"a": index.take(ia).to_numpy() if n else np.empty(0, dtype=object),
                              "b": index.take(ib).to_numpy() if n else np.empty(0, dtype=object),
                              "similarity": r["similarity"], "terms": r["terms"], "contributors": r["contributors"],
                              "common": r["common"], "evidence": r["evidence"], "raw": r["raw"],
                              "propagated": r["propagated"]})
        keep = r["best_a"].ravel() >= 0
        which = np.repeat(np.arange(n, dtype=np.int64), k)[keep]
        value = r["best_value"].ravel()[keep]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            terms = pd.DataFrame({"pair": which, "rank": np.tile(np.arange(1, k + 1, dtype=np.int64), n)[keep],
                                  "via_a": src_index.take(r["best_a"].ravel()[keep]).to_numpy(),
                                  "via_b": src_index.take(r["best_b"].ravel()[keep]).to_numpy(),
                                  "similarity": value, "share": value / r["raw"][which]})
            na, nb = np.diff(r["ptr_a"]), np.diff(r["ptr_b"])
            # per pair a's neighbours, then b's: the two lists interleaved pair by pair
            seg = np.concatenate([np.repeat(2 * np.arange(n), na), np.repeat(2 * np.arange(n) + 1, nb)])
            order = np.argsort(seg, kind="stable")
            pair_of = (seg // 2)[order].astype(np.int64)
            sums = np.concatenate([r["sum_a"], r["sum_b"]])[order]
            neighbors = pd.DataFrame({"pair": pair_of, "of": np.where(seg[order] % 2 == 0, "a", "b").astype(object),
                                      "neighbor": src_index.take(np.concatenate([r["ids_a"], r["ids_b"]])[order]).to_numpy(),
                                      "sum": sums, "share": sums / r["raw"][pair_of]})
        return pairs, terms, neighbors

    @staticmethod
    def _rank_frame(first, who, index, ptr, tptr, tids, score, before, candidates, live=None):
        """Long frame (``first``, target, score, rank, candidates), one row per listed target; ``live``: per basket
        whether it ranks anything at all (a basket that does not has rank 0 and 0 candidates throughout)."""
        from . import _rank
        basket = np.repeat(np.arange(tptr.size - 1), np.diff(tptr))
        rank = _rank.ranks_of(score, before)
        cand = np.asarray(candidates, dtype=np.int64)[basket]
        if live is not None:
            dead = ~np.asarray(live, dtype=bool)[basket]
            rank[dead], cand[dead] = 0, 0
        return pd.DataFrame({first: who.take(basket), "target": index.take(tids.astype(np.intp)),
                             "score": np.asarray(score, dtype=np.float64), "rank": rank, "candidates": cand})

    def rank_sets(self, sets, targets, weights=None, names=None, group=None, exclude="members"):
        """Held-out ranks: for each basket of ``score_sets`` (``sets``, ``weights``, ``names``, ``group`` and ``exclude`` as
        there) and each label of ``targets[q]`` (one sequence of labels of fitted nodes per basket; repeats kept, empty
        lists allowed), where that node comes out in the basket's ranking.

        -> long frame (set, target, score, rank, candidates), one row per listed target in the order given: ``score``
        (float64) the basket's score of the target, bit for bit ``score_sets``' value, or -inf for an excluded target;
        ``rank`` (int64, 1-based) the position of the target's row in what ``score_sets(..., top_k=N, exclude=...)`` returns
        for that basket (score descending, label position ascending), 0 when the target is no candidate (excluded, or
        scored NaN); ``candidates`` (int64) the number of rows that frame has for the basket.  A target listed twice
        gets two equal rows.

        The score rows stay on the device: every target's rank is counted there (libsimrank_rank.so, |targets| x N
        comparisons per basket) and 16 bytes per target cross to the host.  The model is left unchanged."""
        from . import _rank, _sets
        solver, j, labels = self._kept(group)
        index, _ = self._ids(j, labels, [])
        ptr, ids, w, names, _, excl = _sets.prepare(sets, index, weights=weights, names=names,
                                                    top_k=max(1, len(index)), exclude=exclude)
        tptr, tids = _rank.prepare(targets, index, ptr.size - 1)
        who = pd.RangeIndex(ptr.size - 1) if names is None else pd.Index(names)
        score, before, candidates = solver.score_ranks(j, ptr, ids, w, excl, tptr, tids)
        return self._rank_frame("set", who, index, ptr, tptr, tids, score, before, candidates)

    def rank_recommended(self, nodes, targets, group=None, exclude_seen=True):
        """``rank_sets`` for ``recommend``'s baskets: for each fitted node u of ``group`` (its CSR row with the fit's
        weights, ``exclude_seen`` as there) and each label of ``targets[i]`` (nodes of the group the basket lives in: the
        ``neighbor`` column of ``recommend``), the position of that label in ``recommend([u], N)``.

        -> long frame (node, target, score, rank, candidates), one row per listed target.  A node without neighbours
        gets no rows from ``recommend``: its targets have rank 0 and 0 candidates."""
        return self._rank_recommended(nodes, targets, group, exclude_seen)[0]

    def _rank_recommended(self, nodes, targets, group, exclude_seen):
        """(``rank_recommended``'s frame, the offsets of every node's targets in it)"""
        from . import _rank, _sets
        solver, side, j, index, src_j, src_index = self._across(group)
        if not isinstance(exclude_seen, bool):
            raise ValueError(f"exclude_seen must be True or False, not {exclude_seen!r}")
        _, ids = self._ids(j, index, nodes)
        tptr, tids = _rank.prepare(targets, src_index, ids.size)
        spec = solver.specs[side]
        ptr, members, w, excl = _sets.csr_baskets(spec.csr, spec.rowscale, ids, src_j == j, exclude_seen)
        score, before, candidates = solver.score_ranks(src_j, ptr, members, w, excl, tptr, tids)
        return self._rank_frame("node", index.take(ids), src_index, ptr, tptr, tids, score, before, candidates,
                                live=np.diff(ptr) > 0), tptr

    def evaluate(self, nodes, targets, ks=(10,), group=None, exclude_seen=True):
        """Held-out evaluation of ``recommend``: host arithmetic on ``rank_recommended(nodes, targets, ...)``.  ``ks``: a
        non-empty sequence of positive ints (ValueError before any device work).

        -> one row per node of ``nodes``, in their order: node, targets (how many were listed), not_candidates (how many
        of them have rank 0), best_rank (the smallest rank above 0; 0 when there is none), reciprocal_rank (1.0 /
        best_rank; 0.0 when there is none) and, for each k of ``ks``, ``hits@k``: the number of the node's targets with
        1 <= rank <= k."""
        from . import _rank
        ks = _rank.check_ks(ks)
        nodes = list(nodes)
        long, tptr = self._rank_recommended(nodes, targets, group, exclude_seen)
        rank = long["rank"].to_numpy()
        n = len(nodes)
        sizes = np.diff(tptr)
        basket = np.repeat(np.arange(n), sizes)
        count = lambda mask: np.bincount(basket[mask], minlength=n).astype(np.int64)
        best = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
        np.minimum.at(best, basket[rank > 0], rank[rank > 0])
        best[best == np.iinfo(np.int64).max] = 0
        out = {"node": pd.Index(nodes), "targets": sizes, "not_candidates": count(rank == 0), "best_rank": best,
               "reciprocal_rank": np.where(best > 0, 1.0 / np.maximum(best, 1), 0.0)}
        for k in ks:
            out[f"hits@{k}"] = count((rank >= 1) & (rank <= k))
        return pd.DataFrame(out)

    def _all_sides(self, make):
        solver, sides = self._solver_sides()
        out = [make(solver, j, lab) for j, lab in sides]
        return out[0] if len(sides) == 1 else tuple(out)

    def frame(self):
        """What ``fit`` without ``keep`` returns: the dense frame (a tuple of two for the bipartite classes)."""
        return self._all_sides(lambda solver, j, lab: _square_frame(solver.result(j), lab))

    def top_k(self, k):
        """What ``fit(top_k=k)`` returns."""
        from ._query import check_k
        k = check_k(k)
        solver, sides = self._solver_sides()
        self._check_kept_neighbors(solver, [j for j, _ in sides], k)
        return self._all_sides(lambda solver, j, lab: _topk_frame(solver, j, k, lab))

    def pairs(self, min_similarity, max_pairs=2 ** 27):
        """What ``fit(min_similarity=t, max_pairs=m)`` returns."""
        _check_pairs_args(min_similarity, max_pairs)
        return self._all_sides(lambda solver, j, lab: _pairs_frame(solver, j, min_similarity, max_pairs, lab))

    def count_pairs(self, thresholds):
        """int64 array, one entry per threshold in the order given: the number of ordered pairs (a, b) of different nodes
        with ``S[a, b] >= t``, compared in float64 on the bits the dense frame holds: for t > 0 the number of rows
        ``pairs(t)`` returns.  ``thresholds``: 1 to 1024 finite numbers of any sign, in any order, repeats allowed.  NaN
        never counts; -0.0 >= 0.0 does.  One sweep of the iterate in place on the device (libsimrank_profile.so); nothing
        but the counts crosses.  A pruned model is counted on the host from its lists, the absent +0.0 entries added by
        arithmetic.  A tuple of two for the bipartite classes."""
        from . import _profile
        ts = _profile.check_thresholds(thresholds)
        return self._all_sides(lambda solver, j, lab: _profile.count_pairs(solver, j, ts))

    def threshold_for(self, max_pairs):
        """``(t, n)``: the smallest value ``t`` (float64) occurring off the diagonal whose count ``n`` of pairs with
        ``S[a, b] >= t`` is at most ``max_pairs`` (an int >= 1): ``pairs(t, max_pairs=max_pairs)`` then succeeds with
        exactly ``n`` rows when t > 0.  Equal values stay together: when the ``max_pairs``-th and the next largest value
        are equal, ``t`` is the next larger distinct value.  ``(inf, 0)`` when even the largest value occurs more often,
        or there is no pair.  -0.0 and +0.0 are one value, reported as +0.0; NaN is ignored.  A radix select over the
        iterate in place: 3 sweeps of an f32 model, 2 of an fp16-held and 6 of a float64 one, whatever N and
        ``max_pairs``.  A tuple of two for the bipartite classes."""
        from . import _profile
        m = _profile.check_max_pairs(max_pairs)
        return self._all_sides(lambda solver, j, lab: _profile.threshold_for(solver, j, m))

    def components(self, t):
        """Single-linkage clusters at threshold ``t``: the connected components of the graph that joins two different
        nodes a, b iff ``S[a, b] >= t`` or ``S[b, a] >= t``, the comparison ``pairs`` and ``count_pairs`` make (float64 on
        the bits the dense frame holds; NaN never joins, -0.0 >= 0.0 does): iff (a, b) or (b, a) is a row of ``pairs(t)``.
        ``t``: one finite number -> a Series "component" (int64) over the dense frame's labels in its order; a sequence
        of 1 to 8 numbers of any sign, in any order, repeats allowed -> a DataFrame with one such column per threshold,
        labelled ``float(t)``, in the order given.  Components are numbered 0, 1, 2, ... in the order of their first
        member in the frame's order, whatever the device did.  One sweep of the iterate in place for all thresholds
        (libsimrank_cluster.so: a lock-free union-find on integer atomics); N labels per threshold cross.  A pruned
        model is answered on the host for its matrix P, whose absent entries are +0.0: at t <= 0 they join their pairs.
        A tuple of two for the bipartite classes."""
        from . import _cluster
        ts, scalar = _cluster.check_thresholds(t)

        def make(solver, j, lab):
            labels = _cluster.number(_cluster.roots(solver, j, ts))
            index = pd.Index(lab)
            if scalar:
                return pd.Series(labels[0], index=index, name="component", dtype=np.int64)
            return pd.DataFrame(labels.T.reshape(len(index), len(ts)), index=index, columns=[float(x) for x in ts], dtype=np.int64)
        return self._all_sides(make)

    def degrees(self, t):
        """How many neighbours every node has at threshold ``t``: two different nodes a, b are neighbours iff
        ``S[a, b] >= t`` or ``S[b, a] >= t``, the relation of ``components`` (float64 on the bits the dense frame holds;
        NaN never passes, -0.0 >= 0.0 does); a pair that passes in both directions is one neighbour.  ``t``: one finite
        number -> a Series "neighbors" (int64) over the dense frame's labels in its order; a sequence of 1 to 8 numbers
        of any sign, in any order, repeats allowed -> a DataFrame with one such column per threshold, labelled
        ``float(t)``, in the order given.  One sweep of the iterate in place for all thresholds, every element read once
        (libsimrank_density.so: entry (a, b) meets entry (b, a) in the workgroup that holds both of their tiles); a side
        held in several column blocks is packed into one temporary block first.  A pruned model is answered on the host
        for its matrix P and needs ``t > 0``: its absent entries are +0.0 and would make everybody everybody's neighbour.
        The model is left unchanged.  A tuple of two for the bipartite classes."""
        from . import _density
        ts, scalar = _density.check_thresholds(t)
        _density.check_solver(self._solver_sides()[0], ts)

        def make(solver, j, lab):
            deg = _density.degrees(solver, j, ts)
            index = pd.Index(lab)
            if scalar:
                return pd.Series(deg[0], index=index, name="neighbors", dtype=np.int64)
            return pd.DataFrame(deg.T.reshape(len(index), len(ts)), index=index, columns=[float(x) for x in ts], dtype=np.int64)
        return self._all_sides(make)

    def dbscan(self, t, min_samples=5):
        """Density clusters (DBSCAN) at threshold ``t`` (one finite number) over the neighbours of ``degrees(t)``.

        -> DataFrame over the dense frame's labels in its order: ``neighbors`` (int64) is ``degrees(t)``; ``core`` (bool)
        is ``neighbors + 1 >= min_samples``: the node counts itself, as scikit-learn's ``DBSCAN`` counts it
        (``min_samples``: an int >= 1); ``cluster`` (int64): two core nodes that are neighbours are in one cluster,
        transitively; a node that is not core but has a core neighbour is a border node and takes the cluster of its
        FIRST core neighbour in the frame's order (classical DBSCAN leaves that to the scan order; here it is a function
        of the matrix alone); every other node is noise, -1.  Border nodes never extend a cluster: two core nodes that
        share only a border node stay apart.  Clusters are numbered 0, 1, 2, ... in the order of their first member,
        core or border, as ``components`` numbers: ``dbscan(t, 1).cluster`` is ``components(t)``.

        Three sweeps on the device (libsimrank_density.so): the counts, a lock-free union-find over the core nodes on
        integer atomics with an atomic minimum for the border nodes, and the labels; 8 N bytes cross.  Runs where
        ``degrees`` runs, and as it does (a pruned model: ``t > 0``).  The model is left unchanged.  A tuple of two for
        the bipartite classes."""
        from . import _density
        ts, scalar = _density.check_thresholds(t)
        if not scalar:
            raise ValueError(f"dbscan takes one threshold, a finite number, not {t!r}")
        min_neighbors = _density.check_min_samples(min_samples)
        _density.check_solver(self._solver_sides()[0], ts)

        def make(solver, j, lab):
            deg, labels = _density.dbscan(solver, j, float(ts[0]), min_neighbors)
            return pd.DataFrame({"cluster": _density.number(labels), "core": deg >= min_neighbors, "neighbors": deg},
                                index=pd.Index(lab))
        return self._all_sides(make)

    def core_similarity(self, min_samples=5):
        """Every node's core similarity: the (``min_samples`` - 1)-th largest of its pair heights
        ``w(a, b) = max(S[a, b], S[b, a])``, b != a, compared as ``components`` compares (float64 on the bits the dense
        frame holds; a NaN entry is no entry, -0.0 and +0.0 are one value, +0.0).  The node counts itself, as ``dbscan``
        counts (``min_samples``: an int >= 1): +inf at ``min_samples=1``, -inf for a node with fewer pairs.  It is a
        selection, hence exact, and ``core_similarity(m) >= t`` iff ``dbscan(t, m).core`` for every finite t: sorted, it
        is the k-distance plot from which a ``t`` for ``dbscan`` is read.

        -> Series "core_similarity" (float64) over the dense frame's labels in its order.  A radix select on the device
        (libsimrank_hdbscan.so) that pairs entry (a, b) with entry (b, a) as ``degrees`` does: 8 sweeps of an f32 model,
        4 of an fp16-held and 16 of a float64 one, whatever N and ``min_samples``; 8 N bytes cross.  Runs where
        ``degrees`` runs; a pruned model is answered on the host for its matrix P, whose absent entries are +0.0.  The
        model is left unchanged.  A tuple of two for the bipartite classes."""
        from . import _hdbscan
        rank = _hdbscan.check_min_samples(min_samples)
        return self._all_sides(lambda solver, j, lab: pd.Series(
            _hdbscan.core_similarity(solver, j, rank), index=pd.Index(lab), name="core_similarity", dtype=np.float64))

    def hdbscan(self, min_cluster_size=5, min_samples=None, min_similarity=None, selection="eom",
                allow_single_cluster=False):
        """HDBSCAN*: clusters of different density, read off ``linkage(min_samples=m)`` by host arithmetic, with the
        similarity itself as the density level (no distance, no division).  ``min_cluster_size``: an int >= 2;
        ``min_samples``: an int >= 1, by default ``min_cluster_size``; ``min_similarity`` as ``linkage``'s;
        ``selection``: "eom" or "leaf".

        The hierarchy is the multi-way one the table encodes: a class is a component of some ``cut(Z, t)``, its children
        the classes (or leaves) of the next higher level inside it; a class without a parent is a root.  Condensing runs
        top-down from every root of at least ``min_cluster_size`` nodes, whose cluster is born at the height the root
        forms.  At a class of the current cluster C that forms at h: two or more children of at least
        ``min_cluster_size`` nodes end C, and each starts a cluster born at h; exactly one continues C; the members of
        every other child leave C at h.  ``stability(C)`` is the exactly rounded sum of ``leave(p) - birth(C)`` over the
        nodes p of C at its birth.  "eom", bottom-up: a cluster without child clusters is selected with its stability as
        score; another one is selected instead of its descendants when its stability is at least the sum of its
        children's scores and it is no root (or ``allow_single_cluster``); otherwise its score is that sum.  "leaf": the
        clusters without child clusters, a root only with ``allow_single_cluster``.

        -> (labels, clusters).  ``labels``: a DataFrame over the dense frame's labels: ``cluster`` (int64), the selected
        cluster that held the node at its birth, numbered 0, 1, ... by first member, -1 for noise, and
        ``core_similarity`` (float64).  ``clusters``: one row per cluster of the condensed tree, ordered by (smallest
        member, size descending): ``parent`` (the row, or -1), ``birth``, ``size`` at birth, ``stability``, ``selected``,
        ``cluster`` (the label, or -1).  A function of the matrix alone, ties included.  Runs where ``linkage`` runs.
        A tuple of two such pairs for the bipartite classes."""
        from . import _hdbscan, _linkage
        mcs, rank, floor = _hdbscan.check_hdbscan(min_cluster_size, min_samples, min_similarity, selection)
        _linkage.check_solver(self._solver_sides()[0], floor)

        def make(solver, j, lab):
            n, core, left, right, sim, size = _hdbscan.table(solver, j, rank, floor)
            labels, clusters = _hdbscan.condense(n, left, right, sim, size, mcs, selection, bool(allow_single_cluster))
            return (pd.DataFrame({"cluster": labels, "core_similarity": core}, index=pd.Index(lab)), pd.DataFrame(clusters))
        return self._all_sides(make)

    def linkage(self, min_similarity=None, min_samples=None):
        """The single-linkage dendrogram: every ``components(t)`` at once.  Two different nodes a, b fall together at the
        height ``w(a, b) = max(S[a, b], S[b, a])``, compared as ``components`` compares (float64 on the bits the dense frame
        holds); a NaN entry is no entry, -0.0 and +0.0 are one height, reported as +0.0.

        -> DataFrame (left, right: int64; similarity: float64; size: int64) in the shape of a SciPy linkage matrix, with
        similarities that fall where SciPy's distances rise (pass ``1 - similarity`` on).  Cluster ids below N are
        leaves, the positions in the dense frame's label order; row i forms cluster N + i of ``size`` members.  N - 1
        rows when everything joins; fewer when NaN isolates nodes or ``min_similarity`` (a finite number: entries with
        ``w < min_similarity`` are not used) stops the tree.

        The table is a function of the matrix alone, ties included.  With h1 > h2 > ... the distinct heights: every
        component of ``components(h_j)`` that unites m >= 2 components c1 .. cm of ``components(h_(j-1))``, taken in the
        order of their smallest member, gives the m - 1 rows (c1, c2) -> x1, (x1, c3) -> x2, ...; the new components of
        one height come in the order of their smallest member.  ``left`` is the cluster grown so far.

        A maximum spanning forest found on the device by Boruvka's rounds (libsimrank_linkage.so): at most
        ceil(log2 N) + 1 rounds, each one sweep of the iterate in place (two for a float64 model), integer atomics only;
        12 N bytes cross, and the host orders the N - 1 edges.  A pruned model is answered on the host from its lists and
        needs ``min_similarity > 0``: its absent entries are +0.0 and tie everything at 0.  The model is left unchanged.
        A tuple of two for the bipartite classes.

        ``min_samples=m`` (an int >= 1) gives the same table of the MUTUAL REACHABILITY
        ``min(w(a, b), core_m(a), core_m(b))`` with ``core_m = core_similarity(m)``, a pair at -inf being no entry:
        HDBSCAN*'s hierarchy, which chains less through sparse nodes.  ``cut(Z, t=t)`` of it leaves every node that is
        not core in ``dbscan(t, m)`` alone and parts the core nodes as ``dbscan(t, m).cluster`` does; ``m = 1`` is the
        plain table.  One select (``core_similarity``) and the same rounds with the clamped pick of
        libsimrank_hdbscan.so, on the one block ``degrees`` reads.  None takes exactly the path above."""
        from . import _linkage
        floor = _linkage.check_floor(min_similarity)
        rank = None
        if min_samples is not None:
            from . import _hdbscan
            rank = _hdbscan.check_min_samples(min_samples)
        _linkage.check_solver(self._solver_sides()[0], floor)

        def make(solver, j, lab):
            if rank is not None:
                _, _, left, right, sim, size = _hdbscan.table(solver, j, rank, floor)
                return pd.DataFrame(dict(zip(_linkage.COLUMNS, (left, right, sim, size))))
            _, left, right, sim, size = _linkage.table(solver, j, floor)
            return pd.DataFrame(dict(zip(_linkage.COLUMNS, (left, right, sim, size))))
        return self._all_sides(make)

    def cut(self, Z, t=None, n_clusters=None, group=None):
        """Flat clusters from a table ``Z`` of ``linkage`` (of ``group=1 | 2`` for the bipartite classes): host arithmetic
        on Z and the model's labels.  Exactly one of ``t`` and ``n_clusters``:

        ``t`` (a finite number) applies every row with ``similarity >= t``: for ``t`` at or above the ``min_similarity``
        Z was made with, exactly ``components(t)``.  ``n_clusters=k`` applies the first N - k rows and leaves k clusters;
        a ValueError when Z has fewer rows.  Within a tie of similarities the split follows the table's canonical order:
        the tied merges of components with the smallest members come first.

        -> Series "component" (int64) over the dense frame's labels, numbered 0, 1, 2, ... in the order of each
        component's first member, as ``components`` numbers."""
        from . import _linkage
        t, k = _linkage.check_cut(t, n_clusters)
        _, _, labels = self._kept(group)
        return pd.Series(_linkage.cut_labels(len(labels), Z, t, k), index=pd.Index(labels), name="component", dtype=np.int64)

    def _cluster_scores(self, labels, group, want_means=False, max_bytes=None):
        """What the four methods below share: the checked labelling, then the sweep.  -> (the frame's pandas Index,
        clusters int64 [K] ascending, every node's cluster rank, the sizes, own, other, nearest rank or -1, means)."""
        from . import _groups
        solver, j, lab = self._kept(group)
        index, _ = self._ids(j, lab, [])
        clusters, gidx, sizes = _groups.groups_of(_groups.check_labels(labels, index))
        if max_bytes is not None:
            _groups.check_means_bytes(len(index), clusters.size, max_bytes)
        if len(index) == 0:
            empty = np.empty(0, dtype=np.float64)
            return index, clusters, gidx, sizes, empty, empty, np.empty(0, dtype=np.int64), np.empty((0, 0))
        return (index, clusters, gidx, sizes) + tuple(_groups.scores(solver, j, gidx, sizes, want_means))

    def cluster_quality(self, labels, group=None):
        """A clustering scored node by node.  ``labels``: the cluster of every fitted node, as ``cut``, ``components(t)``
        or anything else gives it: a pandas Series indexed by the fitted labels (any order; every node exactly once) or a
        1-D sequence of length N in the dense frame's order; values are integers of any sign (bool, floats, NaN and None
        are a ValueError), a cluster is one distinct value.  A bad argument is a ValueError (a KeyError for an unknown
        label) before any device work.  ``group=1 | 2`` for the bipartite classes.

        For node a and cluster g, ``M_g(a) = {b : labels[b] = g, b != a}``; ``sum(a, g)`` adds ``S[a, b]`` over it in
        float64 (row a, the element ``similarity(a, b)`` reads: the matrices are not symmetric in general; every element
        widened as ``rows`` widens it); ``mean(a, g) = sum / |M_g(a)|``, NaN when the set is empty.  A NaN entry makes its
        (node, cluster) mean NaN; -0.0 counts as zero.

        -> DataFrame, one row per node, index = the dense frame's labels in its order:
        ``cluster`` (int64) the node's; ``own`` (float64) = ``mean(a, labels[a])``, NaN for a singleton; ``other`` the
        best ``mean(a, g)`` over g != labels[a] and ``nearest`` (int64) that cluster, in the order (mean descending,
        cluster value ascending), a NaN mean never chosen; with no candidate ``nearest = labels[a]`` and ``other`` = NaN;
        ``silhouette``, checked in this order: 0.0 for a singleton, NaN if ``own`` or ``other`` is NaN, otherwise
        ``(own - other) / max(own, other)`` when that maximum is > 0, else 0.0.

        One sweep of the iterate in place on the device (libsimrank_groups.so), three numbers per node cross.  The order
        of a sum's additions depends on the layout, the shape and the labelling alone and there are no floating-point
        atomics: two runs give the same bits, and ``|sum - exact| <= m * 2^-52 * sum |S[a, b]|`` over the ``m`` members.
        A model held in several column blocks (``LocalWorld(P)``) is packed into one temporary block first, as ``prune``
        does.  A pruned model is answered on the host from its lists for its matrix P, whose absent entries are +0.0:
        they count in ``|M_g(a)|`` and add nothing.  The model is left unchanged."""
        from . import _groups
        index, clusters, gidx, sizes, own, other, nearest, _ = self._cluster_scores(labels, group)
        near = np.where(nearest >= 0, clusters[np.maximum(nearest, 0)], clusters[gidx]) if len(index) else nearest
        return pd.DataFrame({"cluster": clusters[gidx], "own": own, "nearest": near.astype(np.int64), "other": other,
                             "silhouette": _groups.silhouette(own, other, sizes[gidx])}, index=index.copy())

    def cluster_means(self, labels, group=None, max_bytes=2 ** 30):
        """DataFrame [N x K] float64: ``mean(a, g)`` of ``cluster_quality`` for every node (index: the dense frame's
        labels) and every cluster (columns: the cluster values, ascending).  An answer of ``N * K * 8`` bytes above
        ``max_bytes`` is a ValueError before any transfer."""
        from . import _groups
        index, clusters, _, _, _, _, _, means = self._cluster_scores(labels, group, True, _groups.check_max_bytes(max_bytes))
        return pd.DataFrame(means, index=index.copy(), columns=pd.Index(clusters, name="cluster"))

    def medoids(self, labels, group=None):
        """Series "medoid": cluster -> the label of its medoid, index = the clusters ascending.  The medoid is the member
        with the largest ``own`` of ``cluster_quality``; ties go to the first member in the frame's order, NaN is skipped;
        if every member's ``own`` is NaN (a singleton), the first member."""
        from . import _groups
        index, clusters, gidx, _, own, _, _, _ = self._cluster_scores(labels, group)
        at = _groups.medoid_positions(gidx, clusters.size, own)
        return pd.Series(index.take(at).to_numpy(), index=pd.Index(clusters, name="cluster"), name="medoid")

    def cluster_summary(self, labels, group=None):
        """DataFrame, one row per cluster (index: the clusters ascending): ``size`` (int64), ``medoid`` (as ``medoids``),
        and ``cohesion``, ``separation``, ``silhouette``: ``math.fsum(...) / size`` of the members' ``own``, ``other`` and
        ``silhouette`` of ``cluster_quality``; NaN propagates (a singleton's cohesion is NaN).  Host arithmetic."""
        from . import _groups
        index, clusters, gidx, sizes, own, other, _, _ = self._cluster_scores(labels, group)
        sil = _groups.silhouette(own, other, sizes[gidx])
        at = _groups.medoid_positions(gidx, clusters.size, own)
        cohesion, separation, mean_sil = _groups.summary(gidx, clusters.size, own, other, sil)
        return pd.DataFrame({"size": sizes, "medoid": index.take(at).to_numpy(), "cohesion": cohesion,
                             "separation": separation, "silhouette": mean_sil}, index=pd.Index(clusters, name="cluster"))

    def _seeded(self, seeds, group):
        """What ``assign`` and ``kmedoids`` share: the model and the checked seeds -> (solver, side, the frame's pandas
        Index, the seeds' positions in it)."""
        from . import _kmedoids
        solver, j, lab = self._kept(group)
        index, _ = self._ids(j, lab, [])
        return solver, j, index, _kmedoids.check_seeds(seeds, index)

    def assign(self, seeds, group=None):
        """Every fitted node given to the seed whose row likes it best.  ``seeds``: a sequence of K >= 1 distinct fitted
        labels, or a pandas Series of them (its values are taken: ``medoids(labels)`` is one); cluster j (0 .. K - 1) is
        the j-th seed's.  An empty or repeated seed or a non-sequence is a ValueError, an unknown label a KeyError, before
        any device work.  ``group=1 | 2`` for the bipartite classes.

        ``v(j, a) = S[m_j, a]``: row m_j of the j-th seed, the element ``similarity(m_j, a)`` reads (the matrices are not
        symmetric in general; this is the row whose mean over the members ``cluster_quality`` calls ``own(m_j)``), widened
        as ``rows`` widens it and compared in float64.  Node a gets the first j in the order (``v(j, a)`` descending, j
        ascending): a NaN is never chosen, -0.0 equals +0.0, a seed gets its own cluster, and a node with no candidate
        (every value NaN) gets cluster 0.  A node no seed reaches (every value +0.0) lands in cluster 0 by the tie rule.

        -> DataFrame, one row per node, index = the dense frame's labels in its order: ``cluster`` (int64), ``medoid``
        (that seed's label) and ``similarity`` (float64) = ``v(cluster, a)``; for a seed, its stored diagonal element.

        K rows of the iterate are read in place on the device (libsimrank_kmedoids.so); 12 bytes per node cross.  A model
        held in several column blocks (``LocalWorld(P)``) is packed into one temporary block first; a pruned model is
        answered on the host for its matrix P, whose absent entries are +0.0.  The model is left unchanged."""
        from . import _kmedoids
        solver, j, index, at = self._seeded(seeds, group)
        cluster, value = _kmedoids.assign(solver, j, at)
        return pd.DataFrame({"cluster": cluster, "medoid": index.take(at[cluster]).to_numpy(), "similarity": value},
                            index=index.copy())

    def kmedoids(self, seeds, max_iter=20, group=None):
        """Clusters around medoids: ``assign`` alternated with the move of every cluster's medoid to its most central
        member, until no medoid moves.  ``seeds`` as ``assign`` takes them; ``max_iter``: a positive int (bool refused: a
        ValueError).  Iteration i = 0, 1, ...:

        1. Assign.  i = 0 is ``assign(seeds)``.  From then on a node in cluster c moves to the best j* (the order of
           ``assign``) iff ``v(j*, a) > v(c, a)``, or ``v(c, a)`` is NaN and a candidate exists; otherwise it stays.
           Medoids stay in their clusters.  ``moved`` counts the nodes whose cluster changed (N at i = 0).
        2. Update.  ``own(a)`` of the current labelling is ``cluster_quality``'s: the same kernel on the same lists, the
           same bits.  Cluster j keeps its medoid unless a member has a strictly larger ``own`` (NaN is never larger; a
           NaN incumbent loses to any non-NaN); the new medoid is the member with the largest ``own``, the first in the
           frame's order on a tie.  ``changed`` counts the clusters whose medoid changed.
        3. Stop when ``changed == 0`` (the next assignment would move nothing) or after ``max_iter`` iterations.

        Every change raises ``F = sum of S[m(a), a] over the non-medoids a`` in exact arithmetic, so no configuration
        repeats.

        -> ``(labels, clusters, history)``: ``labels`` is the frame of ``assign`` with the loop's final clusters and
        medoids (under the stay rule a node may sit with a tied medoid of larger j); ``clusters`` has index j and the
        columns ``medoid`` (a label), ``size`` (int64) and ``cohesion`` (float64: the medoid's ``own``, NaN for a
        singleton); ``history`` has one row per iteration: ``moved``, ``changed`` (int64) and ``objective`` (float64) =
        ``math.fsum(cohesion_j * (size_j - 1))`` over the clusters of two members or more, after the update.  The last
        ``changed`` is 0 iff the loop converged.

        Per iteration one ``assign`` kernel, one sweep of ``cluster_quality`` and one pick run on the device; N int32
        labels come to the host, which regroups them and sends the lists back, and two counters come down.  Where
        ``assign`` runs, and as it does for ``LocalWorld(P)`` (packed once per call) and pruned models (on the host).
        The model is left unchanged."""
        from . import _kmedoids
        max_iter = _kmedoids.check_max_iter(max_iter)
        solver, j, index, at = self._seeded(seeds, group)
        cluster, medoids, value, sizes, cohesion, history = _kmedoids.kmedoids(solver, j, at, max_iter)
        labels = pd.DataFrame({"cluster": cluster, "medoid": index.take(medoids[cluster]).to_numpy(), "similarity": value},
                              index=index.copy())
        clusters = pd.DataFrame({"medoid": index.take(medoids).to_numpy(), "size": sizes.astype(np.int64),
                                 "cohesion": np.asarray(cohesion, dtype=np.float64)},
                                index=pd.RangeIndex(len(medoids), name="cluster"))
        moved, changed, objective = zip(*history)
        return labels, clusters, pd.DataFrame({"moved": np.array(moved, dtype=np.int64),
                                               "changed": np.array(changed, dtype=np.int64),
                                               "objective": np.array(objective, dtype=np.float64)})

    def exemplars(self, k, given=None, lazy=True, group=None):
        """Which k nodes stand for all the fitted nodes: greedy facility location.  k times, the node is picked whose row
        raises ``sum over the nodes a of max over the picked m of S[m, a]`` the most; the objective is submodular, so the
        picks are within ``1 - 1/e`` of the best set.  ``picks["exemplar"]`` seeds ``kmedoids``.  ``group=1 | 2`` for the
        bipartite classes.

        Elements.  ``v(m, a) = S[m, a]``: row m, the element ``similarity(m, a)`` reads, widened as ``rows`` widens it
        and then to float64.  This is the orientation of ``assign``: a medoid's ROW covers the nodes.  Every column
        counts, m's own stored diagonal element included.

        Cover.  ``cover[a]`` starts at +0.0: a node nothing stands for is covered at similarity 0.  Applying row p sets
        ``cover[a] = v(p, a)`` iff ``v(p, a) > cover[a]``; that is false for a NaN, which never covers, never counts and
        never gains.  ``given``: None or a sequence of distinct fitted labels; their rows are applied first, in the order
        given, and they are never picked.

        Gain.  ``term(m, a) = v(m, a) - cover[a]`` if ``v(m, a) > cover[a]``, else +0.0: one float64 subtraction, nothing
        fused.  ``gain(m)`` is the float64 sum of the terms over all columns, in an order that depends on the number of
        columns alone and is the same for every storage (include/simrank_exemplars.h states it): no floating-point
        atomics, two runs give the same bits, and ``|gain - exact| <= (N + 1) * 2^-52 * (the exact sum of the terms)``.

        Picks.  k times the candidate (a node neither picked nor given) that is first in the order (gain descending,
        position in the dense frame's label order ascending) is picked and its row applied.  ``1 <= k <= N - len(given)``.

        Monotonicity.  ``cover`` only rises; rounded subtraction is monotone and so is rounded addition in a fixed tree,
        so a gain computed against an older cover is an upper bound of the gain now, in floating point as in exact
        arithmetic.  ``lazy=True`` relies on it: it keeps every candidate's last gain as a bound, refreshes the first
        ``_exemplars.BATCH`` stale candidates in the order above until the first candidate is fresh, and returns the bits
        ``lazy=False`` (one sweep of all rows per pick) returns; only ``evaluated`` differs.  ``lazy=True`` is the
        default because it is the faster one (DESIGN.md 4.33 has the numbers).

        -> ``(picks, coverage)``.  ``picks``: one row per pick, index ``rank`` 0 .. k - 1, columns ``exemplar`` (the
        label), ``gain`` (float64: the fresh gain at the moment of the pick), ``raised`` (int64: the columns whose cover
        the pick raised, exact) and ``evaluated`` (int64: the rows whose gain was computed for this pick; with
        ``lazy=False`` the number of candidates).  ``coverage``: a float64 Series named ``"coverage"`` over the dense
        frame's labels in its order, the final ``cover``: maxima only, so every bit equals ``np.maximum.reduce`` over
        ``rows(given + picked)`` with the +0.0 start and the NaN rule.

        A bad ``k`` (not an int, a bool, below 1, above ``N - len(given)``), a bad ``given`` (a str, a scalar, a
        repeated label), a bad ``lazy`` (no bool) or ``group`` is a ValueError, an unknown label in ``given`` a KeyError,
        all before any device work.

        The rows are read in place on the device (libsimrank_exemplars.so); per round a list of rows goes up and their
        gains come down.  Where ``kmedoids`` runs: kept, compact and loaded models, f32, fp16-held and float64.  A model
        held in several column blocks (``LocalWorld(P)``) is packed into one temporary block once per call.  A pruned
        model is answered on the host for its matrix P: absent entries are +0.0 and never gain, and a gain there is
        ``math.fsum`` of the terms.  The sum runs over the columns as the model holds them, so on a model that still
        holds its plan (the solver's order) a gain may differ in its last bits from the compact model's, and two
        candidates tied to within the rounding bound may then swap; compact and loaded models (the frame's order) are
        the canonical form.  The model is left unchanged."""
        from . import _exemplars
        solver, j, lab = self._kept(group)
        index, _ = self._ids(j, lab, [])
        at = _exemplars.check_given(given, index)
        k = _exemplars.check_k(k, len(index), at.size)
        lazy = _exemplars.check_lazy(lazy)
        picked, gain, raised, evaluated, cover = _exemplars.exemplars(solver, j, k, at, lazy)
        picks = pd.DataFrame({"exemplar": index.take(picked).to_numpy(), "gain": gain, "raised": raised,
                              "evaluated": evaluated}, index=pd.RangeIndex(k, name="rank"))
        return picks, pd.Series(cover, index=index.copy(), name="coverage")

    def compare(self, other, tolerances=(1e-5,), top_k=10, floor=0.0):
        """How far apart two models of one graph are: ``other`` is another estimator holding a model (kept, compact or
        loaded; any mix of f32, fp16-held and float64; ``other is self`` is allowed and gives all zeros).  Both models
        must have the same number of groups, the same labels in the same order per group and live on the same device; a
        pruned model on either side stands for a different matrix P (compare before ``prune``).  Every violation is a
        ValueError before any device work that names the first difference; a released model is the usual RuntimeError.

        For the elements ``a = S[r, c]`` of this model and ``b`` of ``other``, each widened as ``rows`` widens it: ``d`` is
        +0.0 if ``a == b`` (so -0.0 and +0.0 agree, and equal infinities agree) or both are NaN, +inf if exactly one is
        NaN, otherwise ``fabs(a - b)``; ``rel`` is +0.0 if ``d == 0`` or ``max(|a|, |b|) < floor``, +inf if ``d == inf``,
        otherwise ``d / max(|a|, |b|)``, the first rule that applies (a NaN operand is below no floor).  The diagonal is included.  ``tolerances``: 0 to 7 finite numbers >= 0;
        ``floor``: a finite number >= 0; ``top_k``: None or a positive int, clamped to N - 1 (above 4096 after that: a
        ValueError).

        -> ``(summary, nodes, histogram)``; a tuple of two such triples for the bipartite classes.

        ``nodes``, indexed by the dense frame's labels in its order: ``max_abs`` (float64) the largest ``d`` of the
        node's row and ``at`` the label of the first column attaining it, ``max_rel`` and ``at_rel`` the same for
        ``rel``, ``differing`` (int64) the columns with ``d > 0`` and one ``over@<tol>`` column (int64) per tolerance: the
        columns with ``d > tol``.  With ``top_k=k`` also ``overlap``: how many nodes both models' k best OTHER nodes of
        the row share, and ``same_prefix``: the number of leading ranks at which both lists name the same node; the
        lists are ``most_similar``'s, in the project's total order, so they are functions of the matrices alone.

        ``summary``, one row: ``entries`` (N^2), ``differing``, ``max_abs`` with its pair ``node`` and ``neighbor``,
        ``max_rel`` with ``node_rel`` and ``neighbor_rel`` (a maximum attained more than once: the first pair in
        row-major order), the ``over@<tol>`` totals (int64) and, with ``top_k``, ``mean_overlap`` and
        ``identical_lists``: the nodes with ``same_prefix == k``.

        ``histogram``: an int64 Series over the 2048 exponent bins ``bits(d) >> 52``, indexed by the bin number: bin 0
        holds ``d == 0`` and subnormal ``d``, bin e holds ``2^(e-1023) <= d < 2^(e-1022)``, bin 2047 holds ``d == inf``.

        Nothing is a floating-point sum: every number is a function of the two matrices alone, bit for bit.  One sweep
        of both matrices in place on the device (libsimrank_compare.so); a few numbers per node cross.  A compact or
        loaded model is read in place; a model that still holds its plan, or is held in several column blocks
        (``LocalWorld(P)``), is packed into one temporary block in the frame's order first: each such model costs one
        more copy of its matrices (N^2 x 4 | 2 | 8 bytes per side) next to its plan for the length of the call, both
        copies alive at once; ``compact()`` first where that does not fit.  Both models are left unchanged."""
        from . import _compare
        solver, sides = self._solver_sides()
        if not isinstance(other, _KeptModel):
            raise ValueError(f"other must be an estimator holding a model, not {type(other).__name__}")
        other_solver, other_sides = other._solver_sides()
        for which, model in (("this", self), ("the other", other)):
            if model.kept_neighbors is not None:
                raise ValueError(f"{which} model was pruned to kept_neighbors = {model.kept_neighbors}: it stands for a "
                                 "different matrix P; compare before prune()")
        _compare.check_sides(sides, other_sides)
        tols = _compare.check_tolerances(tolerances)
        floor = _compare.check_floor(floor)
        k = _compare.check_top_k(top_k, [len(lab) for _, lab in sides])
        ops, other_ops = next(iter(solver.ops.values())), next(iter(other_solver.ops.values()))
        dev, other_dev = getattr(ops, "device", None), getattr(other_ops, "device", None)
        if dev != other_dev:
            raise ValueError(f"the two models live on different devices ({dev} and {other_dev})")
        swept = tuple(sorted(set(tols) | {0.0}))
        with contextlib.ExitStack() as scope:
            mine = scope.enter_context(_compare.callers_readers(solver))
            theirs = mine if other_solver is solver else scope.enter_context(_compare.callers_readers(other_solver))
            for o in (ops, other_ops):
                o.synchronize()                             # (the two models have streams of their own)
            out = []
            for s, (j, lab) in enumerate(sides):
                got = _compare.compare_readers(mine[s], theirs[s], swept, floor, k)
                other_ops.synchronize()
                out.append(self._compare_frames(self._ids(j, lab, [])[0], got, swept, tols))
        return out[0] if len(out) == 1 else tuple(out)

    @staticmethod
    def _compare_frames(index, got, swept, tols):
        """``compare``'s three frames of one group from the arrays of ``_compare.compare_readers``."""
        n = len(index)
        over = got["over"].astype(np.int64)
        label_at = lambda arg: index.take(np.maximum(arg, 0)).to_numpy() if n else np.empty(0, dtype=object)
        cols = {"max_abs": got["max_abs"], "at": label_at(got["arg_abs"]), "max_rel": got["max_rel"],
                "at_rel": label_at(got["arg_rel"]), "differing": over[:, swept.index(0.0)]}
        for t in tols:
            cols[f"over@{t!r}"] = over[:, swept.index(t)]
        if "overlap" in got:
            cols["overlap"], cols["same_prefix"] = got["overlap"], got["same_prefix"]
        nodes = pd.DataFrame(cols, index=index.copy())
        one = {"entries": np.int64(n) * np.int64(n), "differing": cols["differing"].sum(dtype=np.int64)}
        for value, arg, node, neighbor in (("max_abs", "arg_abs", "node", "neighbor"),
                                           ("max_rel", "arg_rel", "node_rel", "neighbor_rel")):
            r = int(np.argmax(got[value])) if n else -1     # (the first row attaining the maximum; d and rel are never NaN)
            one[value] = got[value][r] if n else 0.0
            one[node] = index[r] if n else None
            one[neighbor] = index[int(got[arg][r])] if n else None
        for t in tols:
            one[f"over@{t!r}"] = cols[f"over@{t!r}"].sum(dtype=np.int64)
        if "overlap" in got:
            one["mean_overlap"] = float(got["overlap"].sum(dtype=np.int64)) / n if n else 0.0
            one["identical_lists"] = np.int64((got["same_prefix"] == got["k"]).sum())
        summary = pd.DataFrame({name: [value] for name, value in one.items()})
        histogram = pd.Series(got["hist"], index=pd.RangeIndex(len(got["hist"]), name="bin"), name="count", dtype=np.int64)
        return summary, nodes, histogram

    def compact(self, precision=None):
        """Cut the kept model loose from its plan: every side's iterate is packed into ONE device matrix in the dense
        frame's order (libsimrank_model.so), then the plan's matrices are released (the evidence counts stay, so the lazy
        ``Evidence`` attributes keep working).  Every query answers as before, bit for bit.  ``precision``: None keeps the
        model's storage (f32, fp16-held or float64); "fp16" also narrows an f32 model to the fp16-held form (value x 2^14
        in binary16, round to nearest even: relative error <= 2^-11 down to 2^-28, absolute <= 2^-39 below), a ValueError
        that names the count, with the model left as it was, when a value does not fit, and a ValueError before any device
        work on a float64 model.  Peak device memory during the call is the plan plus the copy; afterwards N^2 x (4 | 2 |
        8) bytes per side plus, once ``fold_in`` ran, the side's CSR.  Idempotent; returns the estimator.  A pruned model
        (``prune``) is returned unchanged; narrowing one is a ValueError."""
        from . import _model
        _model.check_precision(precision)
        solver, sides = self._solver_sides()
        if self.kept_neighbors is not None:
            if precision is not None:
                raise ValueError("compact(precision='fp16') narrows a model's matrix; a pruned model holds float64 "
                                 "neighbour lists and no matrix")
            return self
        if isinstance(solver, _model.DetachedSolver) and (precision is None or solver.storage == "fp16"):
            return self
        detached = _model.detach(solver, precision)         # (raises with the kept model intact)
        self._model = (detached, sides)
        solver.release()
        return self

    def prune(self, k):
        """Keep, for every node of every group, its ``k`` most similar OTHER nodes and the diagonal element, and release
        the model's matrices (the evidence counts stay, as after ``compact``): N x k x 12 + N x 8 bytes per side instead
        of N^2 x (4 | 2 | 8).  The kept entries are chosen in the total order (value descending, label position
        ascending; -0.0 and +0.0 tie, NaN is never kept; exact zeros count where they fall inside the first k): exactly
        the entries, in the order, that ``most_similar([a], k)`` returned before.  ``k`` is clamped to N - 1 per group.
        Values are stored widened to float64, as every query returns them.

        From then on every query answers for the matrix P that holds the kept entries, the diagonal and +0.0 everywhere
        else, bit for bit as the same query would on a dense model holding P: ``frame``, ``rows``, ``similarity``,
        ``pairs``, ``score_sets`` and ``recommend``; ``most_similar(nodes, k2)`` and ``top_k(k2)`` with ``k2 <= k`` return
        what the unpruned model returned (``k2 > k`` is a ValueError).  P is in general NOT symmetric: ``similarity(a, b)``
        reads a's list, so b may be among a's k best while a is not among b's.  ``fold_in`` needs whole rows and is a
        ValueError: fold in before pruning.  ``save`` writes the lists; ``load_model`` reads them back.

        Works on a kept, a compact and a loaded model; a model held in several column blocks (``LocalWorld(P)``) is packed
        into one temporary block first (peak memory: the plan plus that copy).  On a pruned model ``k`` at most
        ``kept_neighbors`` cuts the lists, a larger one is a ValueError.  Every refusal comes before any device work.
        Returns the estimator."""
        from . import _neighbors
        from ._query import check_k
        check_k(k)                                          # (judged before the model, and again with its sizes)
        solver, sides = self._solver_sides()
        k = _neighbors.check_prune_k(k, solver.n)
        if isinstance(solver, _neighbors.NeighborSolver):
            self._check_kept_neighbors(solver, range(len(solver.n)), k)
            if all(_neighbors.clamp_k(k, n) == kk for n, kk in zip(solver.n, solver.kept_k)):
                return self
            pruned = solver.truncated(k)
        else:
            pruned = _neighbors.prune(solver, k)            # (raises with the kept model intact)
        self._model = (pruned, sides)
        solver.release()
        return self

    @staticmethod
    def _check_kept_neighbors(solver, js, k):
        """ValueError when ``k`` (as the queries clamp it) asks a pruned model for more than it keeps."""
        kept = getattr(solver, "kept_k", None)
        if isinstance(kept, list):
            for j in js:
                if min(k, max(1, solver.n[j] - 1)) > kept[j]:
                    raise ValueError(f"this model was pruned to kept_neighbors = {kept[j]} neighbours per node: k = {k} asks "
                                     f"for more than it keeps")

    @property
    def kept_neighbors(self):
        """k of ``prune(k)`` (as clamped; a tuple of two where the two groups of a bipartite model were clamped
        differently), or None on a model that was not pruned."""
        if self._model is None:
            return None
        kept = getattr(self._model[0], "kept_k", None)
        if not isinstance(kept, list):
            return None
        return kept[0] if len(set(kept)) == 1 else tuple(kept)

    @property
    def device_bytes(self):
        """Bytes of device memory in the model's own matrices: the packed blocks of a compact model; of a model that still
        holds its plan, the iterates the queries read (the plan holds more: see ``compact``); the neighbour lists of a pruned
        model (N x k x 12 + N x 8 per side)."""
        from . import _model
        solver, sides = self._solver_sides()
        if isinstance(solver, _model.DetachedSolver) or self.kept_neighbors is not None:
            return solver.device_bytes
        return sum(_model.block_bytes(b) for j, _ in sides for b in solver._reader(j).blocks)

    def save(self, path):
        """Write the model to one file ``load_model`` reads back (a JSON header, then raw little-endian arrays: the packed
        iterates, the CSR and the row scales; no pickle).  A model that still holds its plan is packed into a temporary
        block first and stays as it is.  Labels must be Python ``int`` (any size) or ``str``, or the integers of one NumPy
        integer type; anything else is a ValueError that names the type.  A pruned model writes its neighbour lists
        instead of the iterates (header "form": "neighbors"; the format version is the same)."""
        from . import _model
        solver, sides = self._solver_sides()
        labels = [lab for _, lab in sides]
        for lab in labels:
            _model.encode_labels(lab)                       # (ValueError before any device work)
        meta = {"class": type(self).__name__, "weighted": bool(getattr(self, "_weighted", False)),
                "strict": self._strict(solver),
                "converged_at": getattr(self, "converged_at", None), "engine_mode": getattr(self, "engine_mode", None)}
        if isinstance(solver, _model.DetachedSolver) or self.kept_neighbors is not None:
            _model.save(path, solver, meta, labels)
            return
        temp = _model.detach(solver)
        try:
            _model.save(path, temp, meta, labels)
        finally:
            temp.release()

    def release(self):
        """Free the kept model's device memory (the lazy ``Evidence`` attributes keep working); queries raise afterwards."""
        if self._model is not None:
            solver = self._model[0]
            self._model = None
            self._model_released = True
            solver.release()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
