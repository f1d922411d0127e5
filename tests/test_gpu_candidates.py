"""libsimrank_candidates.so and the ``among=`` / ``exclude=`` keywords on a real MI355X.  Every comparison is bit for bit:
nothing is summed that was not summed before.

Kernel level, on synthetic blocks (tests/blocks.py, no fit): ``simrank_candidates_topk`` EQUALS ``candidates_ref.ref_topk``
in all four layouts, on the blocks of tests/test_gpu_neighbors.py (a row of one repeated value, a row of both zeros, NaN
and -inf), with the block's column ids a permutation (the id-sorted list has non-monotonic positions), on both sides of
the staging cap (the list that is not staged also at the largest k and with ids), at the largest k and where one
workgroup takes several turns; with every column listed it equals ``simrank_neighbors_select``.

Model level, at N = 300: ``most_similar``, ``score_sets`` and ``recommend`` with ``among=`` equal the NumPy statements on
``model.frame()`` and the unfiltered calls filtered, re-ranked and cut."""
import numpy as np
import pandas as pd
import pytest

from simrank_amd import _candidates, _neighbors, synth
from tests import blocks as B
from tests import candidates_ref as CR
from tests import diverse_ref as D
from tests import sets_ref
from tests.graphs import bipartite_random
from tests.test_gpu_neighbors import dev, device, same_bits, tie_block  # noqa: F401 (the fixtures)
from tests.test_gpu_sets import model_of, same_frame

pytestmark = pytest.mark.gpu


# ---- kernel level ---------------------------------------------------------------------------------------------------------
def topk(dev, blk, rows, cand_pos, cand_ids, k):  # noqa: F811
    """(ids, values) of one call on the block ``blk`` = (device pointer, layout, stride, n_rows, n_cols) for the query rows
    ``rows`` = (device row_pos, device row_ids, n_q); the outputs carry one guard row that must come back untouched."""
    lib, (rp, rid, n_q) = _candidates.load(), rows
    hi, hv = np.full((n_q + 1, k), -9, dtype=np.int32), np.full((n_q + 1, k), 1e300)
    idx, val = dev.put(hi), dev.put(hv)
    cand_pos = np.ascontiguousarray(cand_pos, dtype=np.int32)
    _candidates.check(lib.simrank_candidates_topk(
        *blk, rp, rid, n_q, dev.put(cand_pos) if cand_pos.size else None,
        None if cand_ids is None else dev.put(np.ascontiguousarray(cand_ids, dtype=np.int32)), cand_pos.size, k, idx, val,
        dev.ops.stream), "simrank_candidates_topk")
    got_i, got_v = dev.get(idx, hi), dev.get(val, hv)
    assert (got_i[n_q] == -9).all() and (got_v[n_q] == 1e300).all()
    return got_i[:n_q], got_v[:n_q]


def check_topk(dev, blk, A, rows, row_pos, row_ids, cand_pos, cand_ids, k, what):  # noqa: F811
    got_i, got_v = topk(dev, blk, rows, cand_pos, cand_ids, k)
    want_i, want_v = CR.ref_topk(A, row_pos, row_ids, cand_pos, cand_ids, k)
    same_bits(got_i, want_i, ("ids", what))
    same_bits(got_v, want_v, ("values", what))
    return got_i, got_v


KS = (1, 3, 64, 130)


def candidate_lists(n_cols, k, own_col, rng):
    """name -> columns of the block (any order: the caller sorts them by id)."""
    some = lambda m: rng.permutation(n_cols)[:m]
    lists = {"empty": np.empty(0, dtype=np.int64), "one": some(1), "own": np.array([own_col]), "all": np.arange(n_cols),
             "every second": np.arange(0, n_cols, 2)}
    for m in (k - 1, k, k + 1, 63, 64, 65, 257):
        if 0 < m <= n_cols:
            lists["%d columns" % m] = some(m)
    return lists


@pytest.mark.parametrize("layout", B.LAYOUTS)
@pytest.mark.parametrize("shape", [(67, 130), (5, 2100)])
def test_topk_is_the_contract(dev, layout, shape):  # noqa: F811
    n_rows, n_cols = shape
    nlib, st = _neighbors.load(), dev.ops.stream
    for v, (tag, stride, base) in enumerate(B.variants(layout, n_rows, n_cols)):
        A, raw = tie_block(layout, n_rows, n_cols, stride, 11 + v)
        blk = (dev.put(raw, base), layout, stride, n_rows, n_cols)
        rng = np.random.default_rng([n_cols, layout, v, 5])
        row_pos = np.concatenate([[0, 1, 2], rng.permutation(n_rows)[:4], [n_rows, 1]]).astype(np.int32)
        rng.shuffle(row_pos)                                            # (row 1 twice, one position outside)
        col_ids = rng.permutation(n_cols).astype(np.int32)              # a permutation: positions and ids disagree
        own_cols = (row_pos.astype(np.int64) * 5 + 1) % n_cols
        row_ids = col_ids[own_cols]                                     # every row's own id is the id of some column
        rows = (dev.put(row_pos), dev.put(row_ids), row_pos.size)
        rows_by_pos = (rows[0], dev.put(own_cols.astype(np.int32)), row_pos.size)      # (without ids: own id = own column)
        ids_dev = dev.put(col_ids)
        for k in KS:
            for name, cols in candidate_lists(n_cols, k, own_cols[0], rng).items():
                order = np.argsort(col_ids[cols], kind="stable")        # the caller's list: ascending ids
                pos, ids = cols[order], col_ids[cols][order]
                assert cols.size < 20 or (np.diff(pos) < 0).any()
                what = (layout, shape, tag, name, k)
                got = check_topk(dev, blk, A, rows, row_pos, row_ids, pos, ids, k, what)
                if name == "all":                                       # what the unfiltered selection returns
                    hi, hv = np.full_like(got[0], -9), np.full_like(got[1], 1e300)
                    ni, nv = dev.put(hi), dev.put(hv)
                    _neighbors.check(nlib.simrank_neighbors_select(*blk, *rows, ids_dev, k, ni, nv, st), "select")
                    same_bits(got[0], dev.get(ni, hi), ("ids against neighbors_select", what))
                    same_bits(got[1], dev.get(nv, hv), ("values against neighbors_select", what))
                if name in ("all", "every second", "own"):              # without ids a candidate's id is its position
                    check_topk(dev, blk, A, rows_by_pos, row_pos, own_cols, np.sort(cols), None, k, what + ("no ids",))
            # positions outside the block are not read and are no candidates, wherever they stand in the list
            cols = rng.permutation(n_cols)[:40].astype(np.int64)
            pos = np.concatenate([[-1], cols[:20], [n_cols], cols[20:]])
            ids = np.concatenate([[n_cols + 3], col_ids[cols[:20]], [n_cols + 4], col_ids[cols[20:]]])
            check_topk(dev, blk, A, rows, row_pos, row_ids, pos, ids, k, (layout, shape, tag, "outside", k))
        dev.release()


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_both_sides_of_the_staging_cap_and_the_largest_k(dev, layout):  # noqa: F811
    rng = np.random.default_rng([layout, 77])
    c = _candidates.staged(layout)
    cases = [(2, 5100, [(5000, 4096)])]
    if c > 0:
        cases.append((3, c + 70, [(m, k) for m in (c - 1, c, c + 1) for k in (1, 100)] + [(c + 1, _candidates.MAX_K)]))
    for n_rows, n_cols, runs in cases:
        tag, stride, base = B.variants(layout, n_rows, n_cols)[0]
        blk = B.make_long(layout, n_rows, n_cols, stride, 3)
        where = (dev.put(blk.raw, base), layout, stride, n_rows, n_cols)
        row_pos = np.array([n_rows - 1, 0, n_rows, 1], dtype=np.int32)
        row_ids = np.array([5, n_cols, 0, 7], dtype=np.int32)
        rows = (dev.put(row_pos), dev.put(row_ids), row_pos.size)
        for m, k in runs:
            pos = rng.permutation(n_cols)[:m]                           # (no ids: the list order alone decides the ties)
            check_topk(dev, where, blk.A, rows, row_pos, row_ids, pos, None, k, (layout, n_cols, m, k))
        if c > 0 and n_cols > c:
            # not staged, with ids: the columns' ids a permutation, the list sorted by id, every row's own id in it
            col_ids = rng.permutation(n_cols).astype(np.int32)
            cols = rng.permutation(n_cols)[:c + 1]
            order = np.argsort(col_ids[cols], kind="stable")
            pos, ids = cols[order], col_ids[cols][order]
            own = ids[[7, c, 0, c // 2]]
            assert (np.diff(ids) > 0).all() and (np.diff(pos) < 0).any()
            check_topk(dev, where, blk.A, (rows[0], dev.put(own), row_pos.size), row_pos, own, pos, ids, 100,
                       (layout, n_cols, c + 1, "ids"))
        dev.release()


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_a_workgroup_takes_several_turns(dev, layout):  # noqa: F811
    n_rows, n_cols, k = 5, 70, 3
    tag, stride, base = B.variants(layout, n_rows, n_cols)[0]
    A, raw = tie_block(layout, n_rows, n_cols, stride, 4)
    where = (dev.put(raw, base), layout, stride, n_rows, n_cols)
    n_q = _candidates.MAX_BLOCKS + 5
    row_pos = (np.arange(n_q) % n_rows).astype(np.int32)
    row_ids = (np.arange(n_q) % 7).astype(np.int32)
    pos = np.random.default_rng(layout).permutation(n_cols)[:40]
    got_i, got_v = topk(dev, where, (dev.put(row_pos), dev.put(row_ids), n_q), pos, None, k)
    first = n_rows * 7                                                  # (the pairs (row, own id) repeat with this period)
    want_i, want_v = CR.ref_topk(A, row_pos[:first], row_ids[:first], pos, None, k)
    reps = -(-n_q // first)
    same_bits(got_i, np.tile(want_i, (reps, 1))[:n_q], ("ids", layout))
    same_bits(got_v, np.tile(want_v, (reps, 1))[:n_q], ("values", layout))


# ---- model level ------------------------------------------------------------------------------------------------------------
N = 300


@pytest.fixture(scope="module")
def graph():
    return synth.er_directed(N, 0.008, seed=7)


def as_groups(x):
    return list(x) if isinstance(x, tuple) else [x]


def filtered(long, allowed, k):
    """The unfiltered long frame cut to the neighbours in ``allowed``, re-ranked within each block and cut at k."""
    block = (long["rank"] == 1).cumsum()
    keep = long["neighbor"].isin(set(allowed)).to_numpy()
    out = long[keep].copy()
    out["rank"] = out.groupby(block[keep]).cumcount().to_numpy() + 1
    return out[out["rank"] <= k].reset_index(drop=True)


def candidate_sets(labels, rng):
    n = len(labels)
    pick = lambda m: [labels[i] for i in rng.permutation(n)[:m]]
    return [[], pick(1), pick(max(2, n // 8)), list(labels)]


def check_most_similar(model, frame, group, pruned=False):
    kw = {} if group is None else {"group": group}
    labels, n = list(frame.index), len(frame)
    rng = np.random.default_rng(n)
    for C in candidate_sets(labels, rng):
        inside, outside = list(C[:3]), [x for x in labels if x not in set(C)][:3]
        nodes = inside + outside + inside[:1] + [labels[0]]
        for E in ([], [labels[1]] + list(C[1:4])):
            for k in (1, 10):
                if pruned and min(k, max(1, len(set(C) - set(E)))) > 20:
                    continue
                got = model.most_similar(nodes, k, among=C + C[:2], exclude=E, **kw)
                same_frame(got, CR.ref_most_similar(frame, nodes, k, C, E), ("statement", len(C), len(E), k))
                if not pruned:
                    full = model.most_similar(nodes, n - 1, **kw)
                    same_frame(got, filtered(full, set(C) - set(E), k), ("filtered", len(C), len(E), k))
    # exclude alone: every node but those; both None: the call without the keywords
    nodes = labels[:5]
    if not pruned:
        same_frame(model.most_similar(nodes, 7, exclude=labels[2:40], **kw),
                   CR.ref_most_similar(frame, nodes, 7, None, labels[2:40]), "exclude alone")
    same_frame(model.most_similar(nodes, 7, among=None, exclude=None, **kw), model.most_similar(nodes, 7, **kw), "both None")


def check_score_sets(model, frame, group):
    kw = {} if group is None else {"group": group}
    labels, n = list(frame.index), len(frame)
    rng = np.random.default_rng(n + 1)
    pick = lambda m: [labels[i] for i in rng.permutation(n)[:m]]
    sets = [[], pick(1), [labels[5], labels[7], labels[5]], pick(37), pick(9)]
    weights = [list(rng.choice([-1.0, 1.0], size=len(s)) * 10.0 ** rng.uniform(-6, 3, size=len(s))) for s in sets]
    other = [labels[:3], [], labels[2:n - 9], [], [labels[0]]]
    fulls = [model.score_sets(sets, weights=weights, top_k=n, exclude=X, **kw) for X in ("members", None, other)]
    for C in candidate_sets(labels, rng):
        rest = [x for x in labels if x not in set(C)]
        for X, full in zip(("members", None, other), fulls):
            for k in (1, 10):
                got = model.score_sets(sets, weights=weights, top_k=k, among=C + C[:1], exclude=X, **kw)
                same_frame(got, filtered(full, C, k), ("score_sets", len(C), X if X is None else "x", k))
                # diversity: the statement on the dense band with the columns outside C marked -inf
                gone = [list(s if X == "members" else [] if X is None else x) + rest for s, x in zip(sets, other)]
                same_frame(model.score_sets(sets, weights=weights, top_k=k, among=C, exclude=X, diversity=0.3, **kw),
                           D.score_sets_ref(frame, sets, weights, top_k=k, exclude=gone, diversity=0.3),
                           ("diverse", len(C), X if X is None else "x", k))
    same_frame(model.score_sets(sets, top_k=5, among=None, **kw), model.score_sets(sets, top_k=5, **kw), "among None")


def check_recommend(model, group):
    frames = as_groups(model.frame())
    solver, sides = model._model
    bip = len(sides) == 2
    side = 0 if group in (None, 1) else 1
    own, read = frames[side], frames[len(frames) - 1 - side]
    spec = solver.specs[side]
    rowptr, col, scale = np.asarray(spec.csr.rowptr), np.asarray(spec.csr.col), np.asarray(spec.rowscale)
    labels, src = list(own.index), list(read.index)
    kw = {} if group is None else {"group": group}
    rng = np.random.default_rng(23)
    deg = np.diff(rowptr)
    nodes = [labels[int(np.argmax(deg))], labels[int(np.argmin(deg))]] + [labels[i] for i in rng.permutation(len(labels))[:8]]
    us = [labels.index(x) for x in nodes]
    lists = [list(col[rowptr[u]:rowptr[u + 1]]) for u in us]
    dense = sets_ref.scores(read.values, lists, [np.full(len(l), scale[u]) for l, u in zip(lists, us)])
    fulls = [model.recommend(nodes, len(src), exclude_seen=seen, **kw) for seen in (True, False)]
    for C in candidate_sets(src, rng):
        rest = [i for i, x in enumerate(src) if x not in set(C)]
        for seen, full in zip((True, False), fulls):
            for k in (1, 10):
                got = model.recommend(nodes, k, exclude_seen=seen, among=C, **kw)
                same_frame(got, filtered(full, C, k), ("recommend", len(C), seen, k))
                gone = [(l + ([u] if not bip else []) if seen else []) + rest for l, u in zip(lists, us)]
                want = D.long_frame("node", pd.Index(labels).take(np.asarray(us, dtype=np.int64)), src, dense, read.values,
                                    min(k, len(src)), 0.3, gone, keep=[len(l) > 0 for l in lists])
                same_frame(model.recommend(nodes, k, exclude_seen=seen, among=C, diversity=0.3, **kw), want,
                           ("recommend diverse", len(C), seen, k))
    same_frame(model.recommend(nodes, 5, among=None, **kw), model.recommend(nodes, 5, **kw), "among None")


DIRECTED = [("SimRank", "f32-kept"), ("SimRank", "fp16-kept"), ("SimRank", "f64-kept"), ("SimRankPP", "f32-kept"),
            ("SimRankPP", "fp16-kept"), ("SimRankPP", "f64-kept"), ("SimRank", "f32-compact"),
            ("SimRank", "f32-compact-fp16"), ("SimRank", "loaded"), ("SimRank", "world3-kept"), ("SimRank", "pruned")]


@pytest.mark.parametrize("cls,variant", DIRECTED)
def test_among_on_a_directed_fit(cls, variant, graph, tmp_path):
    pruned = variant == "pruned"
    with model_of(cls, graph, "f32-kept" if pruned else variant, tmp_path) as model:
        if pruned:
            model.prune(20)
        frame = model.frame()
        before = frame.values.copy()
        check_most_similar(model, frame, None, pruned)
        check_score_sets(model, frame, None)
        check_recommend(model, None)
        assert np.array_equal(model.frame().values.view(np.uint64), before.view(np.uint64))    # the model is as it was


def test_among_on_a_bipartite_fit(tmp_path):
    df = bipartite_random(33, 65, 0.15, 12)
    with model_of("BipartiteSimRankPP", df, "f32-kept", tmp_path, strict_reference=False) as model:
        for group, frame in zip((1, 2), model.frame()):
            check_most_similar(model, frame, group)
            check_score_sets(model, frame, group)
            check_recommend(model, group)
