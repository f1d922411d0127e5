"""libsimrank_linkage.so, ``linkage`` and ``cut`` on a real MI355X.

Kernel level, on synthetic blocks (tests/blocks.py, no fit; padding holds a finite sentinel above every value, which a
kernel that reads padding would turn into the first merge): the four C entries, driven round by round, give a forest
whose canonical rows are ``linkage_ref``'s, in all four layouts, with id arrays and without, on shapes around the 8-row
pieces, the 32- and 64-column panels and the vector tails; with NaN and zeros of both signs; with an edge only below the
diagonal; over two column blocks into one forest; on a shuffled path of 2049 nodes with rising weights (one round, one
hook chain across workgroups); on an all-ones block (one round, one N-way tie); under a floor.  The status word stays 0,
the guard words after every array survive, the rounds stay within ceil(log2 n) + 1 and a second run gives the same integers.

Model level: ``linkage`` equals ``linkage_ref`` on ``model.frame()`` for every storage, a ``LocalWorld(3)``, compact,
loaded and pruned models and both groups of a bipartite class; ``cut`` equals ``components``; the model is unchanged."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest

from simrank_amd import _linkage, synth
from tests import blocks as B
from tests import cluster_ref as CR
from tests import linkage_ref as LR
from tests.graphs import bipartite_random
from tests.test_gpu_cluster import GUARD, SHAPES, VARIANTS, Dev, as_groups, id_cases, make_model, off_diagonal, sparse_prior

pytestmark = pytest.mark.gpu

GUARD64 = np.uint64(0x5A5A5A5A5A5A5A5A)
KINDS = ("dyadic", "wide")


@pytest.fixture(scope="module")
def device():
    d = Dev()
    yield d
    d.release()
    d.ops.close()


@pytest.fixture
def dev(device):
    yield device
    device.release()


def floor_ref(layout, floor):
    """The floor as simrank_linkage_pick takes it: NULL, or a host pointer to a value in the compare type."""
    if floor is None:
        return None
    return C.byref(C.c_double(floor) if layout == B.ROWMAJOR_F64 else C.c_float(float(_linkage.edges_f32([floor])[0])))


def forest(dev, blocks, n, layout, floor=None):
    """The four C entries on ``blocks`` [(S, stride, n_rows, n_cols, row_ids, col_ids)], round by round as the header
    says -> (hook_other int32 [n], hook_value float64 [n], the rounds that hooked something).  The status word is 0
    after every round, the guard word after each of the five arrays survives, the slots are empty again and every comp[i]
    is a root."""
    lib, st = _linkage.load(), dev.ops.stream
    wide = layout == B.ROWMAJOR_F64
    comp_h, other_h = np.full(n + 1, GUARD, dtype=np.int32), np.full(n + 1, GUARD, dtype=np.int32)
    best_h, value_h = np.full(2 * n + 1, GUARD64, dtype=np.uint64), np.full(n + 1, GUARD64, dtype=np.uint64)
    state_h = np.full(3, GUARD, dtype=np.int32)
    comp, other, best, value, state = (dev.put(x) for x in (comp_h, other_h, best_h, value_h, state_h))
    status = state + 4
    _linkage.check(lib.simrank_linkage_init(comp, best, other, value, n, state, status, st), "init")
    fl = floor_ref(layout, floor)
    rounds = total = 0
    while True:
        rounds += 1
        assert rounds <= _linkage.max_rounds(n), (rounds, n)
        for phase in range(2 if wide else 1):
            for S, stride, n_rows, n_cols, row_ids, col_ids in blocks:
                _linkage.check(lib.simrank_linkage_pick(S, layout, stride, n_rows, n_cols, row_ids, col_ids, fl, phase, comp,
                                                        best, n, status, st), "pick")
        _linkage.check(lib.simrank_linkage_hook(best, 64 if wide else 32, comp, other, value, n, state, status, st), "hook")
        _linkage.check(lib.simrank_linkage_flatten(comp, best, n, status, st), "flatten")
        words = dev.get(state, state_h)
        assert words[1] == 0 and words[2] == GUARD, words
        if words[0] == total:
            rounds -= 1                                       # (the round that found nothing left to join)
            break
        total = int(words[0])
        if total == n - 1:
            break
    got_comp, got_other, got_best, got_value = (dev.get(p, h) for p, h in ((comp, comp_h), (other, other_h), (best, best_h),
                                                                           (value, value_h)))
    assert got_comp[-1] == GUARD and got_other[-1] == GUARD and got_best[-1] == GUARD64 and got_value[-1] == GUARD64
    assert not got_best[:-1].any()
    got_comp = got_comp[:n]
    assert ((got_comp >= 0) & (got_comp < n)).all() and np.array_equal(got_comp[got_comp], got_comp)
    assert int((got_other[:n] >= 0).sum()) == total == n - np.unique(got_comp).size
    return got_other[:n].copy(), got_value[:n].view(np.float64).copy(), rounds


def rows_of(n, other, value):
    a = np.flatnonzero(other >= 0)
    return _linkage.canonical(n, a, other[a], value[a])


def same(got, want):
    return (len(got) == len(want) == 4 and all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
            and not (np.signbit(got[2]) & (got[2] == 0)).any())


def check_forest(dev, blocks, n, layout, want, what, floor=None):
    """Run twice: the canonical rows equal the reference's, and the second run leaves the same integers.  -> rounds."""
    other, value, rounds = forest(dev, blocks, n, layout, floor)
    assert same(rows_of(n, other, value), want), what
    again = forest(dev, blocks, n, layout, floor)
    assert np.array_equal(again[0], other) and np.array_equal(B.bits(again[1]), B.bits(value)) and again[2] == rounds, what
    return rounds


# ---- 1. the C entries on synthetic blocks --------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_the_forest_gives_the_reference_rows(dev, layout):
    counted = deepest = 0
    for i, (n_rows, n_cols) in enumerate(SHAPES):
        for kind in KINDS:
            for tag, stride, base in B.variants(layout, n_rows, n_cols):
                blk = B.make_block(layout, n_rows, n_cols, stride, 60 + i, kind=kind)
                A = blk.A
                rng = np.random.default_rng([i, layout, stride])
                S = dev.put(blk.raw, base)
                for n, row_ids, col_ids in id_cases(n_rows, n_cols, rng):
                    what = (layout, n_rows, n_cols, kind, tag, row_ids is None)
                    block = (S, stride, n_rows, n_cols, None if row_ids is None else dev.put(row_ids),
                             None if col_ids is None else dev.put(col_ids))
                    want = LR.rows_of_edges(n, *LR.block_edges(A, row_ids, col_ids, n))
                    rounds = check_forest(dev, [block], n, layout, want, what)
                    assert rounds <= _linkage.max_rounds(n), what
                    deepest = max(deepest, rounds)
                    heights, widest = LR.stats(n, want)
                    counted += heights >= 3 and widest >= 3
                    # the binding's own path: one block
                    b = dict(ptr=S, layout=layout, stride=stride, rows=n_rows, cols=n_cols, row_ids=block[4], col_ids=block[5])
                    a2, b2, v2, r2 = _linkage.forest_blocks(dev.ops, [b], n, None)
                    assert same(_linkage.canonical(n, a2, b2, v2), want) and r2 <= rounds + 1, what
                dev.release()
    # Not every input is trivial: in EACH of the four layouts at least 5 cases (20 or more over the parametrisation) have
    # three heights or more and a merge of three classes or more at once, and at least one forest took three rounds or more.
    print(f"layout {layout}: {counted} cases with >= 3 heights and a merge of >= 3 classes, at most {deepest} rounds")
    assert counted >= 5 and deepest >= 3


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_nan_and_zeros_of_both_signs(dev, layout):
    """The block of test_gpu_cluster's test of the same entries: negative values with a few NaN, -0.0, +0.0 and positive
    entries.  The zeros of both signs are one height, reported +0.0; a NaN entry is no entry."""
    n_rows, n_cols = 70, 129
    _, stride, base = B.variants(layout, n_rows, n_cols)[0]
    rng = np.random.default_rng(layout)
    A = -(rng.integers(1, 1000, size=(n_rows, n_cols)) * 2.0 ** -10)
    stored = B.encode(layout, A, stride, B.SENTINEL[(layout, "dyadic")])
    at = B.offsets(layout, n_rows, n_cols, stride)
    rr, cc = rng.integers(0, n_rows, size=160), rng.integers(0, n_cols, size=160)
    for lo, v in ((0, np.nan), (60, -0.0), (100, 0.0), (130, 0.25)):
        hi = {0: 60, 60: 100, 100: 130, 130: 160}[lo]
        A[rr[lo:hi], cc[lo:hi]] = v
        stored[at[rr[lo:hi], cc[lo:hi]]] = v if np.isnan(v) else B.store(layout, v)
    assert np.array_equal(B.bits(B.decode(layout, stored, n_rows, n_cols, stride)), B.bits(A))
    S = dev.put(stored.tobytes(), base)
    n = n_cols
    want = LR.rows_of_edges(n, *LR.block_edges(A, None, None, n))
    check_forest(dev, [(S, stride, n_rows, n_cols, None, None)], n, layout, want, layout)
    sim = want[2]
    assert (sim == 0.25).any() and (sim == 0).any() and (sim < 0).any() and not np.signbit(sim[sim == 0]).any()
    # at 0 the zeros of both signs join together: the cut there is components(0.0) = components(-0.0)
    assert np.array_equal(LR.cut(n, want, t=0.0), CR.labels_of_edges(n, CR.block_edges(A, None, None, n, -0.0)))
    # five nodes with nothing but NaN between them, but for a -0.0 and a +0.0 that meet at node 1
    T = np.full((5, 5), np.nan)
    T[0, 1], T[2, 1] = -0.0, 0.0
    _, stride, base = B.variants(layout, 5, 5)[0]
    raw = B.encode(layout, np.where(np.isnan(T), 1.0, T), stride, B.SENTINEL[(layout, "dyadic")])
    raw[B.offsets(layout, 5, 5, stride)[np.isnan(T)]] = np.nan
    St = dev.put(raw.tobytes(), base)
    other, value, rounds = forest(dev, [(St, stride, 5, 5, None, None)], 5, layout)
    got = rows_of(5, other, value)
    assert same(got, LR.linkage(T)) and got[0].tolist() == [0, 5] and got[1].tolist() == [1, 2]
    assert got[2].tolist() == [0.0, 0.0] and got[3].tolist() == [2, 3]


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_an_edge_only_below_the_diagonal(dev, layout):
    n = 9
    A = np.full((n, n), -1.0)
    A[5, 2] = 1.0                                             # S[5][2] alone: w(2, 5) = 1
    _, stride, base = B.variants(layout, n, n)[0]
    S = dev.put(B.encode(layout, A, stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
    block = [(S, stride, n, n, None, None)]
    check_forest(dev, block, n, layout, LR.linkage(A), layout)
    got = rows_of(n, *forest(dev, block, n, layout)[:2])
    assert got[0].tolist() == [2, 0, 10, 11, 12, 13, 14, 15] and got[1].tolist() == [5, 1, 9, 3, 4, 6, 7, 8]
    assert got[2].tolist() == [1.0] + [-1.0] * 7 and got[3].tolist() == [2, 2, 4, 5, 6, 7, 8, 9]
    for floor in (0.5, 1.0):
        got = rows_of(n, *forest(dev, block, n, layout, floor)[:2])
        assert [x.tolist() for x in got] == [[2], [5], [1.0], [2]]
    assert len(rows_of(n, *forest(dev, block, n, layout, 1.25)[:2])[0]) == 0


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_two_column_blocks_into_one_forest(dev, layout):
    """Two column blocks of one matrix (a ``LocalWorld``'s ranks) picked into one array of slots: the whole matrix's
    dendrogram, which neither block gives alone."""
    rng = np.random.default_rng(3)
    n = 96
    A = rng.integers(-500, 500, size=(n, n)) * 2.0 ** -8
    blocks, alone = [], []
    for lo, hi in ((0, 64), (64, 96)):
        part = np.ascontiguousarray(A[:, lo:hi])
        _, stride, base = B.variants(layout, n, hi - lo)[0]
        S = dev.put(B.encode(layout, part, stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
        blocks.append((S, stride, n, hi - lo, None, dev.put(np.arange(lo, hi, dtype=np.int32))))
        alone.append(rows_of(n, *forest(dev, blocks[-1:], n, layout)[:2]))
    want = LR.linkage(A)
    check_forest(dev, blocks, n, layout, want, ("two blocks", layout))
    assert len(want[0]) == n - 1 and not same(alone[0], want) and not same(alone[1], want)
    bs = [dict(ptr=S, layout=layout, stride=stride, rows=r, cols=c, row_ids=ri, col_ids=ci) for S, stride, r, c, ri, ci in blocks]
    a, b, v, _ = _linkage.forest_blocks(dev.ops, bs, n, None)
    assert same(_linkage.canonical(n, a, b, v), want)


PATH_N = 2049


@functools.lru_cache(maxsize=None)
def path_case():
    """Weights (k + 1) 2^-10 on step k of a path through shuffled positions (each step stored in one direction only), 0
    elsewhere, node ids shuffled again -> (A, ids, the reference rows).  Every node but the last picks the next one."""
    n = PATH_N
    rng = np.random.default_rng(17)
    seq, ids = rng.permutation(n), rng.permutation(n).astype(np.int32)
    flip = rng.random(n - 1) < 0.5
    a, b = np.where(flip, seq[1:], seq[:-1]), np.where(flip, seq[:-1], seq[1:])
    A = np.zeros((n, n))
    A[a, b] = np.arange(1, n) * 2.0 ** -10
    return A, ids, LR.rows_of_edges(n, *LR.block_edges(A, ids, ids, n))


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_a_shuffled_path_with_rising_weights(dev, layout):
    n = PATH_N
    A, ids, want = path_case()
    assert len(want[0]) == n - 1 and np.array_equal(want[2], np.arange(n - 1, 0, -1) * 2.0 ** -10)
    _, stride, base = B.variants(layout, n, n)[0]
    S = dev.put(B.encode(layout, A, stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
    idp = dev.put(ids)
    assert check_forest(dev, [(S, stride, n, n, idp, idp)], n, layout, want, layout) == 1      # one round: one chain of hooks


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_an_all_ones_block(dev, layout):
    """257 x 257 ones: one round, one tie of all nodes; the rows are the left fold over the positions."""
    n = 257
    _, stride, base = B.variants(layout, n, n)[0]
    S = dev.put(B.encode(layout, np.ones((n, n)), stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
    want = (np.r_[0, n + np.arange(n - 2)].astype(np.int64), np.arange(1, n, dtype=np.int64), np.ones(n - 1),
            np.arange(2, n + 1, dtype=np.int64))
    assert same(LR.linkage(np.ones((n, n))), want)
    assert check_forest(dev, [(S, stride, n, n, None, None)], n, layout, want, layout) == 1


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_a_floor(dev, layout):
    """Under a floor the rows are the reference's rows with similarity >= floor: for a floor that is a stored value and
    for one between two stored values."""
    n_rows, n_cols = 129, 257
    _, stride, base = B.variants(layout, n_rows, n_cols)[0]
    blk = B.make_block(layout, n_rows, n_cols, stride, 65, kind="dyadic")
    S = dev.put(blk.raw, base)
    n = n_cols
    edges = LR.block_edges(blk.A, None, None, n)
    full = LR.rows_of_edges(n, *edges)
    hs = np.unique(full[2])
    stored, between = float(hs[hs.size // 2]), float(hs[hs.size // 2] + hs[hs.size // 2 + 1]) / 2
    assert between not in set(np.unique(blk.A).tolist()) and stored in set(np.unique(blk.A).tolist())
    for floor in (stored, between):
        keep = full[2] >= floor
        want = tuple(x[keep] for x in full)
        assert same(LR.rows_of_edges(n, *edges, floor=floor), want) and 0 < keep.sum() < keep.size
        check_forest(dev, [(S, stride, n_rows, n_cols, None, None)], n, layout, want, (layout, floor), floor)
        b = dict(ptr=S, layout=layout, stride=stride, rows=n_rows, cols=n_cols)
        a2, b2, v2, _ = _linkage.forest_blocks(dev.ops, [b], n, floor)
        assert same(_linkage.canonical(n, a2, b2, v2), want)


# ---- 2. through the estimators ------------------------------------------------------------------------------------------------
def check_model(model, floor=None):
    frames = as_groups(model.frame())
    groups = [1, 2] if len(frames) == 2 else [None]
    kw = [{} if g is None else {"group": g} for g in groups]
    rng = np.random.default_rng(len(frames[0]))
    nodes = [[f.index[i] for i in rng.integers(0, len(f), size=9)] for f in frames]
    before = [model.rows(nd, **k).to_numpy().copy() for nd, k in zip(nodes, kw)]
    Zs = as_groups(model.linkage() if floor is None else model.linkage(min_similarity=floor))
    assert len(Zs) == len(frames)
    for Z, f, k in zip(Zs, frames, kw):
        S, n = f.to_numpy(), len(f)
        want = LR.linkage(S, floor)
        assert isinstance(Z, pd.DataFrame) and Z.columns.tolist() == ["left", "right", "similarity", "size"]
        assert Z.dtypes.tolist() == [np.int64, np.int64, np.float64, np.int64]
        assert same(tuple(Z[c].to_numpy() for c in Z.columns), want)
        heights, widest = LR.stats(n, want)
        assert heights >= 3 and len(want[0]) >= 3
        assert floor is not None or len(Z) == n - 1           # a similarity is >= 0: everything joins at last
        # 8 thresholds taken from the data: the model's own stored values, the top, one above, and (no floor) both zeros' side
        pos = np.unique(off_diagonal(S))
        pos = pos[pos > (0 if floor is None else floor)]
        at = lambda q: float(pos[min(pos.size - 1, int(q * pos.size))])
        low = [at(0.0), at(0.05)] if floor is not None else [0.0, -0.25]
        ts = [at(0.9), at(0.3), low[0], at(1.0), low[1], at(0.5), float(np.nextafter(pos[-1], 2.0)), at(0.99)]
        comps = model.components(ts)
        comps = comps[groups.index(k.get("group"))] if len(frames) == 2 else comps
        for i, t in enumerate(ts):
            got = model.cut(Z, t=t, **k)
            assert isinstance(got, pd.Series) and got.name == "component" and got.dtype == np.int64 and got.index.equals(f.index)
            assert np.array_equal(got.to_numpy(), comps.iloc[:, i].to_numpy()), t
        for c in sorted(c for c in {n, n - 1, n // 2, n - len(Z) + 1, n - len(Z)} if 1 <= c and n - c <= len(Z)):
            got = model.cut(Z, n_clusters=c, **k).to_numpy()
            assert np.unique(got).size == c == got.max() + 1
        with pytest.raises(ValueError, match="fewest clusters"):
            if len(Z) < n - 1:
                model.cut(Z, n_clusters=n - len(Z) - 1, **k)
            else:
                model.cut(Z.iloc[:-1], n_clusters=1, **k)
    for nd, k, b in zip(nodes, kw, before):
        assert np.array_equal(B.bits(model.rows(nd, **k).to_numpy()), B.bits(b))           # the model is unchanged
    model.release()
    with pytest.raises(RuntimeError, match="released"):
        model.linkage()


@pytest.fixture(scope="module")
def powerlaw():
    return synth.powerlaw_directed(300, 4.0, seed=11)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_simrankpp_on_a_power_law_graph(variant, powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, variant, tmp_path)
    try:
        check_model(model)
    finally:
        model.release()


def test_a_floor_on_a_kept_model(powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, "f32-kept", tmp_path)
    try:
        pos = np.unique(off_diagonal(model.frame().to_numpy()))
        pos = pos[pos > 0]
        check_model(model, floor=float(pos[pos.size // 3]))
    finally:
        model.release()


# (an asymmetric prior makes S[a, b] != S[b, a]: the larger of the two directions is the weight)
@pytest.mark.parametrize("variant", ["f32-kept", "f32-compact-fp16", "f64-kept", "world3-kept"])
def test_apriori_with_an_asymmetric_prior(variant, tmp_path):
    df = synth.er_directed(150, 0.012, seed=5)
    n = len(set(df["from"]) | set(df["to"]))
    model = make_model("AprioriSimRank", df, variant, tmp_path, sparse_prior(n, False))
    try:
        S = model.frame().to_numpy()
        assert (S != S.T).sum() > n                                       # the directions do differ
        check_model(model)
    finally:
        model.release()


@pytest.mark.parametrize("variant", ["f32-kept", "f64-kept", "world3-kept", "loaded"])
def test_bipartite_simrankpp(variant, tmp_path):
    df = bipartite_random(90, 50, 0.06, 12)
    model = make_model("BipartiteSimRankPP", df, variant, tmp_path, strict_reference=False)
    try:
        check_model(model)
    finally:
        model.release()


def test_a_pruned_model_links_its_matrix_p(powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, "f32-kept", tmp_path)
    try:
        model.prune(10)
        assert model.kept_neighbors == 10
        with pytest.raises(ValueError, match="tie everything at 0"):
            model.linkage()
        P = model.frame().to_numpy()
        pos = np.unique(off_diagonal(P))
        pos = pos[pos > 0]
        check_model(model, floor=float(pos[0]))               # the smallest kept value: every kept entry is used
    finally:
        model.release()
