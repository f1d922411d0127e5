"""``score_sets`` and ``recommend`` on a real MI355X (libsimrank_sets.so): every value and every frame EQUAL, bit for bit
and row for row, to the NumPy statement (tests/sets_ref.py) applied to ``model.frame()`` of the same model: kept, compact
and loaded models, f32, fp16-held and float64 matrices, ``LocalWorld(3)``'s uneven column blocks, baskets that are empty,
repeat a member, outrun the kernel's unroll factor or hold every node, weights of mixed signs over 18 decades, the dense
and the top-k form with and without exclusion, a band boundary, and the lifetime rules.

N = 1100 crosses one 1024-column workgroup chunk and is a multiple of neither 32 nor 64; the graph is sparse enough that
most of S is exactly 0, so the id-ascending tie rule decides most ranks."""
import contextlib
import io

import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

import simrank_amd
import simrank_amd.SimRank as SRA
from simrank_amd import _query, synth
from simrank_amd.driver import LocalWorld
from tests import sets_ref as R
from tests.graphs import bipartite_random

pytestmark = pytest.mark.gpu

N = 1100
UPDATES = 3


def fit(cls, df, *args, **kw):
    est = getattr(SRA, cls)()
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(df, *args, iterations=UPDATES, eps=1e-30, verbose=False, keep=True, **kw)
    return est


@pytest.fixture(scope="module")
def graph():
    df = synth.er_directed(N, 0.002, seed=7)
    assert len(set(df["from"]) | set(df["to"])) == N
    return df


# variant -> (fit keywords, what happens to the kept model afterwards)
VARIANTS = {
    "f32-kept": ({}, None),
    "f32-compact": ({}, "compact"),
    "f32-compact-fp16": ({}, "compact-fp16"),
    "fp16-kept": ({"storage_precision": "fp16"}, None),
    "f64-kept": ({"storage_precision": "f64"}, None),
    "f64-compact": ({"storage_precision": "f64"}, "compact"),
    "world3-kept": ({"world": 3}, None),
    "world3-compact": ({"world": 3}, "compact"),
    "loaded": ({}, "load"),
}


@contextlib.contextmanager
def model_of(cls, df, variant, tmp_path, *args, **more):
    kw, then = VARIANTS[variant]
    kw = dict(kw, **more)
    if "world" in kw:
        kw.update(world=LocalWorld(kw["world"]), mode="sparse")
    model = fit(cls, df, *args, **kw)
    try:
        if then == "compact":
            model.compact()
        elif then == "compact-fp16":
            model.compact(precision="fp16")
        elif then == "load":
            model.save(tmp_path / "model.bin")
            model.release()
            model = simrank_amd.load_model(tmp_path / "model.bin")
        yield model
    finally:
        model.release()


def baskets(labels, seed=3):
    """(sets, weights): empty, one member, a member twice, 37 members (longer than the unroll factor and no multiple of it),
    all N nodes, two baskets sharing most members; weights of mixed signs from 1e-12 to 1e6."""
    rng = np.random.default_rng(seed)
    n = len(labels)
    pick = lambda m: [labels[i] for i in rng.permutation(n)[:m]]
    shared = pick(30)
    sets = [[], pick(1), [labels[5], labels[900 % n], labels[5]], pick(37), list(labels), shared + pick(3), pick(2) + shared]
    weights = [list(rng.choice([-1.0, 1.0], size=len(s)) * 10.0 ** rng.uniform(-12, 6, size=len(s))) for s in sets]
    return sets, weights


def same_frame(got, want, what=""):
    assert_frame_equal(got, want, check_exact=True, obj=str(what))
    for c in want.columns:
        if want[c].dtype == np.float64:
            assert np.array_equal(got[c].to_numpy().view(np.uint64), want[c].to_numpy().view(np.uint64)), (what, c)


def check_score_sets(model, frame, group=None):
    kw = {} if group is None else {"group": group}
    labels = list(frame.index)
    n = len(labels)
    sets, weights = baskets(labels)
    names = ["q%d" % i for i in range(len(sets))]
    # dense form: weighted with names, unweighted with a RangeIndex
    same_frame(model.score_sets(sets, weights=weights, names=names, **kw), R.score_sets_ref(frame, sets, weights, names), "dense")
    plain = model.score_sets(sets, **kw)
    same_frame(plain, R.score_sets_ref(frame, sets), "dense, unit weights")
    assert np.all(plain.values[0] == 0.0) and list(plain.columns) == labels and list(plain.index) == list(range(len(sets)))
    # top-k form
    for k in (1, 10, n):
        for exclude in ("members", None):
            for w in (weights, None):
                got = model.score_sets(sets, weights=w, top_k=k, exclude=exclude, **kw)
                same_frame(got, R.score_sets_ref(frame, sets, w, top_k=k, exclude=exclude), ("top", k, exclude, w is None))
                sizes = got.groupby("set").size().reindex(range(len(sets)), fill_value=0).tolist()
                if exclude == "members":
                    assert sizes[4] == 0                                   # the all-N basket has no candidate left
                    assert sizes[3] == min(k, n - 37) and sizes[2] == min(k, n - 2)
                else:
                    assert sizes == [min(k, n)] * len(sets)
    # labels to exclude instead of the members
    other = [labels[:3], [], labels[2:1000], [], labels[1:], [labels[0]], []]
    same_frame(model.score_sets(sets, weights=weights, top_k=10, exclude=other, **kw),
               R.score_sets_ref(frame, sets, weights, top_k=10, exclude=other), "exclude lists")
    assert model.score_sets([], **kw).shape == (0, n) and len(model.score_sets([], top_k=3, **kw)) == 0


# AprioriSimRank with a prior that is NOT symmetric: the kept iterate is asymmetric and dense, so a kernel that read
# (c, r) for (r, c), or the wrong panel, would not land on the same value
ASYM_VARIANTS = ("f32-kept", "f32-compact", "fp16-kept", "world3-kept")
CASES = [(cls, v) for cls in ("SimRank", "SimRankPP") for v in VARIANTS] + [
    # (fp16-kept refuses an asymmetric prior: the case is named for what it then scores)
    pytest.param("AprioriSimRank", v, id="AprioriSimRank-fp16-kept-refused-so-f32-compact-fp16") if v == "fp16-kept"
    else ("AprioriSimRank", v) for v in ASYM_VARIANTS]


@pytest.mark.parametrize("cls,variant", CASES)
def test_score_sets_is_the_statement(cls, variant, graph, tmp_path):
    args = ()
    if cls == "AprioriSimRank":
        args = (np.random.default_rng(5).random((N, N)) * 0.5,)
    if cls == "AprioriSimRank" and variant == "fp16-kept":
        # a fit that holds its matrices in fp16 takes symmetric priors only (estimators.py says so): the asymmetric
        # fp16-held iterate is the f32 fit's, narrowed by compact(precision="fp16")
        with pytest.raises(ValueError, match="symmetric priors only"):
            fit(cls, graph, *args, storage_precision="fp16")
        variant = "f32-compact-fp16"
    with model_of(cls, graph, variant, tmp_path, *args) as model:
        frame = model.frame()
        if cls == "AprioriSimRank":
            assert not np.array_equal(frame.values, frame.values.T)       # the iterate is not symmetric
        else:
            assert (frame.values == 0).mean() > 0.5                       # most of S is exactly 0: ties everywhere
        check_score_sets(model, frame)


def test_a_band_boundary(graph, tmp_path, monkeypatch):
    """70 baskets in bands of 9 (the Reader's ``SLAB_BYTES`` cut down) equal the one-band result, on one block and on
    LocalWorld(3)'s three."""
    for variant in ("f32-compact", "world3-kept"):
        with model_of("SimRank", graph, variant, tmp_path) as model:
            labels = list(model.frame().index)
            rng = np.random.default_rng(17)
            sets = [[labels[i] for i in rng.integers(0, N, size=rng.integers(0, 12))] for _ in range(70)]
            weights = [list(rng.normal(size=len(s))) for s in sets]
            with monkeypatch.context() as m:
                m.setattr(_query, "SLAB_BYTES", 1 << 28)
                dense, top = model.score_sets(sets, weights=weights), model.score_sets(sets, weights=weights, top_k=10)
            same_frame(dense, R.score_sets_ref(model.frame(), sets, weights), "one band against the statement")
            with monkeypatch.context() as m:
                m.setattr(_query, "SLAB_BYTES", 9 * 8 * N)
                same_frame(model.score_sets(sets, weights=weights), dense, "dense in bands")
                same_frame(model.score_sets(sets, weights=weights, top_k=10), top, "top-k in bands")
            with monkeypatch.context() as m:
                m.setattr(_query, "SLAB_BYTES", 1)                          # one basket per band
                same_frame(model.score_sets(sets[:9], weights=weights[:9], top_k=10),
                           top[top["set"] < 9].reset_index(drop=True), "one basket per band")


# ---- the library on a block of its own: both grid orders, 8 chunks and more, a column map, a position out of range ----------
@pytest.mark.parametrize("n_cols", [1100, 3 * 1024 + 5, 9001])
def test_both_grid_orders_on_a_synthetic_block(n_cols):
    """2, 4 and 9 column chunks (fewer than 8, and more: the two numberings of the chunk-label order), f32 row-major read
    with vector loads, through a column map, and with rows too short for vector loads; a list position outside the
    block poisons its basket with NaN and nothing else."""
    import ctypes as C
    from simrank_amd import _sets
    from simrank_amd.engine import HipOps
    ops, lib = HipOps(0), _sets.load()
    rng = np.random.default_rng(n_cols)
    n_rows = 40
    lists = [rng.integers(0, n_rows, size=m).astype(np.int32) for m in (0, 1, 8, 19, 40, 3)]
    lists[5][1] = n_rows                                                   # outside the block
    ptr, pos = _sets.join(lists)
    w = rng.normal(size=pos.size)
    perm = rng.permutation(n_cols).astype(np.int32)
    held = []
    try:
        for stride, cmap in ((-(-n_cols // 4) * 4, None), (-(-n_cols // 4) * 4, perm), (n_cols + 1, None)):
            S = np.zeros((n_rows, stride), dtype=np.float32)
            S[:, :n_cols] = rng.random((n_rows, n_cols), dtype=np.float32) * (rng.random((n_rows, n_cols)) < 0.3)
            cols = S[:, :n_cols].astype(np.float64) if cmap is None else S[:, cmap].astype(np.float64)
            want = R.scores(cols, [l[l < n_rows] for l in lists], [w[ptr[q]:ptr[q + 1]][l < n_rows] for q, l in enumerate(lists)])
            want[5] = np.nan
            dev = [ops.put(a) for a in (S, ptr, pos, w)] + [ops._malloc(8 * len(lists) * n_cols)]
            held += dev
            cmap_dev = None
            if cmap is not None:
                cmap_dev = ops.put(cmap)
                held.append(cmap_dev)
            for order in (_sets.BASKET_MAJOR, _sets.CHUNK_LABEL):
                got = np.full((len(lists), n_cols), 7.0)
                ops.h2d(dev[4], got)
                _sets.check(lib.simrank_sets_score(dev[0], _query.ROWMAJOR_F32, stride, n_rows, n_cols, cmap_dev, n_cols, dev[1],
                                                   dev[2], dev[3], len(lists), None, None, dev[4], n_cols, order, ops.stream),
                            "simrank_sets_score")
                ops.d2h(got, dev[4])
                ops.synchronize()
                assert np.array_equal(got.view(np.uint64)[:5], want.view(np.uint64)[:5]), (stride, cmap is None, order)
                assert np.isnan(got[5]).all()
    finally:
        ops.synchronize()
        for p in held:
            ops._free(p)
        ops.close()


# ---- recommend ----------------------------------------------------------------------------------------------------------
def bipartite_graph(weighted_seed=2):
    """60 x 45, one user of degree 45 (every item) and one of degree 1: a bipartite fit has no node of degree 0 (a node
    exists through its edges), so the empty basket is checked on the directed graph, whose nodes without in-edges have one."""
    df = bipartite_random(60, 45, 0.1, seed=weighted_seed)
    full = pd.DataFrame({"user": 1000, "item": np.arange(1, 46), "weight": 2})
    df = pd.concat([df[(df["user"] != 1000) & (df["user"] != 1001)], full,
                    df[df["user"] == 1001].iloc[:1]]).drop_duplicates(["user", "item"]).reset_index(drop=True)
    deg = df.groupby("user").size()
    assert deg.max() == 45 and deg.min() == 1 and df["user"].nunique() == 60 and df["item"].nunique() == 45
    return df


def blocks_of(frame, first):
    return {key: grp.reset_index(drop=True) for key, grp in frame.groupby(first, sort=False)}


def check_recommend(model, group=None):
    frames = model.frame()
    solver, sides = model._model
    bip = len(sides) == 2
    side = 0 if group in (None, 1) else 1
    own = frames[side] if bip else frames
    read = frames[1 - side] if bip else frames
    spec = solver.specs[side]
    rowptr, col, scale = np.asarray(spec.csr.rowptr), np.asarray(spec.csr.col), np.asarray(spec.rowscale)
    labels, read_labels = list(own.index), list(read.index)
    kw = {} if group is None else {"group": group}
    rng = np.random.default_rng(23)
    deg = np.diff(rowptr)
    nodes = [labels[int(np.argmax(deg))], labels[int(np.argmin(deg))]] + [labels[i] for i in rng.permutation(len(labels))[:20]]
    n = len(read_labels)
    for k in (1, 10, n):
        for seen in (True, False):
            got = model.recommend(nodes, k, exclude_seen=seen, **kw)
            same_frame(got, R.recommend_ref(read, labels, rowptr, col, scale, nodes, k, seen, also_self=not bip),
                       ("recommend", k, seen))
    # the same baskets and weights through score_sets
    us = [labels.index(x) for x in nodes]
    sets = [[read_labels[c] for c in col[rowptr[u]:rowptr[u + 1]]] for u in us]
    weights = [[scale[u]] * len(s) for u, s in zip(us, sets)]
    full = model.recommend(nodes, n, **kw)
    seen_kw = dict(kw) if bip else {}
    exclude = "members" if bip else [s + [x] for s, x in zip(sets, nodes)]
    by_set = model.score_sets(sets, weights=weights, top_k=n, exclude=exclude, **({"group": 3 - group} if bip else seen_kw))
    keep = [i for i, s in enumerate(sets) if s]
    by_set = by_set[by_set["set"].isin(keep)].reset_index(drop=True)
    assert full["node"].tolist() == [nodes[i] for i in by_set["set"]]
    same_frame(full[["rank", "neighbor", "score"]], by_set[["rank", "neighbor", "score"]], "recommend against score_sets")
    # exclude_seen=False differs exactly in the seen rows
    first = list(dict.fromkeys(nodes))[:6]                                 # (``nodes`` may name a node twice)
    every = blocks_of(model.recommend(first, n, exclude_seen=False, **kw), "node")
    unseen = blocks_of(model.recommend(first, n, **kw), "node")
    for x, s in ((x, sets[nodes.index(x)]) for x in first):
        if not s:
            assert x not in every and x not in unseen
            continue
        gone = set(s) | (set() if bip else {x})
        left = every[x][~every[x]["neighbor"].isin(gone)].reset_index(drop=True)
        assert len(every[x]) == n and len(left) == n - len(gone)
        want = unseen.get(x, left.iloc[:0])
        same_frame(left[["neighbor", "score"]], want[["neighbor", "score"]].reset_index(drop=True), ("seen rows", x))
    return scale


@pytest.mark.parametrize("variant", ["f32-kept", "f32-compact", "loaded"])
@pytest.mark.parametrize("weighted", [False, True])
def test_recommend_on_a_bipartite_fit(variant, weighted, tmp_path):
    df = bipartite_graph()
    with model_of("BipartiteSimRankPP", df, variant, tmp_path, weighted=weighted, strict_reference=False) as model:
        scales = [check_recommend(model, group) for group in (1, 2)]
        one = model.recommend([1000], 5, group=1)                          # the user of degree 45 has seen every item
        assert len(one) == 0 and len(model.recommend([1000], 5, group=1, exclude_seen=False)) == 5
    if weighted:                                                           # the weighted fit's own row scales were used
        with model_of("BipartiteSimRankPP", df, "f32-kept", tmp_path, strict_reference=False) as plain:
            for s, sc in enumerate(scales):
                assert not np.array_equal(sc, np.asarray(plain._model[0].specs[s].rowscale))


@pytest.mark.parametrize("variant", ["f32-kept", "f32-compact", "loaded", "world3-kept"])
def test_recommend_on_a_directed_fit(variant, graph, tmp_path):
    with model_of("SimRank", graph, variant, tmp_path) as model:
        check_recommend(model)
        rowptr = np.asarray(model._model[0].specs[0].csr.rowptr)
        assert (np.diff(rowptr) == 0).any()                                # (a node without in-neighbours was among them)


# ---- lifetime -----------------------------------------------------------------------------------------------------------
def test_lifetime(graph):
    model = fit("SimRank", graph).compact()
    labels = list(model.frame().index)
    before = model.device_bytes
    model.score_sets([labels[:5]], top_k=3)
    model.score_sets([labels[:5]])
    model.recommend(labels[:5], 3)
    assert model.device_bytes == before
    model.release()
    for call in (lambda: model.score_sets([labels[:5]]), lambda: model.recommend(labels[:5], 3)):
        with pytest.raises(RuntimeError, match="released"):
            call()
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().score_sets([[1]])
