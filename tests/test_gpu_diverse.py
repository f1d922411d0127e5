"""``score_sets(diversity=d)`` and ``recommend(diversity=d)`` on a real MI355X (libsimrank_diverse.so): every frame EQUAL,
bit for bit and row for row, to the NumPy statement (tests/diverse_ref.py) applied to ``model.frame()`` of the same model:
the models, graph and baskets of tests/test_gpu_sets.py (kept, compact and loaded models, f32, fp16-held and float64
matrices, ``LocalWorld(3)``'s column blocks packed into one) and a ``prune(50)`` model, whose frame is its matrix P.
tests/test_diverse_cpu.py shows that on this graph the penalty changes the picks, so a device that ignored it fails here;
the asymmetric prior tells the row of a pick from its column.

Greedy picks are prefix-consistent, and the frames are compared at k = 1 and 10 over every combination; the picks to
the end (k = N) run on three of the baskets, where the statement takes a second and not ten."""
import numpy as np
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _query
from tests import diverse_ref as D
from tests.test_gpu_sets import (ASYM_VARIANTS, N, VARIANTS, baskets, bipartite_graph, fit, graph, model_of,  # noqa: F401
                                 same_frame)

pytestmark = pytest.mark.gpu

DS = (0.0, 0.3, 1.0)
PLAIN = ["set", "rank", "neighbor", "score"]


def check_score_sets(model, frame, group=None, full=True):
    kw = {} if group is None else {"group": group}
    labels = list(frame.index)
    n = len(labels)
    sets, weights = baskets(labels)
    names = ["q%d" % i for i in range(len(sets))]
    differ = 0
    for d in DS:
        for k in (1, 10):
            for exclude in ("members", None):
                for w in (weights, None):
                    got = model.score_sets(sets, weights=w, top_k=k, exclude=exclude, diversity=d, **kw)
                    want = D.score_sets_ref(frame, sets, w, top_k=k, exclude=exclude, diversity=d)
                    same_frame(got, want, ("diverse", d, k, exclude, w is None))
                    plain = model.score_sets(sets, weights=w, top_k=k, exclude=exclude, **kw)
                    if d == 0.0:                                           # the picks and scores of the plain selection
                        same_frame(got[PLAIN], plain, ("d = 0 against top_k", k, exclude, w is None))
                    elif len(got) == len(plain):
                        differ += int((got["neighbor"].to_numpy() != plain["neighbor"].to_numpy()).sum())
    # names, and labels to exclude instead of the members
    other = [labels[:3], [], labels[2:1000], [], labels[1:], [labels[0]], []]
    same_frame(model.score_sets(sets, weights=weights, names=names, top_k=10, exclude=other, diversity=0.3, **kw),
               D.score_sets_ref(frame, sets, weights, names, top_k=10, exclude=other, diversity=0.3), "exclude lists")
    assert len(model.score_sets([], top_k=3, diversity=0.3, **kw)) == 0
    if full:                                                               # k = N (and beyond: clamped): picked to the end
        some, some_w = [sets[1], sets[3], sets[4]], [weights[1], weights[3], weights[4]]
        for d, exclude, w in ((0.3, "members", some_w), (1.0, None, None), (0.0, None, some_w)):
            want = D.score_sets_ref(frame, some, w, top_k=n, exclude=exclude, diversity=d)
            same_frame(model.score_sets(some, weights=w, top_k=n + (5 if d else 0), exclude=exclude, diversity=d, **kw), want,
                       ("to the end", d, exclude))
            sizes = want.groupby("set").size().reindex(range(3), fill_value=0).tolist()
            assert sizes == ([n - 1, n - 37, 0] if exclude else [n] * 3)
    return differ


CASES = [(cls, v) for cls in ("SimRank", "SimRankPP") for v in list(VARIANTS) + ["pruned"]] + [
    # (fp16-kept refuses an asymmetric prior: the case scores the f32 fit's iterate narrowed by compact instead)
    ("AprioriSimRank", "f32-compact-fp16" if v == "fp16-kept" else v) for v in ASYM_VARIANTS]


@pytest.mark.parametrize("cls,variant", CASES)
def test_score_sets_diverse_is_the_statement(cls, variant, graph, tmp_path):  # noqa: F811
    args = (np.random.default_rng(5).random((N, N)) * 0.5,) if cls == "AprioriSimRank" else ()
    with model_of(cls, graph, "f32-kept" if variant == "pruned" else variant, tmp_path, *args) as model:
        if variant == "pruned":
            model.prune(50)
            assert model.kept_neighbors == 50
        frame = model.frame()
        before = frame.values.copy()
        if cls == "AprioriSimRank":
            assert not np.array_equal(frame.values, frame.values.T)       # row against column: the iterate is not symmetric
        differ = check_score_sets(model, frame, full=variant in ("f32-kept", "f32-compact", "fp16-kept", "f64-kept",
                                                                 "world3-kept", "pruned"))
        assert differ > 0                                                  # the penalty changed picks on this model
        after = model.frame().values                                       # the model is left as it was
        assert np.array_equal(after.view(np.uint64), before.view(np.uint64))
        assert model.kept_neighbors == (50 if variant == "pruned" else None)


def check_recommend(model, group=None):
    frames = model.frame()
    solver, sides = model._model
    bip = len(sides) == 2
    side = 0 if group in (None, 1) else 1
    own = frames[side] if bip else frames
    read = frames[1 - side] if bip else frames
    spec = solver.specs[side]
    rowptr, col, scale = np.asarray(spec.csr.rowptr), np.asarray(spec.csr.col), np.asarray(spec.rowscale)
    labels = list(own.index)
    kw = {} if group is None else {"group": group}
    rng = np.random.default_rng(23)
    deg = np.diff(rowptr)
    nodes = [labels[int(np.argmax(deg))], labels[int(np.argmin(deg))]] + [labels[i] for i in rng.permutation(len(labels))[:20]]
    n = len(read)
    for d in DS:
        for k, some in ((1, nodes), (10, nodes), (n, nodes[:4])):
            for seen in (True, False):
                got = model.recommend(some, k, exclude_seen=seen, diversity=d, **kw)
                same_frame(got, D.recommend_ref(read, labels, rowptr, col, scale, some, k, seen, also_self=not bip, diversity=d),
                           ("recommend", d, k, seen))
                if d == 0.0:
                    same_frame(got[["node", "rank", "neighbor", "score"]], model.recommend(some, k, exclude_seen=seen, **kw),
                               ("d = 0 against recommend", k, seen))


@pytest.mark.parametrize("variant", ["f32-kept", "f32-compact", "loaded", "world3-kept", "pruned"])
def test_recommend_diverse_on_a_directed_fit(variant, graph, tmp_path):  # noqa: F811
    with model_of("SimRank", graph, "f32-kept" if variant == "pruned" else variant, tmp_path) as model:
        if variant == "pruned":
            model.prune(50)
        check_recommend(model)


@pytest.mark.parametrize("variant", ["f32-kept", "f32-compact", "loaded"])
@pytest.mark.parametrize("weighted", [False, True])
def test_diverse_on_a_bipartite_fit(variant, weighted, tmp_path):
    df = bipartite_graph()
    with model_of("BipartiteSimRankPP", df, variant, tmp_path, weighted=weighted, strict_reference=False) as model:
        check_recommend(model, 1), check_recommend(model, 2)
        check_score_sets_small(model, model.frame()[1], group=2)
        one = model.recommend([1000], 5, group=1, diversity=0.3)          # the user of degree 45 has seen every item
        assert len(one) == 0 and list(one.columns) == ["node", "rank", "neighbor", "score", "penalty", "value"]
        assert len(model.recommend([1000], 5, group=1, exclude_seen=False, diversity=0.3)) == 5


def check_score_sets_small(model, frame, group):
    """``score_sets(group=2)`` of a bipartite model: its own group's matrix scores and punishes."""
    labels = list(frame.index)
    rng = np.random.default_rng(3)
    sets = [[], [labels[0]], [labels[i] for i in rng.permutation(len(labels))[:9]], [labels[2], labels[2]]]
    weights = [list(rng.normal(size=len(s))) for s in sets]
    for d in DS:
        for k in (1, 10, len(labels)):
            for w in (weights, None):
                same_frame(model.score_sets(sets, weights=w, top_k=k, group=group, diversity=d),
                           D.score_sets_ref(frame, sets, w, top_k=k, diversity=d), ("group 2", d, k, w is None))


def test_a_band_boundary(graph, tmp_path, monkeypatch):  # noqa: F811
    """70 baskets in bands of 9 and of 1 (the Reader's ``SLAB_BYTES`` cut down) equal the one-band result, on one block, on
    LocalWorld(3)'s three packed into one, and on a pruned model."""
    for variant in ("f32-compact", "world3-kept", "pruned"):
        with model_of("SimRank", graph, "f32-kept" if variant == "pruned" else variant, tmp_path) as model:
            if variant == "pruned":
                model.prune(50)
            frame = model.frame()
            labels = list(frame.index)
            rng = np.random.default_rng(17)
            sets = [[labels[i] for i in rng.integers(0, N, size=rng.integers(0, 12))] for _ in range(70)]
            with monkeypatch.context() as m:
                m.setattr(_query, "SLAB_BYTES", 1 << 28)
                top = model.score_sets(sets, top_k=10, diversity=0.3)
            same_frame(top, D.score_sets_ref(frame, sets, top_k=10, diversity=0.3), "one band against the statement")
            with monkeypatch.context() as m:
                m.setattr(_query, "SLAB_BYTES", 9 * 8 * N)
                same_frame(model.score_sets(sets, top_k=10, diversity=0.3), top, "in bands of 9")
            with monkeypatch.context() as m:
                m.setattr(_query, "SLAB_BYTES", 1)                          # one basket per band
                same_frame(model.score_sets(sets[:9], top_k=10, diversity=0.3),
                           top[top["set"] < 9].reset_index(drop=True), "one basket per band")


def test_lifetime_and_refusals(graph):  # noqa: F811
    model = fit("SimRank", graph).compact()
    labels = list(model.frame().index)
    before = model.device_bytes
    model.score_sets([labels[:5]], top_k=3, diversity=0.3)
    model.recommend(labels[:5], 3, diversity=0.3)
    assert model.device_bytes == before
    with pytest.raises(ValueError, match="top_k"):
        model.score_sets([labels[:5]], diversity=0.3)
    for bad in (True, "0.3", np.nan, -0.5, 1.5, np.inf):
        with pytest.raises(ValueError, match="diversity"):
            model.score_sets([labels[:5]], top_k=3, diversity=bad)
        with pytest.raises(ValueError, match="diversity"):
            model.recommend(labels[:5], 3, diversity=bad)
    # the default is the plain frame, column for column
    assert list(model.score_sets([labels[:5]], top_k=3, diversity=None).columns) == PLAIN
    model.release()
    for call in (lambda: model.score_sets([labels[:5]], top_k=3, diversity=0.3), lambda: model.recommend(labels[:5], 3, diversity=0.3)):
        with pytest.raises(RuntimeError, match="released"):
            call()
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().score_sets([[1]], top_k=1, diversity=0.3)
