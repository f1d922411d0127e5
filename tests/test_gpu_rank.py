"""``rank_sets``, ``rank_recommended`` and ``evaluate`` on a real MI355X (libsimrank_rank.so): every frame EQUAL, row for
row and bit for bit in ``score``, to the NumPy statement (tests/rank_ref.py) applied to ``model.frame()`` of the same
model, and every rank the row it names of the model's own ``score_sets(top_k=N)`` frame: kept, compact, loaded and pruned
models, f32, fp16-held and float64 matrices, ``LocalWorld(3)``'s uneven column blocks, the bipartite groups, baskets that
are empty, repeat a member or hold every node, target lists that are empty, repeat a target, list members and list every
node (more than four local-memory tiles), a band boundary, and the lifetime rules.

The graph and the variants are tests/test_gpu_sets.py's: N = 1100 crosses one 1024-column workgroup chunk and is a
multiple of neither 32 nor 64, and most of S is exactly 0, so the id-ascending tie rule decides most ranks."""
import contextlib

import numpy as np
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _query, synth
from tests import rank_ref as K
from tests import test_gpu_sets as T
from tests.graphs import bipartite_random

pytestmark = pytest.mark.gpu

N = T.N


@pytest.fixture(scope="module")
def graph():
    df = synth.er_directed(N, 0.002, seed=7)
    assert len(set(df["from"]) | set(df["to"])) == N
    return df


@contextlib.contextmanager
def model_of(variant, df, tmp_path, cls="SimRank", **more):
    with T.model_of(cls, df, "f32-kept" if variant == "pruned" else variant, tmp_path, **more) as model:
        if variant == "pruned":
            model.prune(50)
            assert model.kept_neighbors == 50
        yield model


def targets_for(labels, sets, seed=11):
    """Per basket: 12 random labels, the basket's first two members (no candidates under exclude="members") and the
    first target again; the 37-member basket asks for every node, one of the overlapping baskets for nothing."""
    rng = np.random.default_rng(seed)
    out = []
    for s in sets:
        t = [labels[i] for i in rng.integers(0, len(labels), size=12)]
        out.append(t + list(s[:2]) + t[:1])
    out[3] = list(labels)
    out[5] = []
    return out


def check_against_top_k(model, got, sets, weights, exclude, n, kw):
    """Row ``rank`` of the model's own top-N frame names the target with that score; ``candidates`` is that frame's size."""
    top = model.score_sets(sets, weights=weights, top_k=n, exclude=exclude, **kw)
    sizes = top.groupby("set").size().reindex(range(len(sets)), fill_value=0)
    assert got["candidates"].tolist() == sizes.reindex(got["set"]).tolist()
    ranked = got[got["rank"] > 0]
    rows = ranked.merge(top, on=["set", "rank"], how="left", suffixes=("", "_top"))
    assert len(rows) == len(ranked) and rows["neighbor"].tolist() == ranked["target"].tolist()
    assert np.array_equal(rows["score_top"].to_numpy().view(np.uint64), ranked["score"].to_numpy().view(np.uint64))
    out = got[got["rank"] == 0]
    gone = out.merge(top, left_on=["set", "target"], right_on=["set", "neighbor"], how="inner")
    assert len(gone) == 0 and (out["score"] == -np.inf).all()


def check_rank_sets(model, frame, group=None):
    kw = {} if group is None else {"group": group}
    labels = list(frame.index)
    n = len(labels)
    sets, weights = T.baskets(labels)
    targets = targets_for(labels, sets)
    names = ["q%d" % i for i in range(len(sets))]
    other = [labels[:3], [], labels[2:n - 100], [], labels[1:], [labels[0]], []]
    for exclude in ("members", None, other):
        got = model.rank_sets(sets, targets, weights=weights, exclude=exclude, **kw)
        T.same_frame(got, K.rank_sets_ref(frame, sets, targets, weights, exclude=exclude), ("rank_sets", str(exclude)[:12]))
        assert got["rank"].dtype == np.int64 and got["candidates"].dtype == np.int64
        check_against_top_k(model, got, sets, weights, exclude, n, kw)
        if exclude == "members":
            for q, s in enumerate(sets):                                   # a member is no candidate of its own basket
                mine = got[(got["set"] == q) & got["target"].isin(s)]
                assert (mine["rank"] == 0).all() and (mine["score"] == -np.inf).all()
            assert len(got[(got["set"] == 3) & (got["rank"] == 0)]) == 37 and (got[got["set"] == 4]["candidates"] == 0).all()
            full = got[got["set"] == 3]
            assert len(full) == n and sorted(full["rank"][full["rank"] > 0]) == list(range(1, n - 37 + 1))
        if exclude is None:
            assert (got["rank"] > 0).all() and (got["candidates"] == n).all()
    # unit weights and names; a target listed twice gets two equal rows
    got = model.rank_sets(sets, targets, names=names, **kw)
    T.same_frame(got, K.rank_sets_ref(frame, sets, targets, names=names), "unit weights")
    first, again = got[got["set"] == "q1"].iloc[0], got[got["set"] == "q1"].iloc[-1]
    assert first["target"] == again["target"] and first["rank"] == again["rank"] and first["score"] == again["score"]
    # the empty basket without exclusion scores 0 everywhere: the target at label position p has rank p + 1
    ps = [0, 5, n // 2, n - 1]
    got = model.rank_sets([[]], [[labels[p] for p in ps]], exclude=None, **kw)
    assert got["rank"].tolist() == [p + 1 for p in ps] and (got["score"] == 0.0).all() and (got["candidates"] == n).all()
    assert len(model.rank_sets([], [], **kw)) == 0 and len(model.rank_sets([labels[:3]], [[]], **kw)) == 0


RANK_VARIANTS = list(T.VARIANTS) + ["pruned"]


@pytest.mark.parametrize("variant", RANK_VARIANTS)
def test_rank_sets_is_the_statement(variant, graph, tmp_path):
    with model_of(variant, graph, tmp_path) as model:
        frame = model.frame()
        assert (frame.values == 0).mean() > 0.5                            # most of S is exactly 0: ties everywhere
        check_rank_sets(model, frame)
        assert np.array_equal(model.frame().values.view(np.uint64), frame.values.view(np.uint64))     # left unchanged


def check_recommended(model, group=None):
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
    rng = np.random.default_rng(29)
    deg = np.diff(rowptr)
    hub, least = int(np.argmax(deg)), int(np.argmin(deg))
    us = [hub, least] + [int(i) for i in rng.permutation(len(labels)) if i not in (hub, least)][:20]
    nodes = [labels[u] for u in us]
    n = len(read_labels)
    targets = []
    for u in us:
        seen = [read_labels[c] for c in col[rowptr[u]:rowptr[u + 1]]]
        targets.append([read_labels[i] for i in rng.integers(0, n, size=5)] + seen[:1])
    targets[0] = [read_labels[col[rowptr[hub]]]]                           # the hub's only target is a seen neighbour
    if not bip:
        assert deg[least] == 0                                             # a node without in-neighbours is among them
    for seen in (True, False):
        got = model.rank_recommended(nodes, targets, exclude_seen=seen, **kw)
        want = K.rank_recommended_ref(read, labels, rowptr, col, scale, nodes, targets, seen, also_self=not bip)
        T.same_frame(got, want, ("rank_recommended", seen))
        # the ranks against recommend's own frame
        rec = model.recommend(nodes[:6], n, exclude_seen=seen, **kw)
        for i, x in enumerate(nodes[:6]):
            mine, block = got[got["node"] == x].iloc[:len(targets[i])], rec[rec["node"] == x].reset_index(drop=True)
            assert (mine["candidates"] == len(block)).all()
            for _, r in mine.iterrows():
                if r["rank"]:
                    assert block["neighbor"][r["rank"] - 1] == r["target"] and block["score"][r["rank"] - 1] == r["score"]
                else:
                    assert r["target"] not in set(block["neighbor"])
        ks = (1, 10, n)
        ev = model.evaluate(nodes, targets, ks=ks, exclude_seen=seen, **kw)
        T.same_frame(ev, K.evaluate_ref(want, nodes, targets, ks), ("evaluate", seen))
        assert ev["hits@%d" % n].tolist() == (ev["targets"] - ev["not_candidates"]).tolist()
        if seen:
            assert ev["not_candidates"][0] == 1 and ev["best_rank"][0] == 0 and ev["reciprocal_rank"][0] == 0.0
        if not bip:
            assert ev["best_rank"][1] == 0 and ev["not_candidates"][1] == len(targets[1])     # no neighbours: no ranking
    assert list(model.evaluate(nodes[:2], targets[:2], **kw).columns)[-1] == "hits@10"


@pytest.mark.parametrize("variant", ["f32-kept", "f32-compact", "world3-kept", "loaded", "pruned"])
def test_rank_recommended_and_evaluate_on_a_directed_fit(variant, graph, tmp_path):
    with model_of(variant, graph, tmp_path) as model:
        check_recommended(model)


@pytest.mark.parametrize("variant", ["f32-kept", "f32-compact", "pruned"])
def test_the_bipartite_groups(variant, tmp_path):
    df = bipartite_random(90, 60, 0.1, seed=3)
    with model_of(variant, df, tmp_path, cls="BipartiteSimRankPP", strict_reference=False) as model:
        frames = model.frame()
        for group in (1, 2):
            labels = list(frames[group - 1].index)
            n = len(labels)
            rng = np.random.default_rng(group)
            sets = [[], [labels[3]], [labels[i] for i in rng.permutation(n)[:9]], list(labels)]
            weights = [list(rng.normal(size=len(s))) for s in sets]
            targets = [labels[:4], list(labels), [labels[i] for i in rng.integers(0, n, size=7)], labels[-2:]]
            for exclude in ("members", None):
                got = model.rank_sets(sets, targets, weights=weights, exclude=exclude, group=group)
                T.same_frame(got, K.rank_sets_ref(frames[group - 1], sets, targets, weights, exclude=exclude), (group, exclude))
                check_against_top_k(model, got, sets, weights, exclude, n, {"group": group})
            check_recommended(model, group)


def test_a_band_boundary(graph, tmp_path, monkeypatch):
    """70 baskets in bands of 9 (the Reader's ``SLAB_BYTES`` cut down) equal the one-band result and the statement, on
    one block and on LocalWorld(3)'s three."""
    for variant in ("f32-compact", "world3-kept"):
        with model_of(variant, graph, tmp_path) as model:
            frame = model.frame()
            labels = list(frame.index)
            rng = np.random.default_rng(17)
            sets = [[labels[i] for i in rng.integers(0, N, size=rng.integers(0, 12))] for _ in range(70)]
            weights = [list(rng.normal(size=len(s))) for s in sets]
            targets = [[labels[i] for i in rng.integers(0, N, size=rng.integers(0, 6))] + list(s[:1]) for s in sets]
            with monkeypatch.context() as m:
                m.setattr(_query, "SLAB_BYTES", 1 << 28)
                one = model.rank_sets(sets, targets, weights=weights)
            T.same_frame(one, K.rank_sets_ref(frame, sets, targets, weights), "one band against the statement")
            with monkeypatch.context() as m:
                m.setattr(_query, "SLAB_BYTES", 9 * 8 * N)
                T.same_frame(model.rank_sets(sets, targets, weights=weights), one, "in bands of 9")
            with monkeypatch.context() as m:
                m.setattr(_query, "SLAB_BYTES", 1)                          # one basket per band
                T.same_frame(model.rank_sets(sets[:9], targets[:9], weights=weights[:9]),
                             one[one["set"] < 9].reset_index(drop=True), "one basket per band")


def test_lifetime(graph):
    model = T.fit("SimRank", graph).compact()
    frame = model.frame()
    labels = list(frame.index)
    before = model.device_bytes
    model.rank_sets([labels[:5]], [labels[3:9]])
    model.rank_recommended(labels[:5], [labels[:2]] * 5)
    model.evaluate(labels[:5], [labels[:2]] * 5, ks=(1, 3))
    assert model.device_bytes == before
    assert np.array_equal(model.frame().values.view(np.uint64), frame.values.view(np.uint64))
    model.release()
    for call in (lambda: model.rank_sets([labels[:5]], [labels[:1]]), lambda: model.rank_recommended(labels[:5], [[]] * 5),
                 lambda: model.evaluate(labels[:5], [[]] * 5)):
        with pytest.raises(RuntimeError, match="released"):
            call()
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().rank_sets([[1]], [[1]])
