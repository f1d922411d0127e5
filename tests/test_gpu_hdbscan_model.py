"""``core_similarity``, ``linkage(min_samples=)`` and ``hdbscan`` of a kept model on a real MI355X: all equal
``hdbscan_ref`` on ``model.frame()`` exactly, for every storage (f32, fp16-held, float64), kept, compact, compact to fp16,
saved and loaded, a ``LocalWorld(3)`` and a pruned model, in both groups of a bipartite class and with an asymmetric
prior, where ``S[a, b] != S[b, a]`` and the larger direction is the pair height.

The three identities of the contract are checked against the REAL ``dbscan``, ``degrees`` and ``linkage`` of the same
model, at the levels ``test_gpu_density_model`` uses (a quantile of the frame's positive off-diagonal values), and each
test asserts ON THE REFERENCE that its levels include one with at least two clusters and a node that is not core: a
trivial outcome cannot pass.  The model is left unchanged."""
import numpy as np
import pandas as pd
import pytest

from simrank_amd import synth
from tests import blocks as B
from tests import density_ref as DR
from tests import hdbscan_ref as HR
from tests.graphs import bipartite_random
from tests.test_gpu_cluster import VARIANTS, as_groups, make_model, off_diagonal, sparse_prior
from tests.test_gpu_density_model import level_of
from tests.test_gpu_linkage import same

pytestmark = pytest.mark.gpu

MIN_SAMPLES = (1, 3, 5)
CLUSTER_COLUMNS = ["parent", "birth", "size", "stability", "selected", "cluster"]


def table_of(Z):
    return tuple(Z[c].to_numpy() for c in ("left", "right", "similarity", "size"))


def same_partition(x, y):
    return np.array_equal(x[:, None] == x[None, :], y[:, None] == y[None, :])


def check_hdbscan(got, S, f, mcs, m, floor, selection, single):
    labels, clusters = got
    want_labels, want_core, want = HR.hdbscan(S, mcs, m, floor, selection, single)
    assert isinstance(labels, pd.DataFrame) and labels.index.equals(f.index)
    assert labels.columns.tolist() == ["cluster", "core_similarity"] and labels.dtypes.tolist() == [np.int64, np.float64]
    assert np.array_equal(labels["cluster"].to_numpy(), want_labels), (mcs, m, floor, selection, single)
    assert np.array_equal(B.bits(labels["core_similarity"].to_numpy()), B.bits(want_core))
    assert isinstance(clusters, pd.DataFrame) and clusters.columns.tolist() == CLUSTER_COLUMNS
    for c in CLUSTER_COLUMNS:
        g, w = clusters[c].to_numpy(), want[c]
        assert g.dtype == w.dtype and np.array_equal(B.bits(g) if g.dtype == np.float64 else g,
                                                     B.bits(w) if w.dtype == np.float64 else w), (c, mcs, m, selection)
    return want


def check_model(model, q, pruned=False):
    frames = as_groups(model.frame())
    before = [B.bits(f.to_numpy()).copy() for f in frames]
    groups = [1, 2] if len(frames) == 2 else [None]
    splits, found = [], 0
    for g, f in enumerate(frames):
        S, n = f.to_numpy(), len(f)
        kw = {} if groups[g] is None else {"group": groups[g]}
        t = level_of(S, q)
        pos = np.unique(off_diagonal(S))
        pos = pos[pos > 0]
        # (a pruned model needs a floor: the smallest kept value, so that every kept entry is used)
        floors = (float(pos[0]),) if pruned else (None, float(pos[pos.size // 3]))
        for m in MIN_SAMPLES:
            core = as_groups(model.core_similarity(m))[g]
            assert isinstance(core, pd.Series) and core.name == "core_similarity" and core.dtype == np.float64
            assert core.index.equals(f.index)
            assert np.array_equal(B.bits(core.to_numpy()), B.bits(HR.core(S, m))), m
            # identity 1, against the real dbscan and degrees
            for level in (t, t / 2, float(np.nextafter(t, 2.0))):
                d = as_groups(model.dbscan(level, m))[g]
                deg = as_groups(model.degrees(level))[g]
                assert np.array_equal(core.to_numpy() >= level, d["core"].to_numpy())
                assert np.array_equal(d["core"].to_numpy(), deg.to_numpy() + 1 >= m)
            for fl in floors:
                Z = as_groups(model.linkage(min_samples=m, min_similarity=fl))[g]
                assert Z.columns.tolist() == ["left", "right", "similarity", "size"]
                assert Z.dtypes.tolist() == [np.int64, np.int64, np.float64, np.int64]
                assert same(table_of(Z), HR.linkage(S, m, fl)), (m, fl)
                # identity 2, against the real dbscan: at levels at or above the floor
                for level in (t, 2 * t) if fl is None or t >= fl else ():
                    d = as_groups(model.dbscan(level, m))[g]
                    cut = model.cut(Z, t=level, **kw).to_numpy()
                    is_core, cluster = d["core"].to_numpy(), d["cluster"].to_numpy()
                    sizes = np.bincount(cut, minlength=n)
                    assert (sizes[cut[~is_core]] == 1).all(), (m, level)
                    assert same_partition(cut[is_core], cluster[is_core]), (m, level)
                    want_cluster, want_core, _, _ = DR.dbscan(S, level, m)
                    assert np.array_equal(is_core, want_core)
                    splits.append((int(np.unique(want_cluster[want_core]).size), int((~want_core).sum())))
                # identity 3, against the real linkage
                if m == 1:
                    plain = as_groups(model.linkage(min_similarity=fl))[g]
                    assert same(table_of(Z), table_of(plain))
        for mcs, m, selection, single in ((5, None, "eom", False), (3, 2, "leaf", False), (4, 6, "eom", True)):
            for fl in floors:
                got = as_groups_of_pairs(model.hdbscan(mcs, m, fl, selection, single), len(frames))[g]
                want = check_hdbscan(got, S, f, mcs, mcs if m is None else m, fl, selection, single)
                found += int(want["selected"].sum())
    # the conditions on the reference: a level with two clusters or more and a node that is not core; clusters found
    assert any(c >= 2 and z >= 1 for c, z in splits), splits
    assert found >= 2
    after = as_groups(model.frame())
    for b, f in zip(before, after):
        assert np.array_equal(B.bits(f.to_numpy()), b)                    # the model is unchanged
    for call in (lambda: model.core_similarity(0), lambda: model.linkage(min_samples=2.5), lambda: model.hdbscan(1),
                 lambda: model.hdbscan(5, selection="best"), lambda: model.hdbscan(5, min_similarity=float("nan"))):
        with pytest.raises(ValueError):
            call()
    model.release()
    for call in (lambda: model.core_similarity(3), lambda: model.hdbscan(5), lambda: model.linkage(min_samples=3)):
        with pytest.raises(RuntimeError, match="released"):
            call()


def as_groups_of_pairs(x, n_groups):
    """``hdbscan``'s (labels, clusters), or a tuple of two such pairs for the bipartite classes -> a list of pairs."""
    if n_groups == 1:
        assert isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], pd.DataFrame)
        return [x]
    assert isinstance(x, tuple) and len(x) == 2 and all(isinstance(p, tuple) and len(p) == 2 for p in x)
    return list(x)


@pytest.fixture(scope="module")
def er():
    return synth.er_directed(150, 0.012, seed=5)


@pytest.fixture(scope="module")
def powerlaw():
    return synth.powerlaw_directed(300, 4.0, seed=11)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_simrank_on_a_random_graph(variant, er, tmp_path):
    model = make_model("SimRank", er, variant, tmp_path)
    try:
        check_model(model, 0.98)
    finally:
        model.release()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_simrankpp_on_a_power_law_graph(variant, powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, variant, tmp_path)
    try:
        check_model(model, 0.95)
    finally:
        model.release()


# (every form but "fp16-kept": fit() refuses fp16-held matrices for the two-matrix classes)
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "fp16-kept"])
def test_bipartite_simrankpp(variant, tmp_path):
    df = bipartite_random(120, 110, 0.03, 12)
    model = make_model("BipartiteSimRankPP", df, variant, tmp_path, strict_reference=False)
    try:
        check_model(model, 0.95)
    finally:
        model.release()


# (an asymmetric prior makes S[a, b] != S[b, a]: the larger direction is the pair height.  Every form but "fp16-kept":
# fit(storage_precision="fp16") wants a symmetric prior)
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "fp16-kept"])
def test_apriori_with_an_asymmetric_prior(variant, er, tmp_path):
    n = len(set(er["from"]) | set(er["to"]))
    model = make_model("AprioriSimRank", er, variant, tmp_path, sparse_prior(n, False))
    try:
        S = model.frame().to_numpy()
        assert (S != S.T).sum() > n                                       # the directions do differ
        check_model(model, 0.97)
    finally:
        model.release()


@pytest.mark.parametrize("graph, q", [("er", 0.8), ("powerlaw", 0.8)])
def test_a_pruned_model_on_the_host(graph, q, er, powerlaw, tmp_path):
    """``prune(k)``: the lists' matrix P on the host, against the reference on the pruned model's own ``frame()``.
    ``core_similarity`` is answered always (the absent entries are +0.0 and count); the table and the clusters need a
    positive ``min_similarity``, as ``linkage`` does."""
    model = make_model("SimRank" if graph == "er" else "SimRankPP", er if graph == "er" else powerlaw, "f32-kept", tmp_path)
    try:
        model.prune(10)
        assert model.kept_neighbors == 10
        with pytest.raises(ValueError, match="tie everything at 0"):
            model.linkage(min_samples=3)
        with pytest.raises(ValueError, match="tie everything at 0"):
            model.hdbscan(5)
        P = model.frame().to_numpy()
        for m in (2, 11, 12, len(P), len(P) + 1):                         # past the kept entries the zeros are counted
            assert np.array_equal(B.bits(model.core_similarity(m).to_numpy()), B.bits(HR.core(P, m))), m
        check_model(model, q, pruned=True)
    finally:
        model.release()
