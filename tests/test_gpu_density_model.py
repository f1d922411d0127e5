"""``degrees`` and ``dbscan`` of a kept model on a real MI355X: both equal ``density_ref`` on ``model.frame()`` exactly, for
every storage (f32, fp16-held, float64), kept, compact, compact to fp16, saved and loaded, a ``LocalWorld(3)`` and a
pruned model; ``dbscan(t, 1).cluster`` is ``components(t)``; the counts lie between ``count_pairs(t)`` and twice that and
their sum is even; the scalar and the sequence form of ``degrees`` agree; the model is unchanged.

The level comes from the model's own ``frame()`` (a quantile of its positive off-diagonal values), and each test asserts
ON THE REFERENCE that at min_samples 3 and 5 the level gives at least two clusters, a border node and a noise node: a
trivial outcome cannot pass.  With the float64 oracle the first graph gives 7 / 28 / 49 and 4 / 35 / 89 clusters / border
nodes / noise nodes when converged (11 / 28 / 104 and 2 / 8 / 140 after the three updates fitted here), the second
4 / 13 / 205 and 3 / 37 / 219.  A bipartite fit is checked in both groups, each at a level of its own frame, and a fit
with an asymmetric prior, where ``S[a, b] != S[b, a]``, exercises the OR of the two directions."""
import numpy as np
import pandas as pd
import pytest

from simrank_amd import synth
from tests import blocks as B
from tests import density_ref as DR
from tests.graphs import bipartite_random
from tests.test_gpu_cluster import VARIANTS, as_groups, make_model, off_diagonal, sparse_prior

pytestmark = pytest.mark.gpu

MIN_SAMPLES = (1, 2, 3, 5)


def level_of(S, q):
    v = off_diagonal(S)
    return float(np.quantile(v[v > 0], q))


def check_model(model, q):
    frames = as_groups(model.frame())
    before = [B.bits(f.to_numpy()).copy() for f in frames]
    splits = []
    for g, f in enumerate(frames):                                        # every group at a level of its own frame
        S, n = f.to_numpy(), len(f)
        t = level_of(S, q)
        ts = [t / 2, t, float(np.nextafter(t, 2.0)), t, 2 * t, 1e-30, 10.0]
        one, many = as_groups(model.degrees(t)), as_groups(model.degrees(ts))
        pairs = as_groups(model.count_pairs([t]))
        comps = as_groups(model.components(t))
        results = {m: as_groups(model.dbscan(t, m)) for m in MIN_SAMPLES}
        assert len(one) == len(many) == len(frames)
        want = DR.degrees(S, ts)
        assert isinstance(one[g], pd.Series) and one[g].name == "neighbors" and one[g].dtype == np.int64
        assert one[g].index.equals(f.index) and np.array_equal(one[g].to_numpy(), want[1])
        assert isinstance(many[g], pd.DataFrame) and many[g].index.equals(f.index) and (many[g].dtypes == np.int64).all()
        assert many[g].columns.tolist() == ts and np.array_equal(many[g].to_numpy().T, want)
        assert not want[6].any() and (want[5] > 0).any()                  # above every value; a similarity above 0
        total = int(want[1].sum())
        assert int(pairs[g][0]) <= total <= 2 * int(pairs[g][0]) and total % 2 == 0 and total > 0
        for m in MIN_SAMPLES:
            got = results[m][g]
            cluster, core, deg, _ = DR.dbscan(S, t, m)
            assert isinstance(got, pd.DataFrame) and got.index.equals(f.index)
            assert got.columns.tolist() == ["cluster", "core", "neighbors"]
            assert got.dtypes.tolist() == [np.int64, np.bool_, np.int64]
            assert np.array_equal(got["neighbors"].to_numpy(), deg) and np.array_equal(deg, want[1])
            assert np.array_equal(got["core"].to_numpy(), core), m
            assert np.array_equal(got["cluster"].to_numpy(), cluster), m
            if m >= 3:
                splits.append(DR.counts(cluster, core))
        assert isinstance(comps[g], pd.Series) and np.array_equal(results[1][g]["cluster"].to_numpy(), comps[g].to_numpy())
        assert results[1][g]["core"].all()
        assert np.array_equal(results[2][g]["cluster"].to_numpy() >= 0, results[2][g]["core"].to_numpy())   # no border node
    # the condition on the reference: clusters, border nodes and noise at once
    assert all(c >= 2 and b >= 1 and z >= 1 for c, b, z in splits), splits
    after = as_groups(model.frame())
    for b, f in zip(before, after):
        assert np.array_equal(B.bits(f.to_numpy()), b)                    # the model is unchanged
    model.release()
    for call in (lambda: model.degrees(t), lambda: model.dbscan(t, 3)):
        with pytest.raises(RuntimeError, match="released"):
            call()


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


# (every form but "fp16-kept": fit() refuses fp16-held matrices for the two-matrix classes.  Each group is checked at the
# 0.95 quantile of its own frame; with the float64 oracle that gives 5 / 26 / 55 and 5 / 25 / 87 clusters / border nodes /
# noise nodes in the first group and 10 / 37 / 40 and 5 / 27 / 77 in the second.  The 90 x 50 graph of the other model
# tests has no such level for its second group: 50 nodes at min_samples = 5 give one cluster or none at most quantiles)
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "fp16-kept"])
def test_bipartite_simrankpp(variant, tmp_path):
    df = bipartite_random(120, 110, 0.03, 12)
    model = make_model("BipartiteSimRankPP", df, variant, tmp_path, strict_reference=False)
    try:
        check_model(model, 0.95)
    finally:
        model.release()


# (an asymmetric prior makes S[a, b] != S[b, a]: the OR of the two directions and "both ways is one neighbour" decide.
# Every form but "fp16-kept": fit(storage_precision="fp16") wants a symmetric prior.  With the float64 oracle the 0.97
# quantile gives 7 / 41 / 43 and 6 / 27 / 115)
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "fp16-kept"])
def test_apriori_with_an_asymmetric_prior(variant, er, tmp_path):
    n = len(set(er["from"]) | set(er["to"]))
    model = make_model("AprioriSimRank", er, variant, tmp_path, sparse_prior(n, False))
    try:
        S = model.frame().to_numpy()
        t = level_of(S, 0.97)
        with np.errstate(invalid="ignore"):
            one_way = ((S >= t) != (S.T >= t)) & ~np.eye(n, dtype=bool)
        assert (S != S.T).sum() > n and one_way.sum() > 10                # the directions differ, also at the level
        check_model(model, 0.97)
    finally:
        model.release()


@pytest.mark.parametrize("graph, q", [("er", 0.8), ("powerlaw", 0.8)])
def test_a_pruned_model_on_the_host(graph, q, er, powerlaw, tmp_path):
    """``prune(k)``: the lists' matrix P on the host, against the reference on the pruned model's own ``frame()``.  P keeps
    the 10 largest values of a row, so its positive values are fewer and larger: the 0.8 quantile is the level at which
    the float64 oracle, pruned the same way, gives 6 / 23 / 40 and 2 / 38 / 80 (first graph), 4 / 13 / 205 and 3 / 37 / 219
    (second)."""
    model = make_model("SimRank" if graph == "er" else "SimRankPP", er if graph == "er" else powerlaw, "f32-kept", tmp_path)
    try:
        model.prune(10)
        assert model.kept_neighbors == 10
        with pytest.raises(ValueError, match="t > 0"):
            model.degrees(0.0)
        with pytest.raises(ValueError, match="t > 0"):
            model.dbscan(-0.5, 3)
        check_model(model, q)
    finally:
        model.release()
