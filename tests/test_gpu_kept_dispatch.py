"""The two dispatch decisions of a kept model's queries (``_query.SolverQueries.lists`` / ``one_block``) on a real MI355X:
a model held in three column blocks of unequal width answers, bit for bit, what the same fit on one GPU answers, before
and after ``prune``, and the temporary block a query packs is gone when the query returns.

The graph has 70 nodes: on ``LocalWorld(3)`` that is three blocks of 24, 23 and 23 columns, none a multiple of a panel's
32, the smallest shape with "more than one block, widths unequal, N % 32 != 0".  f32 is the storage a ``LocalWorld`` of
that size holds (the fp16-held form needs N % (32 x ranks) == 0, float64 runs on one GPU only).

The two fits must hold the same bits for their queries to be comparable bit for bit, and on a general graph they do not:
the one-GPU plan and the three-rank plan add a row's terms in different orders (``ring(70, 140)``, SimRank++: one element
of column 0 came out as 0.02133333683 and 0.02133333497).  So the graph is ``exact.regular_graph(70, 4)`` with C = 0.5,
the suite's graph of exact fits: every row scale is 1/4, the iterates of the first four updates lie on a dyadic grid that
float32 holds (``exact.exact_updates``: asserted below), and every sum has the same bits in any order."""
import numpy as np
import pytest
from pandas.testing import assert_frame_equal, assert_series_equal

from oracle import simrank_oracle as O
from simrank_amd import _model
from simrank_amd.driver import LocalWorld
from simrank_amd.engine import HipOps
from tests import exact as X
from tests.test_gpu_cluster import UPDATES, fit

pytestmark = pytest.mark.gpu

N = 70


def same(got, want):
    if isinstance(got, tuple):
        assert isinstance(want, tuple) and len(got) == len(want)
        for g, w in zip(got, want):
            same(g, w)
    elif hasattr(got, "columns"):
        assert_frame_equal(got, want, check_exact=True)
        for c in got.columns:                                # (check_exact compares values: the bits too)
            if got[c].dtype == np.float64:
                assert got[c].to_numpy().tobytes() == want[c].to_numpy().tobytes(), c
    elif hasattr(got, "index"):
        assert_series_equal(got, want, check_exact=True)
    else:
        assert np.asarray(got).dtype == np.asarray(want).dtype and np.asarray(got).tobytes() == np.asarray(want).tobytes()


def test_a_three_block_model_answers_what_the_one_block_model_answers(monkeypatch):
    df = X.regular_graph(N, 4, seed=N + 4)
    assert X.exact_updates(O.directed_graph(df)[1], 0.5, None, mantissa=24, limit=8).updates >= UPDATES
    one, three = fit("SimRank", df, C=0.5), fit("SimRank", df, C=0.5, world=LocalWorld(3), mode="sparse")
    packed = []
    detach = _model.detach
    monkeypatch.setattr(_model, "detach", lambda solver, precision=None: packed.append(solver) or detach(solver, precision))
    try:
        widths = [b["cols"] for b in three._model[0]._reader(0).blocks]
        assert len(widths) == 3 and sum(widths) == N and len(set(widths)) > 1 and len(one._model[0]._reader(0).blocks) == 1
        same(three.frame(), one.frame())                     # the two fits hold the same bits: what follows compares queries
        labels = one.frame().index
        rng = np.random.default_rng(70)
        clustering = rng.integers(0, 5, size=N)
        seeds = [labels[i] for i in rng.choice(N, 6, replace=False)]
        a = [labels[i] for i in rng.integers(0, N, size=12)]
        b = [labels[(labels.get_loc(x) + 1 + int(s)) % N] for x, s in zip(a, rng.integers(0, N - 1, size=12))]
        vals = np.unique(one.frame().to_numpy())
        t1, t2 = float(vals[vals > 0][vals[vals > 0].size // 2]), float(vals[vals > 0][-vals[vals > 0].size // 10])
        packing = {"cluster_quality": lambda m: m.cluster_quality(clustering), "assign": lambda m: m.assign(seeds),
                   "kmedoids": lambda m: m.kmedoids(seeds, max_iter=3), "explain": lambda m: m.explain(a, b, k=4)}
        in_place = {"components": lambda m: m.components([t1, t2]), "count_pairs": lambda m: m.count_pairs([t1, t2, 0.0])}
        for name, query in packing.items():                  # (the first pass also warms the pool's size classes)
            before = len(packed)
            same(query(three), query(one))
            assert len(packed) == before + 1 and packed[-1] is three._model[0], name      # packed once, the model itself
        for name, query in in_place.items():
            before = len(packed)
            same(query(three), query(one))
            assert len(packed) == before, name               # several blocks read in place: nothing is packed
        held, at_rest = three.device_bytes, HipOps.pool_stats()
        for query in list(packing.values()) + list(in_place.values()):
            same(query(three), query(one))
        print("device_bytes", held, three.device_bytes, "pool at rest", at_rest, HipOps.pool_stats())
        assert three.device_bytes == held and HipOps.pool_stats() == at_rest               # the temporaries are gone
        # prune packs once for the model, then every query is answered from the lists
        n_packed = len(packed)
        assert three.prune(5) is three and one.prune(5) is one
        assert len(packed) == n_packed + 1 and three.kept_neighbors == one.kept_neighbors == 5
        assert three.device_bytes == one.device_bytes == N * 5 * 12 + N * 8
        for name, query in packing.items():
            same(query(three), query(one))
        assert len(packed) == n_packed + 1                   # a pruned model packs nothing
    finally:
        one.release()
        three.release()
