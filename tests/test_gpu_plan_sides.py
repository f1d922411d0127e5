"""``side(j)`` of the four plan classes (``engine.Plan``, ``ShardPlans``, ``BiPlan``, ``ShardBiPlans``) end to end, at the
smallest shapes that can still go wrong: 70 nodes (no multiple of 32: a ragged last panel, and ragged column blocks on 3
virtual ranks) and a 90 x 70 two-matrix graph (a side's ``n`` must be its own group's).  Per side: what the side
answers is bit for bit what the class's own entry points answer; its top-k, pairs and rows are elements of its own dense
result (float32 values widened to float64); and the dense result is the float64 oracle's within the parity bar."""
import numpy as np
import pytest

from oracle import simrank_oracle as O
from simrank_amd import ingest, synth
from tests.graphs import bipartite_random
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

UPDATES, K, NODES = 5, 3, (0, 1, 33, 64, 69)


@pytest.fixture(scope="module")
def ops():
    from simrank_amd.engine import HipOps
    return HipOps(0)


@pytest.fixture(scope="module")
def one_matrix():
    """(CSR, [the oracle's S after 5 updates])."""
    df = synth.er_directed(70, 0.12, seed=3)
    _, csr = ingest.directed(df, False, "from", "to", "weight")
    assert csr.n_rows == 70
    _, G = O.directed_graph(df, False)
    return csr, [O.iterate_directed(G, 0.8, UPDATES, 0.0)[0]]


@pytest.fixture(scope="module")
def two_matrix():
    """(CSR12, CSR21, [the oracle's S1, S2 after 5 loop bodies])."""
    df = bipartite_random(90, 70, 0.12, seed=8)
    *_, g12, g21 = ingest.bipartite(df, False, "user", "item", "weight")
    assert (g12.n_rows, g12.n_cols) == (90, 70)
    *_, G12, G21 = O.bipartite_graph(df, False)
    return g12, g21, list(O.iterate_bipartite(G12, G21, 0.8, 0.8, UPDATES, 0.0)[:2])


def _check_side(side, n, legacy, want):
    """``legacy``: the class's own (result, topk(k), pairs_above(t)) for this side."""
    assert side.n == n and len(side.getters) >= 1
    S = side.result()
    assert S.shape == (n, n) and S.dtype == np.float64
    assert_close(S, want)
    off_diag = S[~np.eye(n, dtype=bool)]
    t = float(np.median(off_diag))
    assert t > 0 and 0.3 < (off_diag >= t).mean() < 0.7          # about half of the pairs qualify
    # the side against the entry points the class has always had: the same bits
    assert np.array_equal(S, legacy[0]())
    idx, val = side.topk(K)
    off, ids, vals = side.pairs_above(t)
    for got, old in zip((idx, val, off, ids, vals), legacy[1](K) + legacy[2](t)):
        assert got.dtype == old.dtype and np.array_equal(got, old)
    # ... and against the side's own dense result
    for a in range(n):
        cand = np.array([c for c in range(n) if c != a])
        order = cand[np.lexsort((cand, -S[a, cand]))][:K]
        assert list(idx[a]) == list(order), a
        np.testing.assert_array_equal(val[a].astype(np.float64), S[a, order])
    mask = (S >= t) & ~np.eye(n, dtype=bool)
    r, c = np.nonzero(mask)
    assert off.tolist() == np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).tolist()
    assert np.array_equal(ids, c) and np.array_equal(vals.astype(np.float64), S[r, c])
    nodes = [a for a in NODES if a < n]
    reader = side.reader()
    try:
        rows = reader.rows(nodes)
    finally:
        reader.close()
    assert rows.dtype == np.float64 and np.array_equal(rows, S[nodes])
    if hasattr(side, "rows"):                                    # (the single-GPU libraries' own row read-back)
        assert np.array_equal(side.rows(nodes).astype(np.float64), S[nodes])


@pytest.mark.parametrize("world", [None, 3])
def test_sides_of_a_one_matrix_plan(ops, one_matrix, world):
    from simrank_amd.engine import Plan, ShardPlans
    csr, want = one_matrix
    plan = Plan(ops, csr) if world is None else ShardPlans(ops, csr, world=world, leg2_form=0)
    try:
        assert plan.run(UPDATES, 0.0) == (UPDATES, None)
        _check_side(plan.side(0), 70, (plan.result, plan.topk, plan.pairs_above), want[0])
        if world:
            assert [plan.side(0).info(i) for i in range(world)] == [plan.info(i) for i in range(world)]
            assert sum(i["col_hi"] - i["col_lo"] for i in map(plan.info, range(world))) == 70
    finally:
        plan.free()


@pytest.mark.parametrize("world", [None, 2])
def test_sides_of_a_two_matrix_plan(ops, two_matrix, world):
    from simrank_amd.engine import BiPlan, ShardBiPlans
    g12, g21, want = two_matrix
    if world is None:
        plan = BiPlan(ops, g12, g12.rowscale, g21.rowscale)
        result = plan.result_group
    else:
        plan = ShardBiPlans(ops, g12, g12.rowscale, g21.rowscale, world=world, leg2_form=0)
        result = plan.result
    try:
        assert plan.run(UPDATES, 0.0) == (UPDATES, None)
        for j, n in enumerate((90, 70)):
            g = j + 1
            _check_side(plan.side(j), n, (lambda: result(g), lambda k: plan.topk(g, k), lambda t: plan.pairs_above(g, t)),
                        want[j])
            if world:
                assert [plan.side(j).info(i) for i in range(world)] == [plan.side_info(g, i) for i in range(world)]
                assert plan.side_info(g)["n"] == n
    finally:
        plan.free()
