"""``fit(min_similarity=t)`` on the MI355X: every pair of different nodes at least t similar, selected on the device by
libsimrank_select.so, must be the masked ``np.nonzero`` of the dense frame of an identical fit — labels, order and bits —
for every class, both storage precisions, the sharded loops and at full size; and agree with the float64 oracle."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from oracle import simrank_oracle as O
from simrank_amd import ingest, synth
from simrank_amd.driver import LocalWorld
from tests.graphs import bipartite_random

pytestmark = pytest.mark.gpu

COLUMNS = ["node", "neighbor", "similarity"]


def dense_pairs(frame, t):
    """The reference answer: the dense frame's entries >= t off the diagonal, in np.nonzero order."""
    vals = frame.to_numpy()
    mask = vals >= t
    np.fill_diagonal(mask, False)
    r, c = np.nonzero(mask)
    return pd.DataFrame({"node": frame.index.take(r), "neighbor": frame.columns.take(c), "similarity": vals[r, c]})


def assert_same(got, want):
    assert list(got.columns) == COLUMNS
    assert got["similarity"].dtype == np.float64
    assert len(got) == len(want)
    assert list(got["node"]) == list(want["node"])
    assert list(got["neighbor"]) == list(want["neighbor"])
    assert np.array_equal(got["similarity"].to_numpy().view(np.int64), want["similarity"].to_numpy().view(np.int64))
    pd.testing.assert_frame_equal(got, want, check_exact=True)


def assert_near(got, want, t):
    """A sharded loop's frame against one GPU's: its sums run in another order, so values agree to rounding (1e-6) and the
    pairs agree except where a value lies within that rounding of t."""
    a = {(n, m): v for n, m, v in got.itertuples(index=False)}
    b = {(n, m): v for n, m, v in want.itertuples(index=False)}
    for key in a.keys() & b.keys():
        assert abs(a[key] - b[key]) <= 1e-6 * abs(b[key]), key
    for key in a.keys() ^ b.keys():
        assert abs(a.get(key, b.get(key)) - t) <= 1e-6 * t, key


def thresholds(frame):
    """t between stored values, t equal to a stored value (a hit), t above every value (empty), a small t."""
    vals = frame.to_numpy().copy()
    np.fill_diagonal(vals, 0)
    u = np.unique(vals[vals > 0])
    if u.size == 0:
        return [0.5, 2.0]
    mid = u[u.size // 2]
    above = u[u > mid]
    ts = [float(mid), float(u[-1]) * 1.5 + 1.0, float(u[0])]
    if above.size:
        ts.append((float(mid) + float(above[0])) / 2)      # strictly between two stored values
    if u.size > 3:
        ts.append(float(u[u.size // 4]))
    return ts


def _directed(kind):
    if kind == "er":
        return synth.er_directed(300, 0.02, seed=11)               # 300: no multiple of 32, 64 or 128
    if kind == "powerlaw":
        return synth.powerlaw_directed(1000, 6, seed=12)
    if kind == "isolated":                                          # nodes without in-edges, one pure source
        return pd.DataFrame({"from": [1, 2, 3, 4, 5, 9, 9], "to": [2, 3, 1, 5, 4, 1, 4]})
    return pd.DataFrame({"from": [7], "to": [7]})                  # N = 1


@pytest.mark.parametrize("cls", ["SimRank", "SimRankPP"])
@pytest.mark.parametrize("kind", ["er", "powerlaw", "isolated", "single"])
@pytest.mark.parametrize("storage", ["f32", "fp16"])
def test_directed_classes_match_the_dense_frame(cls, kind, storage):
    df = _directed(kind)
    est = getattr(SRA, cls)
    dense = est().fit(df, verbose=False, storage_precision=storage)
    for t in thresholds(dense):
        got = est().fit(df, verbose=False, storage_precision=storage, min_similarity=t)
        assert_same(got, dense_pairs(dense, t))


@pytest.mark.parametrize("symmetric", [True, False])
def test_apriori_simrank_with_a_symmetric_and_an_asymmetric_prior(symmetric):
    df = synth.er_directed(200, 0.03, seed=13)
    n = len(set(df["from"]) | set(df["to"]))
    rng = np.random.default_rng(5)
    prior = rng.random((n, n)) * 0.5
    if symmetric:
        prior = (prior + prior.T) / 2
    dense = SRA.AprioriSimRank().fit(df, prior, verbose=False)
    for t in thresholds(dense):
        assert_same(SRA.AprioriSimRank().fit(df, prior, verbose=False, min_similarity=t), dense_pairs(dense, t))


@pytest.mark.parametrize("cls", ["BipartiteSimRank", "BipartiteSimRankPP"])
@pytest.mark.parametrize("strict", [True, False])
def test_bipartite_classes_both_groups(cls, strict):
    # strict SimRank++ keeps the reference's broadcast error (quirk Q2) unless n1 == n2
    df = bipartite_random(150, 150, 0.05, seed=21) if strict and cls.endswith("PP") else bipartite_random(170, 90, 0.06,
                                                                                                          seed=22)
    est = getattr(SRA, cls)
    d1, d2 = est().fit(df, verbose=False, strict_reference=strict)
    for t in thresholds(d1)[:3] + thresholds(d2)[:2]:
        p1, p2 = est().fit(df, verbose=False, strict_reference=strict, min_similarity=t)
        assert_same(p1, dense_pairs(d1, t))
        assert_same(p2, dense_pairs(d2, t))


def test_bipartite_apriori():
    df = bipartite_random(120, 80, 0.07, seed=23)
    n1, n2 = df["user"].nunique(), df["item"].nunique()
    rng = np.random.default_rng(6)
    a1, a2 = rng.random((n1, n1)) * 0.3, rng.random((n2, n2)) * 0.3
    a1, a2 = (a1 + a1.T) / 2, (a2 + a2.T) / 2
    d1, d2 = SRA.BipartitleAprioriSimRank().fit(df, a1, a2, verbose=False, strict_reference=False)
    for t in thresholds(d1)[:3]:
        p1, p2 = SRA.BipartitleAprioriSimRank().fit(df, a1, a2, verbose=False, strict_reference=False, min_similarity=t)
        assert_same(p1, dense_pairs(d1, t))
        assert_same(p2, dense_pairs(d2, t))


def test_max_pairs_guard_and_the_empty_frame():
    df = synth.er_directed(300, 0.02, seed=11)
    dense = SRA.SimRank().fit(df, verbose=False)
    t = thresholds(dense)[2]                       # the smallest stored positive value: every pair with support
    want = dense_pairs(dense, t)
    assert len(want) > 1000
    assert_same(SRA.SimRank().fit(df, verbose=False, min_similarity=t, max_pairs=len(want)), want)
    with pytest.raises(ValueError, match=rf"{len(want)} pairs.*max_pairs={len(want) - 1}"):
        SRA.SimRank().fit(df, verbose=False, min_similarity=t, max_pairs=len(want) - 1)
    empty = SRA.SimRank().fit(df, verbose=False, min_similarity=1.5)
    assert list(empty.columns) == COLUMNS and len(empty) == 0
    assert empty.dtypes.equals(want.dtypes)


def test_top_k_with_min_similarity_is_the_top_k_frame_above_t():
    df = synth.er_directed(300, 0.02, seed=11)
    top = SRA.SimRankPP().fit(df, verbose=False, top_k=7)
    t = float(np.median(top["similarity"]))
    got = SRA.SimRankPP().fit(df, verbose=False, top_k=7, min_similarity=t)
    want = top[top["similarity"] >= t].reset_index(drop=True)
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    assert 0 < len(got) < len(top)


@pytest.mark.parametrize("storage", ["f32", "fp16"])
@pytest.mark.parametrize("cls", ["SimRank", "SimRankPP"])
def test_local_world_of_four_ranks_gives_the_single_gpu_frame(cls, storage):
    """Exact against the dense frame of the same world; against one GPU to the rounding in which the sharded loop's sums
    differ (f32: 700 nodes, no multiple of 128; fp16-held shards need a multiple of 4 x 64 nodes)."""
    df = synth.powerlaw_directed(700 if storage == "f32" else 512, 6, seed=14)
    est = getattr(SRA, cls)
    kw = dict(verbose=False, storage_precision=storage)
    dense = est().fit(df, **kw)
    dense4 = est().fit(df, world=LocalWorld(4), **kw)
    for t in thresholds(dense)[:4]:
        one = est().fit(df, min_similarity=t, **kw)
        four = est().fit(df, min_similarity=t, world=LocalWorld(4), **kw)
        assert_same(one, dense_pairs(dense, t))
        assert_same(four, dense_pairs(dense4, t))
        if storage == "f32":
            assert_near(four, one, t)


def test_local_world_bipartite():
    df = bipartite_random(170, 90, 0.06, seed=22)
    d1, d2 = SRA.BipartiteSimRankPP().fit(df, verbose=False, strict_reference=False, world=LocalWorld(3))
    t = thresholds(d1)[0]
    p1, p2 = SRA.BipartiteSimRankPP().fit(df, verbose=False, strict_reference=False, world=LocalWorld(3), min_similarity=t)
    assert_same(p1, dense_pairs(d1, t))
    assert_same(p2, dense_pairs(d2, t))


def test_thread_ranks_give_the_in_process_pieces():
    """Four concurrent ranks (engine.ThreadRanks: the code path of an RCCL rank) select their own columns; the merged
    pieces are bit-equal to the in-process group's, whose pairs are the single plan's (values to rounding)."""
    from simrank_amd import _select
    from simrank_amd.engine import HipOps, Plan, ShardPlans, ThreadRanks
    df = synth.powerlaw_directed(700, 8, seed=15)
    _, csr = ingest.directed(df, False, "from", "to", "weight")
    ops = HipOps(0)
    plan = Plan(ops, csr, coef=0.8)
    plan.run(6, 0.0)
    t = 0.02
    want = plan.pairs_above(t)
    plan.free()
    sp = ShardPlans(ops, csr, world=4)
    sp.run(6, 0.0)
    local = sp.pairs_above(t)
    sp.free()
    for a, b in zip(local[:2], want[:2]):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(local[2], want[2], rtol=1e-6)

    def rank(r, rops, comm):
        spr = ShardPlans(rops, csr, world=4, comm=comm)
        spr.run(6, 0.0)
        sel = spr.selection(t)
        out = (sel.emit(), sel.row_order)
        spr.free()
        return out
    tr = ThreadRanks(4)
    try:
        outs = tr.run(rank, timeout=120.0)
    finally:
        tr.close()
    merged = _select.merge([p for pieces, _ in outs for p in pieces], outs[0][1])
    for a, b in zip(merged, local):
        assert np.array_equal(a, b)
    assert want[1].size > 100


def test_one_rank_torch_world_gives_the_single_gpu_frame():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from tests.conftest import free_port
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(root, "tests", "select_dist_worker.py")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert p.returncode == 0 and "SELECT WORLD ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


@pytest.mark.parametrize("cls,ref", [("SimRank", O.fit_simrank), ("SimRankPP", O.fit_simrank_pp)])
def test_against_the_float64_oracle(cls, ref):
    """N ~ 2000: the selected set is the oracle's S >= t in float64, except pairs within 1e-5 t of the threshold."""
    df = synth.powerlaw_directed(2000, 8, seed=16)
    want = ref(df, verbose=False)
    S = np.asarray(want["S"])
    labels = list(want["labels"])
    off = S.copy()
    np.fill_diagonal(off, 0)
    for t in (float(np.quantile(off[off > 0], 0.999)), float(np.quantile(off[off > 0], 0.9))):
        got = getattr(SRA, cls)().fit(df, verbose=False, min_similarity=t)
        pos = {lab: i for i, lab in enumerate(labels)}
        have = set(zip(got["node"].map(pos), got["neighbor"].map(pos)))
        mask = off >= t
        np.fill_diagonal(mask, False)
        expect = set(zip(*np.nonzero(mask)))
        for a, b in have ^ expect:
            assert abs(S[a, b] - t) <= 1e-5 * t, (a, b, S[a, b], t)
        assert len(have) > 0


@pytest.mark.parametrize("storage", ["f32", "fp16"])
def test_full_size_config4_counts_and_sampled_rows(storage):
    """N = 32768 (BASELINE config 4's graph) through the C plan: per-row counts of the selection against the rows'
    host filter on sampled rows (Plan.rows), and the sampled rows' hits themselves."""
    from simrank_amd.engine import HipOps, Plan
    df = synth.WORKLOADS["pl32768d32"][0]()
    _, csr = ingest.directed(df, False, "from", "to", "weight")
    n = csr.n_rows
    ops = HipOps(0)
    plan = Plan(ops, csr, coef=0.8, storage=storage)
    plan.run(3, 0.0)
    rng = np.random.default_rng(4)
    rows = np.unique(np.concatenate([rng.choice(n, 60, replace=False), [0, n - 1]]))
    R = plan.rows(rows)
    off = R.copy()
    off[np.arange(rows.size), rows] = 0
    t = float(np.quantile(off[off > 0], 0.99))
    offsets, ids, vals = plan.pairs_above(t, max_pairs=2 ** 30)
    plan.free()
    assert offsets.size == n + 1 and offsets[-1] == ids.size
    for k, a in enumerate(rows):
        mask = R[k].astype(np.float64) >= t
        mask[a] = False
        cols = np.flatnonzero(mask)
        seg = slice(offsets[a], offsets[a + 1])
        assert np.array_equal(ids[seg], cols), a
        assert np.array_equal(vals[seg].view(np.uint32), R[k, cols].view(np.uint32)), a
    assert np.all(np.diff(offsets) >= 0) and ids.min() >= 0 and ids.max() < n
