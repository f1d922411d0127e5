"""libsimrank_kmedoids.so and ``assign`` / ``kmedoids`` on a real MI355X.

Kernel level, on synthetic blocks (tests/blocks.py; padding holds a finite sentinel above every value, which a kernel that
reads padding would let win a column).  Both entries compare and copy, no value is added, so every comparison with
``kmedoids_ref`` is bit for bit on any values: ``assign`` in all four layouts with the strides and bases of
``blocks.variants``, on the column counts at both sides of a lane's four columns, a panel and a workgroup's 1024, with
one medoid and with more than the rows (rows listed twice, rows outside), first assignments and the stay rule, a counter
that does not start at zero, guard words after every output and a second run with the same bits; ``pick`` on lists at
both sides of a wave's 64 lanes and beyond, with ties, NaN, and every kind of incumbent.

Model level: ``kmedoids(seeds)`` equals, exactly, the loop of ``kmedoids_ref`` over the model's own public methods
(``rows`` for the medoids' rows, ``cluster_quality`` for ``own``), for every storage, a ``LocalWorld(3)``, compact, loaded
and pruned models and both bipartite groups; on a fit whose iterates are dyadic also the loop on ``model.frame()`` with
``groups_ref``'s sums."""
import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _kmedoids, synth
from tests import blocks as B
from tests import exact as X
from tests import groups_ref as GR
from tests import kmedoids_ref as KR
from tests.graphs import bipartite_random
from tests.test_gpu_cluster import VARIANTS, as_groups, dev, device, make_model  # noqa: F401 (fixtures)
from tests.test_gpu_companion_blocks import same_bits
from tests.test_gpu_groups import planted

pytestmark = pytest.mark.gpu

GUARD_F64 = 1e300
GUARD_I32 = 0x5A5A5A5A
GUARD_U32 = 0xA5A5A5A5
N_COLS = (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025)
N_ROWS = (1, 9, 70)


# ---- the calls -------------------------------------------------------------------------------------------------------------
def run_assign(dev, S, layout, stride, n_rows, n_cols, med_row, med_col, current=None, moved=None):
    """One call of the C entry into pre-filled outputs, each one element longer than it has to be: (cluster, value, the
    counter and the word after it) as the device left them.  ``moved``: what the counter starts at; None: no counter."""
    lib, st = _kmedoids.load(), dev.ops.stream
    cluster_h, value_h = np.full(n_cols + 1, GUARD_I32, dtype=np.int32), np.full(n_cols + 1, GUARD_F64)
    count_h = np.array([moved or 0, GUARD_U32], dtype=np.uint32)
    cluster, value, count = dev.put(cluster_h), dev.put(value_h), dev.put(count_h)
    _kmedoids.check(lib.simrank_kmedoids_assign(
        S, layout, stride, n_rows, n_cols, dev.put(np.ascontiguousarray(med_row, dtype=np.int32)),
        dev.put(np.ascontiguousarray(med_col, dtype=np.int32)), len(med_row),
        None if current is None else dev.put(np.ascontiguousarray(current, dtype=np.int32)), cluster, value,
        None if moved is None else count, st), "assign")
    return dev.get(cluster, cluster_h), dev.get(value, value_h), dev.get(count, count_h)


def check_assign(dev, S, layout, stride, A, med_row, med_col, current, ref, what, moved=None):
    n_rows, n_cols = A.shape
    want_c, want_v, want_moved = ref
    cluster, value, count = run_assign(dev, S, layout, stride, n_rows, n_cols, med_row, med_col, current, moved)
    same_bits(cluster, np.append(want_c, np.int32(GUARD_I32)), (what, "cluster"))
    same_bits(value, np.append(want_v, GUARD_F64), (what, "value"))
    assert count.tolist() == [(moved or 0) + (want_moved if moved is not None else 0), GUARD_U32], (what, "moved")
    return cluster, value


def medoids_of(rng, n_rows, n_cols, k):
    """(med_row, med_col): k medoid rows, distinct while the rows last and then listed again; with k >= 4 one is outside
    the block on either side.  A medoid's own column is (5 r + 1) mod n_cols, as tests/test_gpu_groups.py spreads the
    rows' nodes (a row listed twice names its column twice: the first wins); every third medoid has none."""
    med_row = np.concatenate([rng.permutation(n_rows) for _ in range(-(-k // n_rows))])[:k].astype(np.int32)
    if k >= 4:
        med_row[[1, k - 2]] = [n_rows, -3]
    med_col = np.where(np.arange(k) % 3 == 2, -1, (med_row.astype(np.int64) * 5 + 1) % n_cols).astype(np.int32)
    med_col[(med_row < 0) | (med_row >= n_rows)] = n_cols                   # (a column outside the block: none)
    return med_row, med_col


def currents_of(rng, first, k):
    """A current labelling for the stay rule from the first assignment: a third of the columns where they are (the
    best), a third in a random cluster (tied or worse), the rest outside 0 .. k - 1 (no current)."""
    n = first.size
    kind = rng.integers(0, 3, size=n)
    current = np.where(kind == 0, first, rng.integers(0, k, size=n)).astype(np.int32)
    current[kind == 2] = rng.choice([-1, k, 2 ** 31 - 1, -2 ** 31], size=int((kind == 2).sum()))
    return current


# ---- 1. assign on synthetic blocks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_assign_equals_the_reference(dev, layout):
    stayed = moved_on = 0
    for i, (n_rows, n_cols) in enumerate((r, c) for r in N_ROWS for c in N_COLS):
        blk = B.make_block(layout, n_rows, n_cols, B.variants(layout, n_rows, n_cols)[0][1], 300 + i, kind=("wide", "dyadic")[i % 2])
        A = blk.A
        rng = np.random.default_rng([i, layout, 9])
        cases = []
        for k in sorted({1, 2, 65, min(300, n_rows)}):
            med_row, med_col = medoids_of(rng, n_rows, n_cols, k)
            first = KR.block_assign(A, med_row, med_col)
            current = currents_of(rng, first[0], k)
            cases.append((k, med_row, med_col, first, current, KR.block_assign(A, med_row, med_col, current)))
            stayed += int(((cases[-1][5][0] == current) & (current != first[0])).sum())
            moved_on += int(((cases[-1][5][0] != current) & (current >= 0) & (current < k)).sum())
        for tag, stride, base in B.variants(layout, n_rows, n_cols):
            S = dev.put(B.encode(layout, A, stride, blk.sentinel).tobytes(), base)
            for k, med_row, med_col, first, current, second in cases:
                what = (layout, n_rows, n_cols, tag, k)
                got = check_assign(dev, S, layout, stride, A, med_row, med_col, None, first, what, moved=None if k == 2 else 0)
                check_assign(dev, S, layout, stride, A, med_row, med_col, current, second, what + ("stay",), moved=1000)
                again = run_assign(dev, S, layout, stride, n_rows, n_cols, med_row, med_col)
                for a, b in zip(got, again[:2]):
                    assert np.array_equal(B.bits(a), B.bits(b)), what        # a second run: the same bits
            dev.release()
    assert stayed >= 50 and moved_on >= 50                                   # the stay rule kept some and moved some


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_assign_ties_nan_and_zeros(dev, layout):
    n_rows, n_cols = 9, 150
    column = lambda c, values: {(r, c): v for r, v in enumerate(values)}
    falling = [-1.0 - r / 8 for r in range(n_rows)]
    plant = column(7, [np.nan] * n_rows)                                   # column 7 has no candidate
    plant.update(column(20, falling))                                      # column 20: everything negative but the two zeros
    plant.update({(3, 20): -0.0, (5, 20): 0.0})
    plant.update(column(21, [0.5] * n_rows))                               # column 21: every row ties
    plant.update({(2, c): np.nan for c in range(n_cols)})                  # row 2 is NaN everywhere
    A, stride, base, raw = planted(layout, n_rows, n_cols, plant)
    S = dev.put(raw, base)
    none = np.full(16, -1)

    def check(med_row, current=None, med_col=None, moved=None):
        med_col = none[:len(med_row)] if med_col is None else med_col
        ref = KR.block_assign(A, med_row, med_col, current)
        check_assign(dev, S, layout, stride, A, med_row, med_col, current, ref, (layout, list(med_row)), moved)
        return ref
    cluster, value, _ = check([2, 5, 3, 0, 8])                              # the NaN row first: never chosen
    assert (cluster != 0).sum() == n_cols - 1 and cluster[7] == 0 and np.isnan(value[7])
    assert cluster[20] == 1 and not np.signbit(value[20]) and cluster[21] == 1
    cluster, value, _ = check([3, 5, 0])                                    # -0.0 before +0.0: equal, the first wins
    assert cluster[20] == 0 and np.signbit(value[20]) and value[20] == 0.0
    cluster, _, _ = check([4, 4, 1, 4])                                     # a row listed twice: the first wins everywhere
    assert set(cluster.tolist()) == {0, 2}
    cluster, value, _ = check([n_rows, 6, -1, 2 ** 31 - 1])                 # rows outside the block read NaN
    assert (np.delete(cluster, 7) == 1).all() and cluster[7] == 0
    cluster, value, _ = check([-1, n_rows])                                 # no candidate anywhere: cluster 0, NaN
    assert (cluster == 0).all() and np.isnan(value).all()
    # a medoid's own column: its cluster whatever the values say, its value as stored (NaN for row 2 and in column 7)
    cluster, value, moved = check([2, 5, 0], med_col=[11, 7, 21], moved=5)
    assert cluster[[11, 7, 21]].tolist() == [0, 1, 2] and np.isnan(value[[11, 7]]).all() and value[21] == 0.5
    # the stay rule in column 21, where rows 5, 3 and 0 tie at 0.5, and in column 20 (+0.0, -0.0, -1.0)
    for cur, want21, want20 in ((0, 0, 0), (1, 1, 1), (2, 2, 0)):
        cluster, _, moved = check([5, 3, 0], current=np.full(n_cols, cur), moved=0)
        assert cluster[21] == want21 and cluster[20] == want20              # equal to the best: stays; strictly worse: moves
    # from the NaN row every column moves (but column 7, which has nowhere to go)
    cluster, _, moved = check([5, 2, 0], current=np.full(n_cols, 1), moved=7)
    assert moved == n_cols - 1 and cluster[7] == 1
    # an all-equal block: everything to j = 0
    A1 = np.full((n_rows, n_cols), 0.25)
    _, stride, base = B.variants(layout, n_rows, n_cols)[0]
    S1 = dev.put(B.encode(layout, A1, stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
    ref = KR.block_assign(A1, [3, 1, 8], [-1, -1, -1])
    assert (ref[0] == 0).all() and (ref[1] == 0.25).all()
    check_assign(dev, S1, layout, stride, A1, [3, 1, 8], [-1, -1, -1], None, ref, (layout, "equal"), moved=0)


# ---- 2. pick -------------------------------------------------------------------------------------------------------------------
def run_pick(dev, own, col_pos, group_ptr, med_row, changed=0):
    lib, st, k = _kmedoids.load(), dev.ops.stream, len(med_row)
    med_h = np.append(np.asarray(med_row, dtype=np.int32), np.int32(GUARD_I32))
    coh_h = np.full(k + 1, GUARD_F64)
    count_h = np.array([changed, GUARD_U32], dtype=np.uint32)
    med, coh, count = dev.put(med_h), dev.put(coh_h), dev.put(count_h)
    cp = dev.put(np.ascontiguousarray(col_pos, dtype=np.int32)) if len(col_pos) else dev.put(np.zeros(4, dtype=np.int32))
    _kmedoids.check(lib.simrank_kmedoids_pick(dev.put(np.ascontiguousarray(own, dtype=np.float64)), len(own), cp,
                                              dev.put(np.ascontiguousarray(group_ptr, dtype=np.int64)), k, med, coh, count, st),
                    "pick")
    return dev.get(med, med_h), dev.get(coh, coh_h), dev.get(count, count_h)


def test_pick_equals_the_reference(dev):
    rng = np.random.default_rng(31)
    sizes = [0, 1, 2, 64, 65, 256, 257, 1500, 0, 3, 130, 64]
    n = sum(sizes) + 40
    # few distinct values, so that a list's largest is met several times, and a fifth of them NaN
    own = rng.integers(0, 12, size=n) / 8.0
    own[rng.random(n) < 0.2] = np.nan
    lists = np.split(rng.permutation(n)[:sum(sizes)], np.cumsum(sizes)[:-1])
    lists[5][::37] = [-1, n, 2 ** 31 - 1, -2 ** 31, n + 5, -7, n][:lists[5][::37].size]   # positions outside: skipped
    lists[9][:] = np.flatnonzero(np.isnan(own))[:3]                        # a list of NaN alone: no candidate
    ptr = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=ptr[1:])
    col_pos = np.concatenate(lists)
    best = KR.block_pick(own, col_pos, ptr, [-1] * len(sizes))[0]           # (from no incumbent: every list's candidate)
    ties = sum(int((own[l[(l >= 0) & (l < n)]] == own[b]).sum() > 1) for l, b in zip(lists, best) if b >= 0)
    assert ties >= 6
    nan_at, worst = int(np.flatnonzero(np.isnan(own))[0]), int(np.nanargmin(own))
    incumbents = {
        "none": [-1] * len(sizes),
        "the candidate itself": best,                                       # kept: nothing is strictly larger
        "an equal one later in the list": [
            int(l[np.flatnonzero((l >= 0) & (l < n) & (own[np.clip(l, 0, n - 1)] == own[b]))[-1]]) if b >= 0 else 0
            for l, b in zip(lists, best)],
        "NaN": [nan_at] * len(sizes),
        "the smallest": [worst] * len(sizes),
        "outside": [n, -5, 2 ** 31 - 1] * (len(sizes) // 3),
    }
    seen = set()
    for name, med_row in incumbents.items():
        want = KR.block_pick(own, col_pos, ptr, med_row)
        for start in (0, 77):
            med, coh, count = run_pick(dev, own, col_pos, ptr, med_row, start)
            same_bits(med, np.append(want[0], np.int32(GUARD_I32)), (name, "med_row"))
            same_bits(coh, np.append(want[1], GUARD_F64), (name, "cohesion"))
            assert count.tolist() == [start + want[2], GUARD_U32], name
        seen.add(want[2])
        dev.release()
    kept = KR.block_pick(own, col_pos, ptr, incumbents["an equal one later in the list"])
    assert kept[2] == 0 and np.array_equal(kept[0], incumbents["an equal one later in the list"])
    assert 0 in seen and max(seen) >= 8


# ---- 3. through the estimators ----------------------------------------------------------------------------------------------------
def check_side(model, kw, f, k, dyadic=False):
    """``kmedoids`` and ``assign`` of one side against the reference loop over the model's public methods -> the history."""
    index, n = f.index, len(f)
    seeds = np.random.default_rng(5).choice(n, k, replace=False)
    rows_of = lambda m: model.rows(index[m], **kw).to_numpy()
    own_of = lambda lab: model.cluster_quality(lab, **kw)["own"].to_numpy()
    first = model.assign(index[seeds], **kw)
    want_c, want_v, _ = KR.assign(rows_of(seeds), seeds, rows_only=True)
    assert first.index.equals(index) and first.columns.tolist() == ["cluster", "medoid", "similarity"]
    assert first["cluster"].dtype == np.int64 and first["cluster"].tolist() == want_c.tolist()
    same_bits(first["similarity"].to_numpy(), want_v, (kw, "assign"))
    assert first["medoid"].tolist() == index[seeds[want_c]].tolist()
    out = None
    for max_iter in (1, 20):
        cluster, medoids, sim, sizes, cohesion, steps = KR.kmedoids(rows_of, seeds, max_iter, own_of)
        labels, clusters, history = model.kmedoids(pd.Series(index[seeds]) if max_iter == 1 else list(index[seeds]),
                                                   max_iter=max_iter, **kw)
        what = (kw, max_iter)
        assert labels.index.equals(index) and labels.columns.tolist() == ["cluster", "medoid", "similarity"], what
        assert labels["cluster"].dtype == np.int64 and labels["cluster"].tolist() == cluster.tolist(), what
        assert labels["medoid"].tolist() == index[medoids[cluster]].tolist(), what
        same_bits(labels["similarity"].to_numpy(), sim, (what, "similarity"))
        assert clusters.index.tolist() == list(range(k)) and clusters.columns.tolist() == ["medoid", "size", "cohesion"], what
        assert clusters["medoid"].tolist() == index[medoids].tolist() and clusters["size"].dtype == np.int64, what
        assert clusters["size"].tolist() == sizes.tolist(), what
        same_bits(clusters["cohesion"].to_numpy(), cohesion, (what, "cohesion"))
        assert history.columns.tolist() == ["moved", "changed", "objective"], what
        assert history.dtypes.tolist() == [np.int64, np.int64, np.float64] and len(history) == len(steps) <= max_iter, what
        assert history[["moved", "changed"]].to_numpy().tolist() == [list(s[:2]) for s in steps], what
        same_bits(history["objective"].to_numpy(), np.array([s[2] for s in steps]), (what, "objective"))
        assert history["moved"][0] == n
        if history["changed"].iloc[-1] == 0:
            # converged: no node has a strictly better medoid, so assign(final medoids) finds every node's value again
            again = model.assign(clusters["medoid"], **kw)
            same_bits(again["similarity"].to_numpy(), labels["similarity"].to_numpy(), (what, "assign again"))
        else:
            assert max_iter == 1, what
        out = history
    if dyadic:                                                             # every sum is exact: groups_ref's are the model's
        S = f.to_numpy()
        ref = KR.kmedoids(S, seeds, 20, lambda lab: GR.quality(S, lab)[0])
        assert labels["cluster"].tolist() == ref[0].tolist() and clusters["medoid"].tolist() == index[ref[1]].tolist()
        same_bits(labels["similarity"].to_numpy(), ref[2], "frame: similarity")
        same_bits(clusters["cohesion"].to_numpy(), ref[4], "frame: cohesion")
        same_bits(history["objective"].to_numpy(), np.array([s[2] for s in ref[5]]), "frame: objective")
    return out


def check_model(model, k=12, dyadic=False, converges=True):
    frames = as_groups(model.frame())
    groups = [{"group": 1}, {"group": 2}] if len(frames) == 2 else [{}]
    before = [f.to_numpy().copy() for f in frames]
    histories = [check_side(model, kw, f, k, dyadic) for f, kw in zip(frames, groups)]
    for f, b in zip(as_groups(model.frame()), before):
        assert np.array_equal(B.bits(f.to_numpy()), B.bits(b))                # the model is unchanged
    seeds = [frames[0].index[0]]
    model.release()
    for call in (model.assign, model.kmedoids):
        with pytest.raises(RuntimeError, match="released"):
            call(seeds, **groups[0])
    return histories


@pytest.fixture(scope="module")
def powerlaw():
    return synth.powerlaw_directed(300, 4.0, seed=11)


def not_vacuous(histories):
    for h in histories:
        assert h["changed"][0] > 0 and h["changed"].iloc[-1] == 0 and len(h) < 20, h


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_simrankpp_on_a_power_law_graph(variant, powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, variant, tmp_path)
    try:
        not_vacuous(check_model(model))
    finally:
        model.release()


def test_simrank_on_a_power_law_graph(powerlaw, tmp_path):
    model = make_model("SimRank", powerlaw, "f32-kept", tmp_path)
    try:
        not_vacuous(check_model(model))
    finally:
        model.release()


def test_the_device_history_of_cohesions_is_copied_when_it_is_full(powerlaw, tmp_path, monkeypatch):
    """The cohesions of up to ``HISTORY_ROWS`` iterations wait on the device; with room for one, a loop of two iterations or
    more copies them in pieces and returns what it returns with room for all."""
    model = make_model("SimRankPP", powerlaw, "f32-compact", tmp_path)
    try:
        seeds = model.frame().index[np.random.default_rng(5).choice(300, 12, replace=False)]
        want = model.kmedoids(seeds)
        assert len(want[2]) >= 2
        monkeypatch.setattr(_kmedoids, "HISTORY_ROWS", 1)
        got = model.kmedoids(seeds)
        for g, w in zip(got, want):
            assert g.equals(w)
    finally:
        model.release()


@pytest.mark.parametrize("variant", ["f32-kept", "f64-kept", "world3-kept", "f32-compact-fp16"])
def test_bipartite_simrankpp(variant, tmp_path):
    df = bipartite_random(90, 50, 0.06, 12)
    model = make_model("BipartiteSimRankPP", df, variant, tmp_path, strict_reference=False)
    try:
        check_model(model, k=7)
    finally:
        model.release()


def test_a_pruned_model_clusters_its_matrix_p(powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, "f32-kept", tmp_path)
    try:
        model.prune(10)
        assert model.kept_neighbors == 10
        check_model(model)
    finally:
        model.release()


@pytest.mark.parametrize("variant", ["f32-kept", "f64-kept", "world3-kept", "f32-compact"])
def test_a_fit_with_dyadic_iterates(variant, tmp_path):
    """regular_graph(256, 4) with C = 0.5, as tests/test_gpu_groups.py fits it: the iterate lies on a dyadic grid, every
    float64 sum of its elements is exact in any order, and the loop on the frame with ``groups_ref``'s sums is the model's."""
    import contextlib
    import io
    from oracle import simrank_oracle as O
    from simrank_amd.driver import LocalWorld
    df = X.regular_graph(256, 4, seed=260)
    _, G = O.directed_graph(df)
    updates = X.exact_updates(G, 0.5, None, mantissa=24, limit=8).updates
    assert updates >= 2
    kw, then = VARIANTS[variant]
    kw = dict(kw)
    if "world" in kw:
        kw.update(world=LocalWorld(kw["world"]), mode="sparse")
    est = SRA.SimRank()
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(df, C=0.5, iterations=updates, eps=1e-30, verbose=False, keep=True, **kw)
    if then == "compact":
        est.compact()
    try:
        check_model(est, dyadic=True)
    finally:
        est.release()
