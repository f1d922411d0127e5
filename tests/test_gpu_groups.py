"""libsimrank_groups.so and ``cluster_quality`` & co on a real MI355X.

Kernel level, on synthetic blocks (tests/blocks.py, kind="dyadic": multiples of 2^-8 below 16, so every float64 partial
sum is exact and the comparison with ``groups_ref.block_means`` is bit for bit; padding holds a finite sentinel above
every value, which a kernel that reads padding would add to a sum): all four layouts with the strides and bases of
``blocks.variants``, the shapes of tests/test_gpu_cluster.py, labellings from K = 1 to all singletons with lists on both
sides of the lengths at which the kernel changes the way it sums (8 | 9 positions: a lane | a wave; 1023 | 1024: a wave
| the workgroup) and of 64, 65, 256, 257 and 1025, shuffled lists, rows that exclude nothing and rows that are skipped;
guard words after every output; NaN and -0.0 entries; ties; a second run with the same bits.

Model level: the four methods equal ``groups_ref`` on ``model.frame()`` within the bound of a float64 sum in any order,
for every storage, a ``LocalWorld(3)``, compact, loaded and pruned models, and bit for bit on a fit whose iterates are
dyadic."""
import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _groups, synth
from tests import blocks as B
from tests import exact as X
from tests import groups_ref as GR
from tests.graphs import bipartite_random
from tests.test_gpu_cluster import SHAPES, VARIANTS, as_groups, dev, device, make_model  # noqa: F401 (fixtures)
from tests.test_gpu_companion_blocks import same_bits

pytestmark = pytest.mark.gpu

GUARD_F64 = 1e300
GUARD_I32 = 0x5A5A5A5A
EDGE_SIZES = (8, 9, 64, 65, 256, 257, 1023, 1024, 1025)     # list lengths at which the kernel's path or turn count changes


# ---- the call --------------------------------------------------------------------------------------------------------------
def run_means(dev, S, layout, stride, n_rows, n_cols, row_group, row_col, col_pos, group_ptr, ld=None):
    """One call of the C entry into pre-filled outputs, each one element longer than it has to be: (own, other, nearest,
    means or None) as the device left them, the guard elements and the slack of ``means`` included."""
    lib, st, k = _groups.load(), dev.ops.stream, len(group_ptr) - 1
    own_h, other_h = np.full(n_rows + 1, GUARD_F64), np.full(n_rows + 1, GUARD_F64)
    near_h = np.full(n_rows + 1, GUARD_I32, dtype=np.int32)
    means_h = None if ld is None else np.full(n_rows * ld + 1, GUARD_F64)
    own, other, near = dev.put(own_h), dev.put(other_h), dev.put(near_h)
    means = None if ld is None else dev.put(means_h)
    cp = dev.put(np.ascontiguousarray(col_pos, dtype=np.int32)) if len(col_pos) else dev.put(np.zeros(4, dtype=np.int32))
    _groups.check(lib.simrank_groups_means(
        S, layout, stride, n_rows, n_cols, dev.put(np.ascontiguousarray(row_group, dtype=np.int32)),
        dev.put(np.ascontiguousarray(row_col, dtype=np.int32)), cp, dev.put(np.ascontiguousarray(group_ptr, dtype=np.int64)),
        k, own, other, near, means, 0 if ld is None else ld, st), "means")
    return (dev.get(own, own_h), dev.get(other, other_h), dev.get(near, near_h),
            None if ld is None else dev.get(means, means_h))


def expected(ref, n_rows, k, ld):
    """What ``run_means`` must return for the reference ``ref`` (block_means): guards where nothing may be written."""
    own_r, other_r, near_r, table, _ = ref
    skipped = near_r == -2
    own, other = np.full(n_rows + 1, GUARD_F64), np.full(n_rows + 1, GUARD_F64)
    near = np.full(n_rows + 1, GUARD_I32, dtype=np.int32)
    own[:n_rows], other[:n_rows], near[:n_rows] = (np.where(skipped, GUARD_F64, own_r), np.where(skipped, GUARD_F64, other_r),
                                                  np.where(skipped, GUARD_I32, near_r))
    means = None
    if ld is not None:
        means = np.full(n_rows * ld + 1, GUARD_F64)
        body = means[:n_rows * ld].reshape(n_rows, ld)
        body[:, :k] = np.where(skipped[:, None], GUARD_F64, table)
    return own, other, near, means


def check_call(dev, S, layout, stride, A, case, ref, what):
    """With ``means`` (over-wide) and without; both equal the reference bit for bit, guards and slack intact."""
    n_rows, n_cols = A.shape
    row_group, row_col, col_pos, group_ptr = case
    k = len(group_ptr) - 1
    for ld in (k + 3, None):
        got = run_means(dev, S, layout, stride, n_rows, n_cols, row_group, row_col, col_pos, group_ptr, ld)
        want = expected(ref, n_rows, k, ld)
        for g, w, name in zip(got, want, ("own", "other", "nearest", "means")):
            if w is not None:
                same_bits(g, w, (what, name, ld))
    return got


# ---- labellings of a block's columns -----------------------------------------------------------------------------------------
def lists_of(gidx, rng, shuffle=True):
    """Cluster ranks of the columns -> (col_pos, group_ptr): cluster-major, the members shuffled within a cluster."""
    k = int(gidx.max()) + 1
    lists = [np.flatnonzero(gidx == g) for g in range(k)]
    if shuffle:
        lists = [rng.permutation(l) for l in lists]
    ptr = np.zeros(k + 1, dtype=np.int64)
    np.cumsum([l.size for l in lists], out=ptr[1:])
    return np.concatenate(lists).astype(np.int32), ptr


def labellings(n_cols, rng):
    """name -> cluster rank of every column: K = 1, all singletons, two clusters one of which is a single node, five uneven
    random clusters, and one cluster of exactly m columns (the others spread over three more) for every m of EDGE_SIZES
    that leaves a column over."""
    out = {"one": np.zeros(n_cols, dtype=np.int64), "singletons": rng.permutation(n_cols).astype(np.int64)}
    if n_cols >= 2:
        two = np.zeros(n_cols, dtype=np.int64)
        two[rng.integers(n_cols)] = 1
        out["two"] = two
    if n_cols >= 5:
        five = rng.choice(5, size=n_cols, p=[0.5, 0.25, 0.15, 0.07, 0.03])
        five[rng.permutation(n_cols)[:5]] = np.arange(5)                   # (none is empty)
        out["five"] = five
    for m in EDGE_SIZES:
        if m < n_cols:
            g = 1 + rng.integers(0, 3, size=n_cols)
            g[rng.permutation(n_cols)[:m]] = 0
            out[f"exactly{m}"] = np.unique(g, return_inverse=True)[1].reshape(-1)   # (ranks without a gap)
            assert (out[f"exactly{m}"] == 0).sum() == m
    return out


def rows_of(n_rows, n_cols, gidx, exclude=True):
    """(row_group, row_col): row r holds the node of column (5 r + 1) mod n_cols, as tests/test_gpu_cluster.py spreads
    them; one row in the middle is skipped.  ``exclude=False``: no row has a column of its own (row_col = -1)."""
    col = (np.arange(n_rows) * 5 + 1) % n_cols
    row_group = gidx[col].astype(np.int32)
    if n_rows > 1:
        row_group[n_rows // 2] = -1 - (n_rows % 3)
    return row_group, (col if exclude else np.full(n_rows, -1)).astype(np.int32)


# ---- 1. the C entry on synthetic blocks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_means_equal_the_reference(dev, layout):
    seen_sizes, informative = set(), 0
    for i, (n_rows, n_cols) in enumerate(SHAPES):
        rng = np.random.default_rng([i, layout, 5])
        cases, ranks = {}, labellings(n_cols, rng)
        for name, gidx in ranks.items():
            col_pos, ptr = lists_of(gidx, rng, shuffle=name != "two")        # ("two": one labelling with ascending lists)
            cases[name] = rows_of(n_rows, n_cols, gidx) + (col_pos, ptr)
            seen_sizes.update(np.diff(ptr).tolist())
        most = "five" if "five" in ranks else "one"
        cases["nothing-excluded"] = rows_of(n_rows, n_cols, ranks[most], exclude=False) + cases[most][2:]
        refs = {}
        for tag, stride, base in B.variants(layout, n_rows, n_cols):
            blk = B.make_block(layout, n_rows, n_cols, stride, 80 + i, kind="dyadic")
            A = blk.A
            S = dev.put(blk.raw, base)
            for name, case in cases.items():
                if name not in refs:                                         # (A does not depend on the stride: one reference)
                    refs[name] = GR.block_means(A, *case)
                    near = refs[name][2]
                    informative += int(np.unique(near[near != -2]).size > 1)
                what = (layout, n_rows, n_cols, tag, name)
                first = check_call(dev, S, layout, stride, A, case, refs[name], what)
                again = run_means(dev, S, layout, stride, n_rows, n_cols, *case, None)
                for a, b in zip(first[:3], again[:3]):
                    assert np.array_equal(B.bits(a), B.bits(b)), what        # a second run: the same bits
            dev.release()
    assert {1, 8, 9, 64, 65, 256, 257, 1023, 1024, 1025, 1029} <= seen_sizes
    assert informative >= 10                                                 # `nearest` is not one group everywhere


def planted(layout, n_rows, n_cols, plant, seed=3):
    """A dyadic block with the values of ``plant`` {(r, c): value} written over it: (A, stride, the stored bytes)."""
    _, stride, base = B.variants(layout, n_rows, n_cols)[0]
    blk = B.make_block(layout, n_rows, n_cols, stride, seed, kind="dyadic")
    A, stored = blk.A.copy(), blk.stored.copy()
    at = B.offsets(layout, n_rows, n_cols, stride)
    for (r, c), v in plant.items():
        A[r, c] = v
        stored[at[r, c]] = v if np.isnan(v) else B.store(layout, v)
    assert np.array_equal(B.bits(B.decode(layout, stored, n_rows, n_cols, stride)), B.bits(A))
    return A, stride, base, stored.tobytes()


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_nan_and_negative_zero_entries(dev, layout):
    """A NaN entry makes its (row, group) mean NaN and that group is never nearest, in another cluster and in the row's
    own; a -0.0 counts as zero: a group of -0.0 entries has the mean +0.0."""
    n_rows, n_cols = 9, 150
    rng = np.random.default_rng(layout)
    gidx = np.arange(n_cols) % 4                                             # four clusters of 37 or 38: a wave sums each
    gidx[140:] = 4 + np.arange(10) % 2                                       # and two of five: a lane does
    row_group, row_col = rows_of(n_rows, n_cols, gidx)
    col_pos, ptr = lists_of(gidx, rng)
    r1, r2, r3 = 0, 1, 2                                                     # rows of the nodes 1 (cluster 1), 6 (2), 11 (3)
    plant = {(r1, 4): np.nan, (r1, 141): np.nan,                             # row 0: clusters 0 and 5 are NaN
             (r2, 10): np.nan,                                               # row 1: its own cluster 2 is NaN
             (r3, 22): -0.0}
    for c in np.flatnonzero(gidx == 4):
        plant[(r3, int(c))] = -0.0                                           # row 2: cluster 4 is all -0.0
    A, stride, base, raw = planted(layout, n_rows, n_cols, plant)
    S = dev.put(raw, base)
    ref = GR.block_means(A, row_group, row_col, col_pos, ptr)
    own, other, near, table, _ = ref
    assert np.isnan(table[r1, [0, 5]]).all() and near[r1] not in (0, 5) and not np.isnan(other[r1])
    assert np.isnan(own[r2]) and not np.isnan(other[r2])
    assert table[r3, 4] == 0.0 and not np.signbit(table[r3, 4])
    check_call(dev, S, layout, stride, A, (row_group, row_col, col_pos, ptr), ref, ("nan", layout))
    # NaN in every other cluster: no candidate, nearest = -1 and other = NaN
    gidx2 = (np.arange(n_cols) >= 100).astype(np.int64)
    row_group2, row_col2 = rows_of(n_rows, n_cols, gidx2)
    A2, stride, base, raw = planted(layout, n_rows, n_cols, {(0, 120): np.nan})
    col_pos2, ptr2 = lists_of(gidx2, rng)
    ref2 = GR.block_means(A2, row_group2, row_col2, col_pos2, ptr2)
    assert ref2[2][0] == -1 and np.isnan(ref2[1][0]) and row_group2[0] == 0
    check_call(dev, dev.put(raw, base), layout, stride, A2, (row_group2, row_col2, col_pos2, ptr2), ref2, ("no candidate", layout))


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_equal_means_go_to_the_smaller_group(dev, layout):
    """Groups 1, 3 and 4 hold copies of the same values in every row, above everything else: all three means are equal and
    the best; the smallest group number that is not the row's own is reported, whichever way each is summed (group 3's
    list is reversed; with 12 members the wave sums them, with 6 a lane does)."""
    for m in (12, 6):
        n_rows, n_cols = 20, 5 * m + 7
        rng = np.random.default_rng([layout, m])
        A = rng.integers(-200, 200, size=(n_rows, n_cols)) * 2.0 ** -8
        top = 2.0 + rng.integers(0, 64, size=(n_rows, m)) * 2.0 ** -8
        if layout == B.PANEL_F16:
            A, top = A / 4, top / 4                                          # (binary16: multiples of 2^-10 below 2)
        gidx = np.minimum(np.arange(n_cols) // m, 5)
        for g in (1, 3, 4):
            A[:, g * m:(g + 1) * m] = top
        col_pos, ptr = lists_of(gidx, rng, shuffle=False)
        col_pos[ptr[3]:ptr[4]] = col_pos[ptr[3]:ptr[4]][::-1].copy()
        # the rows' own nodes: columns of the groups 0, 1 and 3 in turn.  A row of group 1 or 3 has one member fewer
        # there, so its own mean is no copy: the tie is among the others
        col = np.array([(0, m + 2, 3 * m + 1)[r % 3] for r in range(n_rows)])
        row_group, row_col = gidx[col].astype(np.int32), col.astype(np.int32)
        _, stride, base = B.variants(layout, n_rows, n_cols)[0]
        S = dev.put(B.encode(layout, A, stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
        ref = GR.block_means(A, row_group, row_col, col_pos, ptr)
        assert ref[2].tolist() == [(1, 3, 1)[r % 3] for r in range(n_rows)]
        assert all(ref[3][r, 1] == ref[3][r, 3] == ref[3][r, 4] == ref[1][r] for r in range(0, n_rows, 3))
        check_call(dev, S, layout, stride, A, (row_group, row_col, col_pos, ptr), ref, ("tie", layout, m))
        dev.release()


# ---- 2. through the estimators ------------------------------------------------------------------------------------------------
def near_enough(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    assert np.all(err <= tol[ok]), (what, float(err.max()), float(tol[ok][np.argmax(err - tol[ok])]))


def check_labelling(model, kw, S, index, lab, exact, what):
    """The four methods on the labelling ``lab`` (int64 in the frame's order) against ``groups_ref`` on the frame ``S``."""
    n = len(lab)
    cl = GR.clusters_of(lab)
    rank = np.searchsorted(cl, lab)
    table, tol = GR.means(S, lab), GR.bound(S, lab)
    own, near, other = GR.quality(S, lab, table)
    q = model.cluster_quality(lab, **kw)
    assert q.index.equals(index) and q.columns.tolist() == ["cluster", "own", "nearest", "other", "silhouette"], what
    assert q.dtypes.tolist() == [np.int64, np.float64, np.int64, np.float64, np.float64], what
    assert q["cluster"].tolist() == lab.tolist(), what
    got_near = q["nearest"].to_numpy()
    m = model.cluster_means(lab, **kw)
    assert m.index.equals(index) and m.columns.tolist() == cl and m.to_numpy().dtype == np.float64, what
    if exact:
        same_bits(q["own"].to_numpy(), own, (what, "own"))
        same_bits(q["other"].to_numpy(), other, (what, "other"))
        assert np.array_equal(got_near, near), what
        same_bits(m.to_numpy(), table, (what, "means"))
    else:
        near_enough(q["own"], own, tol[np.arange(n), rank], (what, "own"))
        near_enough(m.to_numpy(), table, tol, (what, "means"))
        # nearest: a cluster whose reference mean lies within twice its tolerance of the reference best; other: that
        # cluster's reference mean within the bound
        none = np.isnan(other)
        assert np.array_equal(got_near[none], lab[none]) and np.isnan(q["other"].to_numpy()[none]).all(), what
        at = np.searchsorted(cl, got_near)
        assert np.array_equal(np.asarray(cl)[at], got_near) and (got_near[~none] != lab[~none]).all(), what
        picked, picked_tol = table[np.arange(n), at], tol[np.arange(n), at]
        assert np.all(picked[~none] >= other[~none] - 2 * picked_tol[~none]), what
        near_enough(q["other"].to_numpy()[~none], picked[~none], picked_tol[~none], (what, "other"))
    # the host arithmetic, on the numbers the call returned
    g_own, g_other = q["own"].to_numpy(), q["other"].to_numpy()
    sil = GR.silhouettes(lab, g_own, g_other)
    same_bits(q["silhouette"].to_numpy(), sil, (what, "silhouette"))
    med = model.medoids(lab, **kw)
    want_med = GR.medoids(lab, g_own)
    assert med.name == "medoid" and med.index.tolist() == cl and med.tolist() == [index[want_med[g]] for g in cl], what
    s = model.cluster_summary(lab, **kw)
    want = GR.summary(lab, g_own, g_other, sil)
    assert s.index.tolist() == cl and s.columns.tolist() == ["size", "medoid", "cohesion", "separation", "silhouette"], what
    assert s["size"].tolist() == [want[g][0] for g in cl] and s["medoid"].tolist() == med.tolist(), what
    for k, col in enumerate(["cohesion", "separation", "silhouette"]):
        same_bits(s[col].to_numpy(), np.array([want[g][k + 1] for g in cl]), (what, col))
    # the Series form, in another order, is the array form
    shuffled = pd.Series(lab, index=index).sample(frac=1.0, random_state=1)
    assert model.cluster_quality(shuffled, **kw).equals(q), what
    return q


def labellings_of(model, kw, S, pruned, rng):
    """name -> int64 labels in the frame's order: from cut(linkage()), from components(t), and a random labelling with
    negative values and gaps."""
    n = len(S)
    pos = np.unique(S[~np.eye(n, dtype=bool)])
    pos = pos[pos > 0]
    comp = model.components([float(pos[int(f * pos.size)]) for f in (0.9, 0.5, 0.99, 0.999)])
    comp = comp[kw["group"] - 1] if isinstance(comp, tuple) else comp
    said = [c for c in comp.columns if 1 < comp[c].nunique() < n]            # the first threshold that says something
    out = {"components": comp[said[0]].to_numpy(), "random": rng.choice([-7, 3, 1000, 2 ** 40, -2 ** 35], size=n)}
    Z = model.linkage(min_similarity=float(pos[0]) if pruned else None)
    Z = Z[kw["group"] - 1] if isinstance(Z, tuple) else Z
    k = max(12, n - len(Z))
    out["cut"] = model.cut(Z, n_clusters=k, **kw).to_numpy()
    return out


def check_model(model, exact=False, pruned=False):
    frames = as_groups(model.frame())
    groups = [{"group": 1}, {"group": 2}] if len(frames) == 2 else [{}]
    before = [f.to_numpy().copy() for f in frames]
    informative = 0
    for f, kw in zip(frames, groups):
        S = f.to_numpy()
        rng = np.random.default_rng(len(S))
        for name, lab in labellings_of(model, kw, S, pruned, rng).items():
            q = check_labelling(model, kw, S, f.index, np.asarray(lab, dtype=np.int64), exact, (name, kw))
            informative += int(q["nearest"].nunique() > 1 and q["own"].notna().any())
    assert informative >= len(frames)
    for f, b in zip(as_groups(model.frame()), before):
        assert np.array_equal(B.bits(f.to_numpy()), B.bits(b))                # the model is unchanged
    lab = np.zeros(len(frames[0]), dtype=np.int64)
    model.release()
    for call in (model.cluster_quality, model.cluster_means, model.medoids, model.cluster_summary):
        with pytest.raises(RuntimeError, match="released"):
            call(lab, **groups[0])


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


def test_simrank_on_a_power_law_graph(powerlaw, tmp_path):
    model = make_model("SimRank", powerlaw, "f32-kept", tmp_path)
    try:
        check_model(model)
    finally:
        model.release()


@pytest.mark.parametrize("variant", ["f32-kept", "f64-kept", "world3-kept", "f32-compact-fp16"])
def test_bipartite_simrankpp(variant, tmp_path):
    df = bipartite_random(90, 50, 0.06, 12)
    model = make_model("BipartiteSimRankPP", df, variant, tmp_path, strict_reference=False)
    try:
        check_model(model)
    finally:
        model.release()


def test_a_pruned_model_scores_its_matrix_p(powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, "f32-kept", tmp_path)
    try:
        model.prune(10)
        assert model.kept_neighbors == 10
        check_model(model, pruned=True)
    finally:
        model.release()


@pytest.mark.parametrize("variant", ["f32-kept", "f64-kept", "world3-kept", "f32-compact"])
def test_a_fit_with_dyadic_iterates_is_scored_bit_for_bit(variant, tmp_path):
    """regular_graph(256, 4) with C = 0.5: for as many updates as ``exact_updates`` allows the iterate lies on a dyadic
    grid, every float64 sum of its elements is exact in any order, and so is every number of the four methods."""
    from oracle import simrank_oracle as O
    df = X.regular_graph(256, 4, seed=260)
    _, G = O.directed_graph(df)
    updates = X.exact_updates(G, 0.5, None, mantissa=24, limit=8).updates
    assert updates >= 2
    import contextlib
    import io
    from simrank_amd.driver import LocalWorld
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
        check_model(est, exact=True)
    finally:
        est.release()
