"""``_hdbscan`` without a device: the argument checks, the host condensing and selection against ``hdbscan_ref`` on
tie-heavy matrices and on one hand-worked example, the three identities of the contract through the references
(``density_ref``, ``linkage_ref``), the reference's own fast walk against its definition, and the host paths of a pruned
model against the reference on the dense matrix P."""
import math

import numpy as np
import pytest

from simrank_amd import _hdbscan, _linkage
from tests import cluster_ref as CR
from tests import density_ref as DR
from tests import hdbscan_ref as HR
from tests import linkage_ref as LR


def tie_heavy(n, seed, *, nan=0.05, levels=6, negative=True):
    """An asymmetric matrix of few distinct values, with exact zeros of both signs, NaN and (optionally) negatives."""
    rng = np.random.default_rng([seed, n])
    S = rng.integers(-2 if negative else 0, levels, size=(n, n)) / 8.0
    S[rng.random((n, n)) < 0.05] = -0.0
    S[rng.random((n, n)) < nan] = np.nan
    return S


def blobs(n, seed):
    """Three groups of different density on top of a tie-heavy floor: clusters do split."""
    rng = np.random.default_rng([seed, n, 1])
    S = rng.integers(0, 3, size=(n, n)) / 32.0
    group = rng.integers(0, 4, size=n)                       # group 3: scattered nodes
    for g, (lo, hi) in enumerate(((24, 30), (14, 20), (8, 12))):
        at = np.flatnonzero(group == g)
        S[np.ix_(at, at)] = rng.integers(lo, hi, size=(at.size, at.size)) / 32.0
    S[rng.random((n, n)) < 0.03] = np.nan
    return S


CASES = [(tie_heavy(n, s), m) for n, s in ((12, 0), (25, 1), (40, 2)) for m in (1, 2, 3, 5)] + \
        [(tie_heavy(30, 3, nan=0.5), 3), (tie_heavy(30, 4, negative=False, levels=3), 4)] + \
        [(blobs(n, s), m) for n, s in ((40, 0), (60, 1), (60, 2)) for m in (2, 4)]


def same_table(got, want):
    return len(got) == len(want) == 4 and all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))


def same_clusters(got, want):
    assert list(got) == ["parent", "birth", "size", "stability", "selected", "cluster"] == list(want)
    for k in got:
        assert got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k].view(np.uint64) if got[k].dtype == np.float64 else got[k],
                              want[k].view(np.uint64) if want[k].dtype == np.float64 else want[k]), (k, got[k], want[k])


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def test_argument_checks():
    assert _hdbscan.check_min_samples(1) == 0 and _hdbscan.check_min_samples(5) == 4
    assert _hdbscan.check_min_samples(2 ** 40) == 2 ** 31 - 1 and _hdbscan.check_min_samples(np.int64(3)) == 2
    for bad in (0, -1, 2.0, "3", None, True, float("nan")):
        with pytest.raises(ValueError, match="min_samples"):
            _hdbscan.check_min_samples(bad)
    assert _hdbscan.check_hdbscan(5, None, None, "eom") == (5, 4, None)
    assert _hdbscan.check_hdbscan(5, 2, 0.25, "leaf") == (5, 1, 0.25)
    for bad in (1, 0, 2.5, "5", None, True):
        with pytest.raises(ValueError, match="min_cluster_size"):
            _hdbscan.check_hdbscan(bad, None, None, "eom")
    with pytest.raises(ValueError, match="min_samples"):
        _hdbscan.check_hdbscan(5, 0, None, "eom")
    with pytest.raises(ValueError, match="selection"):
        _hdbscan.check_hdbscan(5, None, None, "EOM")
    for bad in (float("nan"), float("inf"), "0.5"):
        with pytest.raises(ValueError, match="min_similarity"):
            _hdbscan.check_hdbscan(5, None, bad, "eom")
    assert [_hdbscan.select_passes(l) for l in range(4)] == [8, 8, 4, 16]


# ---- the reference against its own definition -----------------------------------------------------------------------------------
def shape(x):
    return x if isinstance(x, int) else (tuple(sorted(x.members)), x.height, tuple(shape(c) for c in x.children))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_reference_walk_equals_the_partitions_at_every_height(case):
    S, m = CASES[case]
    M = HR.mutual(S, m)
    assert np.array_equal(M, M.T, equal_nan=True)
    hs = LR.heights(M)
    for floor in (None, float(hs[hs.size // 2]) if hs.size else 0.0):
        assert [shape(x) for x in HR.roots(M, floor)] == [shape(x) for x in HR.roots_by_partitions(M, floor)]


# ---- the host arithmetic against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CASES)))
def test_condense_equals_the_reference(case):
    S, m = CASES[case]
    n = len(S)
    hs = LR.heights(HR.mutual(S, m))
    split = 0
    for floor in (None, float(hs[hs.size // 2]) if hs.size else 0.0):
        table = HR.linkage(S, m, floor)
        for mcs in (2, 3, 5):
            for selection in ("eom", "leaf"):
                for single in (False, True):
                    labels, core, clusters = HR.hdbscan(S, mcs, m, floor, selection, single)
                    got_labels, got = _hdbscan.condense(n, *table, mcs, selection, single)
                    assert got_labels.dtype == np.int64 and np.array_equal(got_labels, labels), (mcs, selection, single)
                    same_clusters(got, clusters)
                    split += clusters["selected"].sum() >= 2
    assert case < 14 or split >= 4                            # the blobs do give several clusters


def test_the_cases_are_not_trivial():
    sizes = [len(HR.hdbscan(S, 3, m)[2]["size"]) for S, m in CASES]
    ties = [LR.stats(len(S), HR.linkage(S, m))[1] for S, m in CASES]
    assert sum(s >= 3 for s in sizes) >= 6 and max(ties) >= 4 and sum(t >= 3 for t in ties) >= 10


def worked_example(bridge):
    """Ten nodes: a tight group {0, 1, 2} at 0.875, a looser one {3, 4, 5, 6} at 0.625, node 7 a bridge that sees node 2
    and node 3 at ``bridge``, node 8 an outlier that sees node 0 at 0.0625, node 9 at 0 to everybody."""
    S = np.zeros((10, 10))
    S[np.ix_([0, 1, 2], [0, 1, 2])] = 0.875
    S[np.ix_([3, 4, 5, 6], [3, 4, 5, 6])] = 0.625
    S[2, 7] = S[7, 3] = bridge                                # one direction each
    S[8, 0] = 0.0625
    return S


def test_a_hand_worked_example():
    """min_samples = 2: a node's core similarity is its largest pair height: 0.875, 0.625, the bridge's, 0.0625 and 0.
    The classes: {0, 1, 2} at 0.875, {3 .. 6} at 0.625, {0 .. 7} at the bridge's height with THREE children, {0 .. 8} at
    0.0625, {0 .. 9} at 0.  With min_cluster_size = 3 the root cluster R is born at 0, loses 9 at 0 and 8 at 0.0625 and
    ends where the two groups part: A and B are born there."""
    S = worked_example(0.25)
    assert HR.core(S, 2).tolist() == [0.875] * 3 + [0.625] * 4 + [0.25, 0.0625, 0.0]
    table = HR.linkage(S, 2)
    assert table[2].tolist() == [0.875] * 2 + [0.625] * 3 + [0.25] * 2 + [0.0625, 0.0]
    for fn in (lambda **kw: HR.hdbscan(S, 3, 2, **kw)[::2], lambda **kw: _hdbscan.condense(10, *table, 3, **kw)):
        labels, clusters = fn(selection="eom", allow_single_cluster=False)
        assert labels.tolist() == [0, 0, 0, 1, 1, 1, 1, -1, -1, -1]
        assert clusters["parent"].tolist() == [-1, 0, 0] and clusters["size"].tolist() == [10, 3, 4]
        assert clusters["birth"].tolist() == [0.0, 0.25, 0.25]
        # R: 9 leaves at 0, 8 at 0.0625, the other eight at 0.25; A: 3 x (0.875 - 0.25); B: 4 x (0.625 - 0.25)
        assert clusters["stability"].tolist() == [0.0625 + 8 * 0.25, 3 * 0.625, 4 * 0.375]
        assert clusters["selected"].tolist() == [False, True, True] and clusters["cluster"].tolist() == [-1, 0, 1]
        # 2.0625 < 1.875 + 1.5: the root loses also when it may be selected
        assert fn(selection="eom", allow_single_cluster=True)[0].tolist() == labels.tolist()
        assert fn(selection="leaf", allow_single_cluster=False)[0].tolist() == labels.tolist()
    # a bridge at 0.5: R = 0.0625 + 8 x 0.5 = 4.0625 beats A + B = 3 x 0.375 + 4 x 0.125, when a root may be selected
    S = worked_example(0.5)
    table = HR.linkage(S, 2)
    for fn in (lambda **kw: HR.hdbscan(S, 3, 2, **kw)[::2], lambda **kw: _hdbscan.condense(10, *table, 3, **kw)):
        labels, clusters = fn(selection="eom", allow_single_cluster=True)
        assert labels.tolist() == [0] * 10 and clusters["stability"].tolist() == [4.0625, 1.125, 0.5]
        assert clusters["selected"].tolist() == [True, False, False] and clusters["cluster"].tolist() == [0, -1, -1]
        assert fn(selection="eom", allow_single_cluster=False)[0].tolist() == [0, 0, 0, 1, 1, 1, 1, -1, -1, -1]
        assert fn(selection="leaf", allow_single_cluster=True)[0].tolist() == [0, 0, 0, 1, 1, 1, 1, -1, -1, -1]
    # min_cluster_size = 4: only the looser group is large enough, the cluster never splits, and alone it is a root
    labels, clusters = _hdbscan.condense(10, *table, 4, "eom", False)
    assert labels.tolist() == [0] * 10 and clusters["size"].tolist() == [10] and clusters["parent"].tolist() == [-1]
    assert _hdbscan.condense(10, *table, 4, "leaf", False)[0].tolist() == [-1] * 10
    # under a floor the tree is a forest: two roots, each a cluster of its own
    table = HR.linkage(S, 2, 0.625)
    labels, clusters = _hdbscan.condense(10, *table, 3, "eom", False)
    assert labels.tolist() == [0, 0, 0, 1, 1, 1, 1, -1, -1, -1] and clusters["parent"].tolist() == [-1, -1]
    assert clusters["stability"].tolist() == [0.0, 0.0] and clusters["birth"].tolist() == [0.875, 0.625]
    same_clusters(clusters, HR.hdbscan(S, 3, 2, 0.625)[2])


def test_stability_is_the_exactly_rounded_sum():
    """Counts times differences that no float64 product or running sum gets right: fsum over every node's own term."""
    terms = [(3, 0.1), (7, 0.7 - 0.1), (11, 1e-17), (5, 0.3)]
    want = math.fsum(d for k, d in terms for _ in range(k))
    assert _hdbscan._exact_sum(terms) == want


# ---- the identities, through the references ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_three_identities(case):
    S, m = CASES[case]
    n = len(S)
    core = HR.core(S, m)
    Zm = HR.linkage(S, m)
    v = np.unique(S[~np.isnan(S)])
    levels = sorted(set(v.tolist()) | {float(v[0]) - 1.0, float(v[-1]) + 1.0, float(v[v.size // 2]) + 1 / 64})
    for t in levels:
        cluster, is_core, deg, _ = DR.dbscan(S, t, m)
        assert np.array_equal(core >= t, is_core) and np.array_equal(is_core, deg + 1 >= m), t          # 1
        cut = LR.cut(n, Zm, t=t)                                                                         # 2
        sizes = np.bincount(cut, minlength=n)
        assert (sizes[cut[~is_core]] == 1).all(), t
        at = np.flatnonzero(is_core)
        assert np.array_equal(cut[at][:, None] == cut[at][None, :], cluster[at][:, None] == cluster[at][None, :]), t
    if m == 1:
        assert same_table(Zm, LR.linkage(S))                                                             # 3
    assert same_table(HR.linkage(S, 1), LR.linkage(S))


# ---- the host paths of a pruned model ----------------------------------------------------------------------------------------
def pruned(S, k):
    """(ids int32 [n, k], vals float64 [n, k]) keeping the k largest off-diagonal entries of each row (-1: an empty slot),
    and the dense P they stand for."""
    n = len(S)
    ids, vals = np.full((n, k), -1, dtype=np.int32), np.zeros((n, k))
    for a in range(n):
        row = np.where(np.arange(n) == a, -np.inf, np.nan_to_num(S[a], nan=-np.inf))
        keep = np.argsort(-row, kind="stable")[:k]
        keep = keep[np.isfinite(row[keep])][:max(0, k - (a % 3 == 0))]          # some lists are not full
        ids[a, :keep.size], vals[a, :keep.size] = keep, S[a, keep]
    return ids, vals, CR.matrix_of_lists(ids, vals)


@pytest.mark.parametrize("seed", range(4))
def test_a_pruned_model_on_the_host(seed):
    S = tie_heavy(30, 10 + seed, negative=seed % 2 == 1) if seed < 2 else blobs(40, seed)
    ids, vals, P = pruned(S, 6)
    if seed == 1:
        vals[3, 0] = vals[5, 1] = np.nan                      # a kept NaN: no entry in that direction
        P = CR.matrix_of_lists(ids, vals)
    n = len(P)
    for m in (1, 2, 3, 5, 8, n, n + 1):
        rank = _hdbscan.check_min_samples(m)
        core = _hdbscan.core_of_lists(ids, vals, rank)
        assert np.array_equal(core.view(np.uint64), HR.core(P, m).view(np.uint64)), m
        pos = np.unique(P[P > 0])
        for floor in (float(pos[0]), float(pos[pos.size // 2])):
            forest = _linkage.forest_of_lists(ids, _hdbscan.clamp_lists(ids, vals, core), floor)
            assert same_table(_linkage.canonical(n, *forest), HR.linkage(P, m, floor)), (m, floor)
