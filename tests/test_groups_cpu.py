"""libsimrank_groups.so (include/simrank_groups.h) and ``cluster_quality`` & co on a machine without a GPU: header, binding
and exports agree, the header is plain C99 and stands alone, the entry refuses bad arguments without a device, the
labels are judged before any device work, the host path of a pruned model equals ``groups_ref`` on hand-made tables, the
reference itself equals exact rational arithmetic, and the silhouette's corners are what the contract says."""
import math
import re
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _groups, _lib, _neighbors, _query
from tests import cluster_ref as CR
from tests import companion_abi as A
from tests import groups_ref as GR
from tests.test_cluster_cpu import HostOps, _FullSpec, boom, guarded_estimator


def same(a, b):
    """Equal bits, or NaN in both."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_groups) == _groups.VERSION == 1
    text = A.header(_groups)
    assert re.search(r"#define SIMRANK_GROUPS_LANE_MAX %d\b" % _groups.LANE_MAX, text)
    assert re.search(r"#define SIMRANK_GROUPS_WAVE_MAX %d\b" % _groups.WAVE_MAX, text)
    assert sorted(_groups.PROTOTYPES) == ["simrank_groups_last_error", "simrank_groups_means", "simrank_groups_version"]
    A.assert_header_stands_alone(_groups)


def test_the_layout_codes_are_the_shared_ones():
    assert A.layout_codes(_groups) == A.layout_codes(_query) and len(A.layout_codes(_groups)) == 4


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_groups)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_groups)


def test_the_main_library_is_unchanged():
    version, names, exports = A.main_library(_groups)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_the_entry_refuses_bad_arguments_without_a_device(tmp_path):
    assert "groups 1 ok" in A.run_c99(_groups, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_groups.h"
#define BAD(call, code) do { if ((call) != SIMRANK_GROUPS_ERR_INVALID) return code; \
                             if (!strlen(simrank_groups_last_error())) return 100 + code; } while (0)
int main(void) {
    /* aligned stand-ins for device memory: nothing below may reach a device */
    static double mem[8];
    static int64_t ptr[3];
    static int32_t ids[8];
    const void* S = mem;
    double* d = mem;
    const int32_t f32 = SIMRANK_GROUPS_ROWMAJOR_F32;
    const int64_t huge = (int64_t)1 << 31;
    if (simrank_groups_version() != SIMRANK_GROUPS_VERSION) return 1;
    /* NULL pointers, one at a time */
    BAD(simrank_groups_means(NULL, f32, 4, 4, 4, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 2);
    BAD(simrank_groups_means(S, f32, 4, 4, 4, NULL, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 3);
    BAD(simrank_groups_means(S, f32, 4, 4, 4, ids, NULL, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 4);
    BAD(simrank_groups_means(S, f32, 4, 4, 4, ids, ids, NULL, ptr, 2, d, d, ids, NULL, 0, NULL), 5);
    BAD(simrank_groups_means(S, f32, 4, 4, 4, ids, ids, ids, NULL, 2, d, d, ids, NULL, 0, NULL), 6);
    BAD(simrank_groups_means(S, f32, 4, 4, 4, ids, ids, ids, ptr, 2, NULL, d, ids, NULL, 0, NULL), 7);
    BAD(simrank_groups_means(S, f32, 4, 4, 4, ids, ids, ids, ptr, 2, d, NULL, ids, NULL, 0, NULL), 8);
    BAD(simrank_groups_means(S, f32, 4, 4, 4, ids, ids, ids, ptr, 2, d, d, NULL, NULL, 0, NULL), 9);
    /* an unknown layout */
    BAD(simrank_groups_means(S, 4, 4, 4, 4, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 10);
    BAD(simrank_groups_means(S, -1, 4, 4, 4, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 11);
    /* a stride too small: columns of a row-major block, rows of a panel block */
    BAD(simrank_groups_means(S, f32, 3, 4, 4, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 12);
    BAD(simrank_groups_means(S, SIMRANK_GROUPS_ROWMAJOR_F64, 3, 4, 4, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 13);
    BAD(simrank_groups_means(S, SIMRANK_GROUPS_PANEL_F32, 3, 4, 2, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 14);
    BAD(simrank_groups_means(S, SIMRANK_GROUPS_PANEL_F16, 3, 4, 2, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 15);
    /* a negative shape, a shape of 2^31 */
    BAD(simrank_groups_means(S, f32, 4, -1, 4, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 16);
    BAD(simrank_groups_means(S, f32, 4, 4, -1, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 17);
    BAD(simrank_groups_means(S, f32, huge, 4, huge, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 18);
    BAD(simrank_groups_means(S, SIMRANK_GROUPS_PANEL_F32, huge, huge, 4, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 19);
    /* no groups */
    BAD(simrank_groups_means(S, f32, 4, 4, 4, ids, ids, ids, ptr, 0, d, d, ids, NULL, 0, NULL), 20);
    BAD(simrank_groups_means(S, f32, 4, 4, 4, ids, ids, ids, ptr, -3, d, d, ids, NULL, 0, NULL), 21);
    /* means with a leading dimension below the groups */
    BAD(simrank_groups_means(S, f32, 4, 4, 4, ids, ids, ids, ptr, 2, d, d, ids, d, 1, NULL), 22);
    if (!strstr(simrank_groups_last_error(), "ld_means")) return 23;
    /* a block that does not start on its element's size */
    BAD(simrank_groups_means((const char*)S + 2, f32, 4, 4, 4, ids, ids, ids, ptr, 2, d, d, ids, NULL, 0, NULL), 24);
    /* no rows: nothing to queue */
    if (simrank_groups_means(NULL, f32, 4, 0, 4, NULL, NULL, ids, ptr, 2, NULL, NULL, NULL, NULL, 0, NULL) != SIMRANK_GROUPS_OK)
        return 25;
    printf("groups %d ok\n", simrank_groups_version());
    return 0;
}
''')


# ---- the labels: judged before any device work ------------------------------------------------------------------------------
INDEX = pd.Index(["a", "b", "c"])
BAD_LABELS = [
    [0, 1], [0, 1, 2, 3], np.array([0, 1]), np.zeros((3, 1), dtype=np.int64),             # the wrong length or shape
    [0.0, 1.0, 2.0], np.array([0.5, 1, 2]), [0, 1, float("nan")], np.array([0, 1, np.nan]),  # floats and NaN
    [True, False, True], np.array([True, False, True]), [0, 1, np.True_],                 # bools
    [0, 1, None], ["x", "y", "z"], [0, 1, 2.0], None, "abc", {"a": 0, "b": 1, "c": 2}, 7, [0, 1, 2 ** 70],
    pd.Series([0, 1], index=["a", "b"]),                                                  # a Series that misses a node
    pd.Series([0, 1, 2], index=["a", "b", "b"]),                                          # ... repeats one
    pd.Series([0, 1, 2, 0], index=["a", "b", "c", "a"]),
    pd.Series([0.0, 1.0, 2.0], index=["a", "b", "c"]),                                    # ... holds floats
    pd.Series([0, 1, None], index=["a", "b", "c"]),                                       # ... or NaN
    pd.Series([True, False, True], index=["a", "b", "c"]),
    pd.DataFrame({"x": [0, 1, 2]}, index=["a", "b", "c"]),
]


def test_what_the_label_check_refuses():
    for bad in BAD_LABELS:
        with pytest.raises(ValueError):
            _groups.check_labels(bad, INDEX)
    for unknown in (pd.Series([0, 1, 2], index=["a", "b", "z"]), pd.Series([0, 1, 2, 3], index=["a", "b", "c", "z"])):
        with pytest.raises(KeyError, match="z"):
            _groups.check_labels(unknown, INDEX)


def test_what_the_label_check_accepts():
    for good in ([5, -3, 5], (5, -3, 5), np.array([5, -3, 5]), np.array([5, -3, 5], dtype=np.int8), [np.int64(5), -3, 5],
                 pd.Series([5, 5, -3], index=["a", "c", "b"]), pd.Series([-3, 5, 5], index=["b", "a", "c"]),
                 pd.Series([5, -3, 5], index=["a", "b", "c"], dtype=object), pd.Index([5, -3, 5])):
        got = _groups.check_labels(good, INDEX)
        assert got.dtype == np.int64 and got.tolist() == [5, -3, 5], good
    assert _groups.check_labels(np.array([1, 2 ** 40, 0], dtype=np.uint64), INDEX).tolist() == [1, 2 ** 40, 0]
    clusters, gidx, sizes = _groups.groups_of(np.array([5, -3, 5, 9], dtype=np.int64))
    assert clusters.tolist() == [-3, 5, 9] and gidx.tolist() == [1, 0, 1, 2] and sizes.tolist() == [1, 2, 1]


def test_argument_checks_need_no_device(monkeypatch):
    monkeypatch.setattr(_groups, "scores", boom)
    monkeypatch.setattr(_groups, "load", boom)
    calls = lambda est, lab, **kw: [lambda: est.cluster_quality(lab, **kw), lambda: est.cluster_means(lab, **kw),
                                    lambda: est.medoids(lab, **kw), lambda: est.cluster_summary(lab, **kw)]
    for call in calls(SRA.SimRank(), [0, 1, 2]):
        with pytest.raises(RuntimeError, match="no kept model"):
            call()
    est = guarded_estimator()
    for bad in BAD_LABELS:
        for call in calls(est, bad):
            with pytest.raises(ValueError):
                call()
    for call in calls(est, pd.Series([0, 1, 2], index=["a", "b", "z"])):
        with pytest.raises(KeyError, match="z"):
            call()
    for call in calls(est, [0, 1, 2], group=2):
        with pytest.raises(ValueError, match="group"):
            call()
    # N * K * 8 = 72 bytes: refused below, and before the labels reach a device
    with pytest.raises(ValueError, match="max_bytes"):
        est.cluster_means([0, 1, 2], max_bytes=71)
    for bad in (0, -1, True, 1.5, None, "1"):
        with pytest.raises(ValueError, match="max_bytes"):
            est.cluster_means([0, 1, 2], max_bytes=bad)
    est.release()
    for call in calls(est, [0, 1, 2]):
        with pytest.raises(RuntimeError, match="released"):
            call()


# ---- the reference against exact arithmetic ---------------------------------------------------------------------------------
def six_nodes():
    """Six nodes, not symmetric, values that are no dyadic fractions: clusters 7 = {0, 2, 5}, -1 = {1, 4}, 3 = {3}."""
    S = np.array([[1.0, 0.1, 0.2, 0.3, 0.7, 0.4],
                  [0.6, 1.0, 0.1, 0.1, 0.3, 0.2],
                  [0.3, 0.3, 1.0, 0.3, 0.3, 0.1],
                  [0.0, -0.0, 0.0, 1.0, 0.0, 0.0],
                  [0.9, 0.1, 0.2, 0.25, 1.0, 0.35],
                  [0.7, 0.0, 0.1, 0.05, 0.05, 1.0]])
    return S, np.array([7, -1, 7, 3, -1, 7])


def test_the_reference_is_exact_rational_arithmetic():
    S, lab = six_nodes()
    cl = GR.clusters_of(lab)
    assert cl == [-1, 3, 7]
    table = GR.means(S, lab)
    for a in range(6):
        for k, g in enumerate(cl):
            m = [b for b in range(6) if lab[b] == g and b != a]
            if not m:
                assert math.isnan(table[a, k]) and (a, g) == (3, 3)
                continue
            exact = sum(Fraction(float(S[a, b])) for b in m)
            assert table[a, k] == float(exact) / len(m), (a, g)            # the exact sum rounded once, then one division
            assert abs(Fraction(float(table[a, k])) - exact / len(m)) <= Fraction(GR.bound(S, lab)[a, k])
    own, nearest, other = GR.quality(S, lab)
    # node 0: its own cluster 7 without itself = {2, 5}: (0.2 + 0.4) / 2; cluster -1: (0.1 + 0.7) / 2 beats 3: 0.3
    assert own[0] == float(Fraction(0.2) + Fraction(0.4)) / 2 and nearest[0] == -1 and other[0] == float(Fraction(0.1) + Fraction(0.7)) / 2
    # node 2: every other mean is 0.3: (0.3 + 0.3) / 2 == 0.3 exactly, and the smaller cluster value wins the tie
    assert table[2, 0] == table[2, 1] == 0.3 and nearest[2] == -1 and other[2] == 0.3
    # node 3 is a singleton: own NaN, its row is all zeros (one of them -0.0): the tie at +0.0 goes to -1
    assert math.isnan(own[3]) and nearest[3] == -1 and other[3] == 0.0 and not np.signbit(other[3])
    sil = GR.silhouettes(lab, own, other)
    assert sil[3] == 0.0 and sil[0] == (own[0] - other[0]) / other[0] and sil[0] < 0
    assert GR.medoids(lab, own) == {-1: 1 if own[1] >= own[4] else 4, 3: 3, 7: int(np.argmax(np.where(lab == 7, own, -1)))}
    size, cohesion, separation, mean_sil = GR.summary(lab, own, other, sil)[7]
    assert size == 3 and cohesion == math.fsum(own[[0, 2, 5]]) / 3 and mean_sil == math.fsum(sil[[0, 2, 5]]) / 3
    assert math.isnan(GR.summary(lab, own, other, sil)[3][1])             # NaN propagates: a singleton has no cohesion
    # the vectorised twin agrees within the bound, and exactly on who is nearest
    own2, near2, other2 = GR.quality_fast(S, lab)
    B = GR.bound(S, lab)
    assert np.array_equal(near2, nearest)
    assert np.all((np.abs(own2 - own) <= B.max()) | (np.isnan(own) & np.isnan(own2))) and np.all(np.abs(other2 - other) <= B.max())


def test_a_nan_entry_and_one_cluster():
    S, lab = six_nodes()
    S[0, 4] = np.nan                                                       # node 0 to cluster -1: NaN, never nearest
    own, nearest, other = GR.quality(S, lab)
    assert math.isnan(GR.means(S, lab)[0, 0]) and nearest[0] == 3 and other[0] == 0.3
    S[0, 3] = np.nan                                                       # ... and to cluster 3: no candidate is left
    own, nearest, other = GR.quality(S, lab)
    assert nearest[0] == 7 and math.isnan(other[0]) and not math.isnan(own[0])
    assert math.isnan(GR.silhouettes(lab, own, other)[0])
    S[2, 5] = np.nan                                                       # in the node's own cluster: own is NaN
    own, nearest, other = GR.quality(S, lab)
    assert math.isnan(own[2]) and nearest[2] == -1 and GR.medoids(lab, own)[7] in (0, 5)
    one = np.zeros(6, dtype=np.int64)                                      # K = 1: nobody has another cluster
    own, nearest, other = GR.quality(S, one)
    assert np.isnan(other).all() and (nearest == 0).all() and np.isnan(GR.silhouettes(one, own, other)).all()


def test_silhouette_corners():
    nan = float("nan")
    cases = [  # own, other, the size of the node's cluster -> silhouette
        (nan, 0.5, 1, 0.0), (0.3, 0.1, 1, 0.0),                            # a singleton comes first, whatever own is
        (0.4, nan, 6, nan),                                                # K = 1: no other cluster
        (0.0, 0.0, 3, 0.0), (-0.0, 0.0, 3, 0.0), (-0.5, -0.25, 2, 0.0),    # no positive mean
        (nan, 0.5, 3, nan), (0.5, nan, 3, nan), (nan, nan, 3, nan),
        (0.5, 0.25, 2, 0.5), (0.25, 0.5, 2, -0.5), (0.5, 0.0, 2, 1.0), (0.0, 0.5, 2, -1.0), (0.5, 0.5, 2, 0.0),
        (0.5, -0.25, 2, 1.5),
    ]
    own, other, size, want = (np.array(x) for x in zip(*cases))
    got = _groups.silhouette(own, other, size)
    assert same(got, want)
    for o, t, s, w in cases:
        assert same(GR.silhouette(o, t, s == 1), w)
    # medoids: the largest own, the first of a tie, NaN skipped, all NaN -> the first member
    gidx = np.array([0, 1, 0, 1, 2, 0, 1, 3, 3])
    own = np.array([0.5, nan, 0.75, 0.25, nan, 0.75, 0.25, nan, nan])
    assert _groups.medoid_positions(gidx, 4, own).tolist() == [2, 3, 4, 7]
    assert GR.medoids(gidx, own) == {0: 2, 1: 3, 2: 4, 3: 7}
    cohesion, separation, sil = _groups.summary(gidx, 4, own, own * 0.5, np.nan_to_num(own))
    assert cohesion[0] == math.fsum([0.5, 0.75, 0.75]) / 3 and math.isnan(cohesion[1]) and sil[1] == 0.5 / 3


# ---- the pruned host path ------------------------------------------------------------------------------------------------------
def table_cases():
    """[(ids, vals, labels)]: hand-made lists.  First: 7 nodes, 2 slots, clusters {0, 1, 2, 3} / {4, 5} / {6}: node 0
    keeps 1 and 4 but not 2 and 3 of its own cluster (absent entries in the node's own cluster; k smaller than the
    cluster), nobody keeps 6 and 6 keeps only 0 (a cluster with no kept entry at all, for everyone), node 3 keeps nothing,
    node 5 keeps only negative values (an absent cluster's +0.0 beats them).  Second: ``test_cluster_cpu.lists_case``
    with a NaN and a -0.0 kept, under three labellings."""
    ids = np.array([[1, 4], [0, 2], [1, 5], [-1, -1], [5, 0], [4, 2], [0, -1]], dtype=np.int32)
    vals = np.array([[0.5, 0.25], [0.75, 0.125], [0.5, 0.375], [0, 0], [0.875, 0.0625], [-0.5, -0.25], [0.3, 0]])
    out = [(ids, vals, np.array([0, 0, 0, 0, 10, 10, -4])), (ids, vals, np.zeros(7, dtype=np.int64)),
           (ids, vals, np.arange(7)[::-1].copy())]
    from tests.test_cluster_cpu import lists_case
    ids2, vals2 = lists_case()
    out += [(ids2, vals2, np.array(l)) for l in ([1, 1, 2, 1, 2, 3], [0, 1, 0, 1, 0, 1], [5, 5, 5, 5, 5, -5])]
    return out


def test_the_host_path_of_pruned_lists_equals_the_reference():
    for ids, vals, lab in table_cases():
        P = CR.matrix_of_lists(ids, vals)
        clusters, gidx, sizes = _groups.groups_of(lab)
        want_means = GR.means(P, lab)
        want_own, want_near, want_other = GR.quality(P, lab, want_means)
        bound = GR.bound(P, lab)
        for with_means in (False, True):
            own, other, nearest, means = _groups.scores_of_lists(ids, vals, gidx, sizes, with_means)
            near = np.where(nearest >= 0, clusters[np.maximum(nearest, 0)], lab)
            assert np.array_equal(near, want_near), (lab, near, want_near)
            pick = lambda of: bound[np.arange(len(lab)), np.searchsorted(clusters, of)]       # the bound of (a, of[a])
            for got, want, tol in ((own, want_own, pick(lab)), (other, want_other, pick(near))):
                assert np.array_equal(np.isnan(got), np.isnan(want)), (lab, got, want)
                ok = ~np.isnan(want)
                assert np.all(np.abs(got[ok] - want[ok]) <= tol[ok]), (lab, got, want)
            if with_means:
                assert np.array_equal(np.isnan(means), np.isnan(want_means))
                ok = ~np.isnan(want_means)
                assert np.all(np.abs(means[ok] - want_means[ok]) <= bound[ok])
            else:
                assert means is None
    # the first table by hand: node 0 (cluster 0 of four): own = 0.5 / 3; cluster 10: 0.25 / 2; cluster -4: absent, +0.0
    ids, vals, lab = table_cases()[0]
    clusters, gidx, sizes = _groups.groups_of(lab)
    own, other, nearest, means = _groups.scores_of_lists(ids, vals, gidx, sizes, True)
    assert clusters.tolist() == [-4, 0, 10] and own[0] == 0.5 / 3 and other[0] == 0.125 and nearest[0] == 2
    assert means[0].tolist() == [0.0, 0.5 / 3, 0.125]
    assert own[3] == 0.0 and other[3] == 0.0 and nearest[3] == 0         # node 3 keeps nothing: zeros, the tie to -4
    assert other[5] == 0.0 and nearest[5] == 0 and own[5] == -0.5         # 0.0 of the absent cluster beats -0.125
    assert math.isnan(own[6]) and other[6] == 0.3 / 4 and nearest[6] == 1


def test_the_four_methods_on_a_pruned_model(monkeypatch):
    monkeypatch.setattr(_groups, "load", boom)                # (a pruned model needs no library)
    ops = HostOps()
    ids, vals, lab = table_cases()[0]
    names = list("abcdefg")
    solver = _neighbors.NeighborSolver(ops, [_FullSpec(7)], [_neighbors.Tables.from_host(ops, ids, vals, np.ones(7))])
    est = SRA.SimRank()._keep(solver, [(0, names)])
    P = CR.matrix_of_lists(ids, vals)
    want_means = GR.means(P, lab)
    own, near, other = GR.quality(P, lab, want_means)
    sil = GR.silhouettes(lab, own, other)
    q = est.cluster_quality(lab)
    assert q.columns.tolist() == ["cluster", "own", "nearest", "other", "silhouette"] and q.index.tolist() == names
    assert q.dtypes.tolist() == [np.int64, np.float64, np.int64, np.float64, np.float64]
    assert q["cluster"].tolist() == lab.tolist() and q["nearest"].tolist() == near.tolist()
    assert same(q["own"], own) and same(q["other"], other) and same(q["silhouette"], sil)      # (dyadic values: exact)
    shuffled = pd.Series(lab, index=names).iloc[[3, 0, 6, 2, 5, 1, 4]]
    assert est.cluster_quality(shuffled).equals(q)                                           # the Series form, reindexed
    m = est.cluster_means(lab)
    assert m.index.tolist() == names and m.columns.tolist() == [-4, 0, 10] and same(m.to_numpy(), want_means)
    med = est.medoids(lab)
    assert med.name == "medoid" and med.index.tolist() == [-4, 0, 10]
    assert med.tolist() == [names[i] for _, i in sorted(GR.medoids(lab, own).items())]
    s = est.cluster_summary(lab)
    want = GR.summary(lab, own, other, sil)
    assert s.columns.tolist() == ["size", "medoid", "cohesion", "separation", "silhouette"] and s.index.tolist() == [-4, 0, 10]
    assert s["size"].tolist() == [1, 4, 2] and s["medoid"].tolist() == med.tolist()
    for k, col in enumerate(["cohesion", "separation", "silhouette"]):
        assert same(s[col], [want[g][k + 1] for g in (-4, 0, 10)])
    assert est.kept_neighbors == 2                            # the model is as it was
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.cluster_quality(lab)
    assert not ops.live
