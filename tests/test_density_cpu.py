"""libsimrank_density.so (include/simrank_density.h), ``degrees`` and ``dbscan`` on a machine without a GPU: header,
binding and exports agree, the header is plain C99 and stands alone, every entry point refuses bad arguments without a
device, the argument checks of the two methods run before any device work, the host path of a pruned model equals
``density_ref`` on hand-made tables, and ``density_ref`` itself is pinned on a hand-made matrix, against ``cluster_ref``
and, where it imports, against scikit-learn."""
import re

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _cluster, _density, _lib, _neighbors, _query
from tests import cluster_ref as CR
from tests import companion_abi as A
from tests import density_ref as DR
from tests.test_cluster_cpu import BAD_THRESHOLDS, HostOps, _FullSpec, boom, guarded_estimator, lists_case


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_density) == _density.VERSION == 1
    text = A.header(_density)
    assert re.search(r"#define SIMRANK_DENSITY_MAX_LEVELS %d\b" % _density.MAX_LEVELS, text) and _density.MAX_LEVELS == 8
    assert _density.MAX_LEVELS == _cluster.MAX_LEVELS                  # (``check_thresholds`` is cluster's)
    assert re.search(r"#define SIMRANK_DENSITY_TILE %d\b" % _density.TILE, text) and _density.TILE == 64
    assert re.search(r"#define SIMRANK_DENSITY_NONE 0x%x\b" % _density.NONE, text) and _density.NONE == 2 ** 31 - 1
    assert re.search(r"SIMRANK_DENSITY_BAD_PARENT = %d\b" % _density.BAD_PARENT, text)
    assert re.search(r"SIMRANK_DENSITY_CAP_REACHED = %d\b" % _density.CAP_REACHED, text)
    A.assert_header_stands_alone(_density)


def test_the_layout_codes_are_the_shared_ones():
    assert A.layout_codes(_density) == A.layout_codes(_query) and len(A.layout_codes(_density)) == 4


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_density)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_density)


def test_the_main_library_is_unchanged():
    version, names, exports = A.main_library(_density)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_every_entry_refuses_bad_arguments_without_a_device(tmp_path):
    assert "density 1 ok" in A.run_c99(_density, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_density.h"
#define BAD(call, code) do { if ((call) != SIMRANK_DENSITY_ERR_INVALID) return code; \
                             if (!strlen(simrank_density_last_error())) return 100 + code; } while (0)
int main(void) {
    /* 16-byte aligned stand-ins for device memory: nothing below may reach a device */
    static int32_t mem[16] __attribute__((aligned(16)));
    int32_t* one = mem;
    int32_t* two = mem + 4;
    int32_t* three = mem + 8;
    int32_t* four = mem + 12;
    float e[1] = {0.5f};
    const int32_t f32 = SIMRANK_DENSITY_ROWMAJOR_F32;
    const int32_t big = SIMRANK_DENSITY_MAX_LEVELS + 1;
    const int64_t huge = (int64_t)1 << 31;
    if (simrank_density_version() != SIMRANK_DENSITY_VERSION) return 1;
    /* init: NULL deg, one of parent / attach alone, negative or huge n, levels 0 and 9, NULL status */
    BAD(simrank_density_init(NULL, two, three, 4, 1, one, NULL), 2);
    BAD(simrank_density_init(one, NULL, three, 4, 1, one, NULL), 3);
    BAD(simrank_density_init(one, two, NULL, 4, 1, one, NULL), 4);
    BAD(simrank_density_init(one, two, three, -1, 1, one, NULL), 5);
    BAD(simrank_density_init(one, two, three, huge, 1, one, NULL), 6);
    BAD(simrank_density_init(one, two, three, 4, 0, one, NULL), 7);
    BAD(simrank_density_init(one, two, three, 4, big, one, NULL), 8);
    if (!strstr(simrank_density_last_error(), "8")) return 9;
    BAD(simrank_density_init(one, two, three, 4, 1, NULL, NULL), 10);
    /* degrees: layout, NULL block, stride, negative and huge n, alignment of a panel block, NULL edges / deg, levels */
    BAD(simrank_density_degrees(one, 9, 4, 4, NULL, e, 1, one, NULL), 20);
    BAD(simrank_density_degrees(NULL, f32, 4, 4, NULL, e, 1, one, NULL), 21);
    BAD(simrank_density_degrees(one, f32, 3, 4, NULL, e, 1, one, NULL), 22);
    BAD(simrank_density_degrees(one, SIMRANK_DENSITY_PANEL_F16, 2, 4, NULL, e, 1, one, NULL), 23);
    BAD(simrank_density_degrees(one, f32, 4, -1, NULL, e, 1, one, NULL), 24);
    BAD(simrank_density_degrees(one, f32, huge, huge, NULL, e, 1, one, NULL), 25);
    BAD(simrank_density_degrees(one + 1, SIMRANK_DENSITY_PANEL_F32, 4, 4, NULL, e, 1, one, NULL), 26);
    BAD(simrank_density_degrees(one, f32, 4, 4, NULL, NULL, 1, one, NULL), 27);
    BAD(simrank_density_degrees(one, f32, 4, 4, NULL, e, 1, NULL, NULL), 28);
    BAD(simrank_density_degrees(one, f32, 4, 4, NULL, e, 0, one, NULL), 29);
    BAD(simrank_density_degrees(one, f32, 4, 4, NULL, e, big, one, NULL), 30);
    if (simrank_density_degrees(NULL, f32, 0, 0, NULL, e, 1, NULL, NULL) != SIMRANK_DENSITY_OK) return 31;
    /* union: layout, NULL block, stride, shape, alignment, NULL edge / deg / parent / attach / status, min_neighbors, n */
    BAD(simrank_density_union(one, 9, 4, 4, 4, NULL, NULL, e, one, 1, two, three, 4, four, NULL), 40);
    BAD(simrank_density_union(NULL, f32, 4, 4, 4, NULL, NULL, e, one, 1, two, three, 4, four, NULL), 41);
    BAD(simrank_density_union(one, f32, 3, 4, 4, NULL, NULL, e, one, 1, two, three, 4, four, NULL), 42);
    BAD(simrank_density_union(one, SIMRANK_DENSITY_PANEL_F16, 2, 4, 4, NULL, NULL, e, one, 1, two, three, 4, four, NULL), 43);
    BAD(simrank_density_union(one, f32, 4, -1, 4, NULL, NULL, e, one, 1, two, three, 4, four, NULL), 44);
    BAD(simrank_density_union(one + 1, SIMRANK_DENSITY_PANEL_F32, 4, 4, 4, NULL, NULL, e, one, 1, two, three, 4, four, NULL), 45);
    BAD(simrank_density_union(one, f32, 4, 4, 4, NULL, NULL, NULL, one, 1, two, three, 4, four, NULL), 46);
    BAD(simrank_density_union(one, f32, 4, 4, 4, NULL, NULL, e, NULL, 1, two, three, 4, four, NULL), 47);
    BAD(simrank_density_union(one, f32, 4, 4, 4, NULL, NULL, e, one, 1, NULL, three, 4, four, NULL), 48);
    BAD(simrank_density_union(one, f32, 4, 4, 4, NULL, NULL, e, one, 1, two, NULL, 4, four, NULL), 49);
    BAD(simrank_density_union(one, f32, 4, 4, 4, NULL, NULL, e, one, 1, two, three, 4, NULL, NULL), 50);
    BAD(simrank_density_union(one, f32, 4, 4, 4, NULL, NULL, e, one, -1, two, three, 4, four, NULL), 51);
    BAD(simrank_density_union(one, f32, 4, 4, 4, NULL, NULL, e, one, 1, two, three, -4, four, NULL), 52);
    BAD(simrank_density_union(one, f32, 4, 4, 4, NULL, NULL, e, one, 1, two, three, huge, four, NULL), 53);
    /* an empty block or no nodes: nothing to queue */
    if (simrank_density_union(NULL, f32, 4, 0, 4, NULL, NULL, e, one, 1, two, three, 4, four, NULL) != SIMRANK_DENSITY_OK) return 54;
    if (simrank_density_union(one, f32, 4, 4, 4, NULL, NULL, e, NULL, 1, NULL, NULL, 0, four, NULL) != SIMRANK_DENSITY_OK) return 55;
    /* labels: NULL parent / attach / deg / labels / status, labels one of the other arrays, min_neighbors, n */
    BAD(simrank_density_labels(NULL, two, three, 1, 4, four, one, NULL), 60);
    BAD(simrank_density_labels(one, NULL, three, 1, 4, four, one, NULL), 61);
    BAD(simrank_density_labels(one, two, NULL, 1, 4, four, one, NULL), 62);
    BAD(simrank_density_labels(one, two, three, 1, 4, NULL, one, NULL), 63);
    BAD(simrank_density_labels(one, two, three, 1, 4, four, NULL, NULL), 64);
    BAD(simrank_density_labels(one, two, three, 1, 4, one, four, NULL), 65);
    BAD(simrank_density_labels(one, two, three, 1, 4, two, four, NULL), 66);
    BAD(simrank_density_labels(one, two, three, 1, 4, three, four, NULL), 67);
    BAD(simrank_density_labels(one, two, three, -1, 4, four, one, NULL), 68);
    BAD(simrank_density_labels(one, two, three, 1, -1, four, one, NULL), 69);
    if (simrank_density_labels(NULL, NULL, NULL, 1, 0, NULL, one, NULL) != SIMRANK_DENSITY_OK) return 70;
    printf("density %d ok\n", simrank_density_version());
    return 0;
}
''')


# ---- argument checks: no device --------------------------------------------------------------------------------------
BAD_MIN_SAMPLES = [0, -1, True, False, np.True_, 2.5, 3.0, "3", None, [3], np.float64(2), float("nan")]


def test_argument_checks_need_no_device(monkeypatch):
    for name in ("degrees", "dbscan", "load", "degrees_block", "dbscan_blocks"):
        monkeypatch.setattr(_density, name, boom)
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().degrees(0.5)
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().dbscan(0.5, 3)
    est = guarded_estimator()
    for bad in BAD_THRESHOLDS:
        for model in (est, SRA.SimRank()):                       # (the argument is judged before the model)
            with pytest.raises(ValueError, match="threshold"):
                model.degrees(bad)
            with pytest.raises(ValueError, match="threshold"):
                model.dbscan(bad, 3)
    for bad in ([0.5], [0.5, 0.1], (0.5,), np.array([0.5])):       # dbscan takes one level
        with pytest.raises(ValueError, match="one threshold"):
            est.dbscan(bad, 3)
    for bad in BAD_MIN_SAMPLES:
        for model in (est, SRA.SimRank()):
            with pytest.raises(ValueError, match="min_samples"):
                model.dbscan(0.5, bad)
            with pytest.raises(ValueError, match="min_samples"):
                model.dbscan(0.5, min_samples=bad)
    # a pruned model (the guarded one is) at t <= 0
    for bad in (0, 0.0, -0.0, -0.5, [0.5, 0.0], [-1, 0.5]):
        with pytest.raises(ValueError, match="t > 0"):
            est.degrees(bad)
    for bad in (0, -0.0, -0.5):
        with pytest.raises(ValueError, match="t > 0"):
            est.dbscan(bad, 3)
    assert est.kept_neighbors == 2                               # the model is as it was
    est.release()
    for call in (lambda: est.degrees(0.5), lambda: est.degrees([0.5, 0.1]), lambda: est.dbscan(0.5), lambda: est.dbscan(0.5, 2)):
        with pytest.raises(RuntimeError, match="released"):
            call()


def test_what_the_min_samples_check_accepts():
    assert [_density.check_min_samples(m) for m in (1, 2, 5, np.int64(7), np.int32(1))] == [0, 1, 4, 6, 0]
    assert _density.check_min_samples(10 ** 30) == 2 ** 31 - 1    # nobody is core: an int32 holds the bound


# ---- the reference, pinned ---------------------------------------------------------------------------------------------
def seven():
    """7 nodes at t = 0.  Edges: 0 - 1 passes only below the diagonal; 1 - 2 passes both ways; 1 - 3 is a -0.0 one way and
    a NaN the other; 3 - 5 a +0.0 above the diagonal; 2 - 5 and 6 - 4 pass below the diagonal only (the other direction of
    6 - 4 is NaN); 4 - 5 passes above it.  Everything else is -1, but for the pair 0 - 6, NaN both ways, and a diagonal that
    would pass."""
    S = np.full((7, 7), -1.0)
    np.fill_diagonal(S, 1.0)
    S[1, 0] = 0.5
    S[1, 2], S[2, 1] = 0.25, 0.75
    S[1, 3], S[3, 1] = -0.0, np.nan
    S[3, 5] = 0.0
    S[5, 2] = 1.0
    S[4, 5] = 2.0
    S[6, 4], S[4, 6] = 0.5, np.nan
    S[0, 6] = S[6, 0] = np.nan
    return S


def test_the_reference_on_a_hand_made_matrix():
    S = seven()
    assert DR.degrees(S, [0.0, -0.0, 0.25, 0.3, 3.0, -1.0]).tolist() == [
        [1, 3, 2, 2, 2, 3, 1], [1, 3, 2, 2, 2, 3, 1], [1, 2, 2, 0, 2, 2, 1], [1, 2, 2, 0, 2, 2, 1], [0] * 7,
        [5, 6, 6, 6, 6, 6, 5]]                                   # at -1 only NaN fails: 0 - 6 both ways; (3, 1) and (4, 6) have a passing mirror
    # min_samples = 4: a core node has 3 neighbours: 1 and 5.  2 and 3 are neighbours of both and go to the smaller, 1;
    # 1 and 5 share only those two border nodes and stay apart; 4 is a border node of 5; 6 has the border node 4 as its
    # only neighbour: noise
    cluster, core, deg, root = DR.dbscan(S, 0.0, 4)
    assert cluster.tolist() == [0, 0, 0, 0, 1, 1, -1] and core.tolist() == [False, True, False, False, False, True, False]
    assert deg.tolist() == [1, 3, 2, 2, 2, 3, 1] and root.tolist() == [1, 1, 1, 1, 5, 5, -1]
    assert DR.counts(cluster, core) == (2, 4, 1)
    # min_samples = 3 at 0.25: (1, 3) and (3, 5) are gone; 1 - 2 - 5 - 4 are core and one cluster, 0 and 6 its border
    # nodes, 3 is noise
    cluster, core, deg, root = DR.dbscan(S, 0.25, 3)
    assert cluster.tolist() == [0, 0, 0, -1, 0, 0, 0] and core.tolist() == [False, True, True, False, True, True, False]
    assert root.tolist() == [1, 1, 1, -1, 1, 1, 1]
    # min_samples = 3 at 0: everybody but 0 and 6 is core; 0 is first and a border node: cluster 0 is numbered by it
    cluster, core, _, root = DR.dbscan(S, 0.0, 3)
    assert cluster.tolist() == [0] * 7 and core.tolist() == [False, True, True, True, True, True, False] and root.tolist() == [1] * 7
    # min_samples = 2: no border node can exist
    for t in (0.0, 0.25, 0.6, 3.0):
        cluster, core, deg, _ = DR.dbscan(S, t, 2)
        assert np.array_equal(core, deg >= 1) and np.array_equal(cluster >= 0, core)
    # nothing passes: all noise, or all singletons at min_samples = 1
    assert DR.dbscan(S, 3.0, 2)[0].tolist() == [-1] * 7 and DR.dbscan(S, 3.0, 1)[0].tolist() == list(range(7))


def random_matrices():
    rng = np.random.default_rng(4)
    for n, density in ((1, 0.5), (2, 0.5), (40, 0.03), (40, 0.08), (90, 0.02), (90, 0.05)):
        S = np.where(rng.random((n, n)) < density, rng.random((n, n)), -rng.random((n, n)))
        S[rng.random((n, n)) < 0.02] = np.nan
        yield S


def test_min_samples_one_is_single_linkage():
    for S in [seven()] + list(random_matrices()):
        for t in (0.0, 0.25, 0.5, -2.0, 3.0):
            cluster, core, deg, root = DR.dbscan(S, t, 1)
            assert core.all() and np.array_equal(cluster, CR.components(S, [t])[0])
            assert np.array_equal(deg, DR.degrees(S, [t])[0])


def test_the_reference_agrees_with_scikit_learn():
    sk = pytest.importorskip("sklearn.cluster")
    seen = 0
    for S in [seven()] + list(random_matrices()):
        for t in (0.0, 0.25, 0.5):
            for min_samples in (1, 2, 3, 4, 5):
                cluster, core, deg, _ = DR.dbscan(S, t, min_samples)
                D = np.where(CR.graph(S, t), 0.0, 1.0)
                np.fill_diagonal(D, 0.0)
                fit = sk.DBSCAN(eps=0.5, min_samples=min_samples, metric="precomputed").fit(D)
                got = np.zeros(len(S), dtype=bool)
                got[fit.core_sample_indices_] = True
                assert np.array_equal(got, core), (t, min_samples)
                # the same partition of the core nodes (a border node's cluster is scan order there: not compared)
                a, b = cluster[core], fit.labels_[core]
                assert (a >= 0).all() and (b >= 0).all()
                assert np.array_equal(a[:, None] == a[None, :], b[:, None] == b[None, :]), (t, min_samples)
                assert np.array_equal(cluster < 0, fit.labels_ < 0)            # noise is noise in any scan order
                seen += DR.counts(cluster, core)[0] >= 2
    assert seen >= 10


# ---- the host half: numbering, and the lists of a pruned model -------------------------------------------------------------
def test_numbering_is_by_first_member_and_noise_stays():
    assert _density.number([1, 1, -1, 5, 1, 0, 5, -1]).tolist() == [0, 0, -1, 1, 0, 2, 1, -1]
    assert _density.number([3, 3, 3]).tolist() == [0, 0, 0] and _density.number([-1, -1]).tolist() == [-1, -1]
    assert _density.number(np.empty(0, dtype=np.int64)).shape == (0,)


THRESHOLDS = [0.75, 0.5, 0.3, 0.125, 1e-9, 1e-300, 2.0]


def host_dbscan(ids, vals, t, min_samples):
    deg, labels = _density.dbscan_of_pairs(len(ids), *_density.neighbour_pairs(ids, vals, t), min_samples - 1)
    return _density.number(labels), deg >= min_samples - 1, deg, labels


def test_the_host_path_of_pruned_lists_equals_the_reference():
    rng = np.random.default_rng(8)
    n, k = 60, 6
    big_ids = np.array([rng.permutation(np.delete(np.arange(n), i))[:k] for i in range(n)], dtype=np.int32)
    big_ids[rng.random((n, k)) < 0.2] = -1
    big_vals = rng.random((n, k))
    big_vals[rng.random((n, k)) < 0.05] = np.nan
    for ids, vals, ts in ((*lists_case(), THRESHOLDS), (big_ids, big_vals, [0.2, 0.5, 0.8, 0.95])):
        P = CR.matrix_of_lists(ids, vals)
        want_deg = DR.degrees(P, ts)
        for i, t in enumerate(ts):
            deg, none = _density.dbscan_of_pairs(len(ids), *_density.neighbour_pairs(ids, vals, t), None)
            assert none is None and deg.dtype == np.int64 and np.array_equal(deg, want_deg[i]), t
            for min_samples in (1, 2, 3, 4, 5):
                got, want = host_dbscan(ids, vals, t, min_samples), DR.dbscan(P, t, min_samples)
                for g, w in zip(got, want):
                    assert g.dtype == w.dtype and np.array_equal(g, w), (t, min_samples)
    # the big case is not trivial: at some level the reference has two clusters, border nodes and noise at once
    P = CR.matrix_of_lists(big_ids, big_vals)
    found = [DR.counts(*DR.dbscan(P, t, m)[:2]) for t in (0.2, 0.5, 0.8, 0.95) for m in (3, 4, 5)]
    assert any(c >= 2 and b >= 1 and z >= 1 for c, b, z in found), found


def test_degrees_and_dbscan_of_a_pruned_model(monkeypatch):
    monkeypatch.setattr(_density, "load", boom)              # (a pruned model needs no library)
    ops = HostOps()
    ids, vals = lists_case()
    solver = _neighbors.NeighborSolver(ops, [_FullSpec(6)], [_neighbors.Tables.from_host(ops, ids, vals, np.ones(6))])
    est = SRA.SimRank()._keep(solver, [(0, list("abcdef"))])
    P = CR.matrix_of_lists(ids, vals)
    one = est.degrees(0.3)
    assert isinstance(one, pd.Series) and one.name == "neighbors" and one.dtype == np.int64
    assert one.index.tolist() == list("abcdef") and one.tolist() == DR.degrees(P, [0.3])[0].tolist() == [2, 1, 0, 3, 1, 1]
    ts = [0.5, 0.75, 0.5, 2.0, 1e-9, 0.3]
    many = est.degrees(ts)
    assert isinstance(many, pd.DataFrame) and many.index.tolist() == list("abcdef")
    assert many.columns.tolist() == [float(t) for t in ts] and (many.dtypes == np.int64).all()
    assert np.array_equal(many.to_numpy().T, DR.degrees(P, ts))
    assert np.array_equal(many.iloc[:, 5].to_numpy(), one.to_numpy())
    for t in (0.3, 0.5, 1e-9):
        for min_samples in (1, 2, 3, 4):
            got = est.dbscan(t, min_samples)
            cluster, core, deg, _ = DR.dbscan(P, t, min_samples)
            assert isinstance(got, pd.DataFrame) and got.columns.tolist() == ["cluster", "core", "neighbors"]
            assert got.index.tolist() == list("abcdef")
            assert got.dtypes.tolist() == [np.int64, np.bool_, np.int64]
            assert got["cluster"].tolist() == cluster.tolist() and got["core"].tolist() == core.tolist()
            assert got["neighbors"].tolist() == deg.tolist()
        assert np.array_equal(est.dbscan(t, 1)["cluster"].to_numpy(), est.components(t).to_numpy())
    assert est.dbscan(0.3).equals(est.dbscan(0.3, min_samples=5))       # the default
    # 0.3, min_samples = 3: 0 (neighbours 1, 3) and 3 (0, 4, 5) are core; 1, 4 and 5 are their border nodes; 2 is noise
    assert est.dbscan(0.3, 3)["cluster"].tolist() == [0, 0, -1, 0, 0, 0]
    with pytest.raises(ValueError, match="t > 0"):
        est.degrees([0.3, 0.0])
    assert est.kept_neighbors == 3                            # the model is as it was
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.dbscan(0.3, 3)
    assert not ops.live
