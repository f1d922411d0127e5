"""libsimrank_linkage.so (include/simrank_linkage.h), ``linkage`` and ``cut`` on a machine without a GPU: header, binding
and exports agree, the header is plain C99 and stands alone, every entry point refuses bad arguments without a device,
the argument checks run before any device work, ``canonical`` gives ``linkage_ref``'s rows from any valid spanning forest,
the host path of a pruned model equals ``linkage_ref`` on hand-made tables, and ``cut`` equals ``cluster_ref``."""
import re

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _lib, _linkage, _neighbors, _query
from tests import cluster_ref as CR
from tests import companion_abi as A
from tests import linkage_ref as LR
from tests.test_cluster_cpu import HostOps, _FullSpec, boom, guarded_estimator, lists_case


def same(got, want):
    return (len(got) == len(want) == 4 and all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
            and not (np.signbit(got[2]) & (got[2] == 0)).any())


# ---- the library -------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    assert A.loaded_version(_linkage) == _linkage.VERSION == 1
    text = A.header(_linkage)
    assert re.search(r"SIMRANK_LINKAGE_BAD_COMPONENT = %d\b" % _linkage.BAD_COMPONENT, text)
    assert re.search(r"SIMRANK_LINKAGE_CAP_REACHED = %d\b" % _linkage.CAP_REACHED, text)
    A.assert_header_stands_alone(_linkage)


def test_the_layout_codes_are_the_shared_ones():
    assert A.layout_codes(_linkage) == A.layout_codes(_query) and len(A.layout_codes(_linkage)) == 4
    lib = _linkage.load()
    assert [lib.simrank_linkage_phases(lay) for lay in range(4)] == [1, 1, 1, 2]
    assert lib.simrank_linkage_phases(4) == -1 and lib.simrank_linkage_phases(-1) == -1


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_linkage)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_linkage)


def test_the_main_library_is_unchanged():
    version, names, exports = A.main_library(_linkage)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_every_entry_refuses_bad_arguments_without_a_device(tmp_path):
    assert "linkage 1 ok" in A.run_c99(_linkage, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_linkage.h"
#define BAD(call, code) do { if ((call) != SIMRANK_LINKAGE_ERR_INVALID) return code; \
                             if (!strlen(simrank_linkage_last_error())) return 100 + code; } while (0)
int main(void) {
    /* 16-byte aligned stand-ins for device memory: nothing below may reach a device */
    static int32_t mem[8] __attribute__((aligned(16)));
    static uint64_t slots[8];
    static double vals[4];
    int32_t* one = mem;
    int32_t* other = mem + 4;
    float f = 0.5f;
    const int32_t f32 = SIMRANK_LINKAGE_ROWMAJOR_F32, f64 = SIMRANK_LINKAGE_ROWMAJOR_F64;
    const int64_t huge = (int64_t)1 << 31;
    if (simrank_linkage_version() != SIMRANK_LINKAGE_VERSION) return 1;
    if (simrank_linkage_phases(f32) != 1 || simrank_linkage_phases(f64) != 2) return 2;
    BAD(simrank_linkage_phases(7), 3);
    /* init: NULL arrays, negative or huge n, NULL counters */
    BAD(simrank_linkage_init(NULL, slots, other, vals, 4, one, one, NULL), 10);
    BAD(simrank_linkage_init(one, NULL, other, vals, 4, one, one, NULL), 11);
    BAD(simrank_linkage_init(one, slots, NULL, vals, 4, one, one, NULL), 12);
    BAD(simrank_linkage_init(one, slots, other, NULL, 4, one, one, NULL), 13);
    BAD(simrank_linkage_init(one, slots, other, vals, -1, one, one, NULL), 14);
    BAD(simrank_linkage_init(one, slots, other, vals, huge, one, one, NULL), 15);
    BAD(simrank_linkage_init(one, slots, other, vals, 4, NULL, one, NULL), 16);
    BAD(simrank_linkage_init(one, slots, other, vals, 4, one, NULL, NULL), 17);
    /* pick: layout, NULL block, stride, shape, alignment of a panel block, phase, NULL comp / best / status, n */
    BAD(simrank_linkage_pick(one, 9, 4, 4, 4, NULL, NULL, &f, 0, one, slots, 4, one, NULL), 20);
    BAD(simrank_linkage_pick(NULL, f32, 4, 4, 4, NULL, NULL, &f, 0, one, slots, 4, one, NULL), 21);
    BAD(simrank_linkage_pick(one, f32, 3, 4, 4, NULL, NULL, &f, 0, one, slots, 4, one, NULL), 22);
    BAD(simrank_linkage_pick(one, SIMRANK_LINKAGE_PANEL_F16, 2, 4, 4, NULL, NULL, &f, 0, one, slots, 4, one, NULL), 23);
    BAD(simrank_linkage_pick(one, f32, 4, -1, 4, NULL, NULL, &f, 0, one, slots, 4, one, NULL), 24);
    BAD(simrank_linkage_pick(one, f32, 4, 4, huge, NULL, NULL, &f, 0, one, slots, 4, one, NULL), 25);
    BAD(simrank_linkage_pick(one + 1, SIMRANK_LINKAGE_PANEL_F32, 4, 4, 4, NULL, NULL, &f, 0, one, slots, 4, one, NULL), 26);
    BAD(simrank_linkage_pick(one, f32, 4, 4, 4, NULL, NULL, NULL, 1, one, slots, 4, one, NULL), 27);
    if (!strstr(simrank_linkage_last_error(), "phase")) return 28;
    BAD(simrank_linkage_pick(one, f64, 4, 1, 1, NULL, NULL, NULL, 2, one, slots, 4, one, NULL), 29);
    BAD(simrank_linkage_pick(one, f32, 4, 4, 4, NULL, NULL, NULL, -1, one, slots, 4, one, NULL), 30);
    BAD(simrank_linkage_pick(one, f32, 4, 4, 4, NULL, NULL, &f, 0, NULL, slots, 4, one, NULL), 31);
    BAD(simrank_linkage_pick(one, f32, 4, 4, 4, NULL, NULL, &f, 0, one, NULL, 4, one, NULL), 32);
    BAD(simrank_linkage_pick(one, f32, 4, 4, 4, NULL, NULL, &f, 0, one, slots, 4, NULL, NULL), 33);
    BAD(simrank_linkage_pick(one, f32, 4, 4, 4, NULL, NULL, &f, 0, one, slots, -4, one, NULL), 34);
    BAD(simrank_linkage_pick(one, f32, 4, 4, 4, NULL, NULL, &f, 0, one, slots, huge, one, NULL), 35);
    /* an empty block or no nodes: nothing to queue */
    if (simrank_linkage_pick(NULL, f32, 4, 0, 4, NULL, NULL, &f, 0, one, slots, 4, one, NULL) != SIMRANK_LINKAGE_OK) return 36;
    if (simrank_linkage_pick(one, f64, 4, 1, 1, NULL, NULL, NULL, 1, NULL, NULL, 0, one, NULL) != SIMRANK_LINKAGE_OK) return 37;
    /* hook: NULL arrays and counters, key_bits, n */
    BAD(simrank_linkage_hook(NULL, 32, one, other, vals, 4, one, one, NULL), 40);
    BAD(simrank_linkage_hook(slots, 32, NULL, other, vals, 4, one, one, NULL), 41);
    BAD(simrank_linkage_hook(slots, 32, one, NULL, vals, 4, one, one, NULL), 42);
    BAD(simrank_linkage_hook(slots, 32, one, other, NULL, 4, one, one, NULL), 43);
    BAD(simrank_linkage_hook(slots, 32, one, other, vals, 4, NULL, one, NULL), 44);
    BAD(simrank_linkage_hook(slots, 32, one, other, vals, 4, one, NULL, NULL), 45);
    BAD(simrank_linkage_hook(slots, 16, one, other, vals, 4, one, one, NULL), 46);
    BAD(simrank_linkage_hook(slots, 0, one, other, vals, 4, one, one, NULL), 47);
    BAD(simrank_linkage_hook(slots, 64, one, other, vals, -1, one, one, NULL), 48);
    if (simrank_linkage_hook(NULL, 64, NULL, NULL, NULL, 0, one, one, NULL) != SIMRANK_LINKAGE_OK) return 49;
    /* flatten: NULL arrays, n */
    BAD(simrank_linkage_flatten(NULL, slots, 4, one, NULL), 50);
    BAD(simrank_linkage_flatten(one, NULL, 4, one, NULL), 51);
    BAD(simrank_linkage_flatten(one, slots, 4, NULL, NULL), 52);
    BAD(simrank_linkage_flatten(one, slots, -2, one, NULL), 53);
    BAD(simrank_linkage_flatten(one, slots, huge, one, NULL), 54);
    if (simrank_linkage_flatten(NULL, NULL, 0, one, NULL) != SIMRANK_LINKAGE_OK) return 55;
    printf("linkage %d ok\n", simrank_linkage_version());
    return 0;
}
''')


def test_the_round_bound():
    assert [_linkage.max_rounds(n) for n in (1, 2, 3, 4, 5, 8, 9, 1024, 1025, 65536)] == [1, 2, 3, 3, 4, 4, 5, 11, 12, 17]


# ---- canonical: one table from any valid forest ------------------------------------------------------------------------------
def tied_matrix():
    """12 nodes, values from {0, 0.25, 0.5, 1} with many ties, both directions different, NaN (node 11 has nothing but
    NaN), -0.0 next to +0.0, and four nodes (2, 5, 7, 9) that fall together at once at 0.5."""
    rng = np.random.default_rng(4)
    S = rng.choice([0.0, -0.0, 0.25, 0.25, 0.5, 1.0], size=(12, 12), p=[0.3, 0.2, 0.2, 0.1, 0.1, 0.1])
    S[rng.random((12, 12)) < 0.1] = np.nan
    for x in (2, 5, 7, 9):
        S[x], S[:, x] = 0.25, -0.0
    S[2, 5] = S[7, 2] = S[9, 2] = S[9, 5] = S[5, 7] = 0.5
    S[11], S[:, 11] = np.nan, np.nan
    return S


def spanning_forest(n, a, b, w, order):
    """Kruskal over the edges in ``order`` (largest first, ties as ``order`` has them) -> the kept edges."""
    parent, keep = list(range(n)), []
    for i in order:
        ra, rb = _linkage._find(parent, int(a[i])), _linkage._find(parent, int(b[i]))
        if ra != rb:
            parent[ra] = rb
            keep.append(i)
    return a[keep], b[keep], w[keep]


def test_canonical_gives_the_reference_from_three_different_forests():
    S = tied_matrix()
    n = len(S)
    want = LR.linkage(S)
    assert same(LR.linkage_by_partitions(S), want)           # the reference's two statements agree
    heights, widest = LR.stats(n, want)
    assert heights >= 3 and widest >= 4 and len(want[0]) == n - 2        # (node 11 joins nothing)
    a, b, w = LR.matrix_edges(S)
    rng = np.random.default_rng(8)
    forests = []
    for tie in (np.arange(len(a)), np.arange(len(a))[::-1], rng.permutation(len(a))):
        order = tie[np.argsort(-w[tie], kind="stable")]
        fa, fb, fw = spanning_forest(n, a, b, w, order)
        flip = rng.random(len(fa)) < 0.5                      # (an edge has no direction)
        forests.append(sorted(zip(np.minimum(fa, fb).tolist(), np.maximum(fa, fb).tolist())))
        assert same(_linkage.canonical(n, np.where(flip, fb, fa), np.where(flip, fa, fb), fw), want)
        shuffled = rng.permutation(len(fa))                   # (nor has the list an order)
        assert same(_linkage.canonical(n, fa[shuffled], fb[shuffled], fw[shuffled]), want)
    assert forests[0] != forests[1] and forests[0] != forests[2] and forests[1] != forests[2]
    # -0.0 comes out as +0.0; an empty forest gives an empty table of the right types
    assert same(_linkage.canonical(3, [0, 1], [1, 2], [-0.0, 0.0]), LR.rows_of_edges(3, [0, 1], [1, 2], [0.0, 0.0]))
    assert same(_linkage.canonical(3, [], [], []), LR.rows_of_edges(3, [], [], []))


def test_canonical_on_random_tied_matrices():
    rng = np.random.default_rng(0)
    for trial in range(25):
        n = int(rng.integers(2, 14))
        S = rng.integers(-2, 4, size=(n, n)) * 0.25
        S[rng.random((n, n)) < 0.15] = np.nan
        S[rng.random((n, n)) < 0.1] = -0.0
        a, b, w = LR.matrix_edges(S)
        for floor in (None, 0.25, 0.3):
            want = LR.linkage(S, floor)
            assert same(LR.linkage_by_partitions(S, floor), want)
            use = np.ones(len(w), dtype=bool) if floor is None else w >= floor
            order = rng.permutation(np.flatnonzero(use))
            order = order[np.argsort(-w[order], kind="stable")]
            assert same(_linkage.canonical(n, *spanning_forest(n, a, b, w, order)), want), (trial, floor)


# ---- cut ---------------------------------------------------------------------------------------------------------------------
def kept(labels, solver=None):
    est = SRA.SimRank()
    est._keep(solver if solver is not None else object(), [(0, list(labels))])
    return est


def test_cut_at_a_threshold_equals_components():
    S = tied_matrix()
    n = len(S)
    est = kept("abcdefghijkl")
    for floor in (None, 0.25):
        Z = pd.DataFrame(dict(zip(_linkage.COLUMNS, LR.linkage(S, floor))))
        ts = [1.5, 1.0, 0.75, 0.5, 0.3, 0.25] + ([] if floor else [0.1, 0.0, -0.0, -1.0])
        for t in ts:
            got = est.cut(Z, t=t)
            assert isinstance(got, pd.Series) and got.name == "component" and got.dtype == np.int64
            assert got.index.tolist() == list("abcdefghijkl")
            assert np.array_equal(got.to_numpy(), CR.components(S, [t])[0]), (floor, t)
            assert np.array_equal(got.to_numpy(), LR.cut(n, LR.linkage(S, floor), t=t))
    assert est.cut(Z, t=0.5, group=1).equals(est.cut(Z, t=0.5))


def test_cut_into_k_clusters():
    S = tied_matrix()
    n = len(S)
    rows = LR.linkage(S)
    Z = pd.DataFrame(dict(zip(_linkage.COLUMNS, rows)))
    est = kept(range(n))
    for k in range(2, n + 1):                                 # (10 rows: 12 nodes come down to 2 clusters)
        got = est.cut(Z, n_clusters=k).to_numpy()
        assert np.unique(got).size == k == got.max() + 1
        assert np.array_equal(got, LR.cut(n, rows, n_clusters=k))
        assert np.array_equal(got, est.cut(Z, n_clusters=np.int64(k)).to_numpy())
    # within a tie the split follows the canonical order: 1, 3, 4, 5 fall together at 0.5 through (3, 5), (5, 1), (4, 1);
    # the rows take them by smallest member, whatever the edges were
    T = np.zeros((6, 6))
    T[3, 5] = T[5, 1] = T[4, 1] = 0.5
    Zt = pd.DataFrame(dict(zip(_linkage.COLUMNS, LR.linkage(T))))
    assert Zt["left"].tolist() == [1, 6, 7, 0, 9] and Zt["right"].tolist() == [3, 4, 5, 8, 2]
    assert Zt["similarity"].tolist() == [0.5, 0.5, 0.5, 0.0, 0.0] and Zt["size"].tolist() == [2, 3, 4, 5, 6]
    assert kept(range(6)).cut(Zt, n_clusters=4).tolist() == [0, 1, 2, 1, 1, 3]
    assert kept(range(6)).cut(Zt, n_clusters=2).tolist() == [0, 0, 1, 0, 0, 0]
    with pytest.raises(ValueError, match="fewest clusters this table reaches is 2"):
        est.cut(Z, n_clusters=1)
    with pytest.raises(ValueError, match="more than the 12 nodes"):
        est.cut(Z, n_clusters=13)


BAD_NUMBERS = [True, np.True_, float("nan"), float("inf"), -float("inf"), "0.5", b"1", [0.5], (), 1 + 2j, 10 ** 400,
               np.array(float("nan")), np.array("x"), {"t": 0.5}]


def test_cut_argument_checks():
    S = tied_matrix()
    Z = pd.DataFrame(dict(zip(_linkage.COLUMNS, LR.linkage(S))))
    est = kept(range(12))
    for both in ({}, {"t": 0.5, "n_clusters": 3}):
        with pytest.raises(ValueError, match="exactly one"):
            est.cut(Z, **both)
    for bad in BAD_NUMBERS:
        with pytest.raises(ValueError, match="finite number"):
            est.cut(Z, t=bad)
    for bad in (0, -1, 2.0, "3", True, [3], np.float64(3)):
        with pytest.raises(ValueError, match="n_clusters"):
            est.cut(Z, n_clusters=bad)
    with pytest.raises(ValueError, match="group"):
        est.cut(Z, t=0.5, group=2)
    with pytest.raises(ValueError, match="columns"):
        est.cut(Z.drop(columns="right"), t=0.5)
    with pytest.raises(ValueError, match="columns"):
        est.cut(None, t=0.5)
    with pytest.raises(ValueError, match="at most 4"):
        kept(range(5)).cut(Z, t=0.5)                          # a table of another model
    with pytest.raises(ValueError, match="size is not the sum"):
        kept(range(40)).cut(Z, t=0.5)
    with pytest.raises(ValueError, match="ids below"):
        est.cut(Z.assign(left=Z["left"].where(Z.index != 0, 12)), t=0.5)
    with pytest.raises(ValueError, match="must fall"):
        est.cut(Z.assign(similarity=Z["similarity"].to_numpy()[::-1]), t=0.5)
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().cut(Z, t=0.5)
    with pytest.raises(ValueError, match="exactly one"):
        SRA.SimRank().cut(Z)                                  # (the arguments are judged before the model)


# ---- linkage(): argument checks need no device ---------------------------------------------------------------------------------
def test_linkage_argument_checks_need_no_device(monkeypatch):
    monkeypatch.setattr(_linkage, "load", boom)
    monkeypatch.setattr(_linkage, "forest_blocks", boom)
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().linkage()
    est = guarded_estimator()                                 # a pruned model whose lists nothing may read
    for bad in BAD_NUMBERS:
        with pytest.raises(ValueError, match="min_similarity must be a finite number"):
            est.linkage(bad)
        with pytest.raises(ValueError, match="min_similarity must be a finite number"):
            SRA.SimRank().linkage(min_similarity=bad)         # (the argument is judged before the model)
    for floor in (None, 0, 0.0, -0.0, -0.5):
        with pytest.raises(ValueError, match=r"\+0\.0 and tie everything at 0"):
            est.linkage(floor)
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.linkage(0.5)


def test_what_the_floor_check_accepts():
    assert _linkage.check_floor(None) is None
    for good in (0.5, -3, 0, np.float32(0.25), np.int64(2), np.array(0.125)):
        got = _linkage.check_floor(good)
        assert isinstance(got, float) and got == float(good)


# ---- the host path of a pruned model --------------------------------------------------------------------------------------------
def test_the_host_path_of_pruned_lists_equals_the_reference():
    ids, vals = lists_case()
    P = CR.matrix_of_lists(ids, vals)
    n = len(P)
    for floor in (1e-300, 1e-9, 0.1, 0.125, 0.3, 0.5, 0.75, 1.0, 2.0):
        want = LR.linkage(P, floor)
        got = _linkage.canonical(n, *_linkage.forest_of_lists(ids, vals, floor))
        assert same(got, want), floor
        assert same(LR.linkage_by_partitions(P, floor), want)
    # 0 - 3 join at 0.5 (0.5 one way, 0.125 the other); 3 - 5 at 1.0; 1 - 0 at 0.75; 3 - 4 at 0.5; 5 - 2 at 0.125
    got = _linkage.canonical(n, *_linkage.forest_of_lists(ids, vals, 0.1))
    assert got[2].tolist() == [1.0, 0.75, 0.5, 0.5, 0.125]
    assert got[0].tolist() == [3, 0, 7, 8, 9] and got[1].tolist() == [5, 1, 6, 4, 2] and got[3].tolist() == [2, 2, 4, 5, 6]


def test_linkage_of_a_pruned_model(monkeypatch):
    monkeypatch.setattr(_linkage, "load", boom)              # (a pruned model needs no library)
    ops = HostOps()
    ids, vals = lists_case()
    solver = _neighbors.NeighborSolver(ops, [_FullSpec(6)], [_neighbors.Tables.from_host(ops, ids, vals, np.ones(6))])
    est = SRA.SimRank()._keep(solver, [(0, list("abcdef"))])
    P = CR.matrix_of_lists(ids, vals)
    Z = est.linkage(min_similarity=0.1)
    assert isinstance(Z, pd.DataFrame) and Z.columns.tolist() == ["left", "right", "similarity", "size"]
    assert Z.dtypes.tolist() == [np.int64, np.int64, np.float64, np.int64]
    assert same(tuple(Z[c].to_numpy() for c in Z.columns), LR.linkage(P, 0.1)) and len(Z) == 5
    assert len(est.linkage(0.6)) == 2 and len(est.linkage(5)) == 0
    for t in (0.1, 0.125, 0.3, 0.5, 0.75, 1.0, 2.0):
        assert est.cut(Z, t=t).equals(est.components(t)), t
    assert est.cut(Z, n_clusters=1).tolist() == [0] * 6 and est.cut(Z, n_clusters=6).tolist() == list(range(6))
    with pytest.raises(ValueError, match="tie everything at 0"):
        est.linkage()
    assert est.kept_neighbors == 3                            # the model is as it was
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.linkage(0.3)
    with pytest.raises(RuntimeError, match="released"):
        est.cut(Z, t=0.3)
    assert not ops.live
