"""libsimrank_kmedoids.so (include/simrank_kmedoids.h) and ``assign`` / ``kmedoids`` on a machine without a GPU: header,
binding and exports agree, the header is plain C99 and stands alone, the entries refuse bad arguments without a device,
the seeds are judged before any device work, the host path of a pruned model equals ``kmedoids_ref`` on hand-made lists,
the reference converges on the oracle's matrices of the suite's power-law graph with an objective that never falls, and
the 4-node matrix on which simultaneous relocation oscillates is kept as a witness."""
import math
import re

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _kmedoids, _lib, _neighbors, _query, synth
from tests import cluster_ref as CR
from tests import companion_abi as A
from tests import groups_ref as GR
from tests import kmedoids_ref as KR
from tests.test_cluster_cpu import HostOps, _FullSpec, boom, guarded_estimator
from tests.test_groups_cpu import same, table_cases


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_kmedoids) == _kmedoids.VERSION == 1
    assert re.search(r"#define SIMRANK_KMEDOIDS_CHUNK %d\b" % _kmedoids.CHUNK, A.header(_kmedoids))
    assert sorted(_kmedoids.PROTOTYPES) == ["simrank_kmedoids_assign", "simrank_kmedoids_last_error",
                                            "simrank_kmedoids_pick", "simrank_kmedoids_version"]
    A.assert_header_stands_alone(_kmedoids)
    A.assert_prototypes_match_the_header_argument_counts(_kmedoids)
    assert A.layout_codes(_kmedoids) == A.layout_codes(_query) and len(A.layout_codes(_kmedoids)) == 4


def test_companion_links_nothing_of_the_main_library_which_is_unchanged():
    A.assert_links_nothing_of_the_main_library(_kmedoids)
    version, names, exports = A.main_library(_kmedoids)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_the_entries_refuse_bad_arguments_without_a_device(tmp_path):
    assert "kmedoids 1 ok" in A.run_c99(_kmedoids, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_kmedoids.h"
#define BAD(call, code) do { if ((call) != SIMRANK_KMEDOIDS_ERR_INVALID) return code; \
                             if (!strlen(simrank_kmedoids_last_error())) return 100 + code; } while (0)
int main(void) {
    /* aligned stand-ins for device memory: nothing below may reach a device */
    static double mem[8];
    static int64_t ptr[3];
    static int32_t ids[8];
    static uint32_t count[1];
    const void* S = mem;
    double* d = mem;
    const int32_t f32 = SIMRANK_KMEDOIDS_ROWMAJOR_F32;
    const int64_t huge = (int64_t)1 << 31;
    if (simrank_kmedoids_version() != SIMRANK_KMEDOIDS_VERSION) return 1;
    /* assign: NULL pointers, one at a time (current and moved may be NULL) */
    BAD(simrank_kmedoids_assign(NULL, f32, 4, 4, 4, ids, ids, 2, NULL, ids, d, count, NULL), 2);
    BAD(simrank_kmedoids_assign(S, f32, 4, 4, 4, NULL, ids, 2, NULL, ids, d, count, NULL), 3);
    BAD(simrank_kmedoids_assign(S, f32, 4, 4, 4, ids, NULL, 2, NULL, ids, d, count, NULL), 4);
    BAD(simrank_kmedoids_assign(S, f32, 4, 4, 4, ids, ids, 2, NULL, NULL, d, count, NULL), 5);
    BAD(simrank_kmedoids_assign(S, f32, 4, 4, 4, ids, ids, 2, NULL, ids, NULL, NULL, NULL), 6);
    /* no medoids */
    BAD(simrank_kmedoids_assign(S, f32, 4, 4, 4, ids, ids, 0, NULL, ids, d, count, NULL), 7);
    BAD(simrank_kmedoids_assign(S, f32, 4, 4, 4, ids, ids, -3, ids, ids, d, count, NULL), 8);
    if (!strstr(simrank_kmedoids_last_error(), "K must")) return 9;
    /* an unknown layout */
    BAD(simrank_kmedoids_assign(S, 4, 4, 4, 4, ids, ids, 2, NULL, ids, d, count, NULL), 10);
    BAD(simrank_kmedoids_assign(S, -1, 4, 4, 4, ids, ids, 2, NULL, ids, d, count, NULL), 11);
    /* a stride too small: columns of a row-major block, rows of a panel block */
    BAD(simrank_kmedoids_assign(S, f32, 3, 4, 4, ids, ids, 2, NULL, ids, d, count, NULL), 12);
    BAD(simrank_kmedoids_assign(S, SIMRANK_KMEDOIDS_ROWMAJOR_F64, 3, 4, 4, ids, ids, 2, NULL, ids, d, count, NULL), 13);
    BAD(simrank_kmedoids_assign(S, SIMRANK_KMEDOIDS_PANEL_F32, 3, 4, 2, ids, ids, 2, NULL, ids, d, count, NULL), 14);
    BAD(simrank_kmedoids_assign(S, SIMRANK_KMEDOIDS_PANEL_F16, 3, 4, 2, ids, ids, 2, NULL, ids, d, count, NULL), 15);
    /* a negative shape, a shape of 2^31 */
    BAD(simrank_kmedoids_assign(S, f32, 4, -1, 4, ids, ids, 2, NULL, ids, d, count, NULL), 16);
    BAD(simrank_kmedoids_assign(S, f32, 4, 4, -1, ids, ids, 2, NULL, ids, d, count, NULL), 17);
    BAD(simrank_kmedoids_assign(S, f32, huge, 4, huge, ids, ids, 2, NULL, ids, d, count, NULL), 18);
    BAD(simrank_kmedoids_assign(S, SIMRANK_KMEDOIDS_PANEL_F32, huge, huge, 4, ids, ids, 2, NULL, ids, d, count, NULL), 19);
    /* a block that does not start on a multiple of its element's size */
    BAD(simrank_kmedoids_assign((const char*)S + 2, f32, 4, 4, 4, ids, ids, 2, NULL, ids, d, count, NULL), 20);
    BAD(simrank_kmedoids_assign((const char*)S + 4, SIMRANK_KMEDOIDS_ROWMAJOR_F64, 4, 1, 4, ids, ids, 2, NULL, ids, d, count, NULL), 21);
    BAD(simrank_kmedoids_assign((const char*)S + 1, SIMRANK_KMEDOIDS_PANEL_F16, 4, 1, 4, ids, ids, 2, NULL, ids, d, count, NULL), 22);
    if (!strstr(simrank_kmedoids_last_error(), "element")) return 23;
    /* no columns: nothing to queue */
    if (simrank_kmedoids_assign(NULL, f32, 4, 4, 0, ids, ids, 2, NULL, NULL, NULL, NULL, NULL) != SIMRANK_KMEDOIDS_OK) return 24;
    /* pick: NULL pointers, one at a time (changed may be NULL), no clusters, a bad number of rows */
    BAD(simrank_kmedoids_pick(NULL, 4, ids, ptr, 2, ids, d, count, NULL), 30);
    BAD(simrank_kmedoids_pick(d, 4, NULL, ptr, 2, ids, d, count, NULL), 31);
    BAD(simrank_kmedoids_pick(d, 4, ids, NULL, 2, ids, d, count, NULL), 32);
    BAD(simrank_kmedoids_pick(d, 4, ids, ptr, 2, NULL, d, count, NULL), 33);
    BAD(simrank_kmedoids_pick(d, 4, ids, ptr, 2, ids, NULL, NULL, NULL), 34);
    BAD(simrank_kmedoids_pick(d, 4, ids, ptr, 0, ids, d, count, NULL), 35);
    BAD(simrank_kmedoids_pick(d, 4, ids, ptr, -1, ids, d, count, NULL), 36);
    BAD(simrank_kmedoids_pick(d, -1, ids, ptr, 2, ids, d, count, NULL), 37);
    BAD(simrank_kmedoids_pick(d, huge, ids, ptr, 2, ids, d, count, NULL), 38);
    printf("kmedoids %d ok\n", simrank_kmedoids_version());
    return 0;
}
''')


# ---- the seeds: judged before any device work --------------------------------------------------------------------------------
INDEX = pd.Index(["a", "b", "c"])
BAD_SEEDS = [[], (), np.array([], dtype=object), pd.Series([], dtype=object),                 # empty
             ["a", "a"], ["a", "b", "a"], pd.Series(["b", "b"]), np.array(["c", "c"]),         # a repeated label
             "abc", b"a", None, 7, 1.5, {"a": 0}, pd.DataFrame({"x": ["a"]}), np.array([["a"]]),  # no sequence of labels
             iter(["a"]), (x for x in "ab"), {"a", "b"}]


def test_what_the_seed_check_refuses_and_accepts():
    for bad in BAD_SEEDS:
        with pytest.raises(ValueError, match="seeds"):
            _kmedoids.check_seeds(bad, INDEX)
    for unknown in (["a", "z"], ["z"], pd.Series(["b", "z"], index=[4, 5]), [0]):
        with pytest.raises(KeyError):
            _kmedoids.check_seeds(unknown, INDEX)
    for good in (["c", "a"], ("c", "a"), np.array(["c", "a"]), pd.Series(["c", "a"], index=[7, -2], name="medoid"),
                 pd.Index(["c", "a"])):
        got = _kmedoids.check_seeds(good, INDEX)
        assert got.dtype == np.int64 and got.tolist() == [2, 0], good
    assert _kmedoids.check_seeds([30, 10], pd.Index([10, 20, 30])).tolist() == [2, 0]
    for bad in (0, -1, True, np.True_, 1.5, None, "3", [3]):
        with pytest.raises(ValueError, match="max_iter"):
            _kmedoids.check_max_iter(bad)
    assert _kmedoids.check_max_iter(np.int64(3)) == 3 and _kmedoids.check_max_iter(1) == 1


def test_argument_checks_need_no_device(monkeypatch):
    for name in ("assign", "kmedoids", "load", "loop_reader", "assign_reader"):
        monkeypatch.setattr(_kmedoids, name, boom)
    calls = lambda est, seeds, **kw: [lambda: est.assign(seeds, **kw), lambda: est.kmedoids(seeds, **kw)]
    for call in calls(SRA.SimRank(), ["a"]):
        with pytest.raises(RuntimeError, match="no kept model"):
            call()
    est = guarded_estimator()
    for bad in BAD_SEEDS:
        for call in calls(est, bad):
            with pytest.raises(ValueError, match="seeds"):
                call()
    for call in calls(est, ["a", "z"]):
        with pytest.raises(KeyError, match="z"):
            call()
    for call in calls(est, ["a"], group=2):
        with pytest.raises(ValueError, match="group"):
            call()
    for bad in (0, -1, True, 1.5, None, "3"):
        with pytest.raises(ValueError, match="max_iter"):
            est.kmedoids(["a"], max_iter=bad)
    est.release()
    for call in calls(est, ["a"]):
        with pytest.raises(RuntimeError, match="released"):
            call()


# ---- the reference by hand ------------------------------------------------------------------------------------------------------
def test_the_reference_by_hand():
    nan = float("nan")
    A_ = np.array([[1.0, 0.5, 0.25, -0.0, nan, 0.0],
                   [0.5, 1.0, 0.25, 0.0, nan, 0.125],
                   [0.0, 0.75, 0.25, 0.0, nan, 0.125]])
    # medoid rows 1, 0, 2, one outside; nobody's own column: column 0 -> row 0 (j = 1); column 1 -> j = 0; column 2: a tie of
    # all three, the first; column 3: -0.0 and +0.0 tie, the first; column 4: no candidate -> 0; column 5: 0.125 at j = 0
    cluster, value, moved = KR.block_assign(A_, [1, 0, 2, 7], [-1, -1, -1, -1])
    assert cluster.tolist() == [1, 0, 0, 0, 0, 0] and moved == 6
    assert same(value, [1.0, 1.0, 0.25, 0.0, nan, 0.125])
    # own columns: column 2 is medoid 2's, column 5 medoid 3's (whose row is outside: NaN), column 4 nobody's
    cluster, value, _ = KR.block_assign(A_, [1, 0, 2, 7], [1, 0, 2, 5])
    assert cluster.tolist() == [1, 0, 2, 0, 0, 3] and same(value, [1.0, 1.0, 0.25, 0.0, nan, nan])
    # the stay rule: equal to the best (stays), tied with a smaller j (stays with the larger), strictly worse (moves), a NaN
    # current value with a candidate (moves) and without (stays), an entry outside 0 .. K - 1 (as the first assignment)
    cluster, value, moved = KR.block_assign(A_, [1, 0, 2, 7], [-1] * 4, np.array([1, 2, 2, 1, 3, 9]))
    assert cluster.tolist() == [1, 0, 2, 1, 3, 0] and moved == 2
    assert same(value, [1.0, 1.0, 0.25, -0.0, nan, 0.125]) and np.signbit(value[3])
    cluster, _, moved = KR.block_assign(A_, [1, 0, 2, 7], [-1] * 4, np.array([0, 3, 0, 0, 0, 3]))
    assert cluster.tolist() == [1, 0, 0, 0, 0, 0] and moved == 3
    # pick: ties to the first in list order, NaN skipped, the incumbent kept on equality and replaced on strictly larger, a
    # NaN incumbent, an incumbent outside, an empty list, positions outside skipped
    own = np.array([0.5, 0.75, 0.75, nan, 0.25, nan, 0.5])
    ptr = np.array([0, 3, 5, 5, 7, 9, 10])
    pos = np.array([2, 0, 1,  3, 4,  5, 6,  -1, 0,  3])
    med, cohesion, changed = KR.block_pick(own, pos, ptr, [1, 3, 4, 6, 99, 3])
    assert med.tolist() == [1, 4, 4, 6, 0, 3] and changed == 2          # (1 keeps 0.75 against the earlier 2; NaN 3 loses to 4)
    assert same(cohesion, [0.75, 0.25, nan, 0.5, 0.5, nan])
    med, _, changed = KR.block_pick(own, pos, ptr, [0, 4, 4, 5, 0, 3])
    assert med.tolist() == [2, 4, 4, 6, 0, 3] and changed == 2          # (0.5 loses to the first 0.75 in list order: 2)


# ---- the host path of a pruned model ------------------------------------------------------------------------------------------------
def matrix_p(ids, vals, diag):
    P = CR.matrix_of_lists(ids, vals)
    P[np.arange(len(P)), np.arange(len(P))] = diag
    return P


def test_the_host_path_of_pruned_lists_equals_the_reference():
    for ids, vals, _ in table_cases():
        n = len(ids)
        diag = 1.0 - 0.125 * (np.arange(n) % 3)
        P = matrix_p(ids, vals, diag)
        own_of = lambda lab: GR.quality(P, lab)[0]
        for seeds in ([0], [n - 1, 0], [1, 4, 2], list(range(n))):
            seeds = np.array(seeds, dtype=np.int64)
            want_c, want_v, _ = KR.assign(P, seeds)
            got_c, got_v, got_moved = _kmedoids.assign_rows(_kmedoids.rows_of_lists(ids, vals, diag, seeds), seeds)
            assert got_c.dtype == np.int64 and np.array_equal(got_c, want_c) and same(got_v, want_v) and got_moved == n
            for max_iter in (1, 20):
                want = KR.kmedoids(P, seeds, max_iter, own_of)
                got = _kmedoids.loop_lists(ids, vals, diag, seeds, max_iter)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (seeds, max_iter)
                assert np.array_equal(got[3], want[3]) and [h[:2] for h in got[5]] == [h[:2] for h in want[5]]
                converged = want[5][-1][1] == 0
                assert (got[2] is not None) == converged and (max_iter == 1 or converged)
                if converged:
                    assert same(got[2], want[2])
                # own: dyadic kept values, so every sum is exact and the means have the same bits
                assert same(got[4], want[4]) and same([h[2] for h in got[5]], [h[2] for h in want[5]])
    # the first table by hand, seeds 1 and 4: node 3 keeps nothing and no medoid keeps it or node 6: +0.0 everywhere, the tie
    # goes to cluster 0; node 0 is kept by both (0.75 by 1, 0.0625 by 4); node 5 by 4 alone
    ids, vals, _ = table_cases()[0]
    cluster, value, _ = _kmedoids.assign_rows(_kmedoids.rows_of_lists(ids, vals, np.ones(7), [1, 4]), [1, 4])
    assert cluster.tolist() == [0, 0, 0, 0, 1, 1, 0] and value.tolist() == [0.75, 1.0, 0.125, 0.0, 1.0, 0.875, 0.0]


def test_the_two_methods_on_a_pruned_model(monkeypatch):
    monkeypatch.setattr(_kmedoids, "load", boom)              # (a pruned model needs no library)
    ops = HostOps()
    ids, vals, _ = table_cases()[0]
    names = list("abcdefg")
    diag = np.array([1.0, 0.5, 1.0, 1.0, 0.75, 1.0, 1.0])
    solver = _neighbors.NeighborSolver(ops, [_FullSpec(7)], [_neighbors.Tables.from_host(ops, ids, vals, diag)])
    est = SRA.SimRank()._keep(solver, [(0, names)])
    P = matrix_p(ids, vals, diag)
    own_of = lambda lab: GR.quality(P, lab)[0]
    a = est.assign(["e", "b"])
    want_c, want_v, _ = KR.assign(P, [4, 1])
    assert a.columns.tolist() == ["cluster", "medoid", "similarity"] and a.index.tolist() == names
    assert a.dtypes.tolist()[0] == np.int64 and a.dtypes.tolist()[2] == np.float64
    assert a["cluster"].tolist() == want_c.tolist() and same(a["similarity"], want_v)
    assert a["medoid"].tolist() == [["e", "b"][c] for c in want_c] and a.at["e", "similarity"] == 0.75
    for max_iter in (1, 20):
        labels, clusters, history = est.kmedoids(pd.Series(["e", "b"], index=[5, 9]), max_iter=max_iter)
        cluster, medoids, sim, sizes, cohesion, steps = KR.kmedoids(P, [4, 1], max_iter, own_of)
        assert labels.index.tolist() == names and labels.columns.tolist() == ["cluster", "medoid", "similarity"]
        assert labels["cluster"].tolist() == cluster.tolist() and same(labels["similarity"], sim)
        assert labels["medoid"].tolist() == [names[medoids[c]] for c in cluster]
        assert clusters.index.tolist() == [0, 1] and clusters.columns.tolist() == ["medoid", "size", "cohesion"]
        assert clusters["medoid"].tolist() == [names[m] for m in medoids] and clusters["size"].tolist() == sizes.tolist()
        assert clusters["size"].dtype == np.int64 and same(clusters["cohesion"], cohesion)
        assert history.columns.tolist() == ["moved", "changed", "objective"] and len(history) == len(steps) <= max_iter
        assert history.dtypes.tolist() == [np.int64, np.int64, np.float64]
        assert history[["moved", "changed"]].values.tolist() == [list(s[:2]) for s in steps]
        assert same(history["objective"], [s[2] for s in steps]) and history["moved"][0] == 7
    assert history["changed"].iloc[-1] == 0 and est.assign(clusters["medoid"])["similarity"].tolist() == labels["similarity"].tolist()
    assert est.kept_neighbors == 2                            # the model is as it was
    est.release()
    for call in (lambda: est.assign(["a"]), lambda: est.kmedoids(["a"])):
        with pytest.raises(RuntimeError, match="released"):
            call()
    assert not ops.live


# ---- the reference on the suite's own graph -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_matrices():
    from oracle import simrank_oracle as O
    df = synth.powerlaw_directed(300, 4.0, seed=11)
    return {"SimRank": O.fit_simrank(df, verbose=False)["S"], "SimRankPP": O.fit_simrank_pp(df, verbose=False)["S"]}


@pytest.mark.parametrize("k", [5, 12, 40])
@pytest.mark.parametrize("which", ["SimRank", "SimRankPP"])
def test_the_alternation_converges_and_its_objective_never_falls(oracle_matrices, which, k):
    S = np.asarray(oracle_matrices[which], dtype=np.float64)
    seeds = np.random.default_rng(5).choice(300, k, replace=False)
    seen = []                                                              # every labelling whose own was asked for

    def own_of(lab):
        seen.append(np.array(lab))
        return GR.quality_fast(S, lab)[0]
    cluster, medoids, sim, sizes, cohesion, history = KR.kmedoids(S, seeds, 20, own_of)
    assert len(history) <= 20 and history[-1][1] == 0                      # converged (the prototype took 3 to 4 iterations)
    assert history[0][0] == 300 and history[0][1] > 0 and len(history) >= 2
    assert sizes.sum() == 300 and sizes.min() >= 1 and (cluster[medoids] == np.arange(k)).all()
    assert same(sim, S[medoids[cluster], np.arange(300)])
    # The objective is a sum over the clusters of (size - 1) means, each within the bound of a float64 sum in any order of
    # its exact value (groups_ref.bound, which covers quality_fast's order of additions); in exact arithmetic it never
    # falls, so two consecutive ones differ by no more than both their bounds
    tol = []
    for lab, (_, _, _) in zip(seen, history):
        B = GR.bound(S, lab)
        tol.append(math.fsum(B[:, j][lab == j].max() * ((lab == j).sum() - 1) for j in range(k)))
    obj = [h[2] for h in history]
    for i in range(1, len(obj)):
        assert obj[i] >= obj[i - 1] - (tol[i] + tol[i - 1]), (i, obj, tol)
    assert obj[-1] > obj[0]


def test_simultaneous_relocation_oscillates_where_the_alternation_converges():
    """The loop this project does NOT ship: every node moves to ``nearest`` when ``other > own``, all at once.  On this
    matrix with the clusters {0, 1} and {2, 3} the nodes 1 and 2 swap for ever (period 2)."""
    S = np.eye(4)
    S[1, 0] = S[2, 3] = 0.125
    S[1, 2] = S[2, 1] = 0.5
    lab = np.array([0, 0, 1, 1])
    seen = [lab]
    for _ in range(6):
        own, nearest, other = GR.quality(S, seen[-1])
        with np.errstate(invalid="ignore"):
            seen.append(np.where(other > own, nearest, seen[-1]))
    assert [s.tolist() for s in seen] == [[0, 0, 1, 1], [0, 1, 0, 1]] * 3 + [[0, 0, 1, 1]]
    cluster, medoids, sim, sizes, cohesion, history = KR.kmedoids(S, [0, 3], 20, lambda l: GR.quality(S, l)[0])
    assert [h[:2] for h in history] == [(4, 1), (0, 0)]                    # converged in two iterations
    assert cluster.tolist() == [0, 0, 0, 1] and medoids.tolist() == [1, 3] and sim.tolist() == [0.125, 1.0, 0.5, 1.0]
    assert cohesion[0] == 0.3125 and math.isnan(cohesion[1]) and history[-1][2] == 0.625
