"""libsimrank_rank.so (include/simrank_rank.h), ``rank_sets``, ``rank_recommended`` and ``evaluate`` on a machine without a
GPU: header, binding and exports agree, the header is plain C99 and stands alone, the NumPy statement (tests/rank_ref.py)
gives the ranks written out here on a hand-made case and names, for every candidate target, the row of
``sets_ref.best`` it claims, and every argument check runs before any device work."""
import re

import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

import simrank_amd.SimRank as SRA
from simrank_amd import _lib, _rank, _sets
from tests import companion_abi as A
from tests import rank_ref as K
from tests import sets_ref as R


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_rank) == _rank.VERSION == 1
    text = A.header(_rank)
    assert re.search(r"#define SIMRANK_RANK_CHUNK %d\b" % _rank.CHUNK, text) and _rank.CHUNK == _sets.CHUNK
    assert re.search(r"#define SIMRANK_RANK_TILE %d\b" % _rank.TILE, text)
    assert re.search(r"#define SIMRANK_RANK_MAX_BLOCKS \(1 << 24\)", text) and _rank.MAX_BLOCKS == 1 << 24
    assert re.search(r"SIMRANK_RANK_ERR_INVALID = -1\b", text) and re.search(r"SIMRANK_RANK_ERR_HIP = -2\b", text)
    A.assert_header_stands_alone(_rank)


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_rank)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_rank)


def test_the_main_library_is_unchanged():
    version, names, exports = A.main_library(_rank)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_a_c_program_links(tmp_path):
    assert "rank 1 ok" in A.run_c99(_rank, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_rank.h"
int main(void) {
    int64_t ptr[2] = {0, 1};
    int32_t one[1] = {0};
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t n[1] = {0};
    if (simrank_rank_version() != SIMRANK_RANK_VERSION) return 1;
    if (SIMRANK_RANK_CHUNK != 1024 || SIMRANK_RANK_TILE != 256) return 2;
    if (simrank_rank_blocks(0, 100) != 0 || simrank_rank_blocks(7, 0) != 0) return 3;
    if (simrank_rank_blocks(7, 1024) != 7 || simrank_rank_blocks(7, 1025) != 14) return 4;
    if (simrank_rank_blocks(-1, 100) != -1 || simrank_rank_blocks(1, -1) != -1) return 5;
    /* a NULL band with a nonzero shape */
    if (simrank_rank_gather(NULL, 4, 1, 4, ptr, one, v, NULL) != SIMRANK_RANK_ERR_INVALID) return 6;
    if (!strstr(simrank_rank_last_error(), "band is NULL")) return 7;
    if (simrank_rank_count(NULL, 4, 1, 4, NULL, ptr, v, one, n, n, NULL) != SIMRANK_RANK_ERR_INVALID) return 8;
    /* ld_band below n_out */
    if (simrank_rank_gather(v, 3, 1, 4, ptr, one, v, NULL) != SIMRANK_RANK_ERR_INVALID) return 9;
    if (simrank_rank_count(v, 3, 1, 4, NULL, ptr, v, one, n, n, NULL) != SIMRANK_RANK_ERR_INVALID) return 10;
    if (!strstr(simrank_rank_last_error(), "bad band shape")) return 11;
    /* negative shapes, NULL offsets, NULL counters */
    if (simrank_rank_count(v, 4, -1, 4, NULL, ptr, v, one, n, n, NULL) != SIMRANK_RANK_ERR_INVALID) return 12;
    if (simrank_rank_gather(v, 4, 1, 4, NULL, one, v, NULL) != SIMRANK_RANK_ERR_INVALID) return 13;
    if (simrank_rank_count(v, 4, 1, 4, NULL, NULL, v, one, n, n, NULL) != SIMRANK_RANK_ERR_INVALID) return 14;
    if (simrank_rank_count(v, 4, 1, 4, NULL, ptr, v, one, n, NULL, NULL) != SIMRANK_RANK_ERR_INVALID) return 15;
    /* too many workgroups for one call: cut into bands */
    if (simrank_rank_count(v, 2000000000, 20000, 2000000000, NULL, ptr, v, one, n, n, NULL)
        != SIMRANK_RANK_ERR_INVALID) return 16;
    if (!strstr(simrank_rank_last_error(), "bands")) return 17;
    /* nothing asked: no device touched */
    if (simrank_rank_gather(NULL, 4, 0, 4, NULL, NULL, NULL, NULL) != SIMRANK_RANK_OK) return 18;
    if (simrank_rank_count(NULL, 0, 3, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != SIMRANK_RANK_OK) return 19;
    printf("rank %d ok\n", simrank_rank_version());
    return 0;
}
''')


# ---- the NumPy statement on a hand-made case ---------------------------------------------------------------------------
def test_the_statement_on_six_columns_with_ties():
    """0.5 twice (one of them excluded), -0.0 and +0.0 tie and go by position, NaN is no candidate."""
    labels = list("abcdef")
    row = np.array([[0.5, -0.0, np.nan, 0.0, 0.5, 0.25]])
    band = K.excluded_rows(row, [[4]])
    assert np.signbit(row[0, 1]) and band[0, 4] == -np.inf and row[0, 4] == 0.5          # (a copy; -0.0 is really -0.0)
    targets = [[0, 1, 2, 3, 4, 5, 3]]                                                    # every column, and d again
    got = K.long_frame("set", pd.RangeIndex(1), labels, band, targets)
    assert list(got.columns) == ["set", "target", "score", "rank", "candidates"]
    assert got["target"].tolist() == list("abcdef") + ["d"]
    assert got["rank"].tolist() == [1, 3, 0, 4, 0, 2, 4] and got["rank"].dtype == np.int64
    assert got["candidates"].tolist() == [4] * 7 and got["candidates"].dtype == np.int64
    assert np.array_equal(got["score"].to_numpy().view(np.uint64),
                          np.array([0.5, -0.0, np.nan, 0.0, -np.inf, 0.25, 0.0]).view(np.uint64))
    # every candidate target is the row of the top-k statement that its rank names
    order, values = R.best(row[0], 6, excluded=[4])
    assert order.tolist() == [0, 5, 1, 3] and len(order) == got["candidates"][0]
    for t, rank in zip(targets[0], got["rank"]):
        if rank:
            assert order[rank - 1] == t
    # the pieces: before and candidates of single targets, with ids that are not the positions
    ids = np.array([50, 40, 30, 20, 10, 0])
    assert K.count(band[0], ids, 0.0, 20) == (2, 4)          # 0.5 and 0.25; -0.0 ties but its id 40 is no smaller
    assert K.count(band[0], ids, -0.0, 40) == (3, 4)         # ... while +0.0's id 20 precedes 40
    assert K.count(band[0], ids, np.nan, 30) == (0, 4) and K.count(band[0], ids, -np.inf, 10) == (4, 4)
    assert K.rank_of(np.nan, 0) == 0 and K.rank_of(-np.inf, 4) == 0 and K.rank_of(0.0, 2) == 3


LABELS = ["a", "b", "c", "d", "e"]
S5 = pd.DataFrame([[1.0, 0.5, 0.0, 0.25, 0.0],
                   [0.5, 1.0, 0.0, 0.0, 0.0],
                   [0.0, 0.0, 1.0, 0.0, 0.0],
                   [0.25, 0.0, 0.0, 1.0, 0.125],
                   [0.0, 0.0, 0.0, 0.125, 1.0]], index=LABELS, columns=LABELS)
SETS = [["a", "b"], [], ["d", "d"], ["b", "a", "e"]]
WEIGHTS = [[1.0, 2.0], [], [0.5, 0.25], [1.0, -1.0, 4.0]]
TARGETS = [["e", "a", "d", "e"], ["c"], [], ["a", "c"]]


def test_the_statement_is_the_row_of_the_top_k_frame():
    got = K.rank_sets_ref(S5, SETS, TARGETS, WEIGHTS, names=["p", "q", "r", "s"])
    want = pd.DataFrame({"set": ["p", "p", "p", "p", "q", "s", "s"], "target": ["e", "a", "d", "e", "c", "a", "c"],
                         "score": [0.0, -np.inf, 0.25, 0.0, 0.0, -np.inf, 0.0], "rank": [3, 0, 1, 3, 3, 0, 2],
                         "candidates": [3, 3, 3, 3, 5, 2, 2]})
    assert_frame_equal(got, want, check_exact=True)
    # without exclusion the members compete: basket p scores (2, 2.5, 0, 0.25, 0), basket s (-0.5, 0.5, 0, 0.25, 4)
    got = K.rank_sets_ref(S5, SETS, TARGETS, WEIGHTS, exclude=None)
    assert got["rank"].tolist() == [5, 2, 3, 5, 3, 5, 4] and got["candidates"].tolist() == [5] * 7
    for exclude in ("members", None, [["b"], LABELS, [], ["e", "b"]]):
        ranks = K.rank_sets_ref(S5, SETS, TARGETS, WEIGHTS, exclude=exclude)
        top = R.score_sets_ref(S5, SETS, WEIGHTS, top_k=5, exclude=exclude)
        for _, r in ranks.iterrows():
            rows = top[top["set"] == r["set"]].reset_index(drop=True)
            assert r["candidates"] == len(rows)
            if r["rank"]:
                assert rows["neighbor"][r["rank"] - 1] == r["target"] and rows["score"][r["rank"] - 1] == r["score"]
            else:
                assert r["target"] not in set(rows["neighbor"]) and r["score"] == -np.inf
    # recommend's baskets on the directed graph c -> a, d -> a, a -> b, e -> d; evaluate from the ranks
    rowptr, col, scale = np.array([0, 2, 3, 3, 4, 4]), np.array([2, 3, 0, 4]), np.array([0.5, 1.0, 0.0, 1.0, 0.0])
    nodes, targets = ["a", "c", "d"], [["e", "b", "c"], ["a"], ["a", "e"]]
    long = K.rank_recommended_ref(S5, LABELS, rowptr, col, scale, nodes, targets, also_self=True)
    assert long["rank"].tolist() == [1, 2, 0, 0, 1, 0] and long["candidates"].tolist() == [2, 2, 2, 0, 3, 3]
    assert long["score"].tolist() == [0.0625, 0.0, -np.inf, 0.0, 0.0, -np.inf]
    ev = K.evaluate_ref(long, nodes, targets, (1, 2))
    assert_frame_equal(ev, pd.DataFrame({"node": nodes, "targets": [3, 1, 2], "not_candidates": [1, 1, 1],
                                         "best_rank": [1, 0, 1], "reciprocal_rank": [1.0, 0.0, 1.0],
                                         "hits@1": [1, 0, 1], "hits@2": [2, 0, 1]}), check_exact=True)


# ---- argument checks: no device --------------------------------------------------------------------------------------
INDEX = pd.Index(["a", "b", "c", "d"])


def test_prepare_normalises_the_targets():
    tptr, tids = _rank.prepare([["c", "a", "c"], [], ["d"]], INDEX, 3)
    assert tptr.tolist() == [0, 3, 3, 4] and tids.tolist() == [2, 0, 2, 3]               # repeats kept, empty allowed
    assert tptr.dtype == np.int64 and tids.dtype == np.int32
    assert _rank.prepare([], INDEX, 0)[0].tolist() == [0]
    assert _rank.prepare([[7, 5]], pd.Index([5, 6, 7]), 1)[1].tolist() == [2, 0]
    assert _rank.check_ks((10,)) == [10] and _rank.check_ks([3, 1, 3]) == [3, 1, 3]
    assert _rank.ranks_of(np.array([0.5, -np.inf, np.nan, -0.0]), np.array([0, 7, 0, 2])).tolist() == [1, 0, 0, 3]
    # the targets as columns of a block that holds the callers 1, 4, 6; of a block that holds them all; of an empty one
    ids = np.array([6, 0, 1, 4, 9], dtype=np.int32)
    assert _rank.block_columns(ids, np.array([1, 4, 6], dtype=np.int32), False).tolist() == [2, -1, 0, 1, -1]
    assert _rank.block_columns(ids, np.arange(10, dtype=np.int32), True).tolist() == ids.tolist()
    assert _rank.block_columns(ids, np.empty(0, dtype=np.int32), False).tolist() == [-1] * 5


def test_argument_errors_need_no_device():
    with pytest.raises(KeyError, match="zz"):
        _rank.prepare([["a"], ["b", "zz"]], INDEX, 2)
    with pytest.raises(ValueError, match=r"one sequence of labels per basket \(2\), not 1"):
        _rank.prepare([["a"]], INDEX, 2)
    with pytest.raises(ValueError, match="one sequence of labels per basket"):
        _rank.prepare("ab", INDEX, 2)
    with pytest.raises(ValueError, match="one sequence of labels per basket"):
        _rank.prepare(None, INDEX, 0)
    with pytest.raises(ValueError, match="sequence of labels"):
        _rank.prepare(["ab"], INDEX, 1)
    with pytest.raises(ValueError, match="sequence of labels"):
        _rank.prepare([3], INDEX, 1)
    for bad in ((), [], "10", 10, None, (0,), (10, -1), (2.5,), (True,)):
        with pytest.raises(ValueError, match="positive integer"):
            _rank.check_ks(bad)


class _Csr:
    rowptr, col = np.array([0, 2, 2, 3], dtype=np.int32), np.array([2, 0, 1], dtype=np.int32)


class _Spec:
    csr, rowscale = _Csr, np.array([0.5, 0.0, 1.0])


class _FakeSolver:
    """Stands in for a kept solver: what the argument checks reach is never the device."""

    def __init__(self, n_sides=1):
        self.specs, self.calls = [_Spec] * n_sides, []

    def release(self):
        pass

    def score_ranks(self, j, ptr, ids, w, excl, tptr, tids):
        self.calls.append((j, ptr.tolist(), ids.tolist(), w.tolist(), None if excl is None else excl[1].tolist(),
                           tptr.tolist(), tids.tolist()))
        score = np.where(np.arange(tids.size) % 2 == 0, 0.5, -np.inf)
        return score, np.arange(tids.size, dtype=np.int64), np.full(ptr.size - 1, 3, dtype=np.int64)


def test_checks_on_the_estimator_need_no_device():
    est = SRA.SimRank()
    for call in (lambda: est.rank_sets([["a"]], [["a"]]), lambda: est.rank_recommended(["a"], [["a"]]),
                 lambda: est.evaluate(["a"], [["a"]])):
        with pytest.raises(RuntimeError, match="no kept model"):
            call()
    solver = _FakeSolver()
    est._keep(solver, [(0, ["a", "b", "c"])])
    got = est.rank_sets([["c", "a"], []], [["b", "b", "c"], ["a"]], names=["x", "y"])
    assert list(got.columns) == ["set", "target", "score", "rank", "candidates"]
    assert got["set"].tolist() == ["x", "x", "x", "y"] and got["target"].tolist() == ["b", "b", "c", "a"]
    assert got["rank"].tolist() == [1, 0, 3, 0] and got["candidates"].tolist() == [3] * 4
    assert got["rank"].dtype == np.int64 and got["candidates"].dtype == np.int64 and got["score"].dtype == np.float64
    assert solver.calls[-1] == (0, [0, 2, 2], [2, 0], [1.0, 1.0], [2, 0], [0, 3, 4], [1, 1, 2, 0])
    est.rank_sets([["a"]], [[]], exclude=None)
    assert solver.calls[-1][4] is None and solver.calls[-1][5:] == ([0, 0], [])
    est.rank_sets([["a"]], [["b"]], exclude=[["c", "b"]])
    assert solver.calls[-1][4] == [2, 1]
    rec = est.rank_recommended(["c", "b", "a"], [["a"], ["a", "c"], []])
    assert list(rec.columns) == ["node", "target", "score", "rank", "candidates"]
    assert solver.calls[-1] == (0, [0, 1, 1, 3], [1, 2, 0], [1.0, 0.5, 0.5], [1, 2, 1, 2, 0, 0], [0, 1, 3, 3], [0, 0, 2])
    assert rec["node"].tolist() == ["c", "b", "b"] and rec["rank"].tolist() == [1, 0, 0]     # b has no in-neighbours
    assert rec["candidates"].tolist() == [3, 0, 0]
    ev = est.evaluate(["c", "b", "a"], [["a"], ["a", "c"], []], ks=(1, 5))
    assert list(ev.columns) == ["node", "targets", "not_candidates", "best_rank", "reciprocal_rank", "hits@1", "hits@5"]
    assert ev["node"].tolist() == ["c", "b", "a"] and ev["targets"].tolist() == [1, 2, 0]
    assert ev["not_candidates"].tolist() == [0, 2, 0] and ev["best_rank"].tolist() == [1, 0, 0]
    assert ev["reciprocal_rank"].tolist() == [1.0, 0.0, 0.0] and ev["hits@1"].tolist() == [1, 0, 0]
    n_calls = len(solver.calls)
    with pytest.raises(KeyError, match="zz"):
        est.rank_sets([["a"]], [["zz"]])
    with pytest.raises(KeyError, match="zz"):
        est.rank_sets([["zz"]], [["a"]])
    with pytest.raises(KeyError, match="zz"):
        est.rank_recommended(["a"], [["zz"]])
    with pytest.raises(ValueError, match=r"per basket \(1\), not 2"):
        est.rank_sets([["a"]], [["a"], ["b"]])
    with pytest.raises(ValueError, match=r"per basket \(2\), not 1"):
        est.rank_recommended(["a", "b"], [["a"]])
    with pytest.raises(ValueError, match="not finite"):
        est.rank_sets([["a"]], [["a"]], weights=[[np.nan]])
    with pytest.raises(ValueError, match="exclude must be"):
        est.rank_sets([["a"]], [["a"]], exclude="seen")
    with pytest.raises(ValueError, match="exclude_seen must be True or False"):
        est.rank_recommended(["a"], [["a"]], exclude_seen="yes")
    for bad in ((), (0,), 10, (1.5,), (True,)):
        with pytest.raises(ValueError, match="positive integer"):
            est.evaluate(["a"], [["a"]], ks=bad)
    for call in (lambda: est.rank_sets([["a"]], [["a"]], group=2), lambda: est.evaluate(["a"], [["a"]], group=2)):
        with pytest.raises(ValueError, match="one node group"):
            call()
    assert len(solver.calls) == n_calls
    est.release()
    for call in (lambda: est.rank_sets([["a"]], [["a"]]), lambda: est.rank_recommended(["a"], [["a"]]),
                 lambda: est.evaluate(["a"], [["a"]])):
        with pytest.raises(RuntimeError, match="released"):
            call()
    # bipartite: rank_recommended(group=1) reads group 2's matrix, and its targets are group-2 labels
    two = SRA.BipartiteSimRankPP()
    fake = _FakeSolver(2)
    two._keep(fake, [(0, [1, 2, 3]), (1, ["x", "y", "z"])])
    with pytest.raises(ValueError, match="group must be 1 or 2"):
        two.rank_sets([[1]], [[1]])
    rec = two.rank_recommended([3, 1], [["z"], ["x", "y"]], group=1)
    assert fake.calls[-1] == (1, [0, 1, 3], [1, 2, 0], [1.0, 0.5, 0.5], [1, 2, 0], [0, 1, 3], [2, 0, 1])
    assert rec["node"].tolist() == [3, 1, 1] and rec["target"].tolist() == ["z", "x", "y"]
    with pytest.raises(KeyError):
        two.rank_recommended([3], [[1]], group=1)
