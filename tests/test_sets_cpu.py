"""libsimrank_sets.so (include/simrank_sets.h), ``score_sets`` and ``recommend`` on a machine without a GPU: header,
binding and exports agree, the header is plain C99 and stands alone, the NumPy statement (tests/sets_ref.py) gives the
frames written out here on a hand-made case and is the reference's ``W @ S`` row by row, and every argument check runs
before any device work."""
import re

import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

import simrank_amd.SimRank as SRA
from simrank_amd import _lib, _query, _sets
from tests import companion_abi as A
from tests import foldin_ref as F
from tests import sets_ref as R
from tests.conftest import Golden


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_sets) == _sets.VERSION == 1
    text = A.header(_sets)
    assert re.search(r"#define SIMRANK_SETS_CHUNK %d\b" % _sets.CHUNK, text)
    assert re.search(r"#define SIMRANK_SETS_MAX_BLOCKS \(1 << 24\)", text) and _sets.MAX_BLOCKS == 1 << 24
    assert re.search(r"SIMRANK_SETS_GRID_BASKET_MAJOR = %d\b" % _sets.BASKET_MAJOR, text)
    assert re.search(r"SIMRANK_SETS_GRID_CHUNK_LABEL = %d\b" % _sets.CHUNK_LABEL, text)
    A.assert_header_stands_alone(_sets)


def test_the_layout_codes_are_the_shared_ones():
    assert A.layout_codes(_sets) == A.layout_codes(_query) == {
        "PANEL_F32": _query.PANEL_F32, "ROWMAJOR_F32": _query.ROWMAJOR_F32, "PANEL_F16": _query.PANEL_F16,
        "ROWMAJOR_F64": _query.ROWMAJOR_F64}


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_sets)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_sets)


def test_the_main_library_is_unchanged():
    version, names, exports = A.main_library(_sets)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_a_c_program_links(tmp_path):
    assert "sets 1 ok" in A.run_c99(_sets, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_sets.h"
int main(void) {
    int64_t ptr[2] = {0, 0};
    int32_t one[1] = {0};
    double w[1] = {1.0};
    if (simrank_sets_version() != SIMRANK_SETS_VERSION) return 1;
    /* the band arithmetic: workgroups per call in both grid orders */
    if (simrank_sets_blocks(0, 100, SIMRANK_SETS_GRID_BASKET_MAJOR) != 0) return 2;
    if (simrank_sets_blocks(7, 1100, SIMRANK_SETS_GRID_BASKET_MAJOR) != 14) return 3;
    if (simrank_sets_blocks(7, 1100, SIMRANK_SETS_GRID_CHUNK_LABEL) != 16) return 4;     /* 2 chunks x 4 labels */
    if (simrank_sets_blocks(7, 3 * 1024, SIMRANK_SETS_GRID_CHUNK_LABEL) != 32) return 5; /* 3 chunks: 3, 3, 2 labels */
    if (simrank_sets_blocks(5, 9 * 1024 + 1, SIMRANK_SETS_GRID_CHUNK_LABEL) != 80) return 6;  /* 10 chunks: 2 per label */
    if (simrank_sets_blocks(5, 100, 2) != -1 || simrank_sets_blocks(-1, 100, 0) != -1) return 7;
    if (simrank_sets_score(NULL, 9, 8, 4, 4, NULL, 4, ptr, one, w, 1, NULL, NULL, NULL, 4, 0, NULL)
        != SIMRANK_SETS_ERR_INVALID) return 8;                                    /* unknown layout */
    if (!strlen(simrank_sets_last_error())) return 9;
    if (simrank_sets_score(NULL, SIMRANK_SETS_PANEL_F32, 8, 4, 4, NULL, 4, ptr, one, w, 1, NULL, NULL, NULL, 4, 0, NULL)
        != SIMRANK_SETS_ERR_INVALID) return 10;                                   /* S is NULL */
    if (simrank_sets_score(one, SIMRANK_SETS_PANEL_F16, 2, 4, 4, NULL, 4, ptr, one, w, 1, NULL, NULL, NULL, 4, 0, NULL)
        != SIMRANK_SETS_ERR_INVALID) return 11;                                   /* stride below the rows */
    if (simrank_sets_score(one, SIMRANK_SETS_ROWMAJOR_F64, 4, 4, 4, NULL, 5, ptr, one, w, 1, NULL, NULL, NULL, 5, 0, NULL)
        != SIMRANK_SETS_ERR_INVALID) return 12;                                   /* 5 columns of 4 without a map */
    if (simrank_sets_score(one, SIMRANK_SETS_ROWMAJOR_F64, 4, 4, 4, NULL, 4, ptr, one, w, 1, NULL, NULL, NULL, 3, 0, NULL)
        != SIMRANK_SETS_ERR_INVALID) return 13;                                   /* ld_out below the columns */
    if (simrank_sets_score(one, SIMRANK_SETS_ROWMAJOR_F64, 4, 4, 4, NULL, 4, ptr, one, w, 1, ptr, NULL, NULL, 4, 0, NULL)
        != SIMRANK_SETS_ERR_INVALID) return 14;                                   /* excl_ptr without excl_cols */
    if (simrank_sets_score(one, SIMRANK_SETS_ROWMAJOR_F64, 4, 4, 4, NULL, 4, ptr, one, w, 1, NULL, NULL, NULL, 4, 7, NULL)
        != SIMRANK_SETS_ERR_INVALID) return 15;                                   /* unknown grid order */
    if (simrank_sets_score(one, SIMRANK_SETS_ROWMAJOR_F64, 4, 4, 4, NULL, 4, ptr, one, w, 1, NULL, NULL, NULL, 4, 0, NULL)
        != SIMRANK_SETS_ERR_INVALID) return 16;                                   /* out is NULL */
    if (simrank_sets_score(one, SIMRANK_SETS_ROWMAJOR_F32, 2000000000, 4, 2000000000, NULL, 2000000000, ptr, one, w,
                           20000, NULL, NULL, w, 2000000000, 0, NULL) != SIMRANK_SETS_ERR_INVALID) return 17;
    if (!strstr(simrank_sets_last_error(), "bands")) return 18;                   /* too many workgroups: cut into bands */
    if (simrank_sets_score(one, SIMRANK_SETS_ROWMAJOR_F64, 4, 4, 4, NULL, 4, ptr, one, w, 0, NULL, NULL, NULL, 4, 0, NULL)
        != SIMRANK_SETS_OK) return 19;                                            /* nothing asked: no device touched */
    if (simrank_sets_topk(NULL, 4, 1, 4, NULL, 0, one, w, NULL) != SIMRANK_SETS_ERR_INVALID) return 20;   /* k = 0 */
    if (simrank_sets_topk(w, 3, 1, 4, NULL, 1, one, w, NULL) != SIMRANK_SETS_ERR_INVALID) return 21;      /* ld below n_out */
    if (simrank_sets_topk(w, 4, 1, 4, NULL, 1, NULL, w, NULL) != SIMRANK_SETS_ERR_INVALID) return 22;
    if (simrank_sets_topk(NULL, 4, 0, 4, NULL, 1, NULL, NULL, NULL) != SIMRANK_SETS_OK) return 23;
    printf("sets %d ok\n", simrank_sets_version());
    return 0;
}
''')


# ---- the NumPy statement on a hand-made case ---------------------------------------------------------------------------
LABELS = ["a", "b", "c", "d", "e"]
S5 = pd.DataFrame([[1.0, 0.5, 0.0, 0.25, 0.0],
                   [0.5, 1.0, 0.0, 0.0, 0.0],
                   [0.0, 0.0, 1.0, 0.0, 0.0],
                   [0.25, 0.0, 0.0, 1.0, 0.125],
                   [0.0, 0.0, 0.0, 0.125, 1.0]], index=LABELS, columns=LABELS)
SETS = [["a", "b"], [], ["d", "d"], ["b", "a", "e"]]
WEIGHTS = [[1.0, 2.0], [], [0.5, 0.25], [1.0, -1.0, 4.0]]


def test_the_statement_on_a_hand_made_case():
    dense = R.score_sets_ref(S5, SETS, WEIGHTS, names=["p", "q", "r", "s"])
    want = pd.DataFrame([[2.0, 2.5, 0.0, 0.25, 0.0],
                         [0.0, 0.0, 0.0, 0.0, 0.0],
                         [0.1875, 0.0, 0.0, 0.75, 0.09375],
                         [-0.5, 0.5, 0.0, 0.25, 4.0]], index=["p", "q", "r", "s"], columns=LABELS)
    assert_frame_equal(dense, want, check_exact=True)
    plain = R.score_sets_ref(S5, SETS)
    assert list(plain.index) == [0, 1, 2, 3] and plain.values[2].tolist() == [0.5, 0.0, 0.0, 2.0, 0.25]
    # the k best outside the members; ties (the zeros) by position; fewer candidates than k give fewer rows
    top = R.score_sets_ref(S5, SETS, WEIGHTS, top_k=3)
    assert_frame_equal(top, pd.DataFrame({
        "set": [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3],
        "rank": [1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2],
        "neighbor": ["d", "c", "e", "a", "b", "c", "a", "e", "b", "d", "c"],
        "score": [0.25, 0.0, 0.0, 0.0, 0.0, 0.0, 0.1875, 0.09375, 0.0, 0.25, 0.0]}), check_exact=True)
    # no exclusion: the members compete; a negative score ranks below the zeros
    top = R.score_sets_ref(S5, SETS, WEIGHTS, top_k=5, exclude=None, names=["p", "q", "r", "s"])
    assert top[top["set"] == "s"]["neighbor"].tolist() == ["e", "b", "d", "c", "a"]
    assert top[top["set"] == "s"]["score"].tolist() == [4.0, 0.5, 0.25, 0.0, -0.5]
    assert top[top["set"] == "q"]["neighbor"].tolist() == LABELS
    # labels to exclude per basket instead of the members
    top = R.score_sets_ref(S5, SETS, WEIGHTS, top_k=2, exclude=[["b"], LABELS, [], ["e", "b"]])
    assert top["set"].tolist() == [0, 0, 2, 2, 3, 3] and top["neighbor"].tolist() == ["a", "d", "d", "a", "d", "c"]
    # recommend on the directed graph c -> a, d -> a, a -> b, e -> d (rows = in-neighbours), scale 1 / in-degree
    rowptr, col, scale = np.array([0, 2, 3, 3, 4, 4]), np.array([2, 3, 0, 4]), np.array([0.5, 1.0, 0.0, 1.0, 0.0])
    rec = R.recommend_ref(S5, LABELS, rowptr, col, scale, ["d", "c", "a"], 2, also_self=True)
    assert_frame_equal(rec, pd.DataFrame({"node": ["d", "d", "a", "a"], "rank": [1, 2, 1, 2],
                                          "neighbor": ["a", "b", "e", "b"], "score": [0.0, 0.0, 0.0625, 0.0]}),
                       check_exact=True)
    rec = R.recommend_ref(S5, LABELS, rowptr, col, scale, ["a"], 9, exclude_seen=False, also_self=True)
    assert rec["neighbor"].tolist() == ["c", "d", "a", "e", "b"] and rec["score"].tolist() == [0.5, 0.5, 0.125, 0.0625, 0.0]


# the largest relative difference between the sequential statement and the BLAS product W @ S observed on these two cases
# (relative to the row's largest entry; x86-64, NumPy's bundled OpenBLAS): 2.25e-16 on BipartiteSimRankPP_b40, 1.32e-16 on
# SimRankPP_er64 -> 4 x the larger one
W_AT_S_RTOL = 4 * 2.25e-16


@pytest.mark.parametrize("name", ["BipartiteSimRankPP_b40", "SimRankPP_er64"])
def test_recommends_statement_is_the_references_w_times_s(name):
    """``recommend``'s score row of u is ``(W @ S)[u]``, W and S the reference's own: leg 1 of its update.  ``W @ S`` is
    one BLAS sum in another order than the sequential loop: that order is the only slack."""
    g = Golden(name)
    r = F.run_oracle(g)
    worst = 0.0
    for sd in F.sides_of(g, r):
        W, S = np.asarray(sd["W"], dtype=np.float64), np.asarray(r[sd["reads"]], dtype=np.float64)
        lists = [np.nonzero(W[u])[0] for u in range(W.shape[0])]
        weights = [W[u, l] for u, l in enumerate(lists)]
        for u, l in enumerate(lists):                 # (every entry of a row of W is the row's one scale)
            assert l.size == 0 or np.all(weights[u] == weights[u][0])
        got, want = R.scores(S, lists, weights), W @ S
        scale = np.abs(want).max(axis=1, keepdims=True)
        scale[scale == 0] = 1.0
        worst = max(worst, float((np.abs(got - want) / scale).max()))
    print("largest relative difference to W @ S:", worst)
    assert worst <= W_AT_S_RTOL


# ---- argument checks: no device --------------------------------------------------------------------------------------
INDEX = pd.Index(["a", "b", "c", "d"])


def test_prepare_normalises_the_baskets():
    ptr, ids, w, names, k, excl = _sets.prepare([["c", "a", "c"], [], ["d"]], INDEX)
    assert ptr.tolist() == [0, 3, 3, 4] and ids.tolist() == [2, 0, 2, 3] and w.tolist() == [1.0] * 4
    assert ptr.dtype == np.int64 and ids.dtype == np.int32 and w.dtype == np.float64
    assert names is None and k is None and excl is None
    ptr, ids, w, names, k, excl = _sets.prepare([["a"], ["b", "c"]], INDEX, weights=[[2], [0.5, -1e6]], names=("x", "y"),
                                                top_k=9)
    assert w.tolist() == [2.0, 0.5, -1e6] and names == ["x", "y"] and k == 4          # k clamped to N
    assert excl[0].tolist() == [0, 1, 3] and excl[1].tolist() == [0, 1, 2]            # the members
    *_, excl = _sets.prepare([["a"], ["b"]], INDEX, top_k=1, exclude=None)
    assert excl is None
    *_, excl = _sets.prepare([["a"], ["b"]], INDEX, top_k=1, exclude=[["d", "a"], []])
    assert excl[0].tolist() == [0, 2, 2] and excl[1].tolist() == [3, 0]
    assert _sets.prepare([], INDEX)[0].tolist() == [0]
    assert _sets.prepare([[7, 5]], pd.Index([5, 6, 7]))[1].tolist() == [2, 0]
    # recommend's baskets: the CSR rows in their order, the row's scale per member, u itself excluded when asked
    class Csr:
        rowptr, col = np.array([0, 2, 2, 3], dtype=np.int32), np.array([2, 0, 1], dtype=np.int32)
    ptr, ids, w, excl = _sets.csr_baskets(Csr, np.array([0.5, 0.0, 3.0]), [2, 0, 1], True, True)
    assert ptr.tolist() == [0, 1, 3, 3] and ids.tolist() == [1, 2, 0] and w.tolist() == [3.0, 0.5, 0.5]
    assert excl[0].tolist() == [0, 2, 5, 6] and excl[1].tolist() == [1, 2, 2, 0, 0, 1]
    *_, excl = _sets.csr_baskets(Csr, np.array([0.5, 0.0, 3.0]), [2, 0], False, True)
    assert excl[1].tolist() == [1, 2, 0]
    assert _sets.csr_baskets(Csr, np.array([0.5, 0.0, 3.0]), [2, 0], True, False)[3] is None
    # the excluded caller ids as the output columns of a block that holds the callers 1, 4, 6
    bp, bc = _sets._block_exclusions((np.array([0, 3, 3, 5]), np.array([6, 0, 1, 4, 9], dtype=np.int32)),
                                     np.array([1, 4, 6], dtype=np.int32), False)
    assert bp.tolist() == [0, 2, 2, 3] and bc.tolist() == [2, 0, 1]


def test_argument_errors_need_no_device():
    with pytest.raises(KeyError, match="zz"):
        _sets.prepare([["a"], ["b", "zz"]], INDEX)
    with pytest.raises(KeyError, match="zz"):
        _sets.prepare([["a"]], INDEX, top_k=1, exclude=[["zz"]])
    with pytest.raises(ValueError, match="one sequence of labels per basket"):
        _sets.prepare("ab", INDEX)
    with pytest.raises(ValueError, match="sequence of labels"):
        _sets.prepare(["ab"], INDEX)
    with pytest.raises(ValueError, match="sequence of labels"):
        _sets.prepare([3], INDEX)
    with pytest.raises(ValueError, match=r"one sequence per basket \(2\)"):
        _sets.prepare([["a"], ["b"]], INDEX, weights=[[1.0]])
    with pytest.raises(ValueError, match=r"weights\[1\] has 2 entries for 1 members"):
        _sets.prepare([["a"], ["b"]], INDEX, weights=[[1.0], [1.0, 2.0]])
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match=r"weights\[0\] holds a value that is not finite"):
            _sets.prepare([["a", "b"]], INDEX, weights=[[1.0, bad]])
    with pytest.raises(ValueError, match="sequence of floats"):
        _sets.prepare([["a"]], INDEX, weights=[["x"]])
    with pytest.raises(ValueError, match="names must have one entry per basket"):
        _sets.prepare([["a"]], INDEX, names=["x", "y"])
    for bad in ("nobody", 3, [["a"], ["b"]], ["a"]):
        with pytest.raises(ValueError, match="exclude|sequence of labels"):
            _sets.prepare([["a"]], INDEX, top_k=1, exclude=bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="k must be a positive integer"):
            _sets.prepare([["a"]], INDEX, top_k=bad)


class _Csr:
    rowptr, col = np.array([0, 2, 2, 3], dtype=np.int32), np.array([2, 0, 1], dtype=np.int32)


class _Spec:
    csr, rowscale = _Csr, np.array([0.5, 0.0, 1.0])


class _FakeSolver:
    """Stands in for a kept solver: what the argument checks reach is never the device."""
    released = 0

    def __init__(self, n_sides=1):
        self.specs, self.calls = [_Spec] * n_sides, []

    def release(self):
        self.released += 1

    def score_sets(self, j, ptr, ids, w, k=None, excl=None):
        self.calls.append((j, ptr.tolist(), ids.tolist(), w.tolist(), k, None if excl is None else excl[1].tolist()))
        n_sets = ptr.size - 1
        if k is None:
            return np.arange(n_sets * 3, dtype=np.float64).reshape(n_sets, 3)
        idx = np.tile(np.arange(k, dtype=np.int32), (n_sets, 1))
        idx[:, -1] = -1                                     # (one empty slot per basket)
        return idx, np.ones((n_sets, k))


def test_checks_on_the_estimator_need_no_device():
    est = SRA.SimRank()
    for call in (lambda: est.score_sets([["a"]]), lambda: est.recommend(["a"], 1)):
        with pytest.raises(RuntimeError, match="no kept model"):
            call()
    solver = _FakeSolver()
    est._keep(solver, [(0, ["a", "b", "c"])])
    got = est.score_sets([["c", "a"], []], names=["x", "y"])
    assert list(got.index) == ["x", "y"] and list(got.columns) == ["a", "b", "c"] and got.values.dtype == np.float64
    assert solver.calls[-1] == (0, [0, 2, 2], [2, 0], [1.0, 1.0], None, None)
    assert list(est.score_sets([["a"]], group=1).index) == [0]
    top = est.score_sets([["a"], ["b", "b"]], top_k=2, names=["x", "y"])
    assert list(top.columns) == ["set", "rank", "neighbor", "score"]
    assert top["set"].tolist() == ["x", "y"] and top["neighbor"].tolist() == ["a", "a"] and top["rank"].tolist() == [1, 1]
    assert solver.calls[-1][4:] == (2, [0, 1, 1])
    est.score_sets([["a"]], top_k=7, exclude=None)
    assert solver.calls[-1][4:] == (3, None)                # k clamped to N
    rec = est.recommend(["c", "b", "a"], 2)
    assert list(rec.columns) == ["node", "rank", "neighbor", "score"]
    assert rec["node"].tolist() == ["c", "a"]               # b has no in-neighbours: no rows
    assert solver.calls[-1] == (0, [0, 1, 1, 3], [1, 2, 0], [1.0, 0.5, 0.5], 2, [1, 2, 1, 2, 0, 0])
    est.recommend(["a"], 1, exclude_seen=False)
    assert solver.calls[-1][5] is None
    n_calls = len(solver.calls)
    with pytest.raises(KeyError, match="zz"):
        est.score_sets([["zz"]])
    with pytest.raises(KeyError, match="zz"):
        est.recommend(["zz"], 1)
    with pytest.raises(ValueError, match="not finite"):
        est.score_sets([["a"]], weights=[[np.nan]])
    with pytest.raises(ValueError, match="has 2 entries for 1"):
        est.score_sets([["a"]], weights=[[1.0, 2.0]])
    with pytest.raises(ValueError, match="exclude must be"):
        est.score_sets([["a"]], top_k=1, exclude="seen")
    with pytest.raises(ValueError, match="exclude_seen must be True or False"):
        est.recommend(["a"], 1, exclude_seen="yes")
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError, match="k must be a positive integer"):
            est.score_sets([["a"]], top_k=bad)
        with pytest.raises(ValueError, match="k must be a positive integer"):
            est.recommend(["a"], bad)
    for call in (lambda: est.score_sets([["a"]], group=2), lambda: est.recommend(["a"], 1, group=2)):
        with pytest.raises(ValueError, match="one node group"):
            call()
    assert len(solver.calls) == n_calls
    est.release()
    for call in (lambda: est.score_sets([["a"]]), lambda: est.recommend(["a"], 1)):
        with pytest.raises(RuntimeError, match="released"):
            call()
    assert len(solver.calls) == n_calls
    # bipartite: score_sets stays inside its group; recommend(group=1) reads group 2's matrix and answers group-2 labels
    two = SRA.BipartiteSimRankPP()
    fake = _FakeSolver(2)
    two._keep(fake, [(0, [1, 2, 3]), (1, ["x", "y", "z"])])
    for call in (lambda: two.score_sets([[1]]), lambda: two.recommend([1], 1)):
        with pytest.raises(ValueError, match="group must be 1 or 2"):
            call()
    assert list(two.score_sets([["y"]], group=2).columns) == ["x", "y", "z"] and fake.calls[-1][0] == 1
    with pytest.raises(KeyError):
        two.score_sets([["y"]], group=1)
    rec = two.recommend([3, 1], 2, group=1)
    assert fake.calls[-1] == (1, [0, 1, 3], [1, 2, 0], [1.0, 0.5, 0.5], 2, [1, 2, 0])      # (u itself is of the other group)
    assert rec["node"].tolist() == [3, 1] and rec["neighbor"].tolist() == ["x", "x"]
    rec = two.recommend(["z"], 1, group=2)
    assert fake.calls[-1][0] == 0 and rec["neighbor"].tolist() == []
    with pytest.raises(KeyError):
        two.recommend(["x"], 1, group=1)
