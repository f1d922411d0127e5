"""libsimrank_candidates.so (include/simrank_candidates.h) and the ``among=`` / ``exclude=`` keywords on a machine without
a GPU: header, binding and exports agree, the header is plain C99 and stands alone, the entry point refuses bad arguments
without a device, ``tests/candidates_ref.py`` is pinned on hand-written cases, ``prepare`` normalises and refuses, the
host path of a pruned model equals the reference on a hand-built P, and every refusal of ``most_similar``,
``score_sets`` and ``recommend`` comes before any device call."""
import re

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _candidates, _diverse, _neighbors, _query, _sets
from tests import candidates_ref as CR
from tests import companion_abi as A
from tests import diverse_ref
from tests.host_doubles import HostOps, RingSpec, boom
from tests.test_cluster_cpu import guarded_estimator
from tests.test_gpu_sets import same_frame


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    assert A.loaded_version(_candidates) == _candidates.VERSION == 1
    text = A.header(_candidates)
    assert re.search(r"#define SIMRANK_CANDIDATES_MAX_K %d\b" % _candidates.MAX_K, text) and _candidates.MAX_K == 4096
    assert re.search(r"#define SIMRANK_CANDIDATES_MAX_BLOCKS \(1 << 16\)", text) and _candidates.MAX_BLOCKS == 1 << 16
    assert "LIST INDEX ascending" in text and "ascending id order" in text      # (the header states the tie rule)
    A.assert_header_stands_alone(_candidates)


def test_the_layout_codes_are_the_shared_ones():
    assert A.layout_codes(_candidates) == A.layout_codes(_query) and len(A.layout_codes(_candidates)) == 4


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_candidates)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_candidates)
    A.main_library(_candidates)


def test_the_staging_cap_is_answered_on_the_host():
    caps = [_candidates.staged(layout) for layout in range(4)]
    assert all(c >= 0 for c in caps) and caps[0] == caps[1] == caps[2]         # (one key width for f32 and binary16)
    assert _candidates.staged(4) == -1 and _candidates.staged(-1) == -1


def test_header_is_c99_and_the_entry_refuses_bad_arguments_without_a_device(tmp_path):
    assert "candidates 1 ok" in A.run_c99(_candidates, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_candidates.h"
#define BAD(call, code) do { if ((call) != SIMRANK_CANDIDATES_ERR_INVALID) return code; \
                             if (!strlen(simrank_candidates_last_error())) return 100 + code; } while (0)
int main(void) {
    int32_t one[1] = {0};
    double w[1] = {1.0};
    const int32_t f32 = SIMRANK_CANDIDATES_ROWMAJOR_F32;
    const int32_t big = SIMRANK_CANDIDATES_MAX_K + 1;
    if (simrank_candidates_version() != SIMRANK_CANDIDATES_VERSION) return 1;
    /* k = 0, k = 4097, an unknown layout, NULL cand_pos with candidates, a stride smaller than the block */
    BAD(simrank_candidates_topk(one, f32, 4, 4, 4, one, one, 1, one, NULL, 1, 0, one, w, NULL), 2);
    BAD(simrank_candidates_topk(one, f32, 4, 4, 4, one, one, 1, one, NULL, 1, big, one, w, NULL), 3);
    if (!strstr(simrank_candidates_last_error(), "4096")) return 4;
    BAD(simrank_candidates_topk(one, 9, 4, 4, 4, one, one, 1, one, NULL, 1, 1, one, w, NULL), 5);
    BAD(simrank_candidates_topk(one, f32, 4, 4, 4, one, one, 1, NULL, NULL, 1, 1, one, w, NULL), 6);
    if (!strstr(simrank_candidates_last_error(), "cand_pos")) return 7;
    BAD(simrank_candidates_topk(one, f32, 3, 4, 4, one, one, 1, one, NULL, 1, 1, one, w, NULL), 8);
    BAD(simrank_candidates_topk(one, SIMRANK_CANDIDATES_PANEL_F16, 2, 4, 4, one, one, 1, one, NULL, 1, 1, one, w, NULL), 9);
    /* NULL block, NULL rows and outputs, negative counts */
    BAD(simrank_candidates_topk(NULL, f32, 4, 4, 4, one, one, 1, one, NULL, 1, 1, one, w, NULL), 10);
    BAD(simrank_candidates_topk(one, f32, 4, 4, 4, NULL, one, 1, one, NULL, 1, 1, one, w, NULL), 11);
    BAD(simrank_candidates_topk(one, f32, 4, 4, 4, one, one, 1, one, NULL, 1, 1, NULL, w, NULL), 12);
    BAD(simrank_candidates_topk(one, f32, 4, 4, 4, one, one, -1, one, NULL, 1, 1, one, w, NULL), 13);
    BAD(simrank_candidates_topk(one, f32, 4, 4, 4, one, one, 1, one, NULL, -1, 1, one, w, NULL), 14);
    /* no queries: OK, nothing launched, whatever else is NULL */
    if (simrank_candidates_topk(one, f32, 4, 4, 4, NULL, NULL, 0, NULL, NULL, 0, 1, NULL, NULL, NULL) != SIMRANK_CANDIDATES_OK)
        return 15;
    if (simrank_candidates_staged(9) != -1 || simrank_candidates_staged(f32) < 0) return 16;
    printf("candidates %d ok\n", simrank_candidates_version());
    return 0;
}
''')


# ---- the reference, pinned ------------------------------------------------------------------------------------------------
def test_ref_topk_on_hand_written_cases():
    A4 = np.array([[0.5, 0.5, 0.5, 0.5, 0.5, 0.5],
                   [-0.0, 0.0, np.nan, -np.inf, 1.0, 0.0],
                   [3.0, 2.0, 1.0, 0.0, -1.0, -2.0]])
    # a row of one repeated value: the first k of the list but the row's own id
    idx, val = CR.ref_topk(A4, [0], [4], [5, 4, 3, 2, 1, 0], [1, 4, 7, 9, 11, 12], 3)
    assert idx.tolist() == [[1, 7, 9]] and val.tolist() == [[0.5, 0.5, 0.5]] and idx.dtype == np.int32
    # without ids the id is the position: the own id 4 is position 4
    idx, _ = CR.ref_topk(A4, [0], [4], [5, 4, 3], None, 3)
    assert idx.tolist() == [[5, 3, -1]]
    # -0.0 before +0.0 by list index, each with its own bits; NaN is never listed; -inf is, last
    idx, val = CR.ref_topk(A4, [1], [99], [0, 1, 2, 3, 5], None, 5)
    assert idx.tolist() == [[0, 1, 5, 3, -1]] and np.signbit(val[0]).tolist() == [True, False, False, True, False]
    assert val[0, 3] == -np.inf and val[0, 4] == 0.0
    idx, val = CR.ref_topk(A4, [1], [99], [1, 0], None, 2)
    assert idx.tolist() == [[1, 0]] and np.signbit(val[0]).tolist() == [False, True]
    # a position outside the block is no candidate; fewer candidates than k leave -1 / 0
    idx, val = CR.ref_topk(A4, [2, 3, -1, 2], [0, 0, 0, 7], [-1, 1, 6, 0], [10, 11, 12, 7], 3)
    assert idx.tolist() == [[7, 11, -1], [-1] * 3, [-1] * 3, [11, -1, -1]]
    assert val.tolist() == [[3.0, 2.0, 0.0], [0.0] * 3, [0.0] * 3, [2.0, 0.0, 0.0]]
    # no candidates at all
    idx, val = CR.ref_topk(A4, [0, 1], [0, 1], [], None, 2)
    assert idx.tolist() == [[-1, -1]] * 2 and val.tolist() == [[0.0, 0.0]] * 2


def test_ref_most_similar_on_a_hand_written_frame():
    labels = list("abcd")
    dense = pd.DataFrame([[9, .5, .5, .25], [.5, 9, np.nan, 1], [.5, 0, 9, -0.0], [0, 0, 0, 9]], index=labels, columns=labels)
    got = CR.ref_most_similar(dense, ["a", "c", "b"], 2, among=["d", "c", "b", "b", "a"], exclude=["d"])
    assert got["node"].tolist() == list("aaccb") and got["rank"].tolist() == [1, 2, 1, 2, 1]
    assert got["neighbor"].tolist() == list("bcaba") and got["similarity"].tolist() == [.5, .5, .5, 0.0, .5]
    assert len(CR.ref_most_similar(dense, ["a"], 3, among=[])) == 0
    assert CR.ref_most_similar(dense, ["d"], 9, exclude=["a"])["neighbor"].tolist() == ["b", "c"]


# ---- prepare ----------------------------------------------------------------------------------------------------------------
def test_prepare_normalises_and_refuses():
    index = pd.Index(list("abcdef"))
    assert _candidates.prepare(None, None, index) is None
    got = _candidates.prepare(["e", "a", "e", "c", "a"], None, index)
    assert got.dtype == np.int32 and got.tolist() == [0, 2, 4]
    assert _candidates.prepare(iter(["c", "a"]), ("a",), index).tolist() == [2]
    assert _candidates.prepare(None, ["b", "b", "f"], index).tolist() == [0, 2, 3, 4]
    assert _candidates.prepare([], None, index).tolist() == [] and _candidates.prepare(["a"], ["a"], index).size == 0
    assert _candidates.prepare(None, [], index).tolist() == list(range(6))
    ints = pd.Index([10, 20, 30])
    assert _candidates.prepare(np.array([30, 10]), None, ints).tolist() == [0, 2]
    for bad in ("ab", b"ab", 3, 2.5):
        with pytest.raises(ValueError, match="among must be None or an iterable"):
            _candidates.prepare(bad, None, index)
        with pytest.raises(ValueError, match="exclude must be None or an iterable"):
            _candidates.prepare(None, bad, index)
    with pytest.raises(KeyError, match="z"):
        _candidates.prepare(["a", "z"], None, index)
    with pytest.raises(KeyError, match="y"):
        _candidates.prepare(["a"], ["y"], index)
    assert _candidates.clamp_k(10, 0) == 1 and _candidates.clamp_k(10, 4) == 4 and _candidates.clamp_k(4096, 9999) == 4096
    with pytest.raises(ValueError, match="at most 4096"):
        _candidates.clamp_k(4097, 9999)
    for bad in (0, -1, 2.5, True, "3", None):
        with pytest.raises(ValueError, match="k must be a positive integer"):
            _candidates.clamp_k(bad, 5)


# ---- the host path of a pruned model ----------------------------------------------------------------------------------------
def pruned_case():
    """Lists of 6 nodes, 3 slots, with a NaN, a -0.0, a kept exact zero, a negative value and an empty list."""
    ids = np.array([[3, 1, -1], [0, 2, 5], [-1, -1, -1], [5, 4, 0], [1, -1, -1], [2, 0, 4]], dtype=np.int32)
    vals = np.array([[0.5, 0.25, 0], [0.75, np.nan, 0.0], [0, 0, 0], [1.0, 0.5, 0.125], [-0.0, 0, 0], [0.125, -0.5, 1e-9]])
    return ids, vals, np.arange(1.0, 7.0)


def test_the_pruned_host_path_equals_the_reference_on_a_hand_built_P(monkeypatch):
    import simrank_amd.estimators as E
    ops = HostOps()
    monkeypatch.setattr(E, "_default_ops_factory", lambda device: lambda rank: ops)
    ids, vals, diag = pruned_case()
    labels = list("abcdef")
    P = pd.DataFrame(diverse_ref.dense_p(ids, vals, diag), index=labels, columns=labels)
    solver = _neighbors.NeighborSolver(ops, [RingSpec(6)], [_neighbors.Tables.from_host(ops, ids, vals, diag)])
    solver._make_reader = boom                                  # (answered from the lists alone)
    solver.lists = lambda j: solver.tables[j].host()
    est = SRA.SimRank()._keep(solver, [(0, labels)])
    nodes = ["d", "a", "b", "c", "f", "e", "a"]
    for among in (None, labels, ["f", "a", "a", "c"], ["b"], [], ["e", "d", "b", "c"]):
        for exclude in (None, [], ["a"], ["c", "f"]):
            if among is None and exclude is None:
                continue
            for k in (1, 2, 3):
                got = est.most_similar(nodes, k, among=among, exclude=exclude)
                same_frame(got, CR.ref_most_similar(P, nodes, k, among, exclude), (among, exclude, k))
    # an absent entry counts as +0.0 and ranks by label position among the zeros: b lists a (0.75), c (NaN), f (0.0)
    got = est.most_similar(["b"], 3, among=["f", "e", "d", "c"])
    assert got["neighbor"].tolist() == ["d", "e", "f"] and got["similarity"].tolist() == [0.0, 0.0, 0.0]
    # the rule of a pruned model: no more than it keeps, after the clamp to the candidates
    with pytest.raises(ValueError, match="kept_neighbors = 3"):
        est.most_similar(["a"], 4, among=labels)
    assert len(est.most_similar(["a"], 4, among=["b", "c", "d"])) == 3          # (4 clamps to the 3 candidates)
    est.release()
    assert not ops.live


# ---- every refusal comes before any device call -----------------------------------------------------------------------------
@pytest.fixture
def guarded(monkeypatch):
    for mod, names in ((_candidates, ("topk_of", "topk_of_lists", "load")), (_sets, ("run", "load")), (_diverse, ("run", "load"))):
        for name in names:
            monkeypatch.setattr(mod, name, boom)
    est = guarded_estimator()
    est._model[0].lists = boom
    return est


BAD_LISTS = ["ab", b"ab", 3, 2.5]


def test_most_similar_refuses_before_any_device_call(guarded):
    est = guarded
    for bad in BAD_LISTS:
        with pytest.raises(ValueError, match="among must be None or an iterable"):
            est.most_similar(["a"], 1, among=bad)
        with pytest.raises(ValueError, match="exclude must be None or an iterable"):
            est.most_similar(["a"], 1, exclude=bad)
    with pytest.raises(KeyError, match="z"):
        est.most_similar(["a"], 1, among=["a", "z"])
    with pytest.raises(KeyError, match="z"):
        est.most_similar(["a"], 1, exclude=["z"])
    for bad in (0, -1, 2.5, True, "3", None):
        with pytest.raises(ValueError, match="k must be a positive integer"):
            est.most_similar(["a"], bad, among=["a"])
    with pytest.raises(KeyError, match="q"):
        est.most_similar(["q"], 1, among=["a"])                  # (an unknown query node: after the lists, before the device)
    with pytest.raises(ValueError, match="group must be None or 1"):
        est.most_similar(["a"], 1, group=2, among=["a"])
    # k clamps to the candidates first; what is left may be at most 4096
    wide = guarded_estimator()
    wide._model[0].n = [5000]
    wide._model[0].kept_k = [4999]
    wide._model = (wide._model[0], [(0, list(range(5000)))])
    with pytest.raises(ValueError, match="at most 4096"):
        wide.most_similar([0], 5000, exclude=[1])
    with pytest.raises(ValueError, match="at most 4096"):
        wide.most_similar([0], 4097, among=range(4097))
    with pytest.raises(AssertionError, match="the device was touched"):
        wide.most_similar([0], 5000, among=range(4096))          # (clamped to 4096: this one goes on to the solver)
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.most_similar(["a"], 1, among=["a"])


def test_the_band_queries_refuse_before_any_device_call(guarded):
    est = guarded
    with pytest.raises(ValueError, match="among narrows a selection: give top_k"):
        est.score_sets([["a"]], among=["a"])
    for bad in BAD_LISTS:
        with pytest.raises(ValueError, match="among must be None or an iterable"):
            est.score_sets([["a"]], top_k=1, among=bad)
        with pytest.raises(ValueError, match="among must be None or an iterable"):
            est.score_sets([["a"]], top_k=1, among=bad, diversity=0.5)
        with pytest.raises(ValueError, match="among must be None or an iterable"):
            est.recommend(["a"], 1, among=bad)
    with pytest.raises(KeyError, match="z"):
        est.score_sets([["a"]], top_k=1, among=["z"])
    with pytest.raises(KeyError, match="z"):
        est.recommend(["a"], 1, among=["z"], diversity=0.25)
    with pytest.raises(ValueError, match="give top_k as well"):
        est.score_sets([["a"]], among=["a"], diversity=0.5)      # (diversity without top_k is named first, as before)
    with pytest.raises(KeyError, match="q"):
        est.score_sets([["q"]], top_k=1, among=["a"])
    with pytest.raises(AssertionError, match="the device was touched"):
        est.score_sets([["a"]], top_k=1, among=["a"])
    with pytest.raises(AssertionError, match="the device was touched"):
        est.recommend(["a"], 1, among=["b"])


def test_without_the_keywords_the_calls_take_the_path_they_took(monkeypatch):
    """``among=None, exclude=None`` reaches ``topk_of`` with the arguments it always had, never ``topk_among``."""
    est = guarded_estimator()
    solver = est._model[0]
    seen = []
    solver.topk_of = lambda j, ids, k: seen.append((j, ids.tolist(), k)) or (np.array([[1]], dtype=np.int32), np.array([[0.5]]))
    solver.topk_among = boom
    a = est.most_similar(["a"], 1)
    b = est.most_similar(["a"], 1, among=None, exclude=None)
    same_frame(a, b)
    assert seen == [(0, [0], 1)] * 2 and a["neighbor"].tolist() == ["b"]
