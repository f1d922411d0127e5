"""libsimrank_diverse.so (include/simrank_diverse.h) and ``diversity=`` of ``score_sets`` / ``recommend`` on a machine
without a GPU: header, binding and exports agree, the header is plain C and stands alone, the NumPy statement
(tests/diverse_ref.py) gives the picks written out here on a hand-made case and at its edges (ties, NaN, the two zeros,
infinities, fewer candidates than k), every argument check runs before any device work, and on the GPU suite's own graph
the penalty changes the picks."""
import ctypes as C
import re

import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

import simrank_amd.SimRank as SRA
from simrank_amd import _diverse, _query, synth
from tests import companion_abi as A
from tests import diverse_ref as D
from tests import sets_ref as R


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_diverse) == _diverse.VERSION == 1
    text = A.header(_diverse)
    assert re.search(r"#define SIMRANK_DIVERSE_CHUNK %d\b" % _diverse.CHUNK, text)
    assert re.search(r"#define SIMRANK_DIVERSE_MAX_BLOCKS \(1 << 24\)", text) and _diverse.MAX_BLOCKS == 1 << 24
    A.assert_header_stands_alone(_diverse)
    A.assert_prototypes_match_the_header_argument_counts(_diverse)
    A.assert_links_nothing_of_the_main_library(_diverse)
    assert A.layout_codes(_diverse) == A.layout_codes(_query)


def test_sizes_and_bad_arguments_need_no_device():
    lib = _diverse.load()
    assert lib.simrank_diverse_blocks(7, 1100) == 7 and lib.simrank_diverse_blocks(0, 5) == 0
    assert lib.simrank_diverse_blocks(-1, 5) == -1 and lib.simrank_diverse_blocks(1, 1 << 31) == -1
    # one pen vector of doubles per basket, each on 16 bytes
    assert lib.simrank_diverse_workspace_bytes(3, 1100) == 3 * 1100 * 8
    assert lib.simrank_diverse_workspace_bytes(3, 7) == 3 * 8 * 8 and lib.simrank_diverse_workspace_bytes(3, -1) == -1
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def pick(layout=3, stride=4, n_rows=4, n_cols=4, n_out=4, band=p, ld=4, n_sets=1, k=1, rel_w=0.5, lam=0.5, idx=p,
             work=p, S=p):
        return lib.simrank_diverse_pick(S, layout, stride, n_rows, n_cols, None, None, n_out, band, ld, n_sets, k, rel_w, lam,
                                        idx, p, p, p, work, None)

    def pick_lists(kk=2, n=4, ld=4, k=1, lam=0.5, ids=p):
        return lib.simrank_diverse_pick_lists(ids, p, None, n, kk, p, ld, 1, k, 1.0 - lam, lam, p, p, p, p, p, None)

    for bad in (pick(layout=9), pick(S=None), pick(stride=3), pick(ld=3), pick(k=0), pick(lam=1.5), pick(lam=-0.25),
                pick(lam=float("nan")), pick(rel_w=float("inf")), pick(idx=None), pick(band=None), pick(work=None),
                pick(band=p + 4), pick(n_sets=(1 << 24) + 1), pick(n_sets=-1),
                pick_lists(kk=-1), pick_lists(ld=3), pick_lists(k=0), pick_lists(lam=2.0), pick_lists(ids=None)):
        assert bad == -1 and _diverse.load().simrank_diverse_last_error()
    assert pick(n_sets=(1 << 24) + 1) == -1 and b"bands" in lib.simrank_diverse_last_error()
    assert pick(n_sets=0) == 0 and pick(n_sets=0, idx=None, band=None, work=None) == 0      # nothing asked: no device touched


# ---- the statement on a matrix worked by hand -------------------------------------------------------------------------------
LABELS = ["a", "b", "c", "d", "e"]
# NOT symmetric: row b holds 0.75 for c, row c holds 0 for b.  Reading column b for pick b would leave c unpunished.
S5 = pd.DataFrame([[1.0, 0.75, 0.5, 0.25, 0.0],
                   [0.5, 1.0, 0.75, 0.0, 0.0],
                   [0.0, 0.0, 1.0, 0.0, 0.125],
                   [0.25, 0.0, 0.0, 1.0, 0.5],
                   [0.0, 0.0, 0.0, 0.125, 1.0]], index=LABELS, columns=LABELS)


def test_the_second_pick_flips_on_a_hand_made_case():
    """Basket [a]: the scores of b, c, d, e are 0.75, 0.5, 0.25, 0.  d = 0: b, c, d, e.  d = 0.5: b first (0.375); row b
    then punishes c by 0.75: c is worth 0.25 - 0.375 = -0.125, d 0.125 - 0 and e 0 - 0: d is second.  Row d holds 0.5 for
    e: c (-0.125) beats e (0 - 0.25); row c's 0.125 for e does not pass 0.5."""
    plain = D.score_sets_ref(S5, [["a"]], top_k=4, diversity=0.0)
    assert plain["neighbor"].tolist() == ["b", "c", "d", "e"] and plain["penalty"].tolist() == [0.0, 0.75, 0.0, 0.5]
    assert plain["value"].tolist() == plain["score"].tolist() == [0.75, 0.5, 0.25, 0.0]
    assert_frame_equal(plain[["set", "rank", "neighbor", "score"]], R.score_sets_ref(S5, [["a"]], top_k=4), check_exact=True)
    half = D.score_sets_ref(S5, [["a"]], top_k=4, diversity=0.5, names=["q"])
    assert_frame_equal(half, pd.DataFrame({
        "set": ["q"] * 4, "rank": [1, 2, 3, 4], "neighbor": ["b", "d", "c", "e"], "score": [0.75, 0.25, 0.5, 0.0],
        "penalty": [0.0, 0.0, 0.75, 0.5], "value": [0.375, 0.125, -0.125, -0.25]}), check_exact=True)
    # the column instead of the row (the transposed matrix) picks c second: the row is part of the statement
    col = D.picks(np.array([-np.inf, 0.75, 0.5, 0.25, 0.0]), lambda b: S5.values[:, b], 2, 0.5)[0]
    assert col.tolist() == [1, 2]
    # d = 1: the score counts for nothing: the first pick is the first candidate, then the least punished
    one = D.score_sets_ref(S5, [["a"]], top_k=4, diversity=1.0)
    assert one["neighbor"].tolist() == ["b", "d", "e", "c"] and one["value"].tolist() == [0.0, 0.0, -0.5, -0.75]
    assert one["penalty"].tolist() == [0.0, 0.0, 0.5, 0.75] and one["score"].tolist() == [0.75, 0.25, 0.0, 0.5]
    # recommend on the directed graph c -> a, d -> a, a -> b, e -> d (rows = in-neighbours), scale 1 / in-degree
    rowptr, col, scale = np.array([0, 2, 3, 3, 4, 4]), np.array([2, 3, 0, 4]), np.array([0.5, 1.0, 0.0, 1.0, 0.0])
    for d in (0.0, 0.5):
        rec = D.recommend_ref(S5, LABELS, rowptr, col, scale, ["d", "c", "a"], 2, also_self=True, diversity=d)
        want = R.recommend_ref(S5, LABELS, rowptr, col, scale, ["d", "c", "a"], 2, also_self=True)
        assert rec["node"].tolist() == want["node"].tolist() == ["d", "d", "a", "a"]
        assert rec[rec["rank"] == 1]["neighbor"].tolist() == want[want["rank"] == 1]["neighbor"].tolist()


def test_d_zero_is_the_plain_selection():
    rng = np.random.default_rng(1)
    S = pd.DataFrame(rng.integers(-8, 9, size=(40, 40)) / 8.0)
    sets = [list(rng.integers(0, 40, size=m)) for m in (0, 1, 5, 40)]
    weights = [list(rng.normal(size=len(s))) for s in sets]
    for k in (1, 7, 40):
        for exclude in ("members", None, [[1, 2], [], [3], []]):
            got = D.score_sets_ref(S, sets, weights, top_k=k, exclude=exclude, diversity=0.0)
            want = R.score_sets_ref(S, sets, weights, top_k=k, exclude=exclude)
            assert_frame_equal(got[["set", "rank", "neighbor", "score"]], want, check_exact=True)
            assert np.array_equal(got["value"].to_numpy().view(np.uint64), got["score"].to_numpy().view(np.uint64))
            assert (got["penalty"] >= 0).all() and not np.signbit(got["penalty"]).any()


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_edges_of_the_statement():
    nan, inf = np.nan, np.inf
    Z = [0.0]                                                              # (a matrix of zeros: every row the scalar 0.0)
    # ties by position; a NaN score and a -inf score are never picked; fewer candidates than k
    pos, s, p, v = D.picks(np.array([1.0, 2.0, nan, 2.0, -inf, 1.0]), lambda b: Z[0], 9, 0.25)
    assert pos.tolist() == [1, 3, 0, 5] and v.tolist() == [1.5, 1.5, 0.75, 0.75] and p.tolist() == [0.0] * 4
    # -0.0 and +0.0 tie, the position decides, each keeps its bits; rel_w * -0.0 = -0.0, minus +0.0 = -0.0
    pos, s, p, v = D.picks(np.array([-0.0, 0.0, -0.0, -1.0]), lambda b: Z[0], 4, 0.0)
    assert pos.tolist() == [0, 1, 2, 3]
    assert np.array_equal(bits(s), bits([-0.0, 0.0, -0.0, -1.0])) and np.array_equal(bits(v), bits([-0.0, 0.0, -0.0, -1.0]))
    # a NaN similarity and a negative one move no pen; pen is never -0.0
    M = np.array([[0.0, nan, -0.5, -0.0, 0.25],
                  [0.0] * 5, [0.0] * 5, [0.0] * 5,
                  [0.0, 0.5, nan, -3.0, 0.0]])
    pos, s, p, v = D.picks(np.array([5.0, 1.0, 1.0, 1.0, 4.0]), lambda b: M[b], 5, 0.5)
    assert pos.tolist() == [0, 4, 2, 3, 1]
    assert np.array_equal(bits(p), bits([0.0, 0.25, 0.0, 0.0, 0.5])) and v.tolist() == [2.5, 1.875, 0.5, 0.5, 0.25]
    # +inf scores: at d = 1 the value is 0 x inf = NaN and is never picked; below 1 the infinity wins and keeps its value
    pos, s, p, v = D.picks(np.array([inf, 1.0, 2.0]), lambda b: Z[0], 3, 1.0)
    assert pos.tolist() == [1, 2] and np.array_equal(bits(v), bits([0.0, 0.0]))
    pos, s, p, v = D.picks(np.array([1.0, inf, 2.0]), lambda b: Z[0], 3, 0.0)
    assert pos.tolist() == [1, 2, 0] and v.tolist() == [inf, 2.0, 1.0]
    # an infinite similarity: d x inf = inf: the value is -inf and still a pick; at d = 0 it is 0 x inf = NaN and none
    I = np.array([[0.0, inf, 0.0], [0.0] * 3, [0.0] * 3])
    assert D.picks(np.array([3.0, 2.0, 1.0]), lambda b: I[b], 3, 0.5)[3].tolist() == [1.5, 0.5, -inf]
    assert D.picks(np.array([3.0, 2.0, 1.0]), lambda b: I[b], 3, 0.0)[0].tolist() == [0, 2]
    # the band form pads with -1 and zeros
    idx, s, p, v = D.band_picks(np.array([[1.0, nan, 2.0], [-inf, -inf, nan]]), lambda b: Z[0], 3, 0.5)
    assert idx.tolist() == [[2, 0, -1], [-1, -1, -1]] and v.tolist() == [[1.0, 0.5, 0.0], [0.0] * 3]
    # the dense P of neighbour tables
    P = D.dense_p(np.array([[2, -1], [0, 2], [7, 1]]), np.array([[0.5, 0.0], [0.25, -1.0], [9.0, 0.125]]), np.array([1.0, 2.0, 3.0]))
    assert P.tolist() == [[1.0, 0.0, 0.5], [0.25, 2.0, -1.0], [0.0, 0.125, 3.0]]


# ---- argument checks: no device ---------------------------------------------------------------------------------------------
def test_check_diversity():
    assert _diverse.check_diversity(None, None) is None and _diverse.check_diversity(None, 3) is None
    for ok in (0, 1, 0.0, 1.0, 0.3, np.float32(0.5), np.float64(0.25), np.int64(1)):
        got = _diverse.check_diversity(ok, 3)
        assert type(got) is float and got == float(ok)
    for bad in (True, False, np.True_, "0.3", [0.3], 1j, None.__class__, np.nan, float("nan"), -0.1, 1.0000001, np.inf, -np.inf):
        with pytest.raises(ValueError, match="diversity"):
            _diverse.check_diversity(bad, 3)
    with pytest.raises(ValueError, match="top_k"):
        _diverse.check_diversity(0.3, None)


class _Csr:
    rowptr, col = np.array([0, 2, 2, 3], dtype=np.int32), np.array([2, 0, 1], dtype=np.int32)


class _Spec:
    csr, rowscale = _Csr, np.array([0.5, 0.0, 1.0])


class _FakeSolver:
    """Stands in for a kept solver: what the argument checks reach is never the device."""

    def __init__(self):
        self.specs, self.calls = [_Spec], []

    def release(self):
        pass

    def score_diverse(self, j, ptr, ids, w, k, excl, d):
        self.calls.append((j, ptr.tolist(), ids.tolist(), k, None if excl is None else excl[1].tolist(), d))
        n_sets = ptr.size - 1
        idx = np.tile(np.arange(k, dtype=np.int32), (n_sets, 1))
        idx[:, -1] = -1                                     # (one empty slot per basket)
        return idx, np.full((n_sets, k), 1.0), np.full((n_sets, k), 2.0), np.full((n_sets, k), 3.0)


def test_the_keyword_on_the_estimator_needs_no_device():
    est = SRA.SimRank()
    solver = _FakeSolver()
    est._keep(solver, [(0, ["a", "b", "c"])])
    top = est.score_sets([["a"], ["b", "b"]], top_k=2, names=["x", "y"], diversity=0.25)
    assert list(top.columns) == ["set", "rank", "neighbor", "score", "penalty", "value"]
    assert top["set"].tolist() == ["x", "y"] and top["neighbor"].tolist() == ["a", "a"] and top["rank"].tolist() == [1, 1]
    assert top["score"].tolist() == [1.0, 1.0] and top["penalty"].tolist() == [2.0, 2.0] and top["value"].tolist() == [3.0, 3.0]
    assert top["penalty"].dtype == top["value"].dtype == np.float64
    assert solver.calls[-1] == (0, [0, 1, 3], [0, 1, 1], 2, [0, 1, 1], 0.25)
    rec = est.recommend(["c", "b", "a"], 2, diversity=1)
    assert list(rec.columns) == ["node", "rank", "neighbor", "score", "penalty", "value"]
    assert rec["node"].tolist() == ["c", "a"]               # b has no in-neighbours: no rows
    assert solver.calls[-1] == (0, [0, 1, 1, 3], [1, 2, 0], 2, [1, 2, 1, 2, 0, 0], 1.0)
    n_calls = len(solver.calls)
    with pytest.raises(ValueError, match="top_k"):
        est.score_sets([["a"]], diversity=0.3)
    for bad in (True, "0.3", np.nan, -0.5, 1.5):
        with pytest.raises(ValueError, match="diversity"):
            est.score_sets([["a"]], top_k=1, diversity=bad)
        with pytest.raises(ValueError, match="diversity"):
            est.recommend(["a"], 1, diversity=bad)
    with pytest.raises(ValueError, match="k must be a positive integer"):
        est.recommend(["a"], 0, diversity=0.3)
    with pytest.raises(KeyError, match="zz"):
        est.score_sets([["zz"]], top_k=1, diversity=0.3)
    assert len(solver.calls) == n_calls
    est.release()
    for call in (lambda: est.score_sets([["a"]], top_k=1, diversity=0.3), lambda: est.recommend(["a"], 1, diversity=0.3)):
        with pytest.raises(RuntimeError, match="released"):
            call()


# ---- the condition the GPU tests stand on -------------------------------------------------------------------------------------
def test_on_the_gpu_suites_graph_the_penalty_changes_the_picks():
    """tests/test_gpu_diverse.py compares frames on ``synth.er_directed(1100, 0.002, seed=7)`` after three updates.  Most
    of that S is exactly 0, so a device that ignored the penalty could pass there if the penalty never mattered.  It
    matters: at d = 0.3, k = 10, the frames of test_gpu_sets' baskets with unit weights (every score >= 0) differ from the
    plain ones in at least one rank, and at least one emitted penalty is positive, for SimRank and SimRank++."""
    from oracle import simrank_oracle as O
    from tests.test_gpu_sets import baskets
    df = synth.er_directed(1100, 0.002, seed=7)
    for fit in (O.fit_simrank, O.fit_simrank_pp):
        r = fit(df, iterations=3, eps=1e-30, verbose=False)
        frame = pd.DataFrame(r["S"], index=r["labels"], columns=r["labels"])
        sets, _ = baskets(list(frame.index))
        plain = R.score_sets_ref(frame, sets, top_k=10)
        got = D.score_sets_ref(frame, sets, top_k=10, diversity=0.3)
        assert len(got) == len(plain) and got["set"].tolist() == plain["set"].tolist()
        differ = int((got["neighbor"].to_numpy() != plain["neighbor"].to_numpy()).sum())
        positive = int((got["penalty"] > 0).sum())
        print(fit.__name__, "ranks that differ:", differ, "of", len(got), "; picks with a positive penalty:", positive)
        assert differ >= 1 and positive >= 1
        zero = D.score_sets_ref(frame, sets, top_k=10, diversity=0.0)
        assert_frame_equal(zero[["set", "rank", "neighbor", "score"]], plain, check_exact=True)
