"""libsimrank_foldin.so (include/simrank_foldin.h) and ``fold_in`` on a machine without a GPU: header, binding and exports
agree, the header is plain C99 and stands alone, the NumPy statement of the formula (tests/foldin_ref.py) is the
reference's own next update, and every argument check of ``fold_in`` runs before any device work."""
import re

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _foldin
from tests import companion_abi as A
from tests import foldin_ref as R
from tests.conftest import Golden


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_foldin) == _foldin.VERSION == 1
    text = A.header(_foldin)
    assert re.search(r"#define SIMRANK_FOLDIN_TILE %d\b" % _foldin.TILE, text)
    assert re.search(r"#define SIMRANK_FOLDIN_LONG_ROW %d\b" % _foldin.LONG_ROW, text)
    A.assert_header_stands_alone(_foldin)
    # the layouts are simrank_query.h's
    from simrank_amd import _query
    for name, value in (("PANEL_F32", _query.PANEL_F32), ("ROWMAJOR_F32", _query.ROWMAJOR_F32),
                        ("PANEL_F16", _query.PANEL_F16), ("ROWMAJOR_F64", _query.ROWMAJOR_F64)):
        assert re.search(r"SIMRANK_FOLDIN_%s = %d\b" % (name, value), text)


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_foldin)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_foldin)


def test_header_is_c99_and_a_c_program_links(tmp_path):
    assert "foldin 1 ok" in A.run_c99(_foldin, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_foldin.h"
int main(void) {
    int32_t one[2] = {0, 0};
    double w[1] = {1.0};
    if (simrank_foldin_version() != SIMRANK_FOLDIN_VERSION) return 1;
    if (simrank_foldin_t_bytes(SIMRANK_FOLDIN_PANEL_F32, 100) != 100 * 32 * 4) return 2;
    if (simrank_foldin_t_bytes(SIMRANK_FOLDIN_PANEL_F16, 100) != 100 * 32 * 4) return 3;
    if (simrank_foldin_t_bytes(SIMRANK_FOLDIN_ROWMAJOR_F64, 100) != 100 * 32 * 8) return 4;
    if (simrank_foldin_t_bytes(9, 100) != -1) return 5;
    if (simrank_foldin_gather(NULL, 9, 8, 4, 4, NULL, 0, one, one, w, 1, NULL, 4, NULL) != SIMRANK_FOLDIN_ERR_INVALID) return 6;
    if (!strlen(simrank_foldin_last_error())) return 7;
    if (simrank_foldin_gather(NULL, SIMRANK_FOLDIN_PANEL_F32, 8, 4, 4, NULL, 0, one, one, w, 1, NULL, 4, NULL)
        != SIMRANK_FOLDIN_ERR_INVALID) return 8;                                  /* S is NULL */
    if (simrank_foldin_gather(NULL, SIMRANK_FOLDIN_PANEL_F32, 8, 4, 4, NULL, 0, one, one, w, 33, NULL, 4, NULL)
        != SIMRANK_FOLDIN_ERR_INVALID) return 9;                                  /* a tile holds 32 */
    if (simrank_foldin_gather(NULL, SIMRANK_FOLDIN_PANEL_F16, 2, 4, 4, NULL, 0, one, one, w, 1, NULL, 4, NULL)
        != SIMRANK_FOLDIN_ERR_INVALID) return 10;                                 /* stride below the rows */
    if (simrank_foldin_gather(NULL, SIMRANK_FOLDIN_ROWMAJOR_F64, 4, 4, 4, NULL, 2, one, one, w, 1, NULL, 4, NULL)
        != SIMRANK_FOLDIN_ERR_INVALID) return 11;                                 /* columns 2 .. 6 of 4 source nodes */
    if (simrank_foldin_gather(NULL, SIMRANK_FOLDIN_ROWMAJOR_F64, 4, 4, 0, NULL, 0, one, one, w, 1, NULL, 4, NULL)
        != SIMRANK_FOLDIN_OK) return 12;                                          /* nothing asked: no device touched */
    if (simrank_foldin_member(one, one, w, 1, NULL, 4, NULL) != SIMRANK_FOLDIN_ERR_INVALID) return 13;
    if (simrank_foldin_member(one, one, w, 1, NULL, 0, NULL) != SIMRANK_FOLDIN_OK) return 14;
    if (simrank_foldin_apply(one, one, w, 1, 1, NULL, 0, NULL, SIMRANK_FOLDIN_PANEL_F32, NULL, 0.8, 0.0, NULL, 0, 1, NULL, 0, NULL)
        != SIMRANK_FOLDIN_ERR_INVALID) return 15;                                 /* ld_out below the fitted nodes */
    if (simrank_foldin_apply(one, one, w, 1, 1, NULL, 1, NULL, SIMRANK_FOLDIN_PANEL_F32, NULL, 0.8, 0.0, NULL, 0, 1, NULL, 1, NULL)
        != SIMRANK_FOLDIN_ERR_INVALID) return 16;                                 /* long rows without their list */
    if (simrank_foldin_apply(one, one, w, 1, 1, NULL, 0, NULL, SIMRANK_FOLDIN_PANEL_F32, NULL, 0.8, 0.0, NULL, 0, 0, NULL, 1, NULL)
        != SIMRANK_FOLDIN_OK) return 17;                                          /* an empty tile */
    if (simrank_foldin_alloc(NULL, 16) != SIMRANK_FOLDIN_ERR_INVALID) return 18;
    if (simrank_foldin_free(NULL) != SIMRANK_FOLDIN_OK) return 19;
    printf("foldin %d ok\n", simrank_foldin_version());
    return 0;
}
''')


# ---- the NumPy statement of the formula is the reference's own next update ----------------------------------------
# golden inputs of all six classes on which neither 3 nor 4 updates at eps = 1e-12 pass a convergence test (asserted)
REFERENCE_CASES = ["SimRank_er128", "SimRank_er64_weighted", "SimRank_quirky", "SimRankPP_pl256", "SimRankPP_er64_cols",
                   "AprioriSimRank_er64", "AprioriSimRank_er64_asym", "AprioriSimRank_quirky_asym", "BipartiteSimRank_b5030",
                   "BipartiteSimRank_b40_weighted", "BipartiteSimRank_k10", "BipartiteSimRankPP_b40",
                   "BipartiteSimRankPP_b40_weighted", "BipartiteSimRankPP_bigints", "BipartitleAprioriSimRank_b40",
                   "BipartitleAprioriSimRank_b40_asym"]


def _assert_rows_off_diagonal(got, want, rtol):
    """Every column of row a but a itself (where the reference writes the diagonal 1), relative."""
    off = ~np.eye(len(want), dtype=bool)
    np.testing.assert_allclose(got[off], want[off], rtol=rtol, atol=0)


def _gated(name):
    return name.split("_")[0] in ("BipartiteSimRankPP", "BipartitleAprioriSimRank")


# (strict_reference is an argument of the bipartite SimRank++ classes: both values there, the default elsewhere)
@pytest.mark.parametrize("name,strict", [(n, s) for n in REFERENCE_CASES for s in ((True, False) if _gated(n) else (True,))])
def test_the_numpy_statement_is_the_references_next_update(name, strict):
    """``fold_in_ref(neighbours of a, S after 3 updates)`` = row a of the reference's matrix after 4 updates, in every
    column but a, for every node a, to 1e-13 relative (the same float64 terms in another association; all non-negative).
    Group 2 of the bipartite classes: by the reference's Gauss-Seidel order, S2 after 3 updates IS the fold-in of every
    group-2 node on S1 after 3 updates (with the group's own evidence: ``strict_reference=False``)."""
    g = Golden(name)
    gated2 = _gated(name)
    r3 = R.run_oracle(g, iterations=3, eps=1e-12, verbose=False, strict_reference=strict)
    r4 = R.run_oracle(g, iterations=4, eps=1e-12, verbose=False, strict_reference=strict)
    assert r3["k"] is None and r4["k"] is None          # 3 and 4 updates were really applied
    for sd in R.sides_of(g, r3):
        lists, w = R.own_lists(sd["G"])
        if sd["group"] == 2 and gated2 and strict:
            continue                                     # (gated by Evidence_N1: what fold_in refuses)
        got = R.fold_in_ref(lists, r3[sd["reads"]], sd["W"], sd["coef"], w, sd["pattern"], sd["lbd"], sd["prior"])
        want = (r3 if sd["group"] == 2 else r4)[sd["writes"]]
        assert got.shape == want.shape and np.all(got >= 0)
        _assert_rows_off_diagonal(got, want, 1e-13)


# ---- argument checks: no device --------------------------------------------------------------------------------------
INDEX = pd.Index(["a", "b", "c", "d"])


def _prep(neighbors, **kw):
    kw.setdefault("n_out", 4)
    kw.setdefault("weighted", False)
    kw.setdefault("has_prior", False)
    return _foldin.prepare(neighbors, INDEX, **kw)


def test_lists_become_ids_and_row_scales():
    lists, w, prior, names, k = _prep([["c", "a"], [], ["d"]])
    assert [l.tolist() for l in lists] == [[2, 0], [], [3]] and all(l.dtype == np.int32 for l in lists)
    assert w.tolist() == [0.5, 0.0, 1.0] and prior is None and names is None and k is None
    # weighted: 1 / sum(weights) for every entry, 0 where that is not finite (a zero sum, an empty list)
    lists, w, *_ = _prep([["a", "b"], ["c"], ["a", "d"], []], weighted=True, weights=[[1, 3], [0.5], [2.0, -2.0], []])
    assert w.tolist() == [0.25, 2.0, 0.0, 0.0]
    np.testing.assert_array_equal(w, R.row_scales([2, 1, 2, 0], [[1, 3], [0.5], [2.0, -2.0], []]))
    assert _foldin.row_scales([3, 0], None, False).tolist() == [1 / 3, 0.0]
    assert _prep([])[0] == []
    lists, *_ = _foldin.prepare([[7, 5]], pd.Index([5, 6, 7]), n_out=3, weighted=False, has_prior=False)
    assert lists[0].tolist() == [2, 0]


def test_argument_errors_need_no_device():
    with pytest.raises(KeyError, match="zz"):
        _prep([["a"], ["b", "zz"]])
    with pytest.raises(ValueError, match="repeats a label"):
        _prep([["a", "b", "a"]])
    with pytest.raises(ValueError, match="one sequence of labels per new node"):
        _prep("ab")
    with pytest.raises(ValueError, match="sequence of labels"):
        _prep(["ab"])
    with pytest.raises(ValueError, match="sequence of labels"):
        _prep([3])
    with pytest.raises(ValueError, match="needs weights"):
        _prep([["a"]], weighted=True)
    with pytest.raises(ValueError, match="takes no weights"):
        _prep([["a"]], weights=[[1.0]])
    with pytest.raises(ValueError, match="one sequence per new node"):
        _prep([["a"], ["b"]], weighted=True, weights=[[1.0]])
    with pytest.raises(ValueError, match=r"weights\[1\] has 2 entries for 1"):
        _prep([["a"], ["b"]], weighted=True, weights=[[1.0], [1.0, 2.0]])
    with pytest.raises(ValueError, match="fitted with a prior"):
        _prep([["a"]], prior=np.zeros((1, 4)))
    with pytest.raises(ValueError, match=r"prior must have shape \(2, 4\)"):
        _prep([["a"], ["b"]], has_prior=True, prior=np.zeros((1, 4)))
    with pytest.raises(ValueError, match=r"prior must have shape \(1, 4\)"):
        _prep([["a"]], has_prior=True, prior=np.zeros((1, 3)))
    assert _prep([["a"]], has_prior=True, prior=[[1, 2, 3, 4]])[2].dtype == np.float64
    with pytest.raises(ValueError, match="names must have one entry per new node"):
        _prep([["a"]], names=["x", "y"])
    assert _prep([["a"]], names=("x",))[3] == ["x"]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="k must be a positive integer"):
            _prep([["a"]], top_k=bad)
    assert _prep([["a"]], top_k=3)[4] == 3
    # k is clamped to N first; what is left may be at most the selection kernel's 1024
    assert _prep([["a"]], top_k=5000)[4] == 5000
    assert _prep([["a"]], top_k=1024, n_out=4000)[4] == 1024
    with pytest.raises(ValueError, match="top_k must be at most 1024"):
        _prep([["a"]], top_k=1025, n_out=4000)
    # group rules, as rows()
    assert _foldin.side_of(1, None) == 0 and _foldin.side_of(1, 1) == 0
    assert _foldin.side_of(2, 1) == 0 and _foldin.side_of(2, 2) == 1
    with pytest.raises(ValueError, match="one node group"):
        _foldin.side_of(1, 2)
    with pytest.raises(ValueError, match="group must be 1 or 2"):
        _foldin.side_of(2, None)
    _foldin.check_strict_group(2, 0, True)
    _foldin.check_strict_group(2, 1, False)
    _foldin.check_strict_group(1, 0, True)
    with pytest.raises(ValueError, match="Evidence_N1.*strict_reference=False"):
        _foldin.check_strict_group(2, 1, True)


class _Spec:
    def __init__(self, csr, evidence_from=None, apriori=None):
        self.csr, self.evidence_from, self.apriori = csr, evidence_from, apriori


class _FakeSolver:
    """Stands in for a kept solver: what the argument checks of ``fold_in`` reach is never the device."""
    mode, released = "sparse", 0

    def __init__(self, specs):
        self.specs, self.calls = specs, []

    def release(self):
        self.released += 1

    def fold_in(self, j, lists, w, prior=None, top_k=None):
        self.calls.append((j, [l.tolist() for l in lists], w.tolist(), prior, top_k))
        n = 3 if len(self.specs) == 1 else (3, 2)[j]
        if top_k is None:
            return np.arange(len(lists) * n, dtype=np.float64).reshape(len(lists), n)
        k = min(top_k, n)
        return (np.tile(np.arange(k, dtype=np.int32), (len(lists), 1)), np.ones((len(lists), k)))


def test_fold_in_checks_on_the_estimator_need_no_device():
    est = SRA.SimRank()
    with pytest.raises(RuntimeError, match="no kept model"):
        est.fold_in([["a"]])
    solver = _FakeSolver([_Spec("g")])
    est._keep(solver, [(0, ["a", "b", "c"])])
    est._weighted = False
    got = est.fold_in([["c", "a"], []], names=["x", "y"])
    assert list(got.index) == ["x", "y"] and list(got.columns) == ["a", "b", "c"] and got.values.dtype == np.float64
    assert solver.calls[-1][:3] == (0, [[2, 0], []], [0.5, 0.0])
    assert list(est.fold_in([["a"]]).index) == [0]
    top = est.fold_in([["a"], ["b"]], top_k=2, names=["x", "y"])
    assert list(top.columns) == ["node", "rank", "neighbor", "similarity"]
    assert top["node"].tolist() == ["x", "x", "y", "y"] and top["neighbor"].tolist() == ["a", "b", "a", "b"]
    assert top["rank"].tolist() == [1, 2, 1, 2]
    with pytest.raises(KeyError, match="zz"):
        est.fold_in([["zz"]])
    with pytest.raises(ValueError, match="repeats a label"):
        est.fold_in([["a", "a"]])
    with pytest.raises(ValueError, match="takes no weights"):
        est.fold_in([["a"]], weights=[[1.0]])
    with pytest.raises(ValueError, match="fitted with a prior"):
        est.fold_in([["a"]], prior=np.zeros((1, 3)))
    with pytest.raises(ValueError, match="one node group"):
        est.fold_in([["a"]], group=2)
    est._weighted = True
    with pytest.raises(ValueError, match="needs weights"):
        est.fold_in([["a"]])
    est.fold_in([["a", "b"]], weights=[[1.0, 3.0]])
    assert solver.calls[-1][2] == [0.25]
    n_calls = len(solver.calls)
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.fold_in([["a"]], weights=[[1.0]])
    assert len(solver.calls) == n_calls
    # bipartite: group 1 is given by group-2 labels and answers over group 1; strict SimRank++ refuses group 2
    g12, g21 = object(), object()
    for strict in (True, False):
        two = SRA.BipartiteSimRankPP()
        fake = _FakeSolver([_Spec(g12, g12), _Spec(g21, g12 if strict else g21)])
        two._keep(fake, [(0, [1, 2, 3]), (1, ["x", "y"])])
        two._weighted = False
        with pytest.raises(ValueError, match="group must be 1 or 2"):
            two.fold_in([["x"]])
        got = two.fold_in([["y", "x"]], group=1)
        assert list(got.columns) == [1, 2, 3] and fake.calls[-1][:2] == (0, [[1, 0]])
        with pytest.raises(KeyError):
            two.fold_in([[1]], group=1)
        if strict:
            with pytest.raises(ValueError, match="Evidence_N1"):
                two.fold_in([[1, 3]], group=2)
        else:
            got = two.fold_in([[3, 1]], group=2)
            assert list(got.columns) == ["x", "y"] and fake.calls[-1][:2] == (1, [[2, 0]])
    plain = SRA.BipartiteSimRank()
    plain._keep(_FakeSolver([_Spec(g12), _Spec(g21)]), [(0, [1, 2, 3]), (1, ["x", "y"])])
    plain._weighted = False
    assert plain.fold_in([[1]], group=2).shape == (1, 2)
    apr = SRA.AprioriSimRank()
    fake = _FakeSolver([_Spec("g", "g", apriori=np.eye(3))])
    apr._keep(fake, [(0, ["a", "b", "c"])])
    apr._weighted = False
    with pytest.raises(ValueError, match=r"prior must have shape \(1, 3\)"):
        apr.fold_in([["a"]], prior=np.zeros((3, 3)))
    apr.fold_in([["a"]], prior=np.ones((1, 3)))
    assert fake.calls[-1][3].shape == (1, 3)
