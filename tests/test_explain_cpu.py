"""libsimrank_explain.so (include/simrank_explain.h) and ``explain`` on a machine without a GPU: header, binding and exports
agree, the header is plain C99 and stands alone, the entries refuse bad arguments without a device, every refusal of
``explain`` comes before any device work, the host path of a pruned model equals ``explain_ref`` on hand-made lists, and
``explain_ref``'s ``propagated`` IS the reference's next update: the anchor of everything the GPU tests compare with."""
import re
import types

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _explain, _lib, _neighbors, _query
from simrank_amd.ingest import CSR
from tests import companion_abi as A
from tests import explain_ref as ER
from tests import foldin_ref as R
from tests.conftest import Golden
from tests.test_cluster_cpu import HostOps, _Csr, _Spec, _Tables, boom, guarded_estimator


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_explain) == _explain.VERSION == 1
    assert re.search(r"#define SIMRANK_EXPLAIN_MAX_K %d\b" % _explain.MAX_K, A.header(_explain))
    assert sorted(_explain.PROTOTYPES) == ["simrank_explain_gather", "simrank_explain_last_error", "simrank_explain_reduce",
                                           "simrank_explain_select", "simrank_explain_version"]
    A.assert_header_stands_alone(_explain)
    A.assert_prototypes_match_the_header_argument_counts(_explain)
    assert A.layout_codes(_explain) == A.layout_codes(_query) and len(A.layout_codes(_explain)) == 4


def test_companion_links_nothing_of_the_main_library_which_is_unchanged():
    A.assert_links_nothing_of_the_main_library(_explain)
    version, names, exports = A.main_library(_explain)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_the_entries_refuse_bad_arguments_without_a_device(tmp_path):
    assert "explain 1 ok" in A.run_c99(_explain, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_explain.h"
#define BAD(call, code) do { if ((call) != SIMRANK_EXPLAIN_ERR_INVALID) return code; \
                             if (!strlen(simrank_explain_last_error())) return 100 + code; } while (0)
int main(void) {
    /* aligned stand-ins for device memory: nothing below may reach a device */
    static double mem[8];
    static int64_t ptr[3];
    static int32_t ids[8];
    const void* S = mem;
    double* d = mem;
    const int32_t f32 = SIMRANK_EXPLAIN_ROWMAJOR_F32;
    const int64_t huge = (int64_t)1 << 31;
    if (simrank_explain_version() != SIMRANK_EXPLAIN_VERSION) return 1;
    /* gather: NULL pointers, one at a time */
    BAD(simrank_explain_gather(NULL, f32, 4, 4, 4, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 2);
    BAD(simrank_explain_gather(S, f32, 4, 4, 4, NULL, ptr, ids, ptr, ptr, 2, 4, d, NULL), 3);
    BAD(simrank_explain_gather(S, f32, 4, 4, 4, ids, NULL, ids, ptr, ptr, 2, 4, d, NULL), 4);
    BAD(simrank_explain_gather(S, f32, 4, 4, 4, ids, ptr, NULL, ptr, ptr, 2, 4, d, NULL), 5);
    BAD(simrank_explain_gather(S, f32, 4, 4, 4, ids, ptr, ids, NULL, ptr, 2, 4, d, NULL), 6);
    BAD(simrank_explain_gather(S, f32, 4, 4, 4, ids, ptr, ids, ptr, NULL, 2, 4, d, NULL), 7);
    BAD(simrank_explain_gather(S, f32, 4, 4, 4, ids, ptr, ids, ptr, ptr, 2, 4, NULL, NULL), 8);
    /* an unknown layout */
    BAD(simrank_explain_gather(S, 4, 4, 4, 4, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 10);
    BAD(simrank_explain_gather(S, -1, 4, 4, 4, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 11);
    /* a stride too small: columns of a row-major block, rows of a panel block */
    BAD(simrank_explain_gather(S, f32, 3, 4, 4, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 12);
    BAD(simrank_explain_gather(S, SIMRANK_EXPLAIN_ROWMAJOR_F64, 3, 4, 4, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 13);
    BAD(simrank_explain_gather(S, SIMRANK_EXPLAIN_PANEL_F32, 3, 4, 2, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 14);
    BAD(simrank_explain_gather(S, SIMRANK_EXPLAIN_PANEL_F16, 3, 4, 2, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 15);
    /* a negative shape, a shape of 2^31, negative sizes */
    BAD(simrank_explain_gather(S, f32, 4, -1, 4, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 16);
    BAD(simrank_explain_gather(S, f32, 4, 4, -1, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 17);
    BAD(simrank_explain_gather(S, f32, huge, 4, huge, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 18);
    BAD(simrank_explain_gather(S, SIMRANK_EXPLAIN_PANEL_F32, huge, huge, 4, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 19);
    BAD(simrank_explain_gather(S, f32, 4, 4, 4, ids, ptr, ids, ptr, ptr, -1, 4, d, NULL), 20);
    BAD(simrank_explain_gather(S, f32, 4, 4, 4, ids, ptr, ids, ptr, ptr, huge, 4, d, NULL), 21);
    BAD(simrank_explain_gather(S, f32, 4, 4, 4, ids, ptr, ids, ptr, ptr, 2, -4, d, NULL), 22);
    /* a block that does not start on a multiple of its element's size */
    BAD(simrank_explain_gather((const char*)S + 2, f32, 4, 4, 4, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 23);
    BAD(simrank_explain_gather((const char*)S + 4, SIMRANK_EXPLAIN_ROWMAJOR_F64, 4, 1, 4, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 24);
    BAD(simrank_explain_gather((const char*)S + 1, SIMRANK_EXPLAIN_PANEL_F16, 4, 1, 4, ids, ptr, ids, ptr, ptr, 2, 4, d, NULL), 25);
    if (!strstr(simrank_explain_last_error(), "element")) return 26;
    /* no pairs, no terms: nothing to queue */
    if (simrank_explain_gather(S, f32, 4, 4, 4, NULL, ptr, NULL, ptr, ptr, 0, 0, NULL, NULL) != SIMRANK_EXPLAIN_OK) return 27;
    if (simrank_explain_gather(S, f32, 4, 4, 4, NULL, ptr, NULL, ptr, ptr, 2, 0, NULL, NULL) != SIMRANK_EXPLAIN_OK) return 28;
    /* reduce: NULL pointers, one at a time; negative sizes */
    BAD(simrank_explain_reduce(NULL, ptr, ptr, ptr, 2, 2, 2, d, d, d, ptr, NULL), 30);
    BAD(simrank_explain_reduce(d, NULL, ptr, ptr, 2, 2, 2, d, d, d, ptr, NULL), 31);
    BAD(simrank_explain_reduce(d, ptr, NULL, ptr, 2, 2, 2, d, d, d, ptr, NULL), 32);
    BAD(simrank_explain_reduce(d, ptr, ptr, NULL, 2, 2, 2, d, d, d, ptr, NULL), 33);
    BAD(simrank_explain_reduce(d, ptr, ptr, ptr, 2, 2, 2, NULL, d, d, ptr, NULL), 34);
    BAD(simrank_explain_reduce(d, ptr, ptr, ptr, 2, 2, 2, d, NULL, d, ptr, NULL), 35);
    BAD(simrank_explain_reduce(d, ptr, ptr, ptr, 2, 2, 2, d, d, NULL, ptr, NULL), 36);
    BAD(simrank_explain_reduce(d, ptr, ptr, ptr, 2, 2, 2, d, d, d, NULL, NULL), 37);
    BAD(simrank_explain_reduce(d, ptr, ptr, ptr, -1, 2, 2, d, d, d, ptr, NULL), 38);
    BAD(simrank_explain_reduce(d, ptr, ptr, ptr, huge, 2, 2, d, d, d, ptr, NULL), 39);
    BAD(simrank_explain_reduce(d, ptr, ptr, ptr, 2, -2, 2, d, d, d, ptr, NULL), 40);
    BAD(simrank_explain_reduce(d, ptr, ptr, ptr, 2, 2, -2, d, d, d, ptr, NULL), 41);
    if (simrank_explain_reduce(NULL, ptr, ptr, ptr, 0, 0, 0, NULL, NULL, NULL, NULL, NULL) != SIMRANK_EXPLAIN_OK) return 42;
    /* select: NULL pointers, one at a time; a bad k; negative sizes */
    BAD(simrank_explain_select(d, NULL, ptr, ptr, 2, 3, ids, ids, d, NULL), 50);
    BAD(simrank_explain_select(d, ptr, NULL, ptr, 2, 3, ids, ids, d, NULL), 51);
    BAD(simrank_explain_select(d, ptr, ptr, NULL, 2, 3, ids, ids, d, NULL), 52);
    BAD(simrank_explain_select(d, ptr, ptr, ptr, 2, 3, NULL, ids, d, NULL), 53);
    BAD(simrank_explain_select(d, ptr, ptr, ptr, 2, 3, ids, NULL, d, NULL), 54);
    BAD(simrank_explain_select(d, ptr, ptr, ptr, 2, 3, ids, ids, NULL, NULL), 55);
    BAD(simrank_explain_select(d, ptr, ptr, ptr, 2, 0, ids, ids, d, NULL), 56);
    BAD(simrank_explain_select(d, ptr, ptr, ptr, 2, -1, ids, ids, d, NULL), 57);
    BAD(simrank_explain_select(d, ptr, ptr, ptr, 2, SIMRANK_EXPLAIN_MAX_K + 1, ids, ids, d, NULL), 58);
    if (!strstr(simrank_explain_last_error(), "k must")) return 59;
    BAD(simrank_explain_select(d, ptr, ptr, ptr, -1, 3, ids, ids, d, NULL), 60);
    BAD(simrank_explain_select(d, ptr, ptr, ptr, huge, 3, ids, ids, d, NULL), 61);
    if (simrank_explain_select(NULL, ptr, ptr, ptr, 0, 3, NULL, NULL, NULL, NULL) != SIMRANK_EXPLAIN_OK) return 62;
    printf("explain %d ok\n", simrank_explain_version());
    return 0;
}
''')


# ---- every refusal comes before any device work -------------------------------------------------------------------------------
def guard(monkeypatch):
    for name in ("run", "run_lists", "load", "pairs_of_lists"):
        monkeypatch.setattr(_explain, name, boom)


def test_argument_checks_need_no_device(monkeypatch):
    guard(monkeypatch)
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().explain(["a"], ["b"])
    est = guarded_estimator()                              # a: neighbours c, a; b: none; c: b
    for a, b in ((["a"], ["b", "c"]), ([], ["a"]), (["a", "b"], ["c"])):
        with pytest.raises(ValueError, match="same length"):
            est.explain(a, b)
    for bad in ("ab", b"a", None, 7, {"a": 0}, {"a"}, iter(["a"])):
        with pytest.raises(ValueError, match="sequence"):
            est.explain(bad, ["b"])
        with pytest.raises(ValueError, match="sequence"):
            est.explain(["b"], bad)
    with pytest.raises(ValueError, match=r"a\[1\] == b\[1\]"):
        est.explain(["a", "c"], ["b", "c"])
    for bad in (0, -1, 1025, True, np.True_, 1.5, None, "3", [3]):
        with pytest.raises(ValueError, match="k must"):
            est.explain(["a"], ["b"], k=bad)
    for bad in (0, -1, True, 1.5, None, "3"):
        with pytest.raises(ValueError, match="max_terms"):
            est.explain(["a"], ["b"], max_terms=bad)
    for bad in (2, 0, "1"):
        with pytest.raises(ValueError, match="group"):
            est.explain(["a"], ["b"], group=bad)
    with pytest.raises(KeyError, match="z"):
        est.explain(["a", "z"], ["b", "c"])
    with pytest.raises(KeyError, match="z"):
        est.explain(["a", "b"], ["b", "z"])
    # |I(a)| * |I(c)| = 2 * 1 terms: the pair is named
    with pytest.raises(ValueError, match=r"\('a', 'c'\).*2 x 1 = 2 terms.*max_terms = 1"):
        est.explain(["b", "a"], ["c", "c"], max_terms=1)
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.explain(["a"], ["b"])


def test_a_strict_bipartite_fit_refuses_group_2_as_fold_in_does(monkeypatch):
    guard(monkeypatch)
    one = types.SimpleNamespace(csr=_Csr, rowscale=_Spec.rowscale, storage="f32", apriori=None, evidence_from=_Csr)
    two = types.SimpleNamespace(csr=_Csr(), rowscale=_Spec.rowscale, storage="f32", apriori=None, evidence_from=_Csr)
    solver = _neighbors.NeighborSolver(None, [one, two], [_Tables(), _Tables()])
    solver._make_reader = boom
    est = SRA.BipartiteSimRank()._keep(solver, [(0, ["a", "b", "c"]), (1, ["x", "y", "z"])])
    with pytest.raises(ValueError, match="strict_reference=True.*Evidence_N1"):
        est.explain(["x"], ["y"], group=2)
    with pytest.raises(ValueError, match="group must be 1 or 2"):
        est.explain(["a"], ["b"])
    with pytest.raises(ValueError, match="max_terms"):            # group 1 passes the gate and reaches the next refusal
        est.explain(["a"], ["c"], group=1, max_terms=1)


# ---- the host path of a pruned model ------------------------------------------------------------------------------------------
def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def hand_made():
    """8 nodes, 3 kept entries each: absent entries (-1), a kept NaN, a kept -0.0, and a plateau of 0.5 that spans several
    rows and columns (ties across via_a and via_b); everything dyadic, so every sum is exact."""
    nan = float("nan")
    ids = np.array([[1, 2, 3], [0, 2, 3], [3, 1, -1], [2, 1, 0], [5, 6, -1], [4, 6, 7], [5, -1, -1], [-1, -1, -1]], dtype=np.int32)
    vals = np.array([[0.5, 0.5, 0.25], [0.5, 0.5, 0.5], [0.75, nan, 0.0], [0.5, 0.5, -0.0], [0.125, 0.0625, 0.0],
                     [0.125, 0.5, -0.25], [0.5, 0.0, 0.0], [0.0, 0.0, 0.0]])
    diag = np.array([1.0, 1.0, 0.5, 1.0, 1.0, 0.75, 1.0, 1.0])
    P = np.zeros((8, 8))
    for r in range(8):
        kept = ids[r] >= 0
        P[r, ids[r][kept]] = vals[r][kept]
        P[r, r] = diag[r]
    # the graph: lists out of order, a node without neighbours (7), common neighbours (0 and 1 share 2 and 3)
    rows = [[3, 1, 2], [2, 0, 3], [1, 3, 0, 2], [0, 1], [6, 5], [7, 4, 6], [5, 2], []]
    rowptr = np.zeros(9, dtype=np.int32)
    np.cumsum([len(r) for r in rows], out=rowptr[1:])
    col = np.array([c for r in rows for c in r], dtype=np.int32)
    csr = CSR(8, 8, rowptr, col, np.ones(col.size))
    scale = np.array([0.5, 0.25, 0.25, 0.5, 0.5, 0.0, 0.5, 0.0])
    return ids, vals, diag, P, csr, scale


@pytest.mark.parametrize("evidence", [False, True])
def test_a_pruned_model_is_explained_on_the_host_for_its_matrix_p(monkeypatch, evidence):
    for name in ("run", "load"):
        monkeypatch.setattr(_explain, name, boom)              # (a pruned model needs no library)
    ids, vals, diag, P, csr, scale = hand_made()
    ops = HostOps()
    coef, lbd = 0.75, (0.25 if evidence else 0.0)
    spec = types.SimpleNamespace(csr=csr, rowscale=scale, coef=coef, lbd=lbd, storage="f32", apriori=None,
                                 evidence_from=csr if evidence else None)
    solver = _neighbors.NeighborSolver(ops, [spec], [_neighbors.Tables.from_host(ops, ids, vals, diag)])
    names = list("abcdefgh")
    est = SRA.SimRank()._keep(solver, [(0, names)])
    pairs_in = [(0, 1), (1, 0), (2, 3), (0, 1), (4, 5), (5, 4), (7, 0), (0, 7), (6, 2), (3, 2)]
    for k in (1, 3, 1024):
        pairs, terms, neighbors = est.explain([names[a] for a, _ in pairs_in], [names[b] for _, b in pairs_in], k=k)
        want, want_terms, want_nb = ER.explain_ref(P, csr, scale, coef, lbd, evidence, pairs_in, k)
        assert pairs.columns.tolist() == ["a", "b", "similarity", "terms", "contributors", "common", "evidence", "raw", "propagated"]
        assert pairs["a"].tolist() == [names[a] for a, _ in pairs_in] and pairs["b"].tolist() == [names[b] for _, b in pairs_in]
        assert same(pairs["similarity"], [P[a, b] for a, b in pairs_in])
        for name in ("terms", "contributors", "common"):
            assert pairs[name].dtype == np.int64 and pairs[name].tolist() == want[name].tolist(), name
        for name in ("evidence", "raw", "propagated"):
            assert pairs[name].dtype == np.float64 and same(pairs[name], want[name]), name
        assert terms.columns.tolist() == ["pair", "rank", "via_a", "via_b", "similarity", "share"]
        assert list(zip(terms["pair"], terms["rank"], terms["via_a"], terms["via_b"])) == \
            [(p, r, names[i], names[j]) for p, r, i, j, _ in want_terms]
        assert same(terms["similarity"], [v for *_, v in want_terms])
        with np.errstate(invalid="ignore", divide="ignore"):
            assert same(terms["share"], [v / want["raw"][p] for p, *_, v in want_terms])
        assert neighbors.columns.tolist() == ["pair", "of", "neighbor", "sum", "share"]
        assert list(zip(neighbors["pair"], neighbors["of"], neighbors["neighbor"])) == [(p, of, names[i]) for p, of, i, _, _ in want_nb]
        assert same(neighbors["sum"], [s for *_, s, _ in want_nb])
    # what the cases are there for
    assert pairs["common"].tolist()[:3] == [2, 2, 2] and pairs["terms"].tolist()[6:8] == [0, 0]
    assert np.isnan(pairs["raw"][2]) and pairs["contributors"][2] < pairs["terms"][2]          # the kept NaN poisons its pair
    assert pairs["raw"][6] == 0.0 and pairs["propagated"][6] == 0.0 and not (terms["pair"] == 6).any()
    assert pairs["evidence"].tolist()[:2] == ([0.75, 0.75] if evidence else [1.0, 1.0])
    assert pairs["common"][5] == 0                            # (f's row scale is 0: the count is not taken)
    t0 = terms[terms["pair"] == 0]
    assert t0["similarity"].tolist() == [1.0, 0.75] + [0.5] * 5                                   # the plateau, in frame order
    assert list(zip(t0["via_a"], t0["via_b"]))[2:] == [("b", "a"), ("b", "c"), ("b", "d"), ("c", "c"), ("d", "c")]
    assert pairs.iloc[0].tolist() == pairs.iloc[3].tolist()  # a repeated pair
    assert est.kept_neighbors == 3                            # the model is as it was
    est.release()
    assert not ops.live


# ---- the anchor to the reference -----------------------------------------------------------------------------------------------
ANCHORS = [("SimRank_er128", True), ("SimRank_er64_weighted", True), ("SimRankPP_er64_cols", True), ("AprioriSimRank_er64", True),
           ("AprioriSimRank_er64_asym", True), ("BipartiteSimRank_b5030", True), ("BipartiteSimRank_b40_weighted", True),
           ("BipartiteSimRankPP_b40", False), ("BipartitleAprioriSimRank_b40", False)]


def side_as_lists(sd):
    """(csr-like, rowscale) of one side of an oracle result: the pattern of its graph, and per row the one value its
    weighted row holds (0 for a row the reference scaled to nothing)."""
    G, W = np.asarray(sd["G"]), np.asarray(sd["W"], dtype=np.float64)
    lists = [np.flatnonzero(G[a] > 0) for a in range(G.shape[0])]
    scale = np.zeros(G.shape[0])
    for a, l in enumerate(lists):
        if l.size:
            scale[a] = W[a, l[0]]
            assert (W[a, l] == scale[a]).all() and np.count_nonzero(W[a]) in (0, l.size)   # W = diag(rowscale) . pattern
    rowptr = np.zeros(G.shape[0] + 1, dtype=np.int64)
    np.cumsum([l.size for l in lists], out=rowptr[1:])
    col = np.concatenate(lists) if rowptr[-1] else np.empty(0, dtype=np.int64)
    return types.SimpleNamespace(rowptr=rowptr, col=col), scale


@pytest.mark.parametrize("name,strict", ANCHORS)
def test_propagated_is_the_references_next_update(name, strict):
    """``propagated (+ lbd * prior[a, b])`` of ``explain_ref`` on the matrices after t = 3 updates against the reference's
    matrix after 4, for EVERY off-diagonal pair, relative within ``(|I(a)| + |I(b)| + 8) * 2^-53``: the reference rounds
    each of its two dot products' |I(a)| and |I(b)| non-zero terms and their sums once each and multiplies three or four
    times; ``explain_ref`` sums exactly, rounds once and multiplies five times (``foldin_ref.tolerance`` derives the same
    bound the same way).  Group 2 of the bipartite classes reads S1 of the SAME update (the reference's Gauss-Seidel
    order), so there S2 after 3 updates is explained from S1 after 3."""
    g = Golden(name)
    r3 = R.run_oracle(g, iterations=3, eps=1e-12, verbose=False, strict_reference=strict)
    r4 = R.run_oracle(g, iterations=4, eps=1e-12, verbose=False, strict_reference=strict)
    assert r3["k"] is None and r4["k"] is None          # 3 and 4 updates were really applied
    checked = 0
    for sd in R.sides_of(g, r3, {"strict_reference": strict}):
        csr, scale = side_as_lists(sd)
        n = scale.size
        pairs_in = [(a, b) for a in range(n) for b in range(n) if a != b]
        evidence = sd["pattern"] is not None
        lbd = 0.0 if sd["lbd"] is None else sd["lbd"]
        got, _, _ = ER.explain_ref(r3[sd["reads"]], csr, scale, sd["coef"], lbd, evidence, pairs_in, 1)
        want = (r3 if sd["group"] == 2 else r4)[sd["writes"]]
        deg = np.diff(csr.rowptr)
        pattern = np.asarray(sd["G"]) > 0
        for p, (a, b) in enumerate(pairs_in):
            value = got["propagated"][p] + (lbd * float(np.asarray(sd["prior"])[a, b]) if sd["prior"] is not None else 0.0)
            tol = (deg[a] + deg[b] + 8) * 2.0 ** -53
            assert abs(value - want[a, b]) <= tol * abs(want[a, b]), (name, sd["group"], a, b, value, want[a, b])
            assert got["terms"][p] == deg[a] * deg[b]
            brute = int((pattern[a] & pattern[b]).sum()) if scale[a] > 0 and scale[b] > 0 else 0
            assert got["common"][p] == brute
        checked += int((want[~np.eye(n, dtype=bool)] > 0).sum())
    assert checked > 50                                   # the pairs do have values to explain
