"""The kept-model queries pinned through the estimator's public methods, on a machine without a GPU: the full result of
every query a pruned model answers on the host (values bit for bit against the suite's references, index, columns and
dtypes), one-sided and two-sided; the cross-side lookup of ``fold_in``, ``recommend``, ``rank_recommended`` and ``explain``
on a recording solver; the long frames of the four device selections; and the order in which every public method of
``_KeptModel`` refuses (no model, a released model, a model whose device and lists raise when touched).  The last section
holds the dispatch scopes of ``_query.SolverQueries`` (``lists``, ``one_block``) on doubles."""
import types

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _model, _neighbors, _query
from simrank_amd.ingest import CSR
from tests import cluster_ref as CR
from tests import explain_ref as ER
from tests import groups_ref as GR
from tests import kmedoids_ref as KR
from tests import linkage_ref as LR
from tests import profile_ref as PR
from tests.test_cluster_cpu import HostOps, _FullSpec, boom, guarded_estimator, lists_case


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def exact(got, want, dtype=np.float64):
    """``got`` has ``dtype`` and the bytes of ``want`` (cast to it): bit for bit, NaN payloads and signed zeros included."""
    got = np.asarray(got)
    assert got.dtype == dtype, (got.dtype, dtype)
    want = np.asarray(want, dtype=dtype)
    assert got.shape == want.shape and np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), (got, want)
    return True


def frame_is(df, index, columns):
    """``columns``: [(name, dtype, values)] in the frame's order; ``index``: its labels (None: 0 .. len - 1)."""
    assert isinstance(df, pd.DataFrame) and df.columns.tolist() == [c for c, _, _ in columns], df.columns.tolist()
    assert df.index.tolist() == (list(range(len(df))) if index is None else list(index))
    for name, dtype, values in columns:
        if dtype is object:
            assert df[name].tolist() == list(values), name
        else:
            exact(df[name].to_numpy(), values, dtype)
    return True


def csr_of(rows, n_cols):
    rowptr = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum([len(r) for r in rows], out=rowptr[1:])
    col = np.array([c for r in rows for c in r], dtype=np.int32)
    return CSR(len(rows), n_cols, rowptr, col, np.ones(col.size))


def matrix_p(ids, vals, diag):
    P = CR.matrix_of_lists(ids, vals)
    P[np.arange(len(P)), np.arange(len(P))] = diag
    return P


def spec_of(csr, scale, evidence_from=None, coef=0.75, lbd=0.0):
    return types.SimpleNamespace(csr=csr, rowscale=np.asarray(scale, dtype=np.float64), coef=coef, lbd=lbd, storage="f32",
                                 apriori=None, evidence_from=evidence_from)


# side A: ``lists_case`` (6 nodes, 3 slots: a kept NaN, a -0.0, a negative value, 1e-9); side B: 7 nodes, 2 slots, dyadic
IDS_A, VALS_A = lists_case()
DIAG_A = np.array([1.0, 0.5, 1.0, 1.0, 0.75, 1.0])
P_A = matrix_p(IDS_A, VALS_A, DIAG_A)
IDS_B = np.array([[1, 4], [0, 2], [1, 5], [-1, -1], [5, 0], [4, 2], [0, -1]], dtype=np.int32)
VALS_B = np.array([[0.5, 0.25], [0.75, 0.125], [0.5, 0.375], [0, 0], [0.875, 0.0625], [-0.5, -0.25], [0.3, 0]])
DIAG_B = np.array([1.0, 1.0, 0.25, 1.0, 1.0, 0.5, 1.0])
P_B = matrix_p(IDS_B, VALS_B, DIAG_B)
NAMES_A, NAMES_B = [10, 20, 30, 40, 50, 60], list("tuvwxyz")
# the graphs.  No list holds node 4 of side A, so that no double sum adds the 1e-9 of P_A[5, 4] to anything: every sum of
# the explain cases is then exact, and the exact reference (math.fsum) has the bits of any order of additions
ROWS_AA = [[3, 1], [2, 0], [1, 3, 0], [0, 1], [5], []]                     # one-sided: side A's in-neighbours, on side A
ROWS_AB = [[1, 4], [0, 2, 6], [5], [3, 1], [], [6, 0]]                     # two-sided: side A's neighbours, on side B
ROWS_BA = [[0, 3], [1, 0], [3, 5], [2], [0, 1, 3], [], [5, 2]]             # side B's neighbours, on side A
SCALE_A, SCALE_B = [0.5, 0.25, 0.25, 0.5, 1.0, 0.0], [0.5, 0.5, 0.25, 1.0, 0.125, 0.0, 0.5]
LABELS_A, LABELS_B = np.array([1, 1, 2, 1, 2, 3]), np.array([0, 0, 0, 0, 10, 10, -4])


def one_sided(ops):
    spec = spec_of(csr_of(ROWS_AA, 6), SCALE_A)
    solver = _neighbors.NeighborSolver(ops, [spec], [_neighbors.Tables.from_host(ops, IDS_A, VALS_A, DIAG_A)])
    return SRA.SimRank()._keep(solver, [(0, list("abcdef"))])


def two_sided(ops, kind="plain"):
    """A pruned bipartite model: "plain" (no evidence), "pp" (every side its own evidence), "strict" (the group-2 update
    gated by group 1's pattern)."""
    g12, g21 = csr_of(ROWS_AB, 7), csr_of(ROWS_BA, 6)
    ev = {"plain": (None, None), "pp": (g12, g21), "strict": (g12, g12)}[kind]
    lbd = 0.0 if kind == "plain" else 0.25
    specs = [spec_of(g12, SCALE_A, ev[0], lbd=lbd), spec_of(g21, SCALE_B, ev[1], coef=0.5, lbd=lbd)]
    tables = [_neighbors.Tables.from_host(ops, IDS_A, VALS_A, DIAG_A), _neighbors.Tables.from_host(ops, IDS_B, VALS_B, DIAG_B)]
    klass = SRA.BipartiteSimRank if kind == "plain" else SRA.BipartiteSimRankPP
    return klass()._keep(_neighbors.NeighborSolver(ops, specs, tables), [(0, NAMES_A), (1, NAMES_B)])


# ---- what each query must return, from the references -------------------------------------------------------------------------
TS = [0.5, 0.0, 0.75, 0.5, -1, 2.0, 1e-9, 0.3]


def check_components(got_one, got_many, P, names):
    assert isinstance(got_one, pd.Series) and got_one.name == "component" and got_one.index.tolist() == names
    exact(got_one.to_numpy(), CR.components(P, [0.3])[0], np.int64)
    assert isinstance(got_many, pd.DataFrame) and got_many.index.tolist() == names
    assert got_many.columns.tolist() == [float(t) for t in TS] and (got_many.dtypes == np.int64).all()
    exact(got_many.to_numpy().T, CR.components(P, TS), np.int64)


def check_linkage(Z, P, floor):
    want = LR.linkage(P, floor)
    frame_is(Z, None, [("left", np.int64, want[0]), ("right", np.int64, want[1]), ("similarity", np.float64, want[2]),
                       ("size", np.int64, want[3])])
    return want


def check_cut(est, Z, P, names, want_rows, **group):
    for t in (0.125, 0.3, 0.75):
        got = est.cut(Z, t=t, **group)
        assert isinstance(got, pd.Series) and got.name == "component" and got.index.tolist() == names
        exact(got.to_numpy(), LR.cut(len(P), want_rows, t=t), np.int64)
        exact(got.to_numpy(), CR.components(P, [t])[0], np.int64)
    m = len(P) - len(Z)
    exact(est.cut(Z, n_clusters=m + 1, **group).to_numpy(), LR.cut(len(P), want_rows, n_clusters=m + 1), np.int64)


def check_profile(counts, thresholds_for, P):
    ts = [0.5, 0.75, 0.1, 0.0, -0.0, -1e-9, -1.0, 2.0, 1e-12]
    exact(counts(ts), PR.count_pairs(P, ts), np.int64)
    for m in (1, 2, 3, 5, 6, 9, 28, 29, 30, 41, 42, 10 ** 9):
        got = thresholds_for(m)
        want = PR.threshold_for(P, m)
        assert isinstance(got, tuple) and isinstance(got[0], float) and isinstance(got[1], int)
        assert exact(np.float64(got[0]), np.float64(want[0])) and got[1] == want[1], m


def check_groups(est, P, lab, names, **group):
    cl = sorted(set(lab.tolist()))
    want_means = GR.means(P, lab)
    own, near, other = GR.quality(P, lab, want_means)
    sil = GR.silhouettes(lab, own, other)
    q = est.cluster_quality(lab, **group)
    frame_is(q, names, [("cluster", np.int64, lab), ("own", np.float64, own), ("nearest", np.int64, near),
                        ("other", np.float64, other), ("silhouette", np.float64, sil)])
    shuffled = pd.Series(lab, index=names).iloc[np.arange(len(names))[::-1]]
    assert est.cluster_quality(shuffled, **group).equals(q)
    m = est.cluster_means(lab, **group)
    assert m.index.tolist() == names and m.columns.tolist() == cl and m.columns.name == "cluster"
    exact(m.to_numpy(), want_means)
    med = est.medoids(lab, **group)
    assert isinstance(med, pd.Series) and med.name == "medoid" and med.index.tolist() == cl and med.index.name == "cluster"
    want_med = [names[i] for _, i in sorted(GR.medoids(lab, own).items())]
    assert med.tolist() == want_med
    s = est.cluster_summary(lab, **group)
    want = GR.summary(lab, own, other, sil)
    assert s.index.tolist() == cl and s.index.name == "cluster"
    frame_is(s, cl, [("size", np.int64, [want[g][0] for g in cl]), ("medoid", object, want_med),
                     ("cohesion", np.float64, [want[g][1] for g in cl]), ("separation", np.float64, [want[g][2] for g in cl]),
                     ("silhouette", np.float64, [want[g][3] for g in cl])])


def check_kmedoids(est, P, names, seeds, **group):
    at = [names.index(s) for s in seeds]
    own_of = lambda lab: GR.quality(P, lab)[0]
    want_c, want_v, _ = KR.assign(P, at)
    a = est.assign(seeds, **group)
    frame_is(a, names, [("cluster", np.int64, want_c), ("medoid", object, [seeds[c] for c in want_c]),
                        ("similarity", np.float64, want_v)])
    for max_iter in (1, 20):
        labels, clusters, history = est.kmedoids(pd.Series(seeds, index=range(5, 5 + len(seeds))), max_iter=max_iter, **group)
        cluster, medoids, sim, sizes, cohesion, steps = KR.kmedoids(P, at, max_iter, own_of)
        frame_is(labels, names, [("cluster", np.int64, cluster), ("medoid", object, [names[medoids[c]] for c in cluster]),
                                 ("similarity", np.float64, sim)])
        assert clusters.index.name == "cluster"
        frame_is(clusters, range(len(seeds)), [("medoid", object, [names[m] for m in medoids]), ("size", np.int64, sizes),
                                               ("cohesion", np.float64, cohesion)])
        frame_is(history, None, [("moved", np.int64, [s[0] for s in steps]), ("changed", np.int64, [s[1] for s in steps]),
                                 ("objective", np.float64, [s[2] for s in steps])])
        assert len(history) <= max_iter


def check_explain(est, P_own, P_src, csr, scale, coef, lbd, evidence, pairs_in, names, src_names, **group):
    a, b = [names[x] for x, _ in pairs_in], [names[y] for _, y in pairs_in]
    for k in (1, 3, 1024):
        pairs, terms, neighbors = est.explain(a, b, k=k, **group)
        want, want_terms, want_nb = ER.explain_ref(P_src, csr, scale, coef, lbd, evidence, pairs_in, k)
        frame_is(pairs, None, [("a", object, a), ("b", object, b), ("similarity", np.float64, [P_own[x, y] for x, y in pairs_in]),
                               ("terms", np.int64, want["terms"]), ("contributors", np.int64, want["contributors"]),
                               ("common", np.int64, want["common"]), ("evidence", np.float64, want["evidence"]),
                               ("raw", np.float64, want["raw"]), ("propagated", np.float64, want["propagated"])])
        with np.errstate(invalid="ignore", divide="ignore"):
            share = [v / want["raw"][p] for p, *_, v in want_terms]
            nb_share = [s / want["raw"][p] for p, _, _, s, _ in want_nb]
        frame_is(terms, None, [("pair", np.int64, [p for p, *_ in want_terms]), ("rank", np.int64, [r for _, r, *_ in want_terms]),
                               ("via_a", object, [src_names[i] for _, _, i, _, _ in want_terms]),
                               ("via_b", object, [src_names[j] for _, _, _, j, _ in want_terms]),
                               ("similarity", np.float64, [v for *_, v in want_terms]), ("share", np.float64, share)])
        frame_is(neighbors, None, [("pair", np.int64, [p for p, *_ in want_nb]), ("of", object, [of for _, of, *_ in want_nb]),
                                   ("neighbor", object, [src_names[i] for _, _, i, _, _ in want_nb]),
                                   ("sum", np.float64, [s for *_, s, _ in want_nb]), ("share", np.float64, nb_share)])


PAIRS_A = [(0, 1), (1, 0), (2, 3), (0, 1), (4, 1), (5, 0), (0, 5), (3, 2), (4, 2)]
PAIRS_B = [(0, 1), (1, 3), (4, 6), (6, 4), (5, 0), (2, 3), (4, 0)]


# ---- a one-sided pruned model -----------------------------------------------------------------------------------------------------
def test_every_host_answered_query_of_a_one_sided_pruned_model():
    ops = HostOps()
    est = one_sided(ops)
    names = list("abcdef")
    P0 = CR.matrix_of_lists(IDS_A, VALS_A)
    before = set(ops.live)
    check_components(est.components(0.3), est.components(TS), P0, names)
    Z = est.linkage(min_similarity=0.1)
    check_cut(est, Z, P0, names, check_linkage(Z, P0, 0.1))
    check_linkage(est.linkage(0.6), P0, 0.6)
    check_profile(est.count_pairs, est.threshold_for, P_A)
    check_groups(est, P_A, LABELS_A, names)
    check_kmedoids(est, P_A, names, ["e", "b"])
    check_kmedoids(est, P_A, names, ["c"])
    spec = est._model[0].specs[0]
    check_explain(est, P_A, P_A, spec.csr, spec.rowscale, 0.75, 0.0, False, PAIRS_A, names, names)
    assert est.kept_neighbors == 3 and est.device_bytes == 6 * 3 * 12 + 6 * 8
    assert set(ops.live) == before                            # nothing was allocated and kept, nothing was freed
    # prune: as many as are kept changes nothing; fewer cuts the lists on the host; more is refused
    solver = est._model[0]
    assert est.prune(3) is est and est._model[0] is solver
    with pytest.raises(ValueError, match="kept_neighbors = 3 neighbours per node: k = 4 asks"):
        one_sided(ops).prune(4)
    assert est.prune(2) is est and est._model[0] is not solver and est.kept_neighbors == 2
    assert est.device_bytes == 6 * 2 * 12 + 6 * 8 and solver.tables[0].ids is None          # the old tables were released
    ids, vals, diag = est._model[0].tables[0].host()
    exact(ids, IDS_A[:, :2], np.int32) and exact(vals, VALS_A[:, :2]) and exact(diag, DIAG_A)
    check_components(est.components(0.3), est.components(TS), CR.matrix_of_lists(IDS_A[:, :2], VALS_A[:, :2]), names)
    est.release()
    assert est.kept_neighbors is None


# ---- a two-sided pruned model: the cross-side lookup ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "pp", "strict"])
def test_every_host_answered_query_of_a_two_sided_pruned_model(kind):
    ops = HostOps()
    est = two_sided(ops, kind)
    P0 = (CR.matrix_of_lists(IDS_A, VALS_A), CR.matrix_of_lists(IDS_B, VALS_B))
    sides = ((1, NAMES_A, P_A, P0[0], LABELS_A, [50, 20]), (2, NAMES_B, P_B, P0[1], LABELS_B, ["x", "u", "z"]))
    one, many, Z = est.components(0.3), est.components(TS), est.linkage(0.1)
    counts, picks = est.count_pairs([0.5, 0.75, 0.1, 0.0, -0.0, -1e-9, -1.0, 2.0, 1e-12]), est.threshold_for(5)
    assert all(isinstance(x, tuple) and len(x) == 2 for x in (one, many, Z, counts, picks))
    for s, (group, names, P, P_off, lab, seeds) in enumerate(sides):
        check_components(one[s], many[s], P_off, names)
        check_cut(est, Z[s], P_off, names, check_linkage(Z[s], P_off, 0.1), group=group)
        check_profile(lambda ts: est.count_pairs(ts)[s], lambda m: est.threshold_for(m)[s], P)
        check_groups(est, P, lab, names, group=group)
        check_kmedoids(est, P, names, seeds, group=group)
        for call in (lambda: est.cluster_quality(lab), lambda: est.assign(seeds), lambda: est.cut(Z[s], t=0.3),
                     lambda: est.explain([names[0]], [names[1]])):
            with pytest.raises(ValueError, match="group must be 1 or 2, not None"):
                call()
    # explain: the pairs of one group, their neighbours and the matrix that is read of the other
    s1, s2 = est._model[0].specs
    evidence, lbd = kind != "plain", 0.0 if kind == "plain" else 0.25
    check_explain(est, P_A, P_B, s1.csr, s1.rowscale, 0.75, lbd, evidence, PAIRS_A, NAMES_A, NAMES_B, group=1)
    if kind == "strict":
        with pytest.raises(ValueError, match="strict_reference=True.*Evidence_N1"):
            est.explain(["t"], ["u"], group=2)
    else:
        check_explain(est, P_B, P_A, s2.csr, s2.rowscale, 0.5, lbd, evidence, PAIRS_B, NAMES_B, NAMES_A, group=2)
    with pytest.raises(KeyError, match="t"):
        est.explain(["t"], ["u"], group=1)                    # (a label of the other group)
    assert est.kept_neighbors == (3, 2) and est.device_bytes == 6 * 3 * 12 + 6 * 8 + 7 * 2 * 12 + 7 * 8
    with pytest.raises(ValueError, match="whole rows"):
        est.fold_in([["t"]], group=1)
    assert est.prune(2) is est and est.kept_neighbors == 2 and est.device_bytes == 6 * 2 * 12 + 6 * 8 + 7 * 2 * 12 + 7 * 8
    ids, vals, _ = est._model[0].tables[0].host()
    exact(ids, IDS_A[:, :2], np.int32) and exact(vals, VALS_A[:, :2])
    ids, vals, _ = est._model[0].tables[1].host()
    exact(ids, IDS_B, np.int32) and exact(vals, VALS_B)
    est.release()
    assert not ops.live


# ---- the cross-side lookup and the long frames of the device selections, on a recording solver --------------------------------------
IDX = np.array([[2, 0, -1], [-1, -1, -1], [1, 2, 0], [0, -1, -1]], dtype=np.int32)
VAL = np.array([[0.5, -0.0, 0.0], [0.0, 0.0, 0.0], [1.0, float("nan"), 0.25], [0.125, 0.0, 0.0]])


class Recorder:
    """Stands in for a kept solver that holds its matrices: records what the estimator asks, answers the device selections
    with the first rows of ``IDX`` / ``VAL`` (-1: an empty slot)."""
    mode = "sparse"

    def __init__(self, specs, n):
        self.specs, self.n, self.calls = specs, n, []

    def release(self):
        pass

    def _best(self, what, j, m, k):
        self.calls.append((what, j, k))
        return IDX[:m, :k].copy(), VAL[:m, :k].copy()

    def topk_of(self, j, ids, k):
        return self._best(("topk_of", ids.tolist()), j, len(ids), k)

    def fold_in(self, j, lists, w, prior=None, top_k=None):
        what = ("fold_in", [l.tolist() for l in lists], w.tolist())
        if top_k is None:
            self.calls.append((what, j, None))
            return np.arange(len(lists) * self.n[j], dtype=np.float64).reshape(len(lists), self.n[j])
        return self._best(what, j, len(lists), top_k)

    def score_sets(self, j, ptr, ids, w, k=None, excl=None):
        what = ("score_sets", ptr.tolist(), ids.tolist(), w.tolist(), None if excl is None else excl[1].tolist())
        if k is None:
            self.calls.append((what, j, None))
            return np.arange((ptr.size - 1) * self.n[j], dtype=np.float64).reshape(ptr.size - 1, self.n[j])
        return self._best(what, j, ptr.size - 1, k)

    def score_ranks(self, j, ptr, ids, w, excl, tptr, tids):
        self.calls.append((("score_ranks", ptr.tolist(), ids.tolist(), w.tolist(), tptr.tolist(), tids.tolist()), j, None))
        score = np.where(np.arange(tids.size) % 2 == 0, 0.5, -np.inf)
        return score, np.arange(tids.size, dtype=np.int64), np.full(ptr.size - 1, 3, dtype=np.int64)


# rows of IDX with their -1 slots dropped: (row, rank, id, value)
KEPT = [(0, 1, 2, 0.5), (0, 2, 0, -0.0), (2, 1, 1, 1.0), (2, 2, 2, float("nan")), (2, 3, 0, 0.25), (3, 1, 0, 0.125)]


def long_frame_is(df, first, value, who, out_names, rows=KEPT):
    frame_is(df, None, [(first, object, [who[r] for r, *_ in rows]), ("rank", np.int64, [k for _, k, *_ in rows]),
                        ("neighbor", object, [out_names[i] for _, _, i, _ in rows]), (value, np.float64, [v for *_, v in rows])])


def test_the_long_frames_of_the_four_device_selections():
    est = SRA.SimRank()
    # d's row has no in-neighbour: recommend drops its rows whatever the device selected
    spec = spec_of(csr_of([[1, 2], [0], [2, 0, 1], []], 4), [0.5, 1.0, 0.25, 0.0])
    solver = Recorder([spec], [4])
    est._keep(solver, [(0, list("abcd"))])
    est._weighted = False
    names = list("abcd")
    long_frame_is(est.most_similar(["d", "a", "b", "d"], 3), "node", "similarity", ["d", "a", "b", "d"], names)
    assert solver.calls[-1] == (("topk_of", [3, 0, 1, 3]), 0, 3)
    got = est.fold_in([["a"], [], ["c", "b"], ["d"]], top_k=3, names=["w", "x", "y", "z"])
    long_frame_is(got, "node", "similarity", ["w", "x", "y", "z"], names)
    assert solver.calls[-1] == (("fold_in", [[0], [], [2, 1], [3]], [1.0, 0.0, 0.5, 1.0]), 0, 3)
    long_frame_is(est.fold_in([["a"], [], ["c", "b"], ["d"]], top_k=3), "node", "similarity", [0, 1, 2, 3], names)
    got = est.score_sets([["a"], [], ["c", "b"], ["d"]], top_k=3, names=["w", "x", "y", "z"])
    long_frame_is(got, "set", "score", ["w", "x", "y", "z"], names)
    assert solver.calls[-1] == (("score_sets", [0, 1, 1, 3, 4], [0, 2, 1, 3], [1.0] * 4, [0, 2, 1, 3]), 0, 3)
    long_frame_is(est.score_sets([["a"], [], ["c", "b"], ["d"]], top_k=3), "set", "score", [0, 1, 2, 3], names)
    # recommend: the keep_rows mask (a node without neighbours) on top of the -1 slots
    got = est.recommend(["c", "b", "a", "d"], 3)
    long_frame_is(got, "node", "score", ["c", "b", "a", "d"], names, [r for r in KEPT if r[0] != 3])
    assert solver.calls[-1][0][1:3] == ([0, 3, 4, 6, 6], [2, 0, 1, 0, 1, 2]) and solver.calls[-1][1:] == (0, 3)
    got = est.recommend(["d", "b", "d", "a"], 2)
    long_frame_is(got, "node", "score", ["d", "b", "d", "a"], names, [(3, 1, 0, 0.125)])
    # the dense answers of the two
    dense = est.fold_in([["a"], ["c", "b"]], names=["w", "y"])
    assert dense.index.tolist() == ["w", "y"] and dense.columns.tolist() == names and exact(dense.to_numpy(), np.arange(8.0).reshape(2, 4))
    dense = est.score_sets([["a"], ["c", "b"]])
    assert dense.index.tolist() == [0, 1] and dense.columns.tolist() == names and exact(dense.to_numpy(), np.arange(8.0).reshape(2, 4))


@pytest.mark.parametrize("strict", [False, True])
def test_the_cross_side_lookup_of_a_two_sided_model(strict):
    g12, g21 = csr_of([[1, 0], [2], []], 3), csr_of([[0], [0, 1], [1]], 3)
    specs = [spec_of(g12, [0.5, 1.0, 0.0], g12), spec_of(g21, [1.0, 0.5, 0.25], g12 if strict else g21)]
    solver = Recorder(specs, [3, 3])
    est = SRA.BipartiteSimRankPP()._keep(solver, [(0, [1, 2, 3]), (1, ["x", "y", "z"])])
    est._weighted = False
    # fold_in: a new group-1 node is given by group-2 labels and answered over group 1
    got = est.fold_in([["y", "x"], ["z"], []], group=1, top_k=2)
    assert solver.calls[-1] == (("fold_in", [[1, 0], [2], []], [0.5, 1.0, 0.0]), 0, 2)
    long_frame_is(got, "node", "similarity", [0, 1, 2], [1, 2, 3], [(0, 1, 2, 0.5), (0, 2, 0, -0.0), (2, 1, 1, 1.0), (2, 2, 2, float("nan"))])
    assert est.fold_in([["y"]], group=1).columns.tolist() == [1, 2, 3]
    with pytest.raises(KeyError):
        est.fold_in([[1]], group=1)
    if strict:
        for call in (lambda: est.fold_in([[1, 3]], group=2), lambda: est.fold_in([["zz"]], group=2, top_k=0)):
            with pytest.raises(ValueError, match="strict_reference=True.*Evidence_N1"):
                call()
    else:
        assert est.fold_in([[3, 1]], group=2).columns.tolist() == ["x", "y", "z"]
        assert solver.calls[-1] == (("fold_in", [[2, 0]], [0.5]), 1, None)
    # recommend: the baskets of group-1 nodes hold group-2 nodes, scored on group 2's matrix, and the other way round
    got = est.recommend([3, 1, 2], 2, group=1)
    assert solver.calls[-1] == (("score_sets", [0, 0, 2, 3], [1, 0, 2], [0.5, 0.5, 1.0], [1, 0, 2]), 1, 2)
    long_frame_is(got, "node", "score", [3, 1, 2], ["x", "y", "z"], [(2, 1, 1, 1.0), (2, 2, 2, float("nan"))])
    got = est.recommend(["z", "x"], 1, group=2, exclude_seen=False)
    assert solver.calls[-1] == (("score_sets", [0, 1, 2], [1, 0], [0.25, 1.0], None), 0, 1)
    long_frame_is(got, "node", "score", ["z", "x"], [1, 2, 3], [(0, 1, 2, 0.5)])
    with pytest.raises(KeyError):
        est.recommend(["x"], 1, group=1)
    # rank_recommended / evaluate: the targets are labels of the group the basket lives in
    got = est.rank_recommended([1, 3], [["z", "x"], ["y"]], group=1)
    assert solver.calls[-1] == (("score_ranks", [0, 2, 2], [1, 0], [0.5, 0.5], [0, 2, 3], [2, 0, 1]), 1, None)
    frame_is(got, None, [("node", object, [1, 1, 3]), ("target", object, ["z", "x", "y"]), ("score", np.float64, [0.5, -np.inf, 0.5]),
                         ("rank", np.int64, [1, 0, 0]), ("candidates", np.int64, [3, 3, 0])])
    ev = est.evaluate(["y"], [[2, 1]], ks=(1, 2), group=2)
    assert solver.calls[-1] == (("score_ranks", [0, 2], [0, 1], [0.5, 0.5], [0, 2], [1, 0]), 0, None)
    assert ev.columns.tolist() == ["node", "targets", "not_candidates", "best_rank", "reciprocal_rank", "hits@1", "hits@2"]
    assert ev.iloc[0].tolist() == ["y", 2, 1, 1, 1.0, 1, 1]
    with pytest.raises(KeyError):
        est.rank_recommended([1], [[2]], group=1)
    # the queries of one side
    long_frame_is(est.most_similar(["z", "x", "y", "x"], 3, group=2), "node", "similarity", ["z", "x", "y", "x"], ["x", "y", "z"])
    assert solver.calls[-1] == (("topk_of", [2, 0, 1, 0]), 1, 3)


# ---- the order of the refusals ------------------------------------------------------------------------------------------------------
NO_MODEL, RELEASED = (RuntimeError, "there is no kept model: call fit"), (RuntimeError, "the kept model was released")
ONE_GROUP = (ValueError, "this class has one node group: group must be None or 1, not 2")
K_POSITIVE = (ValueError, "k must be a positive integer, not 0")
EXCLUDE_SEEN = (ValueError, "exclude_seen must be True or False, not 1")
Z_NONE = None

# (what, the call, "arg": refused the same way in every state | "model": no model / released come first, the refusal of
#  a guarded model (None: the call is not made on it: it would reach the device))
REFUSALS = [
    ("rows: group before labels", lambda e: e.rows(["zz"], group=2), "model", ONE_GROUP),
    ("rows: labels", lambda e: e.rows(["a", "zz"]), "model", (KeyError, "zz")),
    ("similarity: lengths first", lambda e: e.similarity(["a", "b"], ["a"], group=2), "arg", (ValueError, r"same length \(2 != 1\)")),
    ("similarity: group before labels", lambda e: e.similarity(["zz"], ["a"], group=2), "model", ONE_GROUP),
    ("similarity: labels", lambda e: e.similarity(["a"], ["zz"]), "model", (KeyError, "zz")),
    ("most_similar: k first", lambda e: e.most_similar(["zz"], 0, group=2), "arg", K_POSITIVE),
    ("most_similar: group before labels", lambda e: e.most_similar(["zz"], 1, group=2), "model", ONE_GROUP),
    ("most_similar: labels", lambda e: e.most_similar(["zz"], 1), "model", (KeyError, "zz")),
    ("fold_in: pruned before group", lambda e: e.fold_in([["zz"]], group=7), "model", (ValueError, "whole rows of the iterate")),
    ("score_sets: group before sets", lambda e: e.score_sets("ab", group=2), "model", ONE_GROUP),
    ("score_sets: sets", lambda e: e.score_sets("ab", top_k=0), "model", (ValueError, "sets must be a sequence")),
    ("score_sets: labels", lambda e: e.score_sets([["zz"]]), "model", (KeyError, "zz")),
    ("recommend: group first", lambda e: e.recommend(["zz"], 0, group=2, exclude_seen=1), "model", ONE_GROUP),
    ("recommend: exclude_seen before k", lambda e: e.recommend(["zz"], 0, exclude_seen=1), "model", EXCLUDE_SEEN),
    ("recommend: k before labels", lambda e: e.recommend(["zz"], 0), "model", K_POSITIVE),
    ("recommend: labels", lambda e: e.recommend(["zz"], 1), "model", (KeyError, "zz")),
    ("explain: a, b first", lambda e: e.explain("ab", ["b"], k=0, group=2), "arg", (ValueError, "a must be a sequence of fitted labels, not str")),
    ("explain: lengths", lambda e: e.explain(["a"], ["b", "c"], k=0), "arg", (ValueError, r"same length \(1 != 2\)")),
    ("explain: k before max_terms", lambda e: e.explain(["a"], ["b"], k=0, max_terms=0), "arg", (ValueError, r"k must be an integer in 1 \.\. 1024, not 0")),
    ("explain: max_terms before the model", lambda e: e.explain(["a"], ["b"], max_terms=0, group=2), "arg",
     (ValueError, "max_terms must be a positive integer, not 0")),
    ("explain: group before labels", lambda e: e.explain(["zz"], ["b"], group=2), "model", ONE_GROUP),
    ("explain: labels before the diagonal", lambda e: e.explain(["c", "zz"], ["c", "b"]), "model", (KeyError, "zz")),
    ("explain: the diagonal before max_terms", lambda e: e.explain(["a", "c"], ["c", "c"], max_terms=1), "model",
     (ValueError, r"a\[1\] == b\[1\] == 'c'")),
    ("explain: too many terms", lambda e: e.explain(["b", "a"], ["c", "c"], max_terms=1), "model",
     (ValueError, r"\('a', 'c'\) has 2 x 1 = 2 terms, more than max_terms = 1")),
    ("rank_sets: group before sets", lambda e: e.rank_sets("ab", "ab", group=2), "model", ONE_GROUP),
    ("rank_sets: sets before targets", lambda e: e.rank_sets([["zz"]], "ab"), "model", (KeyError, "zz")),
    ("rank_sets: targets", lambda e: e.rank_sets([["a"]], "ab"), "model", (ValueError, "targets must be a sequence")),
    ("rank_recommended: group first", lambda e: e.rank_recommended(["zz"], "ab", group=2, exclude_seen=1), "model", ONE_GROUP),
    ("rank_recommended: exclude_seen before labels", lambda e: e.rank_recommended(["zz"], "ab", exclude_seen=1), "model", EXCLUDE_SEEN),
    ("rank_recommended: nodes before targets", lambda e: e.rank_recommended(["zz"], "ab"), "model", (KeyError, "zz")),
    ("rank_recommended: targets", lambda e: e.rank_recommended(["a"], "ab"), "model", (ValueError, "targets must be a sequence")),
    ("evaluate: ks first", lambda e: e.evaluate(["zz"], "ab", ks=(), group=2), "arg", (ValueError, "ks must be a non-empty sequence")),
    ("evaluate: group", lambda e: e.evaluate(["zz"], "ab", group=2, exclude_seen=1), "model", ONE_GROUP),
    ("evaluate: exclude_seen", lambda e: e.evaluate(["zz"], "ab", exclude_seen=1), "model", EXCLUDE_SEEN),
    ("frame", lambda e: e.frame(), "model", None),
    ("top_k: k first", lambda e: e.top_k(0), "arg", K_POSITIVE),
    ("top_k", lambda e: e.top_k(1), "model", None),
    ("pairs: min_similarity before max_pairs", lambda e: e.pairs(0, max_pairs=0), "arg", (ValueError, "min_similarity must be a finite number > 0, not 0")),
    ("pairs: max_pairs", lambda e: e.pairs(0.5, max_pairs=0), "arg", (ValueError, "max_pairs must be a positive integer, not 0")),
    ("pairs", lambda e: e.pairs(0.5), "model", None),
    ("count_pairs: thresholds first", lambda e: e.count_pairs(0.5), "arg", (ValueError, "thresholds must be a sequence of finite numbers, not 0.5")),
    ("count_pairs: a bool", lambda e: e.count_pairs([0.5, True]), "arg", (ValueError, "every threshold must be a finite number, not True")),
    ("count_pairs", lambda e: e.count_pairs([0.5]), "model", None),
    ("threshold_for: max_pairs first", lambda e: e.threshold_for(True), "arg", (ValueError, "max_pairs must be a positive integer, not True")),
    ("threshold_for", lambda e: e.threshold_for(1), "model", None),
    ("components: thresholds first", lambda e: e.components([0.5, 10 ** 400]), "arg", (ValueError, "a threshold must be a finite number, not 1000")),
    ("components: no number", lambda e: e.components("x"), "arg", (ValueError, "a threshold must be a finite number or a sequence of them, not 'x'")),
    ("components: too many", lambda e: e.components([0.1] * 9), "arg", (ValueError, "components takes 1 to 8 thresholds, not 9")),
    ("components", lambda e: e.components(0.5), "model", None),
    ("linkage: the floor first", lambda e: e.linkage(np.array(float("nan"))), "arg", (ValueError, r"min_similarity must be a finite number, not (np\.float64\()?nan")),
    ("linkage: a pruned model needs a floor", lambda e: e.linkage(), "model", (ValueError, "needs min_similarity > 0")),
    ("linkage: a positive floor", lambda e: e.linkage(-0.5), "model", (ValueError, "needs min_similarity > 0")),
    ("cut: one of the two first", lambda e: e.cut(Z_NONE, t=1, n_clusters=1, group=2), "arg", (ValueError, "cut takes exactly one of t and n_clusters")),
    ("cut: t", lambda e: e.cut(Z_NONE, t=True, group=2), "arg", (ValueError, "t must be a finite number, not True")),
    ("cut: n_clusters", lambda e: e.cut(Z_NONE, n_clusters=0, group=2), "arg", (ValueError, "n_clusters must be an int >= 1, not 0")),
    ("cut: group before the table", lambda e: e.cut(Z_NONE, t=0.5, group=2), "model", ONE_GROUP),
    ("cut: the table", lambda e: e.cut(Z_NONE, t=0.5), "model", (ValueError, "Z must be a table of linkage")),
    ("cluster_quality: group before labels", lambda e: e.cluster_quality("ab", group=2), "model", ONE_GROUP),
    ("cluster_quality: labels", lambda e: e.cluster_quality("ab"), "model", (ValueError, "labels must be a pandas Series indexed")),
    ("cluster_quality: a bool label", lambda e: e.cluster_quality([0, 1, True]), "model", (ValueError, "a cluster label must be an integer, not True")),
    ("cluster_means: max_bytes first", lambda e: e.cluster_means("ab", group=2, max_bytes=0), "arg", (ValueError, "max_bytes must be a positive integer, not 0")),
    ("cluster_means: group", lambda e: e.cluster_means("ab", group=2), "model", ONE_GROUP),
    ("cluster_means: labels before the size", lambda e: e.cluster_means("ab", max_bytes=8), "model", (ValueError, "labels must be a pandas Series indexed")),
    ("cluster_means: the size", lambda e: e.cluster_means([0, 0, 1], max_bytes=8), "model", (ValueError, "is 48 bytes, above max_bytes = 8")),
    ("medoids: group before labels", lambda e: e.medoids("ab", group=2), "model", ONE_GROUP),
    ("medoids: labels", lambda e: e.medoids([0, 1]), "model", (ValueError, "labels has 2 entries for 3 fitted nodes")),
    ("cluster_summary: group before labels", lambda e: e.cluster_summary("ab", group=2), "model", ONE_GROUP),
    ("cluster_summary: labels", lambda e: e.cluster_summary(None), "model", (ValueError, "labels must be a pandas Series indexed")),
    ("assign: group before seeds", lambda e: e.assign("ab", group=2), "model", ONE_GROUP),
    ("assign: seeds", lambda e: e.assign("ab"), "model", (ValueError, "seeds must be a sequence of fitted labels")),
    ("assign: a repeated seed", lambda e: e.assign(["a", "a"]), "model", (ValueError, "seeds repeats a label")),
    ("assign: labels", lambda e: e.assign(["a", "zz"]), "model", (KeyError, "zz")),
    ("kmedoids: max_iter first", lambda e: e.kmedoids("ab", max_iter=True, group=2), "arg", (ValueError, "max_iter must be a positive integer, not True")),
    ("kmedoids: group before seeds", lambda e: e.kmedoids("ab", group=2), "model", ONE_GROUP),
    ("kmedoids: seeds", lambda e: e.kmedoids([]), "model", (ValueError, "seeds is empty")),
    ("compact: precision first", lambda e: e.compact("f32"), "arg", (ValueError, "precision must be None")),
    ("compact: a pruned model is not narrowed", lambda e: e.compact("fp16"), "model", (ValueError, "a pruned model holds float64 neighbour lists")),
    ("prune: k first", lambda e: e.prune(0), "arg", K_POSITIVE),
    ("prune: a bool", lambda e: e.prune(True), "arg", (ValueError, "k must be a positive integer, not True")),
    ("prune", lambda e: e.prune(1), "model", None),
    ("device_bytes", lambda e: e.device_bytes, "model", None),
    ("save", lambda e: e.save("/nonexistent/never-written"), "model", None),
]


def raises(call, est, want, what):
    exc, match = want
    with pytest.raises(exc, match=match):
        call(est)
        pytest.fail(f"{what}: nothing was raised")


@pytest.mark.parametrize("what, call, kind, guarded", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_order_of_the_refusals(what, call, kind, guarded):
    released = guarded_estimator()
    released.release()
    raises(call, SRA.SimRank(), guarded if kind == "arg" else NO_MODEL, what)
    raises(call, released, guarded if kind == "arg" else RELEASED, what)
    if guarded is not None:
        raises(call, guarded_estimator(), guarded, what)


def test_what_a_guarded_model_answers_without_its_device(tmp_path):
    est = guarded_estimator()
    assert est.kept_neighbors == 2 and est.device_bytes == 3 * 2 * 12 + 3 * 8
    assert est.compact() is est and est.prune(2) is est and est.prune(7) is est       # (k as clamped is what is kept)
    assert SRA.SimRank().kept_neighbors is None
    est._model[1][0][1][:] = [1.5, "b", None]
    with pytest.raises(ValueError, match="save\\(\\) writes labels that are Python int or str .*not NoneType, float"):
        est.save(tmp_path / "never")
    assert not (tmp_path / "never").exists()
    est.release()
    est.release()                                             # (idempotent)
    assert est.kept_neighbors is None
    with pytest.raises(RuntimeError, match="was released"):
        est.device_bytes
    with SRA.SimRank() as fresh:
        fresh.release()
    with pytest.raises(RuntimeError, match="there is no kept model"):
        fresh.frame()


def test_no_model_comes_before_the_group_in_the_cross_side_queries():
    """``recommend``, ``rank_recommended`` and ``fold_in`` name the missing model before a bad group; a model that holds
    its matrices judges the group, then (``fold_in``, ``explain``) the strict fit, then the rest."""
    g = csr_of([[1], [0]], 2)
    est = SRA.BipartiteSimRankPP()._keep(Recorder([spec_of(g, [1.0, 1.0], g), spec_of(g, [1.0, 1.0], g)], [2, 2]),
                                         [(0, [1, 2]), (1, ["x", "y"])])
    est._weighted = False
    for call in (lambda e: e.fold_in("ab", group=7, top_k=0), lambda e: e.recommend(["zz"], 0, group=7, exclude_seen=1),
                 lambda e: e.rank_recommended(["zz"], "ab", group=7, exclude_seen=1)):
        raises(call, SRA.BipartiteSimRankPP(), NO_MODEL, "")
        raises(call, est, (ValueError, "group must be 1 or 2, not 7"), "")
    raises(lambda e: e.fold_in("ab", group=2, top_k=0), est, (ValueError, "Evidence_N1"), "")
    raises(lambda e: e.fold_in("ab", group=1, top_k=0), est, (ValueError, "neighbors must be a sequence"), "")
    raises(lambda e: e.fold_in([["x"]], group=1, top_k=0), est, K_POSITIVE, "")
    raises(lambda e: e.fold_in([["x"]], group=1, weights=[[1.0]]), est, (ValueError, "fitted with weighted=False"), "")
    raises(lambda e: e.fold_in([["x"]], group=1, prior=np.zeros((1, 2))), est, (ValueError, "prior needs a class fitted with a prior"), "")


# ====================================================================================================================================
# The dispatch scopes of ``_query.SolverQueries``: ``lists(j)`` and ``one_block(j)``.  These cases name what this file's
# subject introduced; everything above runs unchanged on the tree before it.
# ====================================================================================================================================
def _reader_of(n, blocks):
    cols = [n // blocks + (1 if i < n % blocks else 0) for i in range(blocks)]
    lo = np.concatenate([[0], np.cumsum(cols)[:-1]])
    return types.SimpleNamespace(n=n, closed=0, blocks=[dict(rows=n, cols=c, col_lo=int(l)) for c, l in zip(cols, lo)],
                                 close=lambda: None)


class Blocks(_model.DetachedSolver):
    """A solver double in the shape of a ``DetachedSolver`` whose sides report ``blocks`` column blocks each; counts its
    releases."""

    def __init__(self, n, blocks, specs=None):
        self.n, self._blocks, self.released, self.made = list(n), blocks, 0, []
        self.specs, self.ops, self.mode, self.fitted, self.storage = specs, {0: None}, "sparse", None, "f32"

    def _make_reader(self, j):
        self.made.append(j)
        return _reader_of(self.n[j], self._blocks)

    def release(self):
        self.released += 1
        self._close_readers()


@pytest.fixture
def detaches(monkeypatch):
    """``_model.detach`` replaced by a recorder that hands out one-block doubles."""
    made = []

    def detach(solver, precision=None):
        assert precision is None
        made.append(Blocks(solver.n, 1, solver.specs))
        return made[-1]
    monkeypatch.setattr(_model, "detach", detach)
    return made


def test_scope_one_block_yields_the_readers_own_block_without_packing(detaches):
    solver = Blocks([5], 1)
    with solver.one_block(0) as reader:
        assert reader is solver._reader(0) and len(reader.blocks) == 1
    assert not detaches and solver.released == 0


def test_scope_one_block_packs_several_blocks_once_and_releases_on_both_paths(detaches):
    solver = Blocks([70, 9], 3)
    with solver.one_block(1) as reader:
        assert len(detaches) == 1 and reader is detaches[0]._reader(1) and reader.n == 9 and detaches[0].released == 0
    assert detaches[0].released == 1 and solver.released == 0
    with pytest.raises(KeyError, match="from the body"):
        with solver.one_block(0) as reader:
            assert len(detaches) == 2 and reader is detaches[1]._reader(0) and reader.n == 70
            raise KeyError("from the body")
    assert [d.released for d in detaches] == [1, 1] and solver.released == 0


def test_scope_one_block_checks_that_the_block_holds_every_row_and_column(detaches):
    solver = Blocks([5], 1)
    solver._reader(0).blocks[0]["cols"] = 4
    with pytest.raises(AssertionError):
        with solver.one_block(0):
            pass
    assert not detaches


def test_scope_lists_is_none_with_a_matrix_and_the_host_tables_of_a_pruned_model():
    assert Blocks([5], 1).lists(0) is None and Blocks([5, 4], 3).lists(1) is None
    assert _model.DetachedSolver.lists is _query.SolverQueries.lists
    ops = HostOps()
    solver = _neighbors.NeighborSolver(ops, [_FullSpec(6)], [_neighbors.Tables.from_host(ops, IDS_A, VALS_A, DIAG_A)])
    ids, vals, diag = solver.lists(0)
    exact(ids, IDS_A, np.int32) and exact(vals, VALS_A) and exact(diag, DIAG_A)
    solver.release()
    with pytest.raises(ValueError, match="the model's tables were released"):
        solver.lists(0)
    guarded = guarded_estimator()._model[0]
    with pytest.raises(AssertionError, match="the device was touched"):
        guarded.lists(0)                                      # (the reader is asked first, as every host path asked it)


def test_scope_prune_packs_a_two_sided_several_block_model_once(detaches, monkeypatch):
    selected = []

    def select(reader, k, timing=None):
        selected.append(reader)
        return types.SimpleNamespace(n=reader.n, k=_neighbors.clamp_k(k, reader.n), nbytes=0, ids=1, free=lambda: None)
    monkeypatch.setattr(_neighbors, "select", select)
    solver = Blocks([70, 9], 3, [_FullSpec(70), _FullSpec(9)])
    pruned = _neighbors.prune(solver, 4)
    assert len(detaches) == 1 and detaches[0].released == 1 and solver.released == 0
    assert [r.n for r in selected] == [70, 9] and all(len(r.blocks) == 1 for r in selected)
    assert isinstance(pruned, _neighbors.NeighborSolver) and pruned.kept_k == [4, 4] and pruned.specs == solver.specs
    # one block per side: no packing at all
    whole = Blocks([70, 9], 1, solver.specs)
    _neighbors.prune(whole, 4)
    assert len(detaches) == 1 and whole.released == 0
    # a selection that fails: the temporary is released all the same
    monkeypatch.setattr(_neighbors, "select", boom)
    with pytest.raises(AssertionError, match="the device was touched"):
        _neighbors.prune(solver, 4)
    assert len(detaches) == 2 and detaches[1].released == 1
