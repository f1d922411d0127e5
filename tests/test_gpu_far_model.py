"""The wrappers of the companion libraries at real N: BASELINE config 5 (SimRank++ on ``pl65536``, N = 65536), kept and
compact, so that a row of the model starts up to 2^32 floats into one 17.2 GB matrix and the ctypes prototypes, column
maps and band loops of ``_sets.py``, ``_rank.py``, ``_neighbors.py``, ``_profile.py``, ``_cluster.py``,
``_candidates.py`` and ``_exemplars.py`` run where the README presents them.  Nothing needs the N x N frame on the host: every reference is evaluated on ``model.rows(...)`` of
the rows a query reads (``rows`` at this N is tied to a float64 recomputation by tests/test_gpu_query.py and
tests/test_gpu_fullsize.py), for 64 nodes spread over [0, N), node N - 1 included, and every comparison but one is exact.

``fold_in`` is the one query whose device sums run in f32: on a fitted model no float64 restatement can equal them bit
for bit, and no order-exact one exists off the device.  Its dense rows are therefore held to ``foldin_ref``'s formula, in
float64 from ``model.rows`` of the list members and the model's own CSR, within the DERIVED bound of
tests/test_gpu_foldin.py taken per entry: (|I_q| + |I(b)| + 8) * 2^-24 relative, every term being non-negative (one
rounding per f32 addition of either sum, and 8 for the row scale, the transposed store and the float64 epilogue).  A row,
column map or band read at a wrong address is wrong by orders of magnitude more.  Zeros are exact (an evidence count of
0), and the device top-k is a host selection on those dense rows.  The gather kernel itself is compared bit for bit on
far blocks of exactly summable values in tests/test_gpu_far_blocks.py."""
import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

import simrank_amd.SimRank as SRA
from simrank_amd import _candidates, _exemplars, synth
from simrank_amd.engine import HipOps
from tests import blocks as B
from tests import candidates_ref as CA
from tests import cluster_ref as CR
from tests import exemplars_ref as ER
from tests import foldin_ref as FR
from tests import rank_ref as K
from tests import sets_ref as SR

pytestmark = pytest.mark.gpu

N = 65536
UPDATES = 3


def fit_compact():
    df = synth.WORKLOADS["pl65536"][0]()
    est = SRA.SimRankPP().fit(df, verbose=False, iterations=UPDATES, eps=0, keep=True)
    est.compact()
    return est


@pytest.fixture(scope="module")
def model():
    est = fit_compact()
    labels = list(est._model[1][0][1])
    assert len(labels) == N
    yield est, labels
    est.release()
    HipOps.trim_pool(0)


def sample():
    """64 positions spread over [0, N), the first and the last node among them."""
    P = np.unique(np.linspace(0, N - 1, 64).astype(np.int64))
    assert P.size == 64 and P[0] == 0 and P[-1] == N - 1 and (P >= 1 << 15).sum() >= 30       # rows past 2^31 floats too
    return P


def spread_nodes(deg, lo, hi):
    """64 nodes spread over [0, N) with lo <= deg <= hi: for each sampled position the nearest such node at or after it
    (before it where the end comes first), so that a reference's rows stay a few hundred MB on the host."""
    ok = (deg >= lo) & (deg <= hi)
    us = []
    for p in sample():
        later, earlier = np.flatnonzero(ok[p:]), np.flatnonzero(ok[:p])
        us.append(int(p + later[0]) if later.size else int(earlier[-1]))
    us = np.array(us, dtype=np.int64)
    assert np.unique(us).size == 64 and us[0] < 64 and us[-1] >= N - 64 and (us >= 1 << 15).sum() >= 30
    return us


def graph_of(est):
    """(rowptr, col, rowscale, coef) of the fitted graph in the frame's order: row b holds I(b)."""
    spec = est._model[0].specs[0]
    return (np.asarray(spec.csr.rowptr, dtype=np.int64), np.asarray(spec.csr.col, dtype=np.int64),
            np.asarray(spec.rowscale, dtype=np.float64), float(spec.coef))


def same_bits(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.argwhere(B.bits(np.where(nan, 0, got)) != B.bits(np.where(nan, 0, want)))
    assert bad.size == 0, (what, bad[:5].tolist())


def baskets(P, rng):
    """(positions per basket, weights per basket): 16 baskets of four sampled nodes, one that names the last node twice and
    the first once, one empty."""
    sets = [list(P[4 * q:4 * q + 4]) for q in range(16)] + [[int(P[-1]), int(P[0]), int(P[-1])], []]
    weights = [list(rng.uniform(-2.0, 2.0, size=len(s))) for s in sets]
    return sets, weights


def test_score_sets_and_rank_sets(model):
    est, labels = model
    P, rng = sample(), np.random.default_rng(1)
    lab = pd.Index(labels)
    R = est.rows(lab.take(P)).values                                        # [64, N]: every row a basket reads
    at = {int(p): i for i, p in enumerate(P)}
    sets, weights = baskets(P, rng)
    names = [f"s{q}" for q in range(len(sets))]
    sets_lab = [list(lab.take(np.asarray(s, dtype=np.int64))) for s in sets]
    dense = SR.scores(R, [[at[int(p)] for p in s] for s in sets], [np.asarray(w) for w in weights])
    got = est.score_sets(sets_lab, weights=weights, names=names)
    assert list(got.index) == names and list(got.columns[[0, N - 1]]) == [labels[0], labels[N - 1]]
    same_bits(got.values, dense, "score_sets")
    assert np.count_nonzero(dense[:16]) > 0 and not dense[17].any()
    best = est.score_sets(sets_lab, weights=weights, names=names, top_k=10)
    want = SR.long_frame("set", pd.Index(names), labels, dense, 10, [[int(p) for p in s] for s in sets])
    assert_frame_equal(best.reset_index(drop=True), want.reset_index(drop=True), check_exact=True)
    # held-out ranks: the first and the last node, a member (excluded: rank 0), a node in the middle, one twice
    targets = [[int(P[0]), int(P[-1]), int(s[0]) if s else 7, N // 2 + q, N // 2 + q] for q, s in enumerate(sets)]
    targets[3] = []
    ranks = est.rank_sets(sets_lab, [list(lab.take(np.asarray(t, dtype=np.int64))) for t in targets], weights=weights, names=names)
    want = K.long_frame("set", pd.Index(names), labels, K.excluded_rows(dense, [[int(p) for p in s] for s in sets]), targets)
    assert_frame_equal(ranks.reset_index(drop=True), want.reset_index(drop=True), check_exact=True)
    assert (want["rank"] == 0).sum() >= 16 and (want["rank"] > 0).sum() >= 32 and want["candidates"].max() > N - 5


def test_recommend(model):
    est, labels = model
    lab = pd.Index(labels)
    rowptr, col, rowscale, _ = graph_of(est)
    us = [int(u) for u in spread_nodes(np.diff(rowptr), 1, 12)]             # (a basket's rows cross to the host: <= 768 rows)
    lists = [col[rowptr[u]:rowptr[u + 1]] for u in us]
    members = np.unique(np.concatenate(lists))
    R = est.rows(lab.take(members)).values
    at = {int(p): i for i, p in enumerate(members)}
    dense = SR.scores(R, [[at[int(p)] for p in l] for l in lists], [np.full(len(l), rowscale[u]) for l, u in zip(lists, us)])
    got = est.recommend(list(lab.take(np.asarray(us))), 10)
    want = SR.long_frame("node", lab.take(np.asarray(us)), labels, dense, 10, [list(l) + [u] for l, u in zip(lists, us)])
    assert_frame_equal(got.reset_index(drop=True), want.reset_index(drop=True), check_exact=True)
    assert len(want) == 10 * len(us) == 640


U32 = 2.0 ** -24


def test_fold_in_dense_and_top_k(model):
    """42 new nodes (two tiles): the own lists of 36 of the spread nodes (the row the next update would give them: the
    evidence count of their own column is their degree), four lists of sampled nodes, the last node alone and with the
    first.  Every column of every new row against the float64 formula; see the module's docstring for the bound."""
    est, labels = model
    P = sample()
    lab = pd.Index(labels)
    rowptr, col, rowscale, coef = graph_of(est)
    deg = np.diff(rowptr)
    assert coef == 0.8
    own = spread_nodes(deg, 1, 12)[np.r_[0:64:2, 57:64:2]]
    lists = [col[rowptr[u]:rowptr[u + 1]] for u in own] + [P[a::16] for a in range(4)] + [np.array([N - 1]), np.array([0, N - 1])]
    assert len(lists) == 42 and all(np.unique(l).size == len(l) for l in lists)
    members = np.unique(np.concatenate(lists))
    R = est.rows(lab.take(members)).values
    at = {int(p): i for i, p in enumerate(members)}
    dense = est.fold_in([list(lab.take(np.asarray(l, dtype=np.int64))) for l in lists])
    assert dense.shape == (len(lists), N) and list(dense.columns[[0, N - 1]]) == [labels[0], labels[N - 1]]
    row_of = np.repeat(np.arange(N), deg)
    want, tol = np.zeros((len(lists), N)), np.zeros((len(lists), N))
    for q, l in enumerate(lists):
        t = R[[at[int(i)] for i in l]].sum(axis=0) * (1.0 / len(l))        # w_q . sum_{i in I_q} S[i, :]
        inner = np.bincount(row_of, weights=t[col], minlength=N)            # sum_{j in I(b)} of it
        member = np.zeros(N)
        member[l] = 1.0
        common = np.bincount(row_of, weights=member[col], minlength=N)      # |I_q n I(b)|
        want[q] = (1.0 - 0.5 ** common) * coef * (rowscale * inner)
        tol[q] = (len(l) + deg + 8) * U32
    got = dense.values
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want != 0, err / np.abs(want), 0.0)
    print(f"fold_in at N = {N}: {np.count_nonzero(want)} non-zero entries, worst relative error {rel.max():.3e}, "
          f"worst error / bound {(rel / tol).max():.3e}")
    assert np.array_equal(got != 0, want != 0)                              # an evidence count of 0 is an exact zero
    assert (err <= tol * np.abs(want) + 1e-30).all(), (int((err > tol * np.abs(want) + 1e-30).sum()), float(rel.max()))
    assert (np.count_nonzero(want, axis=1) > 0).all() and np.count_nonzero(want) > 1000
    for q, u in enumerate(own):
        assert want[q, u] > 0                                               # the node's own column: its whole list is shared
    best = est.fold_in([list(lab.take(np.asarray(l, dtype=np.int64))) for l in lists], top_k=10)
    idx, val = FR.topk_ref(got, 10)
    want_k = pd.DataFrame({"node": np.repeat(np.arange(len(lists)), 10), "rank": np.tile(np.arange(1, 11), len(lists)),
                           "neighbor": lab.take(idx.ravel()), "similarity": val.ravel()})
    assert_frame_equal(best.reset_index(drop=True), want_k, check_exact=True, check_dtype=False)


def test_threshold_count_pairs_and_components_agree(model):
    """Three libraries on one global answer: the radix select's (t, n), the count sweep at t, the rows ``pairs(t)`` emits,
    and the union-find's components against a plain union-find on those rows."""
    est, labels = model
    t, n = est.threshold_for(10 * N)
    assert 0 < t < 1 and 0 < n <= 10 * N
    assert int(est.count_pairs([t])[0]) == n
    pairs = est.pairs(t, max_pairs=n)
    assert len(pairs) == n and (pairs["similarity"] >= t).all() and pairs["similarity"].min() == t
    lab = pd.Index(labels)
    a, b = lab.get_indexer(pairs["node"]), lab.get_indexer(pairs["neighbor"])
    assert (a >= 0).all() and (b >= 0).all() and (a != b).all() and max(a.max(), b.max()) >= (1 << 15)
    comp = est.components(t)
    assert list(comp.index[[0, N - 1]]) == [labels[0], labels[N - 1]]
    want = CR.labels_of_edges(N, zip(a.tolist(), b.tolist()))
    assert np.array_equal(comp.to_numpy(), want)
    assert 1 < want.max() + 1 < N                                            # neither one cluster nor none


def long_of(node_labels, lab, idx, val, k):
    """The long frame (node, rank, neighbor, similarity) of a reference's (positions, values) [n_q, k]."""
    keep = idx.ravel() >= 0
    return pd.DataFrame({"node": np.repeat(np.asarray(node_labels), k)[keep], "rank": np.tile(np.arange(1, k + 1), len(idx))[keep],
                         "neighbor": lab.take(idx.ravel()[keep]), "similarity": val.ravel()[keep]})


def spread(m):
    """m distinct positions spread over [0, N), the first and the last node among them."""
    S = np.linspace(0, N - 1, m).astype(np.int64)
    assert np.unique(S).size == m and S[0] == 0 and S[-1] == N - 1
    return S


def test_most_similar_among_and_exclude(model):
    """Candidate sets on both sides of the staging cap (a quarter of the nodes) and ``exclude=`` of five labels alone:
    N - 5 candidates, not staged, 16 index bits.  The reference reads the 64 rows and nothing else."""
    est, labels = model
    lab, P = pd.Index(labels), sample()
    nodes = lab.take(P)
    R = est.rows(nodes).values
    (block,) = est._model[0]._reader(0).blocks
    cap = _candidates.staged(block["layout"])
    assert cap == N // 4
    at_cap = spread(cap)
    one_more = np.union1d(at_cap, [int(np.setdiff1d(np.arange(N // 2, N // 2 + 8), at_cap)[0])])
    gone = np.array([0, 3, N // 2, N - 2, N - 1], dtype=np.int64)
    rest = np.setdiff1d(np.arange(N), gone)
    assert one_more.size == cap + 1 and rest.size == N - 5 > 1 << 15
    far = 0
    for cand, kw in ((at_cap, {"among": lab.take(at_cap)}), (one_more, {"among": lab.take(one_more)}),
                     (rest, {"exclude": lab.take(gone)})):
        for k in (10, _candidates.MAX_K):
            got = est.most_similar(list(nodes), k, **kw)
            idx, val = CA.ref_topk(R, np.arange(P.size), P, cand, cand, k)
            want = long_of(nodes, lab, idx, val, k)
            assert_frame_equal(got.reset_index(drop=True), want, check_exact=True, check_dtype=False)
            assert (idx >= 0).all() and (val[:, 0] > 0).any()
            far += int(((idx >= 1 << 15) & (val > 0)).sum())
    assert far > 0                                                       # neighbours past 2^15: columns of the far panels


def test_score_sets_among(model):
    """The baskets of ``test_score_sets_and_rank_sets`` among one label more than the staging cap and half the sampled
    nodes: the dense scores of that test with the columns outside the set removed."""
    est, labels = model
    P, rng = sample(), np.random.default_rng(1)
    lab = pd.Index(labels)
    R = est.rows(lab.take(P)).values
    at = {int(p): i for i, p in enumerate(P)}
    sets, weights = baskets(P, rng)
    names = [f"s{q}" for q in range(len(sets))]
    sets_lab = [list(lab.take(np.asarray(s, dtype=np.int64))) for s in sets]
    dense = SR.scores(R, [[at[int(p)] for p in s] for s in sets], [np.asarray(w) for w in weights])
    cand = np.union1d(spread(N // 4 + 1), P[::2])
    got = est.score_sets(sets_lab, weights=weights, names=names, top_k=10, among=list(lab.take(cand)))
    inside = [np.searchsorted(cand, [p for p in s if p in set(cand.tolist())]).tolist() for s in sets]
    want = SR.long_frame("set", pd.Index(names), lab.take(cand), dense[:, cand], 10, inside)
    assert_frame_equal(got.reset_index(drop=True), want.reset_index(drop=True), check_exact=True)
    assert sum(len(x) for x in inside) >= 32 and (want["score"] != 0).any()


@pytest.mark.parametrize("with_given", [False, True], ids=["no given", "given the last node"])
def test_exemplars(model, monkeypatch, with_given):
    """Six picks at N = 65536: a ``gains`` row is 16 trips of the unrolled loop, ``cover`` is 512 KiB, and the given row,
    which ``cover`` reads first, starts past 2^32 floats.  Lazy (in rounds of 64) equals plain; coverage, raised counts
    and gains against the NumPy statement on ``rows`` of the given and picked nodes; greedy as far as the 64 sampled
    rows can tell."""
    est, labels = model
    lab, P, k = pd.Index(labels), sample(), 6
    given = [labels[N - 1]] if with_given else None
    at = [N - 1] if with_given else []
    monkeypatch.setattr(_exemplars, "BATCH", 64)
    picks, coverage = est.exemplars(k, given=given, lazy=True)
    monkeypatch.undo()
    plain, coverage_p = est.exemplars(k, given=given, lazy=False)
    assert picks["exemplar"].tolist() == plain["exemplar"].tolist()
    same_bits(picks["gain"].to_numpy(), plain["gain"].to_numpy(), "lazy gain")
    assert picks["raised"].tolist() == plain["raised"].tolist()
    same_bits(coverage.to_numpy(), coverage_p.to_numpy(), "lazy coverage")
    assert plain["evaluated"].tolist() == [N - len(at) - p for p in range(k)]
    assert picks["evaluated"].sum() < plain["evaluated"].sum()
    picked = lab.get_indexer(picks["exemplar"]).tolist()
    assert len(set(picked)) == k and not set(picked) & set(at) and coverage.index.equals(lab)
    Rk = est.rows(lab.take(np.asarray(at + picked, dtype=np.int64))).values
    R = est.rows(lab.take(P)).values
    same_bits(coverage.to_numpy(), ER.coverage(Rk), "coverage")
    gain = picks["gain"].to_numpy()
    cover = np.zeros(N)
    for row in Rk[:len(at)]:
        ER.apply(row, cover)
    others = [i for i, p in enumerate(P) if int(p) not in set(at + picked)]
    for p, row in enumerate(Rk[len(at):]):
        t = ER.terms(row, cover)
        assert abs(gain[p] - ER.exact_sum(t)) <= ER.bound(t), (p, gain[p], ER.exact_sum(t), ER.bound(t))
        # the compact model is the canonical form: the sum runs in the frame's order
        assert gain[p] == ER.ordered_sum(t), (p, gain[p], ER.ordered_sum(t))
        for i in others:
            g = ER.ordered_sum(ER.terms(R[i], cover))
            assert g < gain[p] or (g == gain[p] and P[i] > picked[p]), (p, int(P[i]), g, gain[p])
        assert picks["raised"][p] == ER.apply(row, cover), p
    same_bits(cover, coverage.to_numpy(), "cover")
    assert gain[0] > 0 and (np.diff(gain) <= 0).all() and len(others) >= 64 - k - 1


def test_prune_keeps_the_ten_best_of_every_sampled_row():
    """A second compact model, pruned: the lists of the sampled nodes are the total order on the rows read before."""
    est = fit_compact()
    try:
        labels = list(est._model[1][0][1])
        lab, P = pd.Index(labels), sample()
        R = est.rows(lab.take(P)).values
        est.prune(10)
        got = est.most_similar(list(lab.take(P)), 10)
        idx, val = B.ref_topk(R, np.arange(P.size), P, None, 10)
        keep = idx.ravel() >= 0
        want = pd.DataFrame({"node": lab.take(np.repeat(P, 10)[keep]), "rank": np.tile(np.arange(1, 11), P.size)[keep],
                             "neighbor": lab.take(idx.ravel()[keep]), "similarity": val.ravel()[keep]})
        assert_frame_equal(got.reset_index(drop=True), want, check_exact=True, check_dtype=False)
        assert keep.all() and (val[:, 0] > 0).all()
    finally:
        est.release()
        HipOps.trim_pool(0)
