"""``fit(storage_precision="f64")`` on the MI355X: the reference's float64 loop (libsimrank_f64.so) must give the
reference's own float64 numbers — the golden vectors within 1e-12, the oracle within 1e-11 on mid-size graphs and at an
eps deep enough that the f32 loop cannot follow — with the reference's console text, ``converged_at`` and errors, and
hand-backs (top_k, min_similarity) that are the same fit's dense frame bit for bit."""
import contextlib
import io

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from oracle import simrank_oracle as O
from simrank_amd import synth
from tests.conftest import Golden, golden_names
from tests.graphs import bipartite_random
from tests.helpers import TIME_RE, run_estimator

pytestmark = pytest.mark.gpu

F64 = dict(storage_precision="f64")


def close(got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= tol, err


# ---- the golden vectors, at float64 precision ----
@pytest.mark.parametrize("name", golden_names())
def test_golden_vectors_in_f64(name):
    g = Golden(name)
    if g.raises:
        with pytest.raises(ValueError) as got:
            run_estimator(g, **F64)
        with pytest.raises(ValueError) as f32:
            run_estimator(g)
        assert str(got.value) == str(f32.value)
        return
    est, res, text = run_estimator(g, **F64)
    assert text == g.stdout
    if g.kwargs.get("verbose", True):
        assert (est.converged_at if est.converged_at is not None else -1) == g.k
    if "S" in g.out:
        assert list(res.index) == list(g.out["labels"]) == list(res.columns)
        assert res.values.dtype == np.float64
        close(res.values, g.out["S"], 1e-12)
        if "E" in g.out:
            np.testing.assert_array_equal(est.Evidence, g.out["E"])
    else:
        s1, s2 = res
        assert list(s1.index) == list(g.out["labels1"]) and list(s2.index) == list(g.out["labels2"])
        close(s1.values, g.out["S1"], 1e-12)
        close(s2.values, g.out["S2"], 1e-12)
        if "E1" in g.out:
            np.testing.assert_array_equal(est.Evidence_N1, g.out["E1"])
            np.testing.assert_array_equal(est.Evidence_N2, g.out["E2"])


# ---- a deep eps: the oracle's loop, update by update ----
def _hub_graph(n=2000, hub_degree=1200, seed=11):
    df = synth.er_directed(n, 0.003, seed)
    rng = np.random.default_rng(seed)
    src = rng.choice(np.arange(1, n), size=hub_degree, replace=False)
    hub = pd.DataFrame({"from": src, "to": np.zeros(hub_degree, dtype=src.dtype), "weight": 1.0})
    both = pd.concat([df[["from", "to"]], hub[["from", "to"]]]).drop_duplicates(ignore_index=True)
    return both


def _deep_eps(deltas, near=1e-9):
    """eps between two consecutive update sizes around ``near``: the geometric mean, so that no element sits on the
    boundary; -> (eps, loop index at which the reference's test passes)."""
    k = next(i for i in range(1, len(deltas)) if deltas[i] <= near)      # deltas[i] = max|S_{i+1} - S_i|
    eps = float(np.sqrt(deltas[k - 1] * deltas[k]))
    assert all(d > eps * 1.05 for d in deltas[:k]) and deltas[k] < eps / 1.05, (deltas[k - 1:k + 1], eps)
    return eps, k + 1


def _oracle_directed(W, C, E=None, updates=200):
    n = W.shape[0]
    S, out, deltas = np.eye(n), [np.eye(n)], []
    for _ in range(updates):
        new = O.update(W, S, C, E)
        deltas.append(float(np.abs(new - S).max()))
        S = new
        out.append(S)
        if deltas[-1] < 1e-11:
            break
    return out, deltas


@pytest.mark.parametrize("kind", ["er", "hub", "pp"])
def test_deep_eps_matches_the_oracle_loop(kind):
    if kind == "er":
        df = synth.er_directed(2000, 0.004, 5)
    else:
        df = _hub_graph()
    nodes, G = O.directed_graph(df)
    if kind == "hub":
        assert int((G > 0).sum(axis=1).max()) >= 1000
    W, E = (O.weight(G), O.evidence(G)) if kind == "pp" else (G, None)
    iterates, deltas = _oracle_directed(W, 0.8, E)
    eps, k = _deep_eps(deltas)
    est = SRA.SimRankPP() if kind == "pp" else SRA.SimRank()
    got = est.fit(df, eps=eps, iterations=400, verbose=False, **F64)
    assert list(got.index) == nodes
    assert est.converged_at == k
    close(got.values, iterates[k], 1e-11)
    # (the f32 loop at that eps: no promise, it stops elsewhere or runs to the cap)


def test_deep_eps_bipartite_pp():
    df = bipartite_random(900, 700, 0.02, seed=4)
    set1, set2, lab1, lab2, G12, G21 = O.bipartite_graph(df)
    W1, W2, E1, E2 = O.weight(G12), O.weight(G21), O.evidence(G12), O.evidence(G21)
    S1, S2, it, deltas = np.eye(len(lab1)), np.eye(len(lab2)), [], []
    for _ in range(200):
        n1 = O.update(W1, S2, 0.8, E1)
        n2 = O.update(W2, n1, 0.8, E2)
        deltas.append(max(float(np.abs(n1 - S1).max()), float(np.abs(n2 - S2).max())))
        S1, S2 = n1, n2
        it.append((S1, S2))
        if deltas[-1] < 1e-11:
            break
    eps, k = _deep_eps(deltas)
    est = SRA.BipartiteSimRankPP()
    s1, s2 = est.fit(df, eps=eps, iterations=400, verbose=False, strict_reference=False, **F64)
    assert est.converged_at == k
    close(s1.values, it[k - 1][0], 1e-11)
    close(s2.values, it[k - 1][1], 1e-11)


# ---- mid-size classes against the oracle ----
@pytest.mark.parametrize("weighted", [False, True])
def test_simrank_mid_size(weighted):
    df = synth.er_directed(1500, 0.004, 21)
    want = O.fit_simrank(df, weighted=weighted, verbose=False)
    est = SRA.SimRank()
    got = est.fit(df, weighted=weighted, verbose=False, **F64)
    assert list(got.index) == want["labels"] and est.converged_at == want["k"]
    close(got.values, want["S"], 1e-11)


def test_simrank_pp_mid_size():
    df = synth.powerlaw_directed(1200, 8, 3)
    want = O.fit_simrank_pp(df, verbose=False)
    est = SRA.SimRankPP()
    got = est.fit(df, verbose=False, **F64)
    assert est.converged_at == want["k"]
    close(got.values, want["S"], 1e-11)
    np.testing.assert_array_equal(est.Evidence, want["E"])


@pytest.mark.parametrize("symmetric", [True, False])
def test_apriori_with_a_float64_prior(symmetric):
    df = synth.er_directed(1000, 0.006, 8)
    n = len(O.directed_graph(df)[0])
    rng = np.random.default_rng(3)
    A = rng.random((n, n)) * 0.3
    if symmetric:
        A = (A + A.T) / 2
    want = O.fit_simrank_pp(df, verbose=False, apriori=A, lbd=0.3, eps=1e-8)
    est = SRA.AprioriSimRank()
    got = est.fit(df, A, lbd=0.3, eps=1e-8, verbose=False, **F64)
    assert est.converged_at == want["k"]
    close(got.values, want["S"], 1e-11)
    if not symmetric:
        assert not np.array_equal(got.values, got.values.T)
    rounded = SRA.AprioriSimRank().fit(df, A.astype(np.float32).astype(np.float64), lbd=0.3, eps=1e-8, verbose=False,
                                       **F64)
    assert float(np.abs(rounded.values - got.values).max()) > 1e-9        # the prior is not rounded to float32


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("cls", ["BipartiteSimRank", "BipartiteSimRankPP", "BipartitleAprioriSimRank"])
def test_bipartite_classes(cls, strict):
    n1, n2 = (800, 800) if strict and cls != "BipartiteSimRank" else (900, 600)
    df = bipartite_random(n1, n2, 0.01, seed=9)
    est = getattr(SRA, cls)()
    if cls == "BipartiteSimRank":
        want = O.fit_bipartite(df, verbose=False)
        s1, s2 = est.fit(df, verbose=False, strict_reference=strict, **F64)
    else:
        a1 = a2 = None
        args = ()
        if cls == "BipartitleAprioriSimRank":
            rng = np.random.default_rng(2)
            m1, m2 = df["user"].nunique(), df["item"].nunique()
            a1, a2 = rng.random((m1, m1)) * 0.2, rng.random((m2, m2)) * 0.2          # asymmetric priors
            args = (a1, a2)
        want = O.fit_bipartite_pp(df, verbose=False, strict_reference=strict, apriori1=a1, apriori2=a2)
        s1, s2 = est.fit(df, *args, verbose=False, strict_reference=strict, **F64)
    assert est.converged_at == want["k"]
    assert list(s1.index) == list(want["labels1"] if strict else want["sorted1"])
    close(s1.values, want["S1"], 1e-11)
    close(s2.values, want["S2"], 1e-11)


# ---- hand-backs: the same fit's dense frame, bit for bit ----
def _host_topk(frame, k):
    vals = frame.to_numpy()
    rows = []
    for a in range(vals.shape[0]):
        cand = [(-vals[a, c], c) for c in range(vals.shape[1]) if c != a]
        cand.sort()
        for r, (v, c) in enumerate(cand[:k]):
            rows.append((frame.index[a], r + 1, frame.columns[c], -v))
    return pd.DataFrame(rows, columns=["node", "rank", "neighbor", "similarity"])


def _dense_pairs(frame, t):
    vals = frame.to_numpy()
    mask = vals >= t
    np.fill_diagonal(mask, False)
    r, c = np.nonzero(mask)
    return pd.DataFrame({"node": frame.index.take(r), "neighbor": frame.columns.take(c), "similarity": vals[r, c]})


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def test_handbacks_are_the_dense_frame():
    df = synth.powerlaw_directed(700, 6, 12)
    dense = SRA.SimRankPP().fit(df, verbose=False, **F64)
    again = SRA.SimRankPP().fit(df, verbose=False, **F64)
    assert np.array_equal(_bits(dense.values), _bits(again.values))
    assert np.array_equal(dense.values, dense.values.T) and np.all(np.diag(dense.values) == 1.0)
    for k in (1, 10, 40):
        got = SRA.SimRankPP().fit(df, verbose=False, top_k=k, **F64)
        want = _host_topk(dense, k)
        assert got["similarity"].dtype == np.float64
        assert list(got["node"]) == list(want["node"]) and list(got["neighbor"]) == list(want["neighbor"])
        assert list(got["rank"]) == list(want["rank"])
        assert np.array_equal(_bits(got["similarity"]), _bits(want["similarity"]))
    t = float(np.quantile(dense.values[~np.eye(len(dense), dtype=bool)], 0.99))
    got = SRA.SimRankPP().fit(df, verbose=False, min_similarity=t, **F64)
    want = _dense_pairs(dense, t)
    assert len(got) == len(want) > 0
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    assert np.array_equal(_bits(got["similarity"]), _bits(want["similarity"]))
    with pytest.raises(ValueError, match="max_pairs"):
        SRA.SimRankPP().fit(df, verbose=False, min_similarity=t, max_pairs=len(want) - 1, **F64)


def test_bipartite_handbacks_with_an_asymmetric_prior():
    df = bipartite_random(300, 200, 0.05, seed=6)
    rng = np.random.default_rng(1)
    m1, m2 = df["user"].nunique(), df["item"].nunique()
    a1, a2 = rng.random((m1, m1)) * 0.3, rng.random((m2, m2)) * 0.3
    kw = dict(verbose=False, strict_reference=False, **F64)
    s1, s2 = SRA.BipartitleAprioriSimRank().fit(df, a1, a2, **kw)
    t1, t2 = SRA.BipartitleAprioriSimRank().fit(df, a1, a2, top_k=7, **kw)
    for got, dense in ((t1, s1), (t2, s2)):
        want = _host_topk(dense, 7)
        assert list(got["neighbor"]) == list(want["neighbor"])
        assert np.array_equal(_bits(got["similarity"]), _bits(want["similarity"]))
    p1, p2 = SRA.BipartitleAprioriSimRank().fit(df, a1, a2, min_similarity=0.3, **kw)
    pd.testing.assert_frame_equal(p1, _dense_pairs(s1, 0.3), check_exact=True)
    pd.testing.assert_frame_equal(p2, _dense_pairs(s2, 0.3), check_exact=True)


def test_mirror_form_agrees_with_the_full_form():
    """Symmetric iterates run the upper triangle + mirror; the full form (what asymmetric priors take) on the same
    problem agrees within rounding, and the mirror form is exactly symmetric."""
    import dataclasses
    from simrank_amd import cdouble, ingest
    from simrank_amd.driver import LocalWorld, SideSpec
    from simrank_amd.engine import HipOps
    df = synth.powerlaw_directed(900, 8, 5)
    _, csr = ingest.directed(df, False, "from", "to", "weight")
    spec = SideSpec(csr, ingest.spread(csr) * csr.rowscale, 0.8, evidence_from=csr, storage="f64")
    ops = HipOps(0)
    out = []
    for sym in (True, False):
        sol = cdouble.F64Solver(ops, LocalWorld(1), [dataclasses.replace(spec, symmetric=sym)])
        k = sol.run(100, 1e-10)
        out.append((k, sol.result(0)))
        sol.release()
    (k1, a), (k2, b) = out
    assert k1 == k2 and k1 is not None
    assert np.array_equal(a, a.T)
    close(a, b, 1e-14)


# ---- edge cases ----
def test_edge_cases():
    df = synth.er_directed(200, 0.01, 2)
    n = len(O.directed_graph(df)[0])
    est = SRA.SimRank()
    got = est.fit(df, iterations=0, verbose=False, **F64)
    assert est.converged_at is None and np.array_equal(got.values, np.eye(n))
    got = est.fit(df, eps=1.0, verbose=False, **F64)
    assert est.converged_at == 0 and np.array_equal(got.values, np.eye(n))
    # one node
    one = pd.DataFrame({"from": [7], "to": [7]})
    got = est.fit(one, verbose=False, **F64)
    want = O.fit_simrank(one, verbose=False)
    assert est.converged_at == want["k"] and np.array_equal(got.values, want["S"])
    # rows without in-edges (rowscale 0): a graph with sources
    src = pd.DataFrame({"from": [0, 0, 1, 2, 5, 5], "to": [1, 2, 3, 3, 4, 3]})
    for cls, fit in ((SRA.SimRank, O.fit_simrank), (SRA.SimRankPP, O.fit_simrank_pp)):
        e = cls()
        got = e.fit(src, verbose=False, **F64)
        want = fit(src, verbose=False)
        assert e.converged_at == want["k"]
        close(got.values, want["S"], 1e-15)
    # k > n - 1: every other node
    got = SRA.SimRank().fit(src, verbose=False, top_k=50, **F64)
    m = len(O.directed_graph(src)[0])
    assert len(got) == m * (m - 1)


def _captured(fn):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        try:
            fn()
        except ValueError as e:
            return TIME_RE.sub("<t>", buf.getvalue()), str(e)
    raise AssertionError("no ValueError")


def test_strict_bipartite_broadcast_error_as_in_f32():
    df = bipartite_random(60, 40, 0.1, seed=3)
    f64 = _captured(lambda: SRA.BipartiteSimRankPP().fit(df, **F64))
    f32 = _captured(lambda: SRA.BipartiteSimRankPP().fit(df))
    assert f64 == f32 and "broadcast" in f64[1]


def test_too_large_is_refused_before_allocating():
    n = 200_000                              # three float64 matrices: 960 GB
    ring = pd.DataFrame({"from": np.arange(n), "to": (np.arange(n) + 1) % n})
    from simrank_amd._f64 import F64MemoryError
    with pytest.raises(F64MemoryError, match="needs .* GiB of device memory"):
        SRA.SimRank().fit(ring, verbose=False, **F64)


# ---- full size: config 4 ----
def test_config4_full_size():
    import scipy.sparse as sp
    df = synth.WORKLOADS["pl32768"][0]()
    est = SRA.SimRank()
    S = est.fit(df, verbose=False, **F64)
    k = est.converged_at
    assert k is not None and k > 1
    Sv = S.values
    n = Sv.shape[0]
    assert np.all(np.diag(Sv) == 1.0)
    rng = np.random.default_rng(4)
    rows = rng.choice(n, 24, replace=False)
    assert np.array_equal(Sv[rows], Sv[:, rows].T)
    csr = est._csr
    W = sp.csr_matrix((np.repeat(csr.rowscale, np.diff(csr.rowptr)), csr.col, csr.rowptr), shape=(n, n))
    # one more update: rows of C . W S W^T, from the handed-back S
    want = 0.8 * ((W[rows] @ Sv) @ W.T)
    want = np.asarray(want)
    want[np.arange(24), rows] = 1.0
    prev_rows = Sv[rows].copy()
    del S, Sv
    nxt = SRA.SimRank().fit(df, verbose=False, iterations=k + 1, eps=0.0, **F64).values
    close(nxt[rows], want, 1e-13)
    assert float(np.abs(nxt[rows] - prev_rows).max()) <= 1e-4          # converged at k: one more update moves < eps
