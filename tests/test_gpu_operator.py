"""``matmul`` and ``embed`` on a real MI355X (libsimrank_operator.so), on the models, graph and variants of
tests/test_gpu_sets.py (``synth.er_directed(1100, 0.002, seed=7)`` after three updates) and its small bipartite graph.

``matmul`` is held against ``model.frame().values @ X`` in NumPy, element by element within N 2^-52 sum |S| |X| (derived:
tests/operator_ref.py): kept, compact and loaded models, f32, fp16-held and float64 matrices, ``LocalWorld(2)``'s column
blocks packed into one, a pruned model against its own frame, both groups of a bipartite model; ndarray, Series and
DataFrame input in shuffled label order; 70 columns, which are two bands.  AprioriSimRank with a prior that is not
symmetric keeps an iterate that is not symmetric: there ``S @ X`` and ``S.T @ X`` differ and a wrong direction fails.  A
product with columns of the identity has one non-zero term per sum and must equal the frame's columns, or rows, bit for
bit.  ``embed`` is held to its invariants with the derived constants c1 and c2, on the fitted models and on a planted
matrix of exact rank 4."""
import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _model
from simrank_amd.engine import HipOps
from tests import operator_ref as R
from tests.test_gpu_sets import N, bipartite_graph, fit, graph, model_of  # noqa: F401

pytestmark = pytest.mark.gpu

D = 70                                             # two bands of the device: 64 + 6


def check_matmul(model, frame, group=None, wide=True):
    kw = {} if group is None else {"group": group}
    S = frame.values
    labels = list(frame.index)
    n = len(labels)
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, D if wide else 5))
    worst = 0.0
    for transpose in (False, True):
        want, bound = R.matmul_ref(S, X, transpose), R.product_bound(S, X, transpose)
        got = model.matmul(X, transpose=transpose, **kw)
        assert isinstance(got, pd.DataFrame) and list(got.index) == labels and list(got.columns) == list(range(X.shape[1]))
        assert got.values.dtype == np.float64
        err = np.abs(got.values - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), ("ndarray", transpose)
        again = model.matmul(X, transpose=transpose, **kw)
        assert np.array_equal(again.values.view(np.uint64), got.values.view(np.uint64))      # the same bits twice
        # a DataFrame in shuffled label order, with columns of its own: the same product, the same bits
        order = rng.permutation(n)
        cols = ["c%d" % i for i in range(X.shape[1])]
        shuffled = pd.DataFrame(X[order], index=[labels[i] for i in order], columns=cols)
        by_label = model.matmul(shuffled, transpose=transpose, **kw)
        assert list(by_label.columns) == cols and list(by_label.index) == labels
        assert np.array_equal(by_label.values.view(np.uint64), got.values.view(np.uint64))
        # a Series in shuffled order gives a Series: column 0 of the product, within the bound
        s = model.matmul(pd.Series(X[order, 0], index=[labels[i] for i in order], name="signal"), transpose=transpose, **kw)
        assert isinstance(s, pd.Series) and s.name == "signal" and list(s.index) == labels
        assert (np.abs(s.to_numpy() - want[:, 0]) <= bound[:, 0]).all(), ("series", transpose)
        v = model.matmul(X[:, 1], transpose=transpose, **kw)
        assert isinstance(v, pd.Series) and (np.abs(v.to_numpy() - want[:, 1]) <= bound[:, 1]).all()
    print("largest error / bound:", worst)
    # one non-zero term per sum: exact
    eye = np.eye(n)[:, :5]
    assert np.array_equal(model.matmul(eye, **kw).values.view(np.uint64), np.ascontiguousarray(S[:, :5]).view(np.uint64))
    a = n // 3
    row = model.matmul(np.eye(n)[:, a], transpose=True, **kw)
    assert np.array_equal(row.to_numpy().view(np.uint64), np.ascontiguousarray(S[a]).view(np.uint64))
    return got


CASES = [("SimRank", v, {}) for v in ("f32-kept", "fp16-kept", "f64-kept", "f32-compact", "loaded")] + [
    ("SimRank", "f32-kept", {"world": 2}), ("SimRankPP", "f64-compact", {}),
    ("AprioriSimRank", "f32-kept", {}), ("AprioriSimRank", "f32-compact", {}), ("AprioriSimRank", "f32-compact-fp16", {})]


@pytest.mark.parametrize("cls,variant,more", CASES, ids=["-".join([c, v] + ["world%d" % x for x in m.values()]) for c, v, m in CASES])
def test_matmul_is_the_numpy_product(cls, variant, more, graph, tmp_path):  # noqa: F811
    args = (np.random.default_rng(5).random((N, N)) * 0.5,) if cls == "AprioriSimRank" else ()
    with model_of(cls, graph, variant, tmp_path, *args, **more) as model:
        frame = model.frame()
        before = frame.values.copy()
        if cls == "AprioriSimRank":
            S = frame.values
            assert not np.array_equal(S, S.T)
            X = np.random.default_rng(N).standard_normal((N, D))
            # the two directions differ by far more than the bound: a wrong direction cannot pass
            assert (np.abs(S @ X - S.T @ X) > 4 * R.product_bound(S, X)).any()
        check_matmul(model, frame)
        assert np.array_equal(model.frame().values.view(np.uint64), before.view(np.uint64))  # the model is left as it was


def test_matmul_on_a_pruned_model_is_the_product_with_its_own_frame(graph, tmp_path):  # noqa: F811
    with model_of("SimRank", graph, "f32-kept", tmp_path) as model:
        model.prune(10)
        assert model.kept_neighbors == 10
        frame = model.frame()
        assert not np.array_equal(frame.values, frame.values.T)           # P is not symmetric
        check_matmul(model, frame)
        V, w = model.embed(3)
        R.check_embedding(V.values, w.to_numpy(), R.sym(frame.values), 11, "pruned")


@pytest.mark.parametrize("variant", ["f32-kept", "f32-compact", "loaded"])
def test_matmul_on_both_groups_of_a_bipartite_model(variant, tmp_path):
    df = bipartite_graph()
    with model_of("BipartiteSimRankPP", df, variant, tmp_path, weighted=True, strict_reference=False) as model:
        frames = model.frame()
        for group in (1, 2):
            check_matmul(model, frames[group - 1], group=group, wide=group == 1)
        with pytest.raises(ValueError, match="group"):
            model.matmul(np.zeros((len(frames[0]), 1)))
        V, w = model.embed(4, group=2)
        R.check_embedding(V.values, w.to_numpy(), R.sym(frames[1].values), 12, "group 2")


@pytest.mark.parametrize("variant", ["f32-compact", "fp16-kept", "f64-kept"])
def test_embed_invariants_on_a_fitted_model(variant, graph, tmp_path):  # noqa: F811
    with model_of("SimRank", graph, variant, tmp_path) as model:
        frame = model.frame()
        M = R.sym(frame.values)
        V, w = model.embed(10)
        assert isinstance(V, pd.DataFrame) and V.shape == (N, 10) and list(V.index) == list(frame.index)
        assert isinstance(w, pd.Series) and w.dtype == np.float64 and len(w) == 10
        R.check_embedding(V.values, w.to_numpy(), M, 18, variant)
        V2, w2 = model.embed(10)                                            # the same call, the same bits
        assert np.array_equal(V2.values.view(np.uint64), V.values.view(np.uint64))
        assert np.array_equal(w2.to_numpy().view(np.uint64), w.to_numpy().view(np.uint64))
        if variant == "f32-compact":
            V1, w1 = model.embed(1, oversample=0, power_iterations=16, seed=3)
            R.check_embedding(V1.values, w1.to_numpy(), M, 1, "dim = 1")
            Vn, wn = model.embed(N, oversample=0, power_iterations=0)
            R.check_embedding(Vn.values, wn.to_numpy(), M, N, "dim = N")
            assert Vn.shape == (N, N)
        assert np.array_equal(model.frame().values.view(np.uint64), frame.values.view(np.uint64))


def test_embed_on_a_planted_matrix_of_exact_rank():
    """A float64 model over an uploaded block that holds a symmetric matrix of exact rank 4 at N = 257 (every entry a
    multiple of 2^-8): the four eigenvalues are ``eigvalsh``'s within (N + c2(p)) 2^-52 ||M||_F;
    tests/test_operator_cpu.py shows that the NumPy statement alone stays inside that bound."""
    M = R.planted()
    n, dim = M.shape[0], 4
    p = dim + 8
    ops = HipOps(0)
    block = _model.Block(ops, "f64", n)
    host = np.zeros((n, block.stride))
    host[:, :n] = M
    ops.h2d(block.ptr, host)
    ops.synchronize()
    est = SRA.SimRank()
    est._keep(_model.DetachedSolver(ops, [None], [block]), [(0, list(range(n)))])
    try:
        assert np.array_equal(est.frame().values, M)
        V, w = est.embed(dim)
        want = np.sort(np.linalg.eigvalsh(M))[::-1][:dim]
        bound = (n + R.c2(p, n)) * R.U * np.linalg.norm(M, "fro")
        print("max |w - eigvalsh| =", np.abs(w.to_numpy() - want).max(), "bound", bound)
        assert (np.abs(w.to_numpy() - want) <= bound).all()
        R.check_embedding(V.values, w.to_numpy(), M, p, "planted")
        # M @ X with an exact operand: bit for bit through the public method
        X = R.exact_operand(np.random.default_rng(1), n, 3, 3)
        R.assert_exact(M, X)
        assert np.array_equal(est.matmul(X).values, M @ X)
    finally:
        est.release()
        ops.close()


def test_lifetime_and_refusals(graph):  # noqa: F811
    model = fit("SimRank", graph).compact()
    before = model.device_bytes
    model.matmul(np.ones(N))
    model.embed(2, power_iterations=0)
    assert model.device_bytes == before
    assert model.matmul(np.zeros((N, 0))).shape == (N, 0)
    for bad in (np.zeros((N, 2), dtype=bool), np.zeros((N - 1, 2)), np.array([["x"]] * N, dtype=object)):
        with pytest.raises(ValueError):
            model.matmul(bad)
    for kw in (dict(dim=0), dict(dim=N + 1), dict(dim=2, oversample=-1), dict(dim=2, power_iterations=17), dict(dim=2, seed=-1)):
        with pytest.raises(ValueError):
            model.embed(**kw)
    model.release()
    for call in (lambda: model.matmul(np.ones(N)), lambda: model.embed(2)):
        with pytest.raises(RuntimeError, match="released"):
            call()
