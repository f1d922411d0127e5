"""libsimrank_operator.so (include/simrank_operator.h), ``matmul`` and ``embed`` on a machine without a GPU: header, binding
and exports agree, the header is plain C and stands alone, every bad argument is refused with a message and without a
device, the argument checks of the two methods run before any device work (on a stub solver), the host route of a
pruned model is the product with its dense matrix P, and the NumPy statement of ``embed`` (tests/operator_ref.py) alone
meets the bounds the GPU tests hold the device to."""
import ctypes as C
import re

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _operator, _query
from tests import companion_abi as A
from tests import operator_ref as R
from tests.diverse_ref import dense_p


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_operator) == _operator.VERSION == 1
    text = A.header(_operator)
    assert re.search(r"#define SIMRANK_OPERATOR_MAX_D %d\b" % _operator.MAX_D, text) and _operator.MAX_D == 64
    A.assert_header_stands_alone(_operator)
    A.assert_prototypes_match_the_header_argument_counts(_operator)
    A.assert_links_nothing_of_the_main_library(_operator)
    assert A.layout_codes(_operator) == A.layout_codes(_query)


def test_sizes_and_bad_arguments_need_no_device():
    lib = _operator.load()
    # d > 8: strips of 128 rows, the contraction's tiles of 32 dealt to at most 64 parts
    assert lib.simrank_operator_parts(70, 1100, 0, 64) == 35 and lib.simrank_operator_parts(70, 1100, 1, 9) == 3
    assert lib.simrank_operator_parts(32768, 32768, 0, 32) == 6 and lib.simrank_operator_parts(32768, 32768, 1, 64) == 6
    # d <= 8: strips of 16 rows and tiles of 256, or strips of 1024 columns and tiles of 64
    assert lib.simrank_operator_parts(70, 1100, 0, 3) == 5 and lib.simrank_operator_parts(70, 1100, 1, 8) == 2
    assert lib.simrank_operator_parts(32768, 32768, 0, 1) == 1 and lib.simrank_operator_parts(32768, 32768, 1, 1) == 47
    assert lib.simrank_operator_parts(1, 1, 0, 1) == 1 and lib.simrank_operator_parts(0, 0, 1, 64) == 1
    # more than 64 tiles: a workgroup walks several (tests/operator_ref.LONG_CASES, what the GPU test runs).  In the
    # table's order: (parts, tiles per part, tiles of the last part)
    want = [(34, 2, 1), (34, 2, 1), (44, 3, 3), (34, 2, 1), (44, 3, 3), (33, 2, 2), (43, 3, 3), (33, 2, 1), (33, 2, 2), (44, 3, 1)]
    tiles = [67, 67, 132, 67, 132, 66, 129, 65, 66, 130]
    assert len(want) == len(R.LONG_CASES)
    for case, w, n_tiles in zip(R.LONG_CASES, want, tiles):
        for d in case[4]:
            assert R.split_of(lib, case, d) == (n_tiles,) + w, (case, d)
    R.assert_long_cases_walk_several_tiles(lib)
    assert lib.simrank_operator_parts(-1, 5, 0, 1) == -1 and lib.simrank_operator_parts(5, 5, 2, 1) == -1
    assert lib.simrank_operator_parts(5, 5, 0, 0) == -1 and lib.simrank_operator_parts(5, 5, 0, 65) == -1
    assert re.search(r"#define SIMRANK_OPERATOR_NARROW 8\b", A.header(_operator))
    assert lib.simrank_operator_workspace_bytes(70, 1100, 0, 3) == 5 * 70 * 3 * 8
    assert lib.simrank_operator_workspace_bytes(70, 1100, 1, 64) == 3 * 1100 * 64 * 8
    assert lib.simrank_operator_workspace_bytes(0, 0, 0, 1) == 8
    for bad in ((70, 1100, 0, 0), (70, 1100, 0, 65), (70, -1, 0, 1), (1 << 31, 1, 0, 1), (4, 4, 7, 1)):
        assert lib.simrank_operator_workspace_bytes(*bad) == -1
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def apply(S=p, layout=3, stride=4, n_rows=4, n_cols=4, transpose=0, X=p, ld_x=2, d=2, out=p, ld_out=2, work=p):
        return lib.simrank_operator_apply(S, layout, stride, n_rows, n_cols, None, None, transpose, X, ld_x, d, 1.0, 0.0, out,
                                          ld_out, work, None)

    for bad in (apply(S=None), apply(X=None), apply(out=None), apply(work=None), apply(d=0), apply(d=65, ld_x=65, ld_out=65),
                apply(layout=9), apply(layout=-1), apply(n_rows=-1), apply(n_cols=-1), apply(stride=3), apply(ld_x=1),
                apply(ld_out=1), apply(transpose=2), apply(transpose=-1), apply(X=p + 4), apply(out=p + 4),
                apply(layout=0, stride=3)):
        assert bad == -1 and lib.simrank_operator_last_error()
    assert apply(d=65, ld_x=65, ld_out=65) == -1 and b"bands" in lib.simrank_operator_last_error()
    assert apply(n_rows=0, stride=4, out=None, work=None, X=None) == 0       # no output row: nothing asked, no device touched
    assert apply(n_cols=0, stride=0, transpose=1, S=None, out=None, work=None) == 0


# ---- argument checks of the two methods: no device ----------------------------------------------------------------------------
class _FakeSolver:
    """Stands in for a kept solver: what the argument checks reach is never the device."""

    def __init__(self, n):
        self.n, self.calls = [n], []

    def release(self):
        pass

    def apply_operator(self, j, X, transpose=False):
        self.calls.append(("matmul", j, X.copy(), transpose))
        return X * (2.0 if transpose else 1.0)

    def embed_operator(self, j, dim, p, power_iterations, seed):
        self.calls.append(("embed", j, dim, p, power_iterations, seed))
        return np.ones((self.n[0], dim)), np.arange(dim, 0, -1.0)


LABELS = ["a", "b", "c", "d"]


def kept(n=4):
    est, solver = SRA.SimRank(), _FakeSolver(n)
    est._keep(solver, [(0, LABELS[:n])])
    return est, solver


def test_matmul_takes_frames_series_and_arrays_in_the_frames_order():
    est, solver = kept()
    X = np.arange(8.0).reshape(4, 2)
    got = est.matmul(X)
    assert isinstance(got, pd.DataFrame) and list(got.index) == LABELS and list(got.columns) == [0, 1]
    assert got.values.dtype == np.float64 and np.array_equal(got.values, X) and solver.calls[-1][3] is False
    # a frame in shuffled label order is put into the frame's order and keeps its columns
    shuffled = pd.DataFrame(X, index=LABELS, columns=["u", "v"]).loc[["c", "a", "d", "b"]]
    got = est.matmul(shuffled, transpose=True)
    assert list(got.columns) == ["u", "v"] and np.array_equal(got.values, 2 * X) and solver.calls[-1][3] is True
    assert np.array_equal(solver.calls[-1][2], X)
    # a Series gives a Series with its name, a 1-D array a Series, integers are widened
    s = est.matmul(pd.Series([3, 1, 2, 0], index=["d", "b", "c", "a"], name="r"))
    assert isinstance(s, pd.Series) and s.name == "r" and s.tolist() == [0.0, 1.0, 2.0, 3.0] and s.dtype == np.float64
    v = est.matmul(np.array([1, 2, 3, 4], dtype=np.int32))
    assert isinstance(v, pd.Series) and v.tolist() == [1.0, 2.0, 3.0, 4.0] and list(v.index) == LABELS
    assert est.matmul(np.array([np.inf, np.nan, -0.0, 1.0])).isna().sum() == 1       # finite or not
    assert est.matmul(np.float32([[1], [2], [3], [4]])).shape == (4, 1)
    assert est.matmul([[1.5], [2], [3], [4]]).iloc[0, 0] == 1.5                        # any array-like


def test_matmul_and_embed_refusals_come_before_any_device_work():
    est, solver = kept()
    ok = np.zeros((4, 2))
    for bad in (np.zeros((4, 2), dtype=bool), np.array([["a"] * 2] * 4, dtype=object), np.zeros((4, 2), dtype=complex),
                np.zeros((3, 2)), np.zeros((4, 2, 1)), np.zeros(()), pd.Series([True] * 4, index=LABELS),
                pd.DataFrame({"x": [1.0] * 4, "y": ["s"] * 4}, index=LABELS),
                pd.Series([1.0, 2.0, 3.0], index=LABELS[:3]), pd.Series([1.0] * 5, index=LABELS + ["a"])):
        with pytest.raises(ValueError):
            est.matmul(bad)
    with pytest.raises(KeyError, match="zz"):
        est.matmul(pd.Series([1.0] * 4, index=["a", "b", "c", "zz"]))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="transpose"):
            est.matmul(ok, transpose=bad)
    with pytest.raises(ValueError, match="group"):
        est.matmul(ok, group=2)
    for kw in (dict(dim=0), dict(dim=5), dict(dim=2.0), dict(dim=True), dict(dim="2"), dict(dim=2, oversample=-1),
               dict(dim=2, oversample=1.5), dict(dim=2, oversample=True), dict(dim=2, power_iterations=-1),
               dict(dim=2, power_iterations=17), dict(dim=2, power_iterations=2.0), dict(dim=2, seed=-1),
               dict(dim=2, seed=0.5), dict(dim=2, seed=None), dict(dim=2, seed=True), dict(dim=2, group=2)):
        with pytest.raises(ValueError):
            est.embed(**kw)
    assert solver.calls == []
    V, w = est.embed(2, oversample=8, power_iterations=0, seed=np.int64(3))
    assert solver.calls == [("embed", 0, 2, 4, 0, 3)]                                 # p = min(dim + oversample, N)
    assert V.shape == (4, 2) and list(V.index) == LABELS and w.dtype == np.float64 and w.tolist() == [2.0, 1.0]
    est.release()
    for call in (lambda: est.matmul(ok), lambda: est.embed(2)):
        with pytest.raises(RuntimeError, match="released"):
            call()
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().matmul(ok)


# ---- the host route of a pruned model ----------------------------------------------------------------------------------------
def test_the_pruned_route_is_the_product_with_the_dense_p():
    rng = np.random.default_rng(2)
    n, kk = 70, 7
    ids = np.full((n, kk), -1, dtype=np.int32)
    vals = np.zeros((n, kk))
    for a in range(n):
        m = int(rng.integers(0, kk + 1))
        slots = np.sort(rng.choice(kk, size=m, replace=False))
        ids[a, slots] = rng.choice(np.delete(np.arange(n), a), size=m, replace=False)
        vals[a, slots] = rng.normal(size=m)
    diag = rng.normal(size=n)
    P = dense_p(ids, vals, diag)
    assert not np.array_equal(P, P.T)
    X = rng.normal(size=(n, 5))
    for transpose in (False, True):
        got = _operator.product_lists(ids, vals, diag, X, transpose)
        want = R.matmul_ref(P, X, transpose)
        assert (np.abs(got - want) <= R.product_bound(P, X, transpose)).all()
    # dyadic values: bit for bit
    Xd = R.exact_operand(rng, n, 3, 3)
    Pd = dense_p(ids, np.round(vals * 16) / 16, np.round(diag * 16) / 16)
    got = _operator.product_lists(ids, np.round(vals * 16) / 16, np.round(diag * 16) / 16, Xd, True)
    assert np.array_equal(got, Pd.T @ Xd)
    # the solver's dispatch: ``lists`` answers on the host

    class Pruned(_query.SolverQueries):
        n = [ids.shape[0]]

        def lists(self, j):
            return ids, vals, diag

    assert np.array_equal(Pruned().apply_operator(0, X, True), _operator.product_lists(ids, vals, diag, X, True))
    M = R.sym(P)
    V, w = Pruned().embed_operator(0, 3, 11, 2, 0)
    R.check_embedding(V, w, M, 11, "pruned")


# ---- the statement of embed alone meets the bounds -----------------------------------------------------------------------------
def test_embed_ref_alone_meets_the_bounds_on_a_planted_matrix():
    """The condition tests/test_gpu_operator.py's planted-matrix test stands on: with the product in NumPy, the four
    eigenvalues of the exact-rank-4 matrix at N = 257 come out within (N + c2(p)) u ||M||_F of ``eigvalsh``'s."""
    M = R.planted()
    N, dim = M.shape[0], 4
    p = dim + 8
    assert np.linalg.matrix_rank(M) == dim
    V, w = R.embed_ref(lambda Q: M @ Q, N, dim)
    want = np.sort(np.linalg.eigvalsh(M))[::-1][:dim]
    assert np.allclose(want, [4.0, 3.0, 2.0, 1.0], rtol=0, atol=1e-12)
    bound = (N + R.c2(p, N)) * R.U * np.linalg.norm(M, "fro")
    print("max |w - eigvalsh| =", np.abs(w - want).max(), "bound", bound)
    assert (np.abs(w - want) <= bound).all()
    R.check_embedding(V, w, M, p, "planted")
    # the package's host half is the same statement
    V2, w2 = _operator.embed_host(lambda Q: M @ Q, N, dim, p, 2, 0)
    assert np.array_equal(V2, V) and np.array_equal(w2, w)


def test_embed_ref_edges():
    rng = np.random.default_rng(4)
    S = rng.random((40, 40))
    M = R.sym(S)
    for dim, over in ((1, 8), (40, 0), (40, 8), (7, 0)):
        V, w = R.embed_ref(lambda Q: M @ Q, 40, dim, oversample=over)
        R.check_embedding(V, w, M, min(dim + over, 40), (dim, over))
        assert V.shape == (40, dim) and w.shape == (dim,)
    # dim = N spans everything: the eigenvalues are eigvalsh's
    V, w = R.embed_ref(lambda Q: M @ Q, 40, 40, oversample=0)
    assert np.allclose(w, np.sort(np.linalg.eigvalsh(M))[::-1], rtol=0, atol=1e-12)
    # a wrong product shows: the wrong weight, or one row of the operand not read, misses the Rayleigh bound.  (S @ Q alone
    # does not: B is symmetrised, and Q.T S Q symmetrised is Q.T M Q; the matmul tests tell S from S.T.)
    def blind(Q):
        Q = Q.copy()
        Q[3] = 0.0
        return M @ Q
    for wrong in (lambda Q: 0.5 * (S @ Q) + 1.0 * (S.T @ Q), blind):
        V, w = R.embed_ref(wrong, 40, 5)
        with pytest.raises(AssertionError):
            R.check_embedding(V, w, M, 13, "wrong product")
