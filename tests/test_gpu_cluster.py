"""libsimrank_cluster.so and ``components`` on a real MI355X.

Kernel level, on synthetic blocks (tests/blocks.py, no fit; padding holds a finite sentinel above every value, which a
kernel that reads padding would turn into edges): the three C entries give ``cluster_ref``'s components, and as roots
each component's SMALLEST id, in all four layouts, with id arrays and without, 8 levels at once, on shapes around the
8-row pieces, the 32- and 64-column panels and the vector tails; with NaN and -0.0 entries; with an edge only below the
diagonal; over two column blocks into one forest; on a shuffled path of 2049 nodes (deep trees across workgroups) and on
an all-ones block (every lane at one root).  The status word stays 0 everywhere and a second run gives the same integers.

Model level: ``components`` equals ``cluster_ref`` on ``model.frame()`` for every storage, a ``LocalWorld(3)``, compact,
loaded and pruned models; the scalar and the sequence form agree; the model is unchanged."""
import contextlib
import io

import numpy as np
import pandas as pd
import pytest

import simrank_amd
import simrank_amd.SimRank as SRA
from simrank_amd import _cluster, synth
from simrank_amd.driver import LocalWorld
from simrank_amd.engine import HipOps
from tests import blocks as B
from tests import cluster_ref as CR
from tests.graphs import bipartite_random

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A


class Dev:
    """Device memory of one test through HipOps: freed together at the end."""

    def __init__(self):
        self.ops, self.held = HipOps(0), []

    def put(self, host, base=0):
        host = np.frombuffer(host, dtype=np.uint8) if isinstance(host, (bytes, bytearray)) else np.ascontiguousarray(host)
        ptr = self.ops._malloc(host.nbytes + base + 16)
        self.held.append(ptr)
        if host.nbytes:
            self.ops.h2d(ptr + base, host)
        return ptr + base

    def get(self, ptr, like):
        out = np.empty_like(like)
        self.ops.d2h(out, ptr)
        self.ops.synchronize()
        return out

    def release(self):
        self.ops.synchronize()
        for p in self.held:
            self.ops._free(p)
        self.held = []


@pytest.fixture(scope="module")
def device():
    d = Dev()
    yield d
    d.release()
    d.ops.close()


@pytest.fixture
def dev(device):
    yield device
    device.release()


# (3, 1029): a row-major f32 row past one group of four chunks in flight (1024 columns), with a ragged tail
SHAPES = [(1, 1), (7, 33), (8, 64), (9, 65), (33, 31), (129, 257), (64, 700), (3, 1029)]


def edges_for(layout, ts):
    ts = np.asarray(ts, dtype=np.float64)
    return np.ascontiguousarray(ts if layout == B.ROWMAJOR_F64 else _cluster.edges_f32(ts))


def forest(dev, blocks, n, layout, ts):
    """The three C entries on ``blocks`` [(S, stride, n_rows, n_cols, row_ids, col_ids)]: (roots int32 [len(ts), n], the
    status word).  A guard word after each of the two arrays must survive; the parent array must keep parent[x] <= x."""
    lib, st, m = _cluster.load(), dev.ops.stream, len(ts)
    host = np.full(m * n + 2, GUARD, dtype=np.int32)
    parent, out = dev.put(host), dev.put(host)
    status = out + 4 * m * n
    edges = dev.put(edges_for(layout, ts))
    _cluster.check(lib.simrank_cluster_init(parent, n, m, status, st), "init")
    for S, stride, n_rows, n_cols, row_ids, col_ids in blocks:
        _cluster.check(lib.simrank_cluster_union(S, layout, stride, n_rows, n_cols, row_ids, col_ids, edges, m, parent, n,
                                                 status, st), "union")
    _cluster.check(lib.simrank_cluster_labels(parent, n, m, out, status, st), "labels")
    got, par = dev.get(out, host), dev.get(parent, host)
    assert got[-1] == GUARD and par[-1] == GUARD and par[-2] == GUARD
    par = par[:m * n].reshape(m, n)
    assert (par <= np.arange(n)).all() and (par >= 0).all()             # the invariant, at rest
    return got[:m * n].reshape(m, n), int(got[m * n])


def want_roots(labels):
    """Labels numbered by first member -> per node the first member (the smallest id) of its component."""
    first = np.full(int(labels.max()) + 1, -1, dtype=np.int64)
    for x in range(labels.size - 1, -1, -1):
        first[labels[x]] = x
    return first[labels]


def levels_of(A):
    """8 thresholds of a block: its largest stored value, a midpoint just below, stored values that leave few and more
    edges, both zeros, one below everything (negative) and one above everything."""
    v = np.unique(A[~np.isnan(A)])
    q = lambda f: float(v[min(v.size - 1, int(f * v.size))])
    mid = float(v[-1] + v[max(0, v.size - 2)]) / 2
    return [q(0.9), float(v[-1]), 0.0, mid, float(v[0]) - 1.0, q(0.97), -0.0, float(v[-1]) + 1.0]


def id_cases(n_rows, n_cols, rng):
    """[(n, row_ids, col_ids)]: NULL (positions: row r and column r are one node), and ids scattered over a larger id
    space: most rows are also columns somewhere in the block, some rows and columns are nodes of their own, and a few ids
    lie outside 0 .. n - 1 (padding: skipped)."""
    n = n_rows + n_cols + 5
    spread = rng.permutation(n)
    col_ids = spread[:n_cols].astype(np.int32)
    row_ids = np.where(rng.random(n_rows) < 0.6, col_ids[(np.arange(n_rows) * 5 + 1) % n_cols],
                       spread[n_cols + np.arange(n_rows) % (n - n_cols)]).astype(np.int32)
    if n_rows > 4:
        row_ids[[1, n_rows - 1]] = [-7, n]
    if n_cols > 6:
        col_ids[[0, 5, n_cols - 1]] = [n + 3, -1, 2 ** 31 - 1]
    return [(max(n_rows, n_cols), None, None), (n, row_ids, col_ids)]


def check_levels(dev, blocks, n, layout, ts, want_edges, what):
    """Run twice; both runs equal the reference and each other."""
    got, status = forest(dev, blocks, n, layout, ts)
    assert status == 0, what
    for i, t in enumerate(ts):
        want = CR.labels_of_edges(n, want_edges(t))
        assert np.array_equal(got[i], want_roots(want)), (what, t)
        assert np.array_equal(_cluster.number(got[i:i + 1])[0], want), (what, t)
    again, status = forest(dev, blocks, n, layout, ts)
    assert status == 0 and np.array_equal(again, got), what
    return got


# ---- 1. the C entries on synthetic blocks --------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_union_equals_the_reference(dev, layout):
    nontrivial = 0
    for i, (n_rows, n_cols) in enumerate(SHAPES):
        for tag, stride, base in B.variants(layout, n_rows, n_cols):
            blk = B.make_block(layout, n_rows, n_cols, stride, 60 + i, kind=("dyadic", "wide")[i % 2])
            A = blk.A
            rng = np.random.default_rng([i, layout, stride])
            S = dev.put(blk.raw, base)
            ts = levels_of(A)
            for n, row_ids, col_ids in id_cases(n_rows, n_cols, rng):
                what = (layout, n_rows, n_cols, tag, row_ids is None)
                block = (S, stride, n_rows, n_cols, None if row_ids is None else dev.put(row_ids),
                         None if col_ids is None else dev.put(col_ids))
                got = check_levels(dev, [block], n, layout, ts, lambda t: CR.block_edges(A, row_ids, col_ids, n, t), what)
                assert np.array_equal(got[7], np.arange(n)), what                # above every value: nothing joins
                sizes = [np.bincount(np.unique(g, return_inverse=True)[1].reshape(-1)) for g in got]
                nontrivial += sum(1 for s in sizes if s.size >= 2 and s.max() >= 2)
                # the binding's own path: one block
                b = dict(ptr=S, layout=layout, stride=stride, rows=n_rows, cols=n_cols, row_ids=block[4], col_ids=block[5])
                assert np.array_equal(_cluster.roots_blocks(dev.ops, [b], n, ts), got), what
            dev.release()
    assert nontrivial >= 20                                               # the levels are not all "nothing" or "everything"


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_nan_and_negative_zero_entries(dev, layout):
    """A block of negative values with a few NaN, -0.0, +0.0 and positive entries: at 0.0 and at -0.0 exactly the zeros
    of both signs and the positive entries join; NaN joins nothing at any level."""
    n_rows, n_cols = 70, 129
    _, stride, base = B.variants(layout, n_rows, n_cols)[0]
    rng = np.random.default_rng(layout)
    A = -(rng.integers(1, 1000, size=(n_rows, n_cols)) * 2.0 ** -10)
    stored = B.encode(layout, A, stride, B.SENTINEL[(layout, "dyadic")])
    at = B.offsets(layout, n_rows, n_cols, stride)
    rr, cc = rng.integers(0, n_rows, size=160), rng.integers(0, n_cols, size=160)
    for lo, v in ((0, np.nan), (60, -0.0), (100, 0.0), (130, 0.25)):
        hi = {0: 60, 60: 100, 100: 130, 130: 160}[lo]
        A[rr[lo:hi], cc[lo:hi]] = v
        stored[at[rr[lo:hi], cc[lo:hi]]] = v if np.isnan(v) else B.store(layout, v)
    assert np.array_equal(B.bits(B.decode(layout, stored, n_rows, n_cols, stride)), B.bits(A))
    S = dev.put(stored.tobytes(), base)
    n = n_cols
    ts = [0.0, -0.0, 0.25, 2.0 ** -10, -2.0 ** -10, -0.5, -2.0, 0.5]
    got = check_levels(dev, [(S, stride, n_rows, n_cols, None, None)], n, layout, ts,
                       lambda t: CR.block_edges(A, None, None, n, t), layout)
    assert np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[4])
    assert 2 < np.unique(got[0]).size < n and np.unique(got[6]).size == 1 and np.unique(got[7]).size == n


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_an_edge_only_below_the_diagonal(dev, layout):
    n = 9
    A = np.full((n, n), -1.0)
    A[5, 2] = 1.0                                             # S[5][2] >= t while S[2][5] is not: the OR joins 2 and 5
    _, stride, base = B.variants(layout, n, n)[0]
    S = dev.put(B.encode(layout, A, stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
    got, status = forest(dev, [(S, stride, n, n, None, None)], n, layout, [0.5, 1.0, 1.25])
    assert status == 0
    assert got[0].tolist() == [0, 1, 2, 3, 4, 2, 6, 7, 8] == got[1].tolist() and got[2].tolist() == list(range(n))


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_two_column_blocks_into_one_forest(dev, layout):
    """Two column blocks of one matrix (a ``LocalWorld``'s ranks) accumulated into one parent array: the whole matrix's
    components, which neither block gives alone."""
    rng = np.random.default_rng(3)
    n = 96
    A = rng.integers(-500, 500, size=(n, n)) * 2.0 ** -8
    ts = [1.9, 1.8, 1.7, 1.6, 1.5, 1.2, 0.0, 2.5]
    blocks, alone = [], []
    for lo, hi in ((0, 64), (64, 96)):
        part = np.ascontiguousarray(A[:, lo:hi])
        _, stride, base = B.variants(layout, n, hi - lo)[0]
        S = dev.put(B.encode(layout, part, stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
        blocks.append((S, stride, n, hi - lo, None, dev.put(np.arange(lo, hi, dtype=np.int32))))
        alone.append(forest(dev, blocks[-1:], n, layout, ts)[0])
    got = check_levels(dev, blocks, n, layout, ts, lambda t: CR.block_edges(A, None, None, n, t), ("two blocks", layout))
    assert np.array_equal(_cluster.number(got), CR.components(A, ts))
    assert not np.array_equal(got, alone[0]) and not np.array_equal(got, alone[1])
    sizes = [np.unique(g).size for g in got]
    assert any(1 < s < n for s in sizes)


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_a_shuffled_path_of_2049_nodes(dev, layout):
    """Values 1 on a path through shuffled positions (each step stored in one direction only), 0 elsewhere, node ids
    shuffled again: the trees get deep and every union crosses workgroups.  One component at 1, singletons above."""
    n = 2049
    rng = np.random.default_rng(17)
    seq, ids = rng.permutation(n), rng.permutation(n).astype(np.int32)
    flip = rng.random(n - 1) < 0.5
    a, b = np.where(flip, seq[1:], seq[:-1]), np.where(flip, seq[:-1], seq[1:])
    A = np.zeros((n, n))
    A[a, b] = 1.0
    _, stride, base = B.variants(layout, n, n)[0]
    S = dev.put(B.encode(layout, A, stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
    idp = dev.put(ids)
    ts = [1.0, float(np.nextafter(1.0, 2.0)), 0.5, 1.5]
    got, status = forest(dev, [(S, stride, n, n, idp, idp)], n, layout, ts)
    assert status == 0
    assert not got[0].any() and not got[2].any()              # one component: every root is node 0
    assert np.array_equal(got[1], np.arange(n)) and np.array_equal(got[3], np.arange(n))
    again, status = forest(dev, [(S, stride, n, n, idp, idp)], n, layout, ts)
    assert status == 0 and np.array_equal(again, got)


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_an_all_ones_block(dev, layout):
    """257 x 257 ones: every entry is an edge of every level at once and every union meets at one root."""
    n = 257
    _, stride, base = B.variants(layout, n, n)[0]
    S = dev.put(B.encode(layout, np.ones((n, n)), stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
    ts = [1.0, 0.5, 0.0, -1.0, 1.0, 0.25, 0.125, 1.5]
    for _ in range(2):
        got, status = forest(dev, [(S, stride, n, n, None, None)], n, layout, ts)
        assert status == 0 and not got[:7].any() and np.array_equal(got[7], np.arange(n))


# ---- 2. through the estimators ------------------------------------------------------------------------------------------------
UPDATES = 3


def fit(cls, df, *args, **kw):
    est = getattr(SRA, cls)()
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(df, *args, iterations=UPDATES, eps=1e-30, verbose=False, keep=True, **kw)
    return est


VARIANTS = {
    "f32-kept": ({}, None),
    "f32-compact": ({}, "compact"),
    "f32-compact-fp16": ({}, "compact-fp16"),
    "fp16-kept": ({"storage_precision": "fp16"}, None),
    "f64-kept": ({"storage_precision": "f64"}, None),
    "world3-kept": ({"world": 3}, None),
    "loaded": ({}, "load"),
}


def make_model(cls, df, variant, tmp_path, *args, **more):
    kw, then = VARIANTS[variant]
    kw = dict(kw, **more)
    if "world" in kw:
        kw.update(world=LocalWorld(kw["world"]), mode="sparse")
    model = fit(cls, df, *args, **kw)
    if then == "compact":
        model.compact()
    elif then == "compact-fp16":
        model.compact(precision="fp16")
    elif then == "load":
        model.save(tmp_path / "dense.bin")
        model.release()
        model = simrank_amd.load_model(tmp_path / "dense.bin")
    return model


def as_groups(x):
    return list(x) if isinstance(x, tuple) else [x]


def off_diagonal(S):
    return S[~np.eye(len(S), dtype=bool)]


def check_model(model):
    frames = as_groups(model.frame())
    bip = len(frames) == 2
    groups = [1, 2] if bip else [None]
    rng = np.random.default_rng(len(frames[0]))
    nodes = [[f.index[i] for i in rng.integers(0, len(f), size=9)] for f in frames]
    before = [model.rows(nd, **({} if g is None else {"group": g})).to_numpy().copy() for nd, g in zip(nodes, groups)]
    # the model's own positive stored values at the quantiles 0 / 0.5 / 0.9 / 0.99 / 1, both zeros' side, a negative
    # threshold and one above everything: 8 levels, not in order
    vals = np.unique(np.concatenate([off_diagonal(f.to_numpy()) for f in frames]))
    pos = vals[vals > 0]
    assert pos.size > 10
    at = lambda f: float(pos[min(pos.size - 1, int(f * pos.size))])
    ts = [at(0.9), at(0.0), 0.0, at(1.0), -0.25, at(0.5), float(np.nextafter(pos[-1], 2.0)), at(0.99)]
    got = as_groups(model.components(ts))
    assert len(got) == len(frames)
    for g, f in zip(got, frames):
        S = f.to_numpy()
        want = CR.components(S, ts)
        assert isinstance(g, pd.DataFrame) and g.index.equals(f.index) and (g.dtypes == np.int64).all()
        assert g.columns.tolist() == ts
        assert np.array_equal(g.to_numpy().T, want)
        # at least one level says something: two components or more, one of them with two members or more
        sizes = [np.bincount(w) for w in want]
        assert any(s.size >= 2 and s.max() >= 2 for s in sizes), [(s.size, int(s.max())) for s in sizes]
        assert sizes[4].size == 1                                         # a similarity is >= 0 > -0.25: everything joins
        assert sizes[6].size == len(S)                                    # above every value: singletons
    for k in (0, 7, 2):                                                   # the scalar form: the same column
        one = as_groups(model.components(ts[k]))
        for s, g, f in zip(one, got, frames):
            assert isinstance(s, pd.Series) and s.name == "component" and s.dtype == np.int64 and s.index.equals(f.index)
            assert np.array_equal(s.to_numpy(), g.iloc[:, k].to_numpy())
    for nd, g, b in zip(nodes, groups, before):
        after = model.rows(nd, **({} if g is None else {"group": g})).to_numpy()
        assert np.array_equal(B.bits(after), B.bits(b))                   # the model is unchanged
    model.release()
    for call in (lambda: model.components(0.5), lambda: model.components([0.5, 0.1])):
        with pytest.raises(RuntimeError, match="released"):
            call()


@pytest.fixture(scope="module")
def powerlaw():
    return synth.powerlaw_directed(300, 4.0, seed=11)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_simrankpp_on_a_power_law_graph(variant, powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, variant, tmp_path)
    try:
        check_model(model)
    finally:
        model.release()


def sparse_prior(n, symmetric):
    prior = np.random.default_rng(5).random((n, n)) * 0.5
    prior = np.where(np.random.default_rng(6).random((n, n)) < 0.85, 0.0, prior)       # most of it zero
    return (prior + prior.T) / 2 if symmetric else prior


@pytest.mark.parametrize("variant", list(VARIANTS))                    # (a symmetric prior: fit() takes storage_precision="fp16")
def test_apriori_with_a_symmetric_prior(variant, tmp_path):
    df = synth.er_directed(150, 0.012, seed=5)
    n = len(set(df["from"]) | set(df["to"]))
    model = make_model("AprioriSimRank", df, variant, tmp_path, sparse_prior(n, True))
    try:
        check_model(model)
    finally:
        model.release()


# (an asymmetric prior makes S[a, b] != S[b, a]: the OR of the two directions decides.  Every form but "fp16-kept":
# fit(storage_precision="fp16") wants a symmetric prior; compact(precision="fp16") narrows a matrix of any symmetry)
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "fp16-kept"])
def test_apriori_with_an_asymmetric_prior(variant, tmp_path):
    df = synth.er_directed(150, 0.012, seed=5)
    n = len(set(df["from"]) | set(df["to"]))
    model = make_model("AprioriSimRank", df, variant, tmp_path, sparse_prior(n, False))
    try:
        S = model.frame().to_numpy()
        assert (S != S.T).sum() > n                                       # the directions do differ
        check_model(model)
    finally:
        model.release()


# (every form but "fp16-kept": fit() refuses fp16-held matrices for the two-matrix classes)
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "fp16-kept"])
def test_bipartite_simrankpp(variant, tmp_path):
    df = bipartite_random(90, 50, 0.06, 12)
    model = make_model("BipartiteSimRankPP", df, variant, tmp_path, strict_reference=False)
    try:
        check_model(model)
    finally:
        model.release()


# ---- 3. the pruned model: its matrix P, on the host ---------------------------------------------------------------------------
def test_a_pruned_model_clusters_its_matrix_p(powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, "f32-kept", tmp_path)
    try:
        model.prune(10)
        assert model.kept_neighbors == 10
        check_model(model)
    finally:
        model.release()
