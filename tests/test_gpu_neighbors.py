"""libsimrank_neighbors.so and ``prune(k)`` on a real MI355X.

Kernel level, on synthetic blocks (tests/blocks.py, no fit): ``simrank_neighbors_select`` EQUALS ``blocks.ref_topk`` bit for
bit, and ``simrank_query_topk`` where that kernel takes the k, in all four layouts, on blocks full of exact zeros and
repeated values, with a row of one repeated value, a row that is mostly zeros and a row holding -0.0, NaN and -inf;
``simrank_neighbors_rows`` / ``_pairs`` / ``_score`` equal NumPy on hand-built tables.

Model level: after ``prune(k)`` every query equals the same statement on the matrix P built in NumPy from the unpruned
model's ``frame()`` and ``most_similar(all, k)``: the kept entries, the diagonal, +0.0 elsewhere."""
import contextlib
import io
import os

import numpy as np
import pandas as pd
import pytest

import simrank_amd
import simrank_amd.SimRank as SRA
from simrank_amd import _neighbors, _query, synth
from simrank_amd.driver import LocalWorld
from simrank_amd.engine import HipOps
from tests import blocks as B
from tests import sets_ref as R
from tests.graphs import bipartite_random
from tests.test_gpu_sets import baskets, same_frame

pytestmark = pytest.mark.gpu

INVALID = -1


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


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        got, want = np.where(nan, 0, got), np.where(nan, 0, want)
    bad = np.argwhere(B.bits(got) != B.bits(want))
    assert bad.size == 0, (what, "first differences at", bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- select ---------------------------------------------------------------------------------------------------------------
def tie_block(layout, n_rows, n_cols, stride, seed):
    """(A float64 [n_rows, n_cols], the block's bytes): ``make_block`` with as many zeros as it allows, then row 0 = one
    repeated value, row 1 = -0.0, NaN and -inf among its values, row 2 = zeros of both signs but for a few values."""
    blk = B.make_block(layout, n_rows, n_cols, stride, seed, kind="dyadic", zero_fraction=0.2)
    A, stored = blk.A.copy(), blk.stored.copy()
    at = B.offsets(layout, n_rows, n_cols, stride)
    rng = np.random.default_rng([seed, 99])
    scale = B.HALF_SCALE if layout == B.PANEL_F16 else 1.0

    def plant(r, cols, value):
        A[r, cols] = value
        with np.errstate(invalid="ignore"):
            stored[at[r, cols]] = np.asarray(value * scale).astype(stored.dtype)

    plant(0, np.arange(n_cols), 0.5)
    cols = rng.permutation(n_cols)
    third = max(1, n_cols // 8)
    plant(1, cols[:third], -0.0)
    plant(1, cols[third:2 * third], np.nan)
    plant(1, cols[2 * third:2 * third + 3], -np.inf)
    cols = rng.permutation(n_cols)
    plant(2, cols[:n_cols - 5], 0.0)
    plant(2, cols[:n_cols // 3], -0.0)
    assert np.array_equal(np.isnan(B.decode(layout, stored, n_rows, n_cols, stride)), np.isnan(A))
    return A, stored.tobytes()


@pytest.mark.parametrize("layout", B.LAYOUTS)
@pytest.mark.parametrize("shape", [(67, 130), (5, 2100)])
def test_select_is_the_total_order(dev, layout, shape):
    n_rows, n_cols = shape
    lib, qlib, st = _neighbors.load(), _query.load(), dev.ops.stream
    for v, (tag, stride, base) in enumerate(B.variants(layout, n_rows, n_cols)):
        A, raw = tie_block(layout, n_rows, n_cols, stride, 11 + v)
        S = dev.put(raw, base)
        rng = np.random.default_rng([n_cols, layout, v])
        row_pos = np.concatenate([[0, 1, 2], rng.permutation(n_rows)[:min(n_rows, 30)], [n_rows, 1]]).astype(np.int32)
        rng.shuffle(row_pos)
        n_q = row_pos.size
        rp = dev.put(row_pos)
        col_ids = (rng.permutation(n_cols + 7)[:n_cols] * 3 + 1).astype(np.int32)      # no identity, not monotonic
        own = col_ids[(row_pos.astype(np.int64) * 5 + 1) % n_cols].astype(np.int32)   # the id of some column
        for ids, row_ids in ((col_ids, own), (None, row_pos)):
            ids_dev, rid_dev = None if ids is None else dev.put(ids), dev.put(row_ids)
            for k in (1, 2, 63, 64, 65, n_cols - 1, n_cols):
                what = (layout, shape, tag, ids is None, k)
                hi, hv = np.full((n_q + 1, k), -9, dtype=np.int32), np.full((n_q + 1, k), 1e300)
                idx, val = dev.put(hi), dev.put(hv)
                _neighbors.check(lib.simrank_neighbors_select(S, layout, stride, n_rows, n_cols, rp, rid_dev, n_q, ids_dev, k,
                                                              idx, val, st), "select")
                hi[:n_q], hv[:n_q] = B.ref_topk(A, row_pos, row_ids, ids, k)
                got_i, got_v = dev.get(idx, hi), dev.get(val, hv)
                same_bits(got_i, hi, ("ids", what))
                same_bits(got_v, hv, ("values", what))
                if k <= 1024:
                    qi, qv = dev.put(np.full_like(hi, -9)), dev.put(np.full_like(hv, 1e300))
                    _query.check(qlib.simrank_query_topk(S, layout, stride, n_rows, n_cols, rp, rid_dev, n_q, ids_dev, k, qi,
                                                         qv, st), "topk")
                    same_bits(got_i, dev.get(qi, hi), ("ids against query_topk", what))
                    same_bits(got_v, dev.get(qv, hv), ("values against query_topk", what))
        dev.release()


# ---- rows, pairs, score on hand-built tables --------------------------------------------------------------------------------
N, K = 1100, 3


def hand_tables(seed=4):
    """(ids int32 [N, K], values [N, K], diag [N], P float64 [N, N]): lists of 3, 2, 1 and 0 entries (row 7 full, row 8
    empty), values of both signs over many binades and an exact zero that is KEPT."""
    rng = np.random.default_rng(seed)
    ids = np.full((N, K), -1, dtype=np.int32)
    vals = np.zeros((N, K))
    for a in range(N):
        m = 3 if a == 7 else 0 if a == 8 else int(rng.integers(0, K + 1))
        others = rng.permutation(N - 1)[:m]
        ids[a, :m] = others + (others >= a)
        vals[a, :m] = np.sort(rng.normal(size=m) * 10.0 ** rng.uniform(-9, 3, size=m))[::-1]
    vals[7, 2] = 0.0
    diag = rng.random(N) + 0.5
    P = np.zeros((N, N))
    for a in range(N):
        P[a, ids[a][ids[a] >= 0]] = vals[a][ids[a] >= 0]
    P[np.arange(N), np.arange(N)] = diag
    return ids, vals, diag, P


def test_rows_pairs_score_on_hand_built_tables(dev):
    lib, st = _neighbors.load(), dev.ops.stream
    ids, vals, diag, P = hand_tables()
    tables = (dev.put(ids), dev.put(vals), dev.put(diag), N, K)
    rng = np.random.default_rng(1)
    # rows: the full and the empty list, a row twice, positions outside
    row_pos = np.concatenate([[7, 8, 8, N, -1, N - 1, 0], rng.integers(0, N, size=20)]).astype(np.int32)
    ld = N + 3
    host = np.full((row_pos.size + 1, ld), 1e300)
    out = dev.put(host)
    _neighbors.check(lib.simrank_neighbors_rows(*tables, dev.put(row_pos), row_pos.size, out, ld, st), "rows")
    ok = (row_pos >= 0) & (row_pos < N)
    host[:row_pos.size, :N] = np.where(ok[:, None], P[np.where(ok, row_pos, 0)], np.nan)
    same_bits(dev.get(out, host), host, "rows")
    # pairs: diagonal, present, absent, outside
    a = np.concatenate([[7, 7, 7, 7, 8, 8, N, 3, -1], np.repeat(np.arange(20), 2)]).astype(np.int32)
    b = np.concatenate([[7, ids[7, 0], ids[7, 2], (ids[7, 0] + 1) % N, 8, 9, 3, N, 3],
                        np.stack([ids[:20, 0], np.arange(20)], axis=1).ravel()]).astype(np.int32)
    b[b < 0] = 5
    want = np.array([P[x, y] if 0 <= x < N and 0 <= y < N else np.nan for x, y in zip(a, b)])
    host = np.full(a.size + 2, 1e300)
    out = dev.put(host)
    _neighbors.check(lib.simrank_neighbors_pairs(*tables, dev.put(a), dev.put(b), a.size, out, st), "pairs")
    host[:a.size] = want
    same_bits(dev.get(out, host), host, "pairs")
    # score: the baskets of tests/test_gpu_sets.py, with and without exclusion lists, and a position out of range
    sets, weights = baskets(list(range(N)))
    ptr, pos = np.zeros(len(sets) + 1, dtype=np.int64), np.concatenate([np.asarray(s, dtype=np.int32) for s in sets])
    np.cumsum([len(s) for s in sets], out=ptr[1:])
    w = np.concatenate([np.asarray(x, dtype=np.float64) for x in weights])
    want = R.scores(P, sets, weights)
    assert not np.signbit(want[want == 0]).any()            # (a sum is never -0.0: skipping absent entries is exact)
    excl = [[0, 5], [], [1099, 1024, 1023], [], list(range(0, N, 2)), [7], []]
    xptr, xcols = np.zeros(len(sets) + 1, dtype=np.int64), np.concatenate([np.asarray(x, dtype=np.int32) for x in excl])
    np.cumsum([len(x) for x in excl], out=xptr[1:])
    bad_pos = pos.copy()
    bad_pos[ptr[3] + 5] = N                                 # one member of the 37-member basket is outside
    dev_ptr, dev_w = dev.put(ptr), dev.put(w)
    for name, p, x in (("plain", pos, None), ("excluded", pos, (xptr, xcols)), ("poisoned", bad_pos, (xptr, xcols))):
        host = np.full((len(sets) + 1, ld), 1e300)
        out = dev.put(host)
        _neighbors.check(lib.simrank_neighbors_score(*tables, dev_ptr, dev.put(p), dev_w, len(sets),
                                                     None if x is None else dev.put(x[0]), None if x is None else dev.put(x[1]),
                                                     out, ld, st), "score")
        ref = want.copy()
        if name == "poisoned":
            ref[3] = np.nan
        if x is not None:
            for q, cols in enumerate(excl):
                ref[q, cols] = -np.inf
        host[:len(sets), :N] = ref
        got = dev.get(out, host)
        same_bits(got, host, ("score", name))
        assert np.all(got[0, :N][np.isfinite(got[0, :N])] == 0.0)
    assert lib.simrank_neighbors_score(*tables[:3], N, 0, dev_ptr, dev.put(pos), dev_w, len(sets), None, None, out, ld, st) == INVALID


# ---- model level -------------------------------------------------------------------------------------------------------------
UPDATES = 3


def fit(cls, df, *args, **kw):
    est = getattr(SRA, cls)()
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(df, *args, iterations=UPDATES, eps=1e-30, verbose=False, keep=True, **kw)
    return est


@pytest.fixture(scope="module")
def graph():
    df = synth.er_directed(N, 0.002, seed=7)
    assert len(set(df["from"]) | set(df["to"])) == N
    return df


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


def pruned_matrix(dense, ms, k):
    """P of one group in NumPy: the first k entries of every node's ``most_similar`` block, the diagonal, +0.0 elsewhere."""
    labels = list(dense.index)
    at = {lab: i for i, lab in enumerate(labels)}
    P = np.zeros(dense.shape)
    P[np.arange(len(labels)), np.arange(len(labels))] = np.diag(dense.values)
    part = ms[ms["rank"] <= k]
    P[[at[x] for x in part["node"]], [at[x] for x in part["neighbor"]]] = part["similarity"].to_numpy()
    return pd.DataFrame(P, index=dense.index.copy(), columns=dense.columns.copy())


def as_groups(x):
    return list(x) if isinstance(x, tuple) else [x]


def kept_of(k, ns):
    ks = [min(k, max(1, n - 1)) for n in ns]
    return ks[0] if len(set(ks)) == 1 else tuple(ks)


def check_queries(model, Ps, mss, k, light=False):
    """Every query of the pruned ``model`` against the statements on ``Ps`` (one frame per group)."""
    groups = [None] if len(Ps) == 1 else [1, 2]
    frames = as_groups(model.frame())
    for P, got in zip(Ps, frames):
        same_frame(got, P, "frame")
    ns = [len(P) for P in Ps]
    assert model.kept_neighbors == kept_of(k, ns)
    assert model.device_bytes == sum(n * min(k, max(1, n - 1)) * 12 + n * 8 for n in ns)
    for g, P, ms in zip(groups, Ps, mss):
        kw = {} if g is None else {"group": g}
        labels, n = list(P.index), len(P)
        kk = min(k, max(1, n - 1))
        rng = np.random.default_rng(k)
        nodes = [labels[i] for i in rng.integers(0, n, size=12)] + [labels[0]]
        same_frame(model.rows(nodes, **kw), P.loc[nodes], "rows")
        first = ms[ms["rank"] == 1]
        a = nodes + list(first["node"][:10]) + nodes
        b = nodes + list(first["neighbor"][:10]) + nodes[::-1]
        want = np.array([P.at[x, y] for x, y in zip(a, b)])
        assert np.array_equal(model.similarity(a, b, **kw).view(np.uint64), want.view(np.uint64))
        for k2 in sorted({1, kk // 2 or 1, kk}):
            part = ms[ms["node"].isin(set(nodes)) & (ms["rank"] <= k2)]
            want = pd.concat([part[part["node"] == x] for x in nodes]).reset_index(drop=True)
            same_frame(model.most_similar(nodes, k2, **kw), want, ("most_similar", k2))
        if kk < n - 1:                                          # (k = N - 1 keeps every other node: nothing is more)
            with pytest.raises(ValueError, match="kept_neighbors"):
                model.most_similar(nodes, kk + 1, **kw)
    # top_k and pairs: the statements of the existing functions, on P
    k2 = max(1, min(k, min(ns) - 1) // 2)
    for got, ms in zip(as_groups(model.top_k(k2)), mss):
        same_frame(got, ms[ms["rank"] <= k2].reset_index(drop=True), ("top_k", k2))
    t = 1e-3
    total = 0
    for got, P in zip(as_groups(model.pairs(t)), Ps):
        hit = P.values >= t
        np.fill_diagonal(hit, False)
        rr, cc = np.nonzero(hit)
        want = pd.DataFrame({"node": P.index.take(rr), "neighbor": P.index.take(cc), "similarity": P.values[rr, cc]})
        same_frame(got, want, "pairs")
        total += len(want)
    if total > 1:
        with pytest.raises(ValueError, match="max_pairs"):
            model.pairs(t, max_pairs=1)
    # baskets: tests/sets_ref.py on model.frame()
    for g, frame in zip(groups, frames):
        kw = {} if g is None else {"group": g}
        labels = list(frame.index)
        sets, weights = baskets(labels)
        names = ["q%d" % i for i in range(len(sets))]
        same_frame(model.score_sets(sets, weights=weights, names=names, **kw), R.score_sets_ref(frame, sets, weights, names), "dense")
        if not light:
            same_frame(model.score_sets(sets, **kw), R.score_sets_ref(frame, sets), "dense, unit weights")
        other = [labels[:3], [], labels[2:len(labels) - 9], [], labels[1:], [labels[0]], []]
        for exclude in ("members", None, other):
            same_frame(model.score_sets(sets, weights=weights, top_k=10, exclude=exclude, **kw),
                       R.score_sets_ref(frame, sets, weights, top_k=10, exclude=exclude), ("top", exclude if exclude is None else "x"))
    solver, sides = model._model
    bip = len(sides) == 2
    for side, g in enumerate(groups):
        kw = {} if g is None else {"group": g}
        own, read = frames[side], frames[len(frames) - 1 - side]
        spec = solver.specs[side]
        rowptr, col, scale = np.asarray(spec.csr.rowptr), np.asarray(spec.csr.col), np.asarray(spec.rowscale)
        labels = list(own.index)
        deg = np.diff(rowptr)
        nodes = [labels[int(np.argmax(deg))], labels[int(np.argmin(deg))]] + [labels[i] for i in np.random.default_rng(23).permutation(len(labels))[:20]]
        for seen in (True, False):
            same_frame(model.recommend(nodes, 10, exclude_seen=seen, **kw),
                       R.recommend_ref(read, labels, rowptr, col, scale, nodes, 10, seen, also_self=not bip), ("recommend", seen))
    with pytest.raises(ValueError, match="fold in before"):
        model.fold_in([[as_groups(model.frame())[0].index[0]]], **({} if len(Ps) == 1 else {"group": 1}))
    if any(min(k, max(1, n - 1)) < n - 1 for n in ns):
        with pytest.raises(ValueError, match="kept_neighbors"):
            model.prune(max(min(k, max(1, n - 1)) for n in ns) + 1)
    assert model.compact() is model
    with pytest.raises(ValueError, match="pruned"):
        model.compact(precision="fp16")


def unpruned_most_similar(model, dense, k, group):
    """``most_similar(all, k)`` of the model BEFORE pruning.  Its selection, simrank_query_topk, takes k up to 1024; a
    longer list (k = N - 1 at N = 1100) is that statement written out on the dense frame by ``blocks.ref_topk``: the total
    order, the node itself excluded, NaN never listed."""
    labels, n = list(dense.index), len(dense)
    kk = min(k, max(1, n - 1))
    if kk <= 1024:
        return model.most_similar(labels, k, **({} if group is None else {"group": group}))
    at = np.arange(n, dtype=np.int32)
    idx, val = B.ref_topk(dense.to_numpy(), at, at, None, kk)
    keep = idx.ravel() >= 0
    return pd.DataFrame({"node": dense.index.take(np.repeat(at.astype(np.intp), kk)[keep]),
                         "rank": np.tile(np.arange(1, kk + 1), n)[keep],
                         "neighbor": dense.index.take(idx.ravel()[keep]),
                         "similarity": val.ravel()[keep]})


def check_prune(model, k, tmp_path, light=False):
    dense = as_groups(model.frame())
    groups = [None] if len(dense) == 1 else [1, 2]
    mss = [unpruned_most_similar(model, d, k, g) for g, d in zip(groups, dense)]
    assert model.kept_neighbors is None
    assert model.prune(k) is model
    check_queries(model, [pruned_matrix(d, ms, k) for d, ms in zip(dense, mss)], mss, k, light)
    # save -> release -> load: the same answers, and the file holds the header, the tables and the CSR
    path = tmp_path / "pruned.bin"
    model.save(path)
    solver = model._model[0]
    payload = sum(t.nbytes for t in solver.tables) + sum(4 * (s.csr.rowptr.size + s.csr.col.size) + 8 * s.rowscale.size for s in solver.specs)
    with open(path, "rb") as f:
        from simrank_amd import _model
        meta, arrays = _model.parse_header(f)
    assert meta["form"] == "neighbors" and meta["format"] == 1
    head = min(a["offset"] for a in arrays.values())
    assert payload + head <= os.path.getsize(path) <= payload + head + 64 * len(arrays)
    model.release()
    with pytest.raises(RuntimeError, match="released"):
        model.rows([dense[0].index[0]], **({} if len(dense) == 1 else {"group": 1}))
    loaded = simrank_amd.load_model(path)
    try:
        with pytest.raises(AttributeError, match="loaded from a file, not fitted"):
            loaded.Graph if len(dense) == 1 else loaded.Graph_N1_N2
        check_queries(loaded, [pruned_matrix(d, ms, k) for d, ms in zip(dense, mss)], mss, k, light=True)
        # pruning again cuts the lists: what pruning the original with k // 2 gives
        if k // 2 >= 1:
            assert loaded.prune(k // 2) is loaded
            check_queries(loaded, [pruned_matrix(d, ms, k // 2) for d, ms in zip(dense, mss)],
                          [ms[ms["rank"] <= k // 2].reset_index(drop=True) for ms in mss], k // 2, light=True)
    finally:
        loaded.release()


CASES = [("f32-kept", 1), ("f32-kept", 10), ("f32-kept", 64), ("f32-kept", N - 1), ("f32-compact", 10), ("f32-compact", N - 1),
         ("f32-compact-fp16", 10), ("fp16-kept", 10), ("fp16-kept", 64), ("f64-kept", 10), ("f64-kept", 64), ("world3-kept", 10),
         ("world3-kept", 64), ("loaded", 10), ("loaded", 64)]


@pytest.mark.parametrize("variant,k", CASES)
def test_prune_on_a_directed_fit(variant, k, graph, tmp_path):
    model = make_model("SimRankPP" if k == 64 else "SimRank", graph, variant, tmp_path)
    try:
        check_prune(model, k, tmp_path, light=k == N - 1)
    finally:
        model.release()


@pytest.mark.parametrize("k", [1, 10, 39])
def test_prune_with_an_asymmetric_prior(k, tmp_path):
    """AprioriSimRank on a ring of 40 with a prior that is not symmetric: the iterate is dense and asymmetric, so is P."""
    n = 40
    df = pd.DataFrame({"from": np.arange(n), "to": (np.arange(n) + 1) % n})
    df = pd.concat([df, pd.DataFrame({"from": [0, 5, 9], "to": [20, 30, 2]})]).reset_index(drop=True)
    prior = np.random.default_rng(5).random((n, n)) * 0.5
    model = fit("AprioriSimRank", df, prior)
    try:
        frame = model.frame()
        assert not np.array_equal(frame.values, frame.values.T)
        check_prune(model, k, tmp_path)
    finally:
        model.release()


@pytest.mark.parametrize("variant,k", [("f32-kept", 10), ("f32-kept", 64), ("f32-compact", 10), ("loaded", 64)])
def test_prune_on_a_bipartite_fit(variant, k, tmp_path):
    df = bipartite_random(33, 65, 0.15, 12)
    model = make_model("BipartiteSimRankPP", df, variant, tmp_path, strict_reference=False)
    try:
        check_prune(model, k, tmp_path)
        assert kept_of(64, [33, 65]) == (32, 64)
    finally:
        model.release()


def test_lifetime(graph):
    model = fit("SimRank", graph)
    labels = list(model.frame().index)
    model.prune(5)
    before = model.device_bytes
    assert before == N * 5 * 12 + N * 8
    model.score_sets([labels[:5]], top_k=3)
    model.recommend(labels[:5], 3)
    model.rows(labels[:2])
    assert model.device_bytes == before
    tables = model._model[0].tables
    model.fit(graph, iterations=1, verbose=False, keep=True)   # a second fit frees the tables
    assert all(t.ids is None and t.vals is None and t.diag is None for t in tables)
    assert model.kept_neighbors is None
    with model:
        model.prune(3)
    for call in (lambda: model.rows(labels[:1]), lambda: model.most_similar(labels[:1], 1), lambda: model.prune(2),
                 lambda: model.score_sets([labels[:5]]), lambda: model.frame()):
        with pytest.raises(RuntimeError, match="released"):
            call()
