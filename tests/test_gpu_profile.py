"""libsimrank_profile.so, ``count_pairs`` and ``threshold_for`` on a real MI355X.

Kernel level, on synthetic blocks (tests/blocks.py, no fit; padding holds a finite sentinel above every value, which a
kernel that reads padding would count): the count sweep EQUALS NumPy in all four layouts, with id arrays and without, on
shapes around the 8-row pieces, the 32- and 64-column panels and the vector tails, and a second call into the same
counters doubles them; the digit sweeps, driven by the host half of the select, give ``profile_ref``'s answer on a block
of distinct values and on a tie-heavy one.

Model level: both calls equal ``profile_ref`` on ``model.frame()`` for every storage, a ``LocalWorld(3)``, compact, loaded
and pruned models; ``pairs(t, max_pairs=M)`` then returns exactly n rows; the model is unchanged."""
import contextlib
import io
import math

import numpy as np
import pytest

import simrank_amd
import simrank_amd.SimRank as SRA
from simrank_amd import _profile, synth
from simrank_amd.driver import LocalWorld
from simrank_amd.engine import HipOps
from tests import blocks as B
from tests import profile_ref as PR
from tests.graphs import bipartite_random

pytestmark = pytest.mark.gpu


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


def id_cases(n_rows, n_cols, rng):
    """[(row_ids, col_ids, skip mask)]: NULL (positions), and ids that are no positions: every row shares its id with one
    column somewhere in the block, but row 0, whose id no column has."""
    pos = np.arange(n_rows)[:, None] == np.arange(n_cols)[None, :]
    col_ids = (rng.permutation(n_cols + 7)[:n_cols] * 3 + 1).astype(np.int32)
    row_ids = col_ids[(np.arange(n_rows, dtype=np.int64) * 5 + 1) % n_cols].astype(np.int32)
    row_ids[0] = -7
    return [(None, None, pos), (row_ids, col_ids, row_ids[:, None] == col_ids[None, :])]


def thresholds_of(A, rng):
    """Equal to stored values, strictly between two neighbours, below the minimum, above the maximum, both signs, both
    zeros; shuffled, with a repeat."""
    v = np.unique(A)
    some = v[rng.permutation(v.size)[:6]]
    mids = [(a + b) / 2 for a, b in zip(v[:-1], v[1:])]
    mids = [mids[i] for i in rng.permutation(len(mids))[:6]]
    near = [np.nextafter(some[0], np.inf), np.nextafter(some[0], -np.inf), float(some[0]) * (1 + 2.0 ** -30)]
    ts = np.array(list(some) + mids + near + [v[0] - 1.0, v[-1] + 1.0, v[0], v[-1], 0.0, -0.0, 1e-300, -1e-300, float(some[0])])
    rng.shuffle(ts)
    return ts


def interval_counts(v, edges):
    """uint64 [len(edges) + 1]: entries with exactly j of the sorted edges <= v."""
    return np.bincount(np.searchsorted(edges, v, side="right"), minlength=edges.size + 1).astype(np.uint64)


# ---- 1. the count sweep ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_count_equals_numpy_and_accumulates(dev, layout):
    lib, st = _profile.load(), dev.ops.stream
    for i, (n_rows, n_cols) in enumerate(SHAPES):
        for tag, stride, base in B.variants(layout, n_rows, n_cols):
            blk = B.make_block(layout, n_rows, n_cols, stride, 40 + i, kind=("dyadic", "wide")[i % 2])
            A = blk.A
            rng = np.random.default_rng([i, layout, stride])
            S = dev.put(blk.raw, base)
            ts = thresholds_of(A, rng)
            order = np.argsort(ts, kind="stable")
            edges = ts[order] if layout == B.ROWMAJOR_F64 else _profile.edges_f32(ts[order])
            edges_dev = dev.put(edges)
            for row_ids, col_ids, skip in id_cases(n_rows, n_cols, rng):
                what = (layout, n_rows, n_cols, tag, row_ids is None)
                v = A[~skip]
                want = PR.count_pairs(A, ts, skip)
                # the intervals the kernel counts are those of the edges AS COMPARED; in float64 with the caller's ts
                # they are the same sets (edges_f32), so both statements must hold
                ivals = interval_counts(v, edges.astype(np.float64))
                host = np.zeros(ts.size + 2, dtype=np.uint64)
                host[-1] = 77                                             # a guard after the last counter
                counts = dev.put(host)
                args = (S, layout, stride, n_rows, n_cols, None if row_ids is None else dev.put(row_ids),
                        None if col_ids is None else dev.put(col_ids), edges_dev, ts.size, counts, st)
                for times in (1, 2):                                      # the second call adds to the first
                    _profile.check(lib.simrank_profile_count(*args), "count")
                    got = dev.get(counts, host)
                    assert got[-1] == 77, what
                    assert np.array_equal(got[:-1], times * ivals), (what, times)
                    at_least = np.empty(ts.size, dtype=np.int64)
                    at_least[order] = np.cumsum(got[:-1][::-1].astype(np.int64))[::-1][1:]
                    assert np.array_equal(at_least, times * want), (what, times)
                assert int(got[:-1].sum()) == 2 * v.size                  # every entry, once per call: no padding, no diagonal
                # the binding's own path: one block, the caller's order
                block = dict(ptr=S, layout=layout, stride=stride, rows=n_rows, cols=n_cols, row_ids=args[5], col_ids=args[6])
                got = _profile.count_blocks(dev.ops, [block], ts)
                assert got.dtype == np.int64 and np.array_equal(got, want), what
            dev.release()


def test_count_with_nan_and_the_most_thresholds(dev):
    """1024 thresholds (the full binary search), NaN entries (never counted), -0.0 entries (>= 0.0)."""
    lib, st = _profile.load(), dev.ops.stream
    n_rows, n_cols = 70, 129
    for layout in B.LAYOUTS:
        _, stride, base = B.variants(layout, n_rows, n_cols)[0]
        blk = B.make_block(layout, n_rows, n_cols, stride, 5, kind="dyadic", zero_fraction=0.2)
        A, stored = blk.A.copy(), blk.stored.copy()
        at = B.offsets(layout, n_rows, n_cols, stride)
        rng = np.random.default_rng(layout)
        rr, cc = rng.integers(0, n_rows, size=200), rng.integers(0, n_cols, size=200)
        A[rr[:100], cc[:100]] = np.nan
        stored[at[rr[:100], cc[:100]]] = np.nan
        A[rr[100:], cc[100:]] = -0.0
        stored[at[rr[100:], cc[100:]]] = -0.0
        S = dev.put(stored.tobytes(), base)
        v = np.unique(A[~np.isnan(A)])
        stored_ts = v[rng.permutation(v.size)[:600]]
        ts = np.concatenate([stored_ts, rng.uniform(v[0] - 1, v[-1] + 1, size=1022 - stored_ts.size), [0.0, -0.0]])
        assert ts.size == _profile.MAX_EDGES
        block = dict(ptr=S, layout=layout, stride=stride, rows=n_rows, cols=n_cols)
        got = _profile.count_blocks(dev.ops, [block], ts)
        assert np.array_equal(got, PR.count_pairs(A, ts, np.eye(n_rows, n_cols, dtype=bool))), layout
        dev.release()


# ---- 2. the digit sweeps -------------------------------------------------------------------------------------------------------
def device_sweep(dev, blk_args, layout):
    lib, ops = _profile.load(), dev.ops
    bins = 1 << _profile.MAX_DIGIT_BITS
    calls = []

    def sweep(prefix, pbits, d, want_min):
        host = np.zeros(bins + 2, dtype=np.uint64)
        host[bins], host[bins + 1] = 2 ** 64 - 1, 77
        buf = dev.put(host)
        _profile.check(lib.simrank_profile_digits(*blk_args, prefix, pbits, d, buf, buf + 8 * bins if want_min else None,
                                                  ops.stream), "digits")
        got = dev.get(buf, host)
        assert got[bins + 1] == 77 and not got[1 << d:bins].any()          # nothing past the 2^d bins
        calls.append(d)
        return got[:1 << d].copy(), int(got[bins])
    return sweep, calls


@pytest.mark.parametrize("layout", B.LAYOUTS)
@pytest.mark.parametrize("kind", ["distinct", "ties"])
def test_digit_passes_reach_the_reference(dev, layout, kind):
    for n_rows, n_cols in ((33, 31), (9, 65)):
        rng = np.random.default_rng([layout, n_rows, kind == "ties"])
        if kind == "distinct":
            A = ((rng.permutation(n_rows * n_cols) - n_rows * n_cols // 2) * 2.0 ** -10).reshape(n_rows, n_cols)
        else:
            A = rng.choice([-0.0, 0.0, 2.0 ** -20, 0.25, 1.0], size=(n_rows, n_cols))
        _, stride, base = B.variants(layout, n_rows, n_cols)[0]
        S = dev.put(B.encode(layout, A, stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
        for row_ids, col_ids, skip in id_cases(n_rows, n_cols, rng):
            args = (S, layout, stride, n_rows, n_cols, None if row_ids is None else dev.put(row_ids),
                    None if col_ids is None else dev.put(col_ids))
            entries = int((~skip).sum())
            bits = _profile.key_bits(layout)
            for m in (1, 2, entries - 1, entries, entries + 1):
                sweep, calls = device_sweep(dev, args, layout)
                got = _profile.radix_select(sweep, bits, m)
                want = PR.threshold_for(A, m, skip)
                assert got == want and not (got[0] == 0 and np.signbit(got[0])), (layout, kind, n_rows, row_ids is None, m, got, want)
                assert len(calls) <= {32: 4, 16: 2, 64: 8}[bits]          # the sweeps do not depend on the data or on m
        dev.release()


def test_digits_accumulate_over_blocks(dev):
    """Two column blocks of one matrix into one histogram: the sum, and the smaller of the two minima."""
    lib, st = _profile.load(), dev.ops.stream
    rng = np.random.default_rng(3)
    A = (rng.integers(-500, 500, size=(40, 96)) * 2.0 ** -8)
    keys = np.array([lib.simrank_profile_key_f32(float(x)) for x in A.ravel()], dtype=np.uint64).reshape(A.shape)
    host = np.zeros(257, dtype=np.uint64)
    host[256] = 2 ** 64 - 1
    buf = dev.put(host)
    prefix = int(np.sort(keys.ravel())[keys.size // 3]) >> 24           # (a third of the keys lie below: some prefix is above)
    for lo, hi in ((0, 64), (64, 96)):
        part = np.ascontiguousarray(A[:, lo:hi])
        S = dev.put(B.encode(B.PANEL_F32, part, 43, 1024.0).tobytes())
        ids = dev.put(np.arange(lo, hi, dtype=np.int32))
        _profile.check(lib.simrank_profile_digits(S, B.PANEL_F32, 43, 40, hi - lo, None, ids, prefix, 8, 8, buf, buf + 8 * 256, st),
                       "digits")
    got = dev.get(buf, host)
    off = ~np.eye(40, 96, dtype=bool)
    under = off & ((keys >> np.uint64(24)) == prefix)
    assert np.array_equal(got[:256], np.bincount(((keys[under] >> np.uint64(16)) & np.uint64(255)).astype(np.int64), minlength=256))
    over = off & ((keys >> np.uint64(24)) > prefix)
    assert got[256] == keys[over].min()


# ---- 3. through the estimators ------------------------------------------------------------------------------------------------
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


def check_model(model):
    frames = as_groups(model.frame())
    bip = len(frames) == 2
    groups = [1, 2] if bip else [None]
    rng = np.random.default_rng(len(frames[0]))
    nodes = [[f.index[i] for i in rng.integers(0, len(f), size=9)] for f in frames]
    before = [model.rows(nd, **({} if g is None else {"group": g})).to_numpy().copy() for nd, g in zip(nodes, groups)]
    # thresholds from both groups' values: stored values, midpoints, the zeros, a negative one, one above everything
    vals = np.unique(np.concatenate([PR.off_diagonal(f.to_numpy()) for f in frames]))
    pos = vals[vals > 0]
    assert pos.size > 10
    some = pos[rng.permutation(pos.size)[:8]]
    ts = list(some) + [(a + b) / 2 for a, b in zip(pos[:5], pos[1:6])] + [pos[-1], np.nextafter(pos[-1], 2.0), pos[0], 0.0, -0.0, -0.25,
                                                                          1e-3, 1e-300, 0.5, float(some[0])]
    got = as_groups(model.count_pairs(ts))
    assert len(got) == len(frames)
    for g, f in zip(got, frames):
        assert isinstance(g, np.ndarray) and g.dtype == np.int64
        assert np.array_equal(g, PR.count_pairs(f.to_numpy(), ts))
    for f, g, c in zip(frames, groups, got):
        S = f.to_numpy()
        n = len(f)
        positive = int((PR.off_diagonal(S) > 0).sum())
        assert 2 < positive < n * (n - 1)                                 # there are zeros to land in
        for m in (1, 2, 7, positive // 2, positive - 1, positive, positive + 1, (positive + n * (n - 1)) // 2, n * (n - 1), 10 ** 12):
            res = model.threshold_for(m)
            t, cnt = res[groups.index(g)] if bip else res
            want = PR.threshold_for(S, m)
            assert (t, cnt) == want and isinstance(t, float) and isinstance(cnt, int), (g, m, (t, cnt), want)
            if t > 0 and math.isfinite(t):
                assert cnt <= m
                assert as_groups(model.count_pairs([t]))[groups.index(g)].tolist() == [cnt]
                # one max_pairs serves both groups of a bipartite model: the larger of their counts at t is the tightest
                # bound that lets the call through, and one less refuses it
                bound = m if not bip else max(int(x[0]) for x in as_groups(model.count_pairs([t])))
                assert len(as_groups(model.pairs(t, max_pairs=bound))[groups.index(g)]) == cnt
                if bip and bound > 1:
                    with pytest.raises(ValueError, match="max_pairs"):
                        model.pairs(t, max_pairs=bound - 1)
        # a cut that lands in the zeros keeps every positive pair and none of the zeros
        assert PR.threshold_for(S, positive + 1)[1] == positive
    for nd, g, b in zip(nodes, groups, before):
        after = model.rows(nd, **({} if g is None else {"group": g})).to_numpy()
        assert np.array_equal(B.bits(after), B.bits(b))                   # the model is unchanged
    model.release()
    for call in (lambda: model.count_pairs([0.5]), lambda: model.threshold_for(10)):
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


@pytest.mark.parametrize("variant", list(VARIANTS))                    # (a symmetric prior: fit() takes storage_precision="fp16")
def test_apriori_with_a_symmetric_prior(variant, tmp_path):
    df = synth.er_directed(150, 0.012, seed=5)
    n = len(set(df["from"]) | set(df["to"]))
    prior = np.random.default_rng(5).random((n, n)) * 0.5
    prior = np.where(np.random.default_rng(6).random((n, n)) < 0.85, 0.0, prior)       # most of it zero: there are ties at 0
    prior = (prior + prior.T) / 2
    model = make_model("AprioriSimRank", df, variant, tmp_path, prior)
    try:
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


# ---- 4. the pruned model (a function of its own: prune(k) has its own kernels) -----------------------------------------------
def test_a_pruned_model_counts_its_matrix_p(powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, "f32-kept", tmp_path)
    try:
        model.prune(10)
        assert model.kept_neighbors == 10
        check_model(model)
    finally:
        model.release()
