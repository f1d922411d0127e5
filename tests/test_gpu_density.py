"""libsimrank_density.so on a real MI355X, kernel level, on synthetic blocks (tests/blocks.py, no fit): ``A[r][c] !=
A[c][r]``, both signs, and padding that holds a finite sentinel above every value, so a wrong transposed read or a read
of padding becomes a wrong count.

The four C entries give ``density_ref``'s integers exactly (the counts, the core flags, as roots each cluster's SMALLEST
core node, -1 for noise) in all four layouts, with the strides and bases of ``blocks.variants``, with ``ids = NULL`` and
with a permutation that has a few ids out of range, for 1 and for 8 levels at once, at n on both sides of the 64 x 64
tile: one tile, a diagonal tile plus off-diagonal pairs, a ragged last tile.  Guard words after every output array
survive, ``parent[x] <= x`` at rest, the status word stays 0 and a second run gives the same integers.  Planted cases: a
pass only below the diagonal, a pair in two different tiles that passes both ways, NaN and -0.0, an all-ones block, a
block where nothing passes, and the union sweep accumulated over two column blocks."""
import numpy as np
import pytest

from simrank_amd import _density
from tests import blocks as B
from tests import density_ref as DR
from tests.test_gpu_cluster import GUARD, dev, device, edges_for  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 127, 129, 200)
MIN_SAMPLES = (1, 2, 3, 5)


def itemsize(layout):
    return 8 if layout == B.ROWMAJOR_F64 else 4                    # of a threshold


def run_degrees(dev, S, layout, stride, n, ids, ts):
    """simrank_density_init + _degrees on the square block: (int32 [len(ts), n], the device counts, the device edges)."""
    lib, st, m = _density.load(), dev.ops.stream, len(ts)
    host = np.full(m * n + 2, GUARD, dtype=np.int32)
    deg = dev.put(host)
    status = deg + 4 * m * n
    edges = dev.put(edges_for(layout, ts))
    _density.check(lib.simrank_density_init(deg, None, None, n, m, status, st), "init")
    _density.check(lib.simrank_density_degrees(S, layout, stride, n, ids, edges, m, deg, st), "degrees")
    got = dev.get(deg, host)
    assert got[-1] == GUARD and got[m * n] == 0
    return got[:m * n].reshape(m, n), deg, edges


def run_clusters(dev, blocks, layout, n, edge, deg, min_samples):
    """simrank_density_init (on counters of its own), one _union per block of ``blocks`` [(S, stride, n_rows, n_cols,
    row_ids, col_ids)] at the device threshold ``edge`` over the device counts ``deg``, then _labels: int32 [n], the
    roots; the forest at rest is in order and no guard word is touched."""
    lib, st = _density.load(), dev.ops.stream
    host = np.full(n + 2, GUARD, dtype=np.int32)
    parent, attach, labels, spare = dev.put(host), dev.put(host), dev.put(host), dev.put(host)
    status = labels + 4 * n
    _density.check(lib.simrank_density_init(spare, parent, attach, n, 1, status, st), "init")
    for S, stride, n_rows, n_cols, row_ids, col_ids in blocks:
        _density.check(lib.simrank_density_union(S, layout, stride, n_rows, n_cols, row_ids, col_ids, edge, deg,
                                                 min_samples - 1, parent, attach, n, status, st), "union")
    _density.check(lib.simrank_density_labels(parent, attach, deg, min_samples - 1, n, labels, status, st), "labels")
    got, par, att, zero = dev.get(labels, host), dev.get(parent, host), dev.get(attach, host), dev.get(spare, host)
    assert got[n] == 0, "status"
    for a in (got, par, att, zero):
        assert a[-1] == GUARD
    assert par[n] == GUARD and att[n] == GUARD and zero[n] == GUARD and not zero[:n].any()
    assert (par[:n] <= np.arange(n)).all() and (par[:n] >= 0).all()     # the invariant, at rest
    assert (((att[:n] >= 0) & (att[:n] < n)) | (att[:n] == _density.NONE)).all()
    return got[:n]


def check(dev, S, layout, stride, n, ids, A, ts, cluster_levels, what, blocks=None):
    """Counts of all levels at once and of the first alone, clusters at ``cluster_levels`` for every min_samples, each
    run twice: all equal the reference and each other.  -> the counts."""
    ids_dev = None if ids is None else dev.put(np.asarray(ids, dtype=np.int32))
    graphs = [DR.block_graph(A, ids, n, t) for t in ts]
    want = np.array([W.sum(axis=1) for W in graphs], dtype=np.int64).reshape(len(ts), n)
    got, deg, edges = run_degrees(dev, S, layout, stride, n, ids_dev, ts)
    assert np.array_equal(got, want), what
    assert np.array_equal(run_degrees(dev, S, layout, stride, n, ids_dev, ts)[0], got), what
    assert np.array_equal(run_degrees(dev, S, layout, stride, n, ids_dev, ts[:1])[0], got[:1]), what
    blocks = blocks or [(S, stride, n, n, ids_dev, ids_dev)]
    for l in cluster_levels:
        for m in MIN_SAMPLES:
            _, core, _, root = DR.dbscan_of_graph(graphs[l], m)
            args = (dev, blocks, layout, n, edges + l * itemsize(layout), deg + 4 * l * n, m)
            roots = run_clusters(*args)
            assert np.array_equal(roots, root), (what, ts[l], m)
            assert np.array_equal(got[l] >= m - 1, core), (what, ts[l], m)
            assert np.array_equal(run_clusters(*args), roots), (what, ts[l], m)
    return got


def levels_of(A):
    """8 thresholds taken from the block's own values, not in order: each passes some entries and fails others."""
    v = np.unique(A[~np.isnan(A)])
    q = lambda f: float(v[min(v.size - 1, int(f * v.size))])
    return [q(0.97), q(0.5), float(v[-1]), 0.0 if v[0] < 0 < v[-1] else q(0.4), q(0.99), q(0.2), q(0.9), q(0.7)]


def id_cases(n, rng):
    """NULL (positions), and a permutation of the nodes in which a few positions are padding instead (ids out of range)."""
    perm = rng.permutation(n).astype(np.int32)
    if n > 4:
        perm[[1, n // 2, n - 1]] = [-7, n, 2 ** 31 - 1]
    return [None, perm]


# ---- 1. the reference, on synthetic blocks ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_the_entries_equal_the_reference(dev, layout, n):
    splits = 0
    for i, (tag, stride, base) in enumerate(B.variants(layout, n, n)):
        blk = B.make_block(layout, n, n, stride, 90 + i, kind=("dyadic", "wide")[i % 2])
        S = dev.put(blk.raw, base)
        ts = levels_of(blk.A)
        for ids in id_cases(n, np.random.default_rng([i, layout, n])):
            got = check(dev, S, layout, stride, n, ids, blk.A, ts, (0, 4), (layout, n, tag, ids is None))
            splits += sum(1 for g in got if 0 < g.sum() < n * (n - 1))
        dev.release()
    assert n < 3 or splits >= 8                                           # the levels do split the block


# ---- 2. planted cases ------------------------------------------------------------------------------------------------------
def put(dev, layout, A):
    n = len(A)
    _, stride, base = B.variants(layout, n, n)[0]
    return dev.put(B.encode(layout, A, stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base), stride


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_one_direction_below_the_diagonal_and_both_directions_across_tiles(dev, layout):
    n = 130
    A = np.full((n, n), -1.0)
    A[5, 2] = 1.0                                             # S[5][2] passes while S[2][5] does not: 2 and 5 are neighbours
    A[3, 100] = A[100, 3] = 1.0                               # tiles (0, 1) and (1, 0): ONE neighbour each
    A[70, 129], A[129, 70] = 1.0, 0.5                         # tiles (1, 2) and (2, 1), the ragged last tile
    A[64, 63] = 0.5                                           # next to the corner of two diagonal tiles
    S, stride = put(dev, layout, A)
    got = check(dev, S, layout, stride, n, None, A, [0.5, 1.0, 1.25], (0, 1), layout)
    want = np.zeros((3, n), dtype=np.int64)
    want[0, [2, 5, 3, 100, 70, 129, 63, 64]] = 1
    want[1, [2, 5, 3, 100, 70, 129]] = 1
    assert np.array_equal(got, want)


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_nan_and_negative_zero_entries(dev, layout):
    """Negative values with a few NaN, -0.0, +0.0 and positive entries: at 0.0 and at -0.0 exactly the zeros of both signs
    and the positive entries pass; NaN passes nothing at any level."""
    n = 129
    _, stride, base = B.variants(layout, n, n)[0]
    rng = np.random.default_rng(layout)
    A = -(rng.integers(1, 1000, size=(n, n)) * 2.0 ** -10)
    stored = B.encode(layout, A, stride, B.SENTINEL[(layout, "dyadic")])
    at = B.offsets(layout, n, n, stride)
    rr, cc = rng.integers(0, n, size=320), rng.integers(0, n, size=320)
    for lo, hi, v in ((0, 120, np.nan), (120, 200, -0.0), (200, 260, 0.0), (260, 320, 0.25)):
        A[rr[lo:hi], cc[lo:hi]] = v
        stored[at[rr[lo:hi], cc[lo:hi]]] = v if np.isnan(v) else B.store(layout, v)
    assert np.array_equal(B.bits(B.decode(layout, stored, n, n, stride)), B.bits(A))
    S = dev.put(stored.tobytes(), base)
    ts = [0.0, -0.0, 0.25, 2.0 ** -10, -2.0 ** -10, -0.5, -2.0, 0.5]
    got = check(dev, S, layout, stride, n, None, A, ts, (0, 1, 2), layout)
    assert np.array_equal(got[0], got[1]) and 0 < got[2].sum() < got[0].sum() < got[4].sum() and not got[7].any()
    assert np.array_equal(got[6], DR.degrees(A, [-2.0])[0])               # below every value: only NaN fails


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_an_all_ones_block_and_a_block_where_nothing_passes(dev, layout):
    """257 x 257 ones: every node has 256 neighbours, everything is core and one cluster, and every lane meets at one
    root.  Above 1 nothing passes: all noise, or all singletons at min_samples = 1."""
    n = 257
    S, stride = put(dev, layout, np.ones((n, n)))
    ts = [1.0, 0.5, 0.0, -1.0, 1.0, 0.25, 0.125, 1.5]
    got, deg, edges = run_degrees(dev, S, layout, stride, n, None, ts)
    assert (got[:7] == n - 1).all() and not got[7].any()
    block = [(S, stride, n, n, None, None)]
    for m in (1, 5, n, n + 1):
        for _ in range(2):
            roots = run_clusters(dev, block, layout, n, edges, deg, m)
            assert np.array_equal(roots, np.full(n, -1 if m == n + 1 else 0)), m
    top = (edges + 7 * itemsize(layout), deg + 4 * 7 * n)
    assert np.array_equal(run_clusters(dev, block, layout, n, *top, 1), np.arange(n))
    assert np.array_equal(run_clusters(dev, block, layout, n, *top, 2), np.full(n, -1))


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_the_union_sweep_over_two_column_blocks(dev, layout):
    """Two column blocks of one matrix (a ``LocalWorld``'s ranks) accumulated into one forest and one ``attach`` array:
    the whole matrix's clusters, which neither block gives alone."""
    rng = np.random.default_rng(3)
    n = 96
    A = rng.integers(-500, 500, size=(n, n)) * 2.0 ** -8
    ts = [1.9, 1.85]                                          # 13 and 26 of 1000 values pass: 2.5 and 5 neighbours a node
    S, stride = put(dev, layout, A)
    blocks = []
    for lo, hi in ((0, 64), (64, 96)):
        part = np.ascontiguousarray(A[:, lo:hi])
        _, pstride, base = B.variants(layout, n, hi - lo)[0]
        P = dev.put(B.encode(layout, part, pstride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
        blocks.append((P, pstride, n, hi - lo, None, dev.put(np.arange(lo, hi, dtype=np.int32))))
    check(dev, S, layout, stride, n, None, A, ts, (0, 1), ("two blocks", layout), blocks=blocks)
    # the condition that makes this a test: at some level the whole has clusters, border nodes and noise, and one block
    # alone gives other labels
    _, deg, edges = run_degrees(dev, S, layout, stride, n, None, ts)
    seen = 0
    for l, t in enumerate(ts):
        for m in (3, 5):
            cluster, core, _, root = DR.dbscan(A, t, m)
            alone = run_clusters(dev, blocks[:1], layout, n, edges + l * itemsize(layout), deg + 4 * l * n, m)
            seen += min(DR.counts(cluster, core)) >= 1 and DR.counts(cluster, core)[0] >= 2 and not np.array_equal(alone, root)
    assert seen >= 1
