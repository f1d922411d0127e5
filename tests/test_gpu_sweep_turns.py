"""The shared sweep of the companion libraries (companion.h: ``plan_launch``, ``WALK_GEOMETRY``) where a wave takes a SECOND
turn: ``select``, ``profile``, ``cluster``, ``linkage``, ``density`` (union) and ``hdbscan`` (clamped pick) at their C
interface on tall blocks of tests/blocks.make_long.

The grid is capped at 2 048 workgroups of four waves and a wave walks ``r0 += nwaves * R``: a row-major wave takes one row
(a second turn begins at row 8 192), a panel wave eight (at row 65 536).  No other kernel-level test has more than 257
rows, so the state that must survive or start afresh at a turn (the row's id, the cached last threshold of ``profile``'s
count, a row's running best in ``linkage``'s pick, the workgroup's 32-bit bins) runs here only.  Row counts: 8 197 (a
second turn of five live waves) and 24 577 (four turns, the last of one row) in the row-major layouts; 65 536 (exactly at
the cap: one turn) and 65 545 (a second turn of one full wave and one wave with a single live row) in the panel layouts.
40 columns: a ragged second f32 panel, a ragged binary16 panel, a row-major row that ends on the scalar tail.  Strides
and bases are those of ``blocks.variants``.

References are those of the per-library tests, on the whole tall block.  The four graph libraries cannot have a dense
reference at these row counts; their contract "an id outside the nodes is padding" gives a small one: about 150 rows,
among them the first and the last of every turn, are nodes of a graph of 200, every other row has an id out of range and
holds values above everything in range, so that a row read under a stale or wrong id would win every pick and join every
component.  Every library is also handed the block as two row bands, rows [0, 8 192) and the rest, and must leave what
the single call leaves."""
import ctypes as C

import numpy as np
import pytest

from simrank_amd import _profile, _select
from tests import blocks as B
from tests import cluster_ref as CR
from tests import density_ref as DR
from tests import hdbscan_ref as HR
from tests import linkage_ref as LR
from tests import profile_ref as PR
from tests import test_gpu_hdbscan as H
from tests import test_gpu_linkage as K
from tests.test_gpu_cluster import check_levels, levels_of
from tests.test_gpu_companion_blocks import Dev, out_of, run_select, same_bits
from tests.test_gpu_density import run_clusters
from tests.test_gpu_cluster import edges_for
from tests.test_gpu_profile import device_sweep, interval_counts, thresholds_of
from tests.test_gpu_profile import id_cases as profile_ids

pytestmark = pytest.mark.gpu

MAX_GRID, WAVES = 2048, 4                         # kSweepMaxGrid, kSweepThreads / 64 (tests/test_sweep_caps_cpu.py reads them)
N_COLS = 40
BAND = 8192                                       # the two row bands of the accumulation checks: [0, BAND) and the rest
N_NODES = 200
ABOVE = {B.PANEL_F32: 100.0, B.ROWMAJOR_F32: 100.0, B.PANEL_F16: 2.5, B.ROWMAJOR_F64: 100.0}    # above every value, below the sentinel


def turn_rows(layout):
    """Rows one turn of the whole grid takes: a panel wave takes eight rows, a row-major wave one."""
    return MAX_GRID * WAVES * (8 if layout in B.PANEL else 1)


ROWS = {layout: ((65536, 65545) if layout in B.PANEL else (8197, 24577)) for layout in B.LAYOUTS}
CASES = [(layout, n_rows) for layout in B.LAYOUTS for n_rows in ROWS[layout]]
IDS = ["layout%d-%d" % c for c in CASES]
SELECT_CASES = [c for c in CASES if c[0] != B.ROWMAJOR_F64]


def turns_of(layout, n_rows):
    step = turn_rows(layout)
    return [(lo, min(lo + step, n_rows)) for lo in range(0, n_rows, step)]


def ends_of(turns):
    """The first and the last row of every turn."""
    return sorted({r for lo, hi in turns for r in (lo, hi - 1)})


def band_of(S, layout, stride, lo):
    """The address of the block that starts at row ``lo`` of the block at S (same stride)."""
    item = np.dtype(B.STORED[layout]).itemsize
    return S + lo * (B.PANEL[layout] if layout in B.PANEL else stride) * item


@pytest.fixture(scope="module")
def device():
    d = Dev()
    yield d
    d.close()


@pytest.fixture
def dev(device):
    yield device
    device.release()


def test_the_row_counts_lie_past_the_cap():
    for layout, n_rows in CASES:
        turns = turns_of(layout, n_rows)
        assert len(turns) == -(-n_rows // turn_rows(layout))
        assert len(turns) >= 2 or n_rows == turn_rows(layout), (layout, n_rows)
    assert [len(turns_of(B.ROWMAJOR_F32, r)) for r in ROWS[B.ROWMAJOR_F32]] == [2, 4]
    assert [len(turns_of(B.PANEL_F16, r)) for r in ROWS[B.PANEL_F16]] == [1, 2]
    assert turns_of(B.ROWMAJOR_F64, 24577)[-1] == (24576, 24577) and turns_of(B.PANEL_F32, 65545)[-1] == (65536, 65545)


# ---- select ------------------------------------------------------------------------------------------------------------------
def own_columns(A, turns, rng, value):
    """(row_ids, col_ids): the rows' ids a permutation, the columns' the ids of 40 rows, the first and the last row of every
    turn among them; A[r][c] = ``value`` (a hit, or an entry of its own) where row r and column c are one node, so that in
    every turn the id of the row decides something, and in the column after it, which stays a hit under every id."""
    n_rows, n_cols = A.shape
    row_ids = rng.permutation(n_rows).astype(np.int32)
    ends = ends_of(turns)[:n_cols]
    rest = rng.permutation(np.setdiff1d(np.arange(n_rows), ends))[:n_cols - len(ends)]
    rows = rng.permutation(np.concatenate([ends, rest]).astype(np.int64))
    A[rows, np.arange(n_cols)] = value
    A[rows, (np.arange(n_cols) + 1) % n_cols] = value
    return row_ids, row_ids[rows].copy()


@pytest.mark.parametrize("layout,n_rows", SELECT_CASES, ids=["layout%d-%d" % c for c in SELECT_CASES])
def test_select_count_offsets_emit(dev, layout, n_rows):
    lib = _select.load()
    turns = turns_of(layout, n_rows)
    for i, (tag, stride, base) in enumerate(B.variants(layout, n_rows, N_COLS)):
        rng = np.random.default_rng([layout, n_rows, i, 1])
        A = B.make_long(layout, n_rows, N_COLS, stride, 30 + i).A.copy()
        pos = np.sort(A[A > 0].astype(np.float32))
        t32 = float(pos[(98 * pos.size) // 100])                            # about one hit in a hundred entries
        row_ids, col_ids = own_columns(A, turns, rng, float(pos[-1]))
        blk = B.Block(layout, A, stride, B.SENTINEL[(layout, "dyadic")], np.argwhere(A == 0), np.zeros((0, 3), dtype=np.int64), {})
        B.check_long(blk)
        S = dev.put(blk.raw, base)
        own = (row_ids[:, None] == col_ids[None, :]) & (A.astype(np.float32) >= np.float32(t32))
        for ids in ((None, None), (row_ids, col_ids)):
            what = (layout, n_rows, tag, ids[0] is None)
            counts = run_select(dev, lib, blk, S, layout, ids[0], ids[1], t32, what)
            for lo, hi in turns:                                          # hits in the rows of every turn, its ends included
                assert counts[lo:hi].sum() > 0 and (hi - lo < 64 or (counts[lo:hi] == 0).any()), (what, lo, hi)
                assert own[lo].any() and own[hi - 1].any() and A[lo].max() >= t32 and A[hi - 1].max() >= t32
            if ids[0] is not None:
                plain = (A.astype(np.float32) >= np.float32(t32)).sum(axis=1)
                assert np.array_equal(plain - counts, own.sum(axis=1))    # the row's own column is the one hit left out
        # two row bands into one array of counts
        if n_rows > BAND:
            cnt, hc = out_of(dev, n_rows + 1, np.int32, -9)
            rid, cid = dev.put(row_ids), dev.put(col_ids)
            for lo, hi in ((0, BAND), (BAND, n_rows)):
                _select.check(lib.simrank_select_count(band_of(S, layout, stride, lo), layout, stride, hi - lo, N_COLS, rid + 4 * lo,
                                                       cid, C.c_float(t32), cnt + 4 * lo, dev.ops.stream), "count")
            hc[:n_rows] = counts
            same_bits(dev.get(cnt, hc), hc, ("two bands", layout, n_rows, tag))
        dev.release()


# ---- profile -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,n_rows", CASES, ids=IDS)
def test_profile_count_and_digits(dev, layout, n_rows):
    lib, st = _profile.load(), dev.ops.stream
    turns = turns_of(layout, n_rows)
    for i, (tag, stride, base) in enumerate(B.variants(layout, n_rows, N_COLS)):
        rng = np.random.default_rng([layout, n_rows, i, 2])
        A = B.make_long(layout, n_rows, N_COLS, stride, 50 + i).A.copy()
        perm, perm_cols = own_columns(A, turns, rng, float(A.max()))
        blk = B.Block(layout, A, stride, B.SENTINEL[(layout, "dyadic")], np.argwhere(A == 0), np.zeros((0, 3), dtype=np.int64), {})
        B.check_long(blk)
        S = dev.put(blk.raw, base)
        ts = thresholds_of(A, rng)
        order = np.argsort(ts, kind="stable")
        edges = ts[order] if layout == B.ROWMAJOR_F64 else _profile.edges_f32(ts[order])
        edges_dev = dev.put(edges)
        cases = profile_ids(n_rows, N_COLS, rng) + [(perm, perm_cols, perm[:, None] == perm_cols[None, :])]
        for j, (row_ids, col_ids, skip) in enumerate(cases if i == 0 else cases[1:]):
            what = (layout, n_rows, tag, j)
            for lo, hi in turns:                                          # distinct values, so distinct digits, in every turn
                v = A[lo:hi][~skip[lo:hi]]
                assert np.unique(v).size >= min(30, v.size // 2), (what, lo)
                assert row_ids is None or skip[hi - 1].any()                # and an entry the row's id leaves out
            rid, cid = None if row_ids is None else dev.put(row_ids), None if col_ids is None else dev.put(col_ids)
            v = A[~skip]
            ivals = interval_counts(v, edges.astype(np.float64))
            host = np.zeros(ts.size + 2, dtype=np.uint64)
            host[-1] = 77
            counts = dev.put(host)
            _profile.check(lib.simrank_profile_count(S, layout, stride, n_rows, N_COLS, rid, cid, edges_dev, ts.size, counts, st),
                           "count")
            got = dev.get(counts, host)
            assert got[-1] == 77 and np.array_equal(got[:-1], ivals), what
            at_least = np.empty(ts.size, dtype=np.int64)
            at_least[order] = np.cumsum(got[:-1][::-1].astype(np.int64))[::-1][1:]
            assert np.array_equal(at_least, PR.count_pairs(A, ts, skip)), what
            assert int(got[:-1].sum()) == v.size                           # every entry once: no padding
            if n_rows > BAND and row_ids is not None:                       # two row bands into one set of counters
                counts = dev.put(host)                                      # (NULL ids are positions: a band's rows start at 0)
                for lo, hi in ((0, BAND), (BAND, n_rows)):
                    _profile.check(lib.simrank_profile_count(band_of(S, layout, stride, lo), layout, stride, hi - lo, N_COLS,
                                                             rid + 4 * lo, cid, edges_dev, ts.size, counts, st), "count")
                assert np.array_equal(dev.get(counts, host), got), (what, "two bands")
            if j != 1:
                continue
            # the digit sweeps with a prefix and the smallest key above it, driven by the host half of the select
            for m in (1, 100001):
                sweep, calls = device_sweep(dev, (S, layout, stride, n_rows, N_COLS, rid, cid), layout)
                assert _profile.radix_select(sweep, _profile.key_bits(layout), m) == PR.threshold_for(A, m, skip), (what, m)
                assert len(calls) >= 2
        dev.release()


# ---- the four graph libraries ------------------------------------------------------------------------------------------------
def node_block(layout, n_rows, stride, seed):
    """-> (Block, row_ids, col_ids, M float64 [200, 200], the live rows): about 150 rows of the tall block, the first and the
    last of every turn and two more of every turn among them, are distinct nodes of 0 .. 199; the columns are 40 distinct
    nodes; every other row has an id out of range (-7, n, 2^31 - 1) and holds ``ABOVE`` everywhere.  M is the node
    matrix: M[row node][column node] = the entry, NaN where no entry is."""
    rng = np.random.default_rng([seed, layout, n_rows, 3])
    A = B.make_long(layout, n_rows, N_COLS, stride, seed).A.copy()
    turns = turns_of(layout, n_rows)
    live = set(ends_of(turns))
    for lo, hi in turns:
        live |= set(rng.permutation(np.arange(lo + 1, max(lo + 1, hi - 1)))[:2].tolist())
    rest = np.setdiff1d(np.arange(n_rows), sorted(live))
    live = np.array(sorted(live | set(rng.permutation(rest)[:150 - len(live)].tolist())), dtype=np.int64)
    assert 140 <= live.size <= 160
    row_ids = np.array([-7, N_NODES, 2 ** 31 - 1], dtype=np.int32)[rng.integers(0, 3, size=n_rows)]
    row_ids[live] = rng.permutation(N_NODES)[:live.size]
    col_ids = rng.permutation(N_NODES)[:N_COLS].astype(np.int32)
    dead = np.ones(n_rows, dtype=bool)
    dead[live] = False
    A[dead] = ABOVE[layout]
    assert np.abs(A[live]).max() < ABOVE[layout] < B.SENTINEL[(layout, "dyadic")]
    M = np.full((N_NODES, N_NODES), np.nan)
    M[np.ix_(row_ids[live], col_ids)] = A[live]
    blk = B.Block(layout, A, stride, B.SENTINEL[(layout, "dyadic")], np.argwhere(A == 0), np.zeros((0, 3), dtype=np.int64), {})
    B.check_long(blk)
    for lo, hi in turns:                                                  # every turn holds nodes, its ends among them
        assert not dead[lo] and not dead[hi - 1] and (~dead[lo:hi]).sum() >= min(3, hi - lo)
    assert np.intersect1d(row_ids[live], col_ids).size >= 5                # entries between a node and itself: no edges
    return blk, row_ids, col_ids, M, live


def blocks_of(dev, blk, base, row_ids, col_ids):
    """(the one block, the same rows as two bands) as the tuples the per-library helpers take."""
    layout, stride, n_rows = blk.layout, blk.stride, blk.n_rows
    S, rid, cid = dev.put(blk.raw, base), dev.put(row_ids), dev.put(col_ids)
    whole = [(S, stride, n_rows, N_COLS, rid, cid)]
    if n_rows <= BAND:
        return whole, None
    return whole, [(S, stride, BAND, N_COLS, rid, cid),
                   (band_of(S, layout, stride, BAND), stride, n_rows - BAND, N_COLS, rid + 4 * BAND, cid)]


def variants_of(layout, n_rows):
    return list(enumerate(B.variants(layout, n_rows, N_COLS)))


@pytest.mark.parametrize("layout,n_rows", CASES, ids=IDS)
def test_cluster_union(dev, layout, n_rows):
    split = 0
    for i, (tag, stride, base) in variants_of(layout, n_rows):
        blk, row_ids, col_ids, M, live = node_block(layout, n_rows, stride, 110 + i)
        whole, bands = blocks_of(dev, blk, base, row_ids, col_ids)
        ts = levels_of(blk.A[live])
        edges = lambda t: np.argwhere(np.triu(CR.graph(M, t)))
        got = check_levels(dev, whole, N_NODES, layout, ts, edges, (layout, n_rows, tag))
        assert np.array_equal(got[7], np.arange(N_NODES))                   # above every value in range: nothing joins
        split += sum(1 for g in got if 1 < np.unique(g).size < N_NODES)
        # the later turns' rows decide: without them the components are others
        first = live[live < turn_rows(layout)]
        if first.size < live.size:
            M1 = np.full_like(M, np.nan)
            M1[np.ix_(row_ids[first], col_ids)] = blk.A[first]
            assert any(not np.array_equal(CR.components(M1, [t])[0], CR.components(M, [t])[0]) for t in ts)
        if bands:
            assert np.array_equal(check_levels(dev, bands, N_NODES, layout, ts, edges, (layout, n_rows, tag, "two bands")), got)
        dev.release()
    assert split >= 2


@pytest.mark.parametrize("layout,n_rows", CASES, ids=IDS)
def test_linkage_pick(dev, layout, n_rows):
    for i, (tag, stride, base) in variants_of(layout, n_rows):
        blk, row_ids, col_ids, M, live = node_block(layout, n_rows, stride, 120 + i)
        whole, bands = blocks_of(dev, blk, base, row_ids, col_ids)
        want = LR.linkage(M)
        heights, widest = LR.stats(N_NODES, want)
        assert heights >= 3 and len(want[0]) >= N_NODES // 2
        K.check_forest(dev, whole, N_NODES, layout, want, (layout, n_rows, tag))
        if bands:
            K.check_forest(dev, bands, N_NODES, layout, want, (layout, n_rows, tag, "two bands"))
        dev.release()


@pytest.mark.parametrize("layout,n_rows", CASES, ids=IDS)
def test_density_union(dev, layout, n_rows):
    seen = 0
    for i, (tag, stride, base) in variants_of(layout, n_rows):
        blk, row_ids, col_ids, M, live = node_block(layout, n_rows, stride, 130 + i)
        whole, bands = blocks_of(dev, blk, base, row_ids, col_ids)
        v = np.unique(blk.A[live])
        for t in (float(v[int(0.97 * v.size)]), float(v[int(0.9 * v.size)])):
            W = DR.graph(M, t)
            edge = dev.put(edges_for(layout, [t]))
            deg = dev.put(W.sum(axis=1).astype(np.int32))
            for m in (1, 3, 5):
                cluster, core, _, root = DR.dbscan_of_graph(W, m)
                what = (layout, n_rows, tag, t, m)
                roots = run_clusters(dev, whole, layout, N_NODES, edge, deg, m)
                assert np.array_equal(roots, root), what
                assert np.array_equal(run_clusters(dev, whole, layout, N_NODES, edge, deg, m), roots), what
                if bands:
                    assert np.array_equal(run_clusters(dev, bands, layout, N_NODES, edge, deg, m), roots), (what, "two bands")
                seen += m > 1 and int(cluster.max()) >= 0 and (cluster < 0).any()
        dev.release()
    assert seen >= 1                                                      # clusters and noise at some level


@pytest.mark.parametrize("layout,n_rows", CASES, ids=IDS)
def test_hdbscan_clamped_pick(dev, layout, n_rows):
    clamped = 0
    for i, (tag, stride, base) in variants_of(layout, n_rows):
        blk, row_ids, col_ids, M, live = node_block(layout, n_rows, stride, 140 + i)
        whole, bands = blocks_of(dev, blk, base, row_ids, col_ids)
        m = 3
        core, want = HR.core(M, m), HR.linkage(M, m)
        core_dev = dev.put(core.astype(H.cmp_type(layout)))
        got = K.rows_of(N_NODES, *H.forest(dev, whole, N_NODES, layout, core_dev))
        assert K.same(got, want), (layout, n_rows, tag)
        assert K.same(K.rows_of(N_NODES, *H.forest(dev, whole, N_NODES, layout, core_dev)), got)      # a second run
        if bands:
            assert K.same(K.rows_of(N_NODES, *H.forest(dev, bands, N_NODES, layout, core_dev)), want), (layout, n_rows, tag, "bands")
        clamped += not K.same(want, LR.linkage(M))
        dev.release()
    assert clamped >= 1                                                   # the clamp does change the table
