"""libsimrank_hdbscan.so on a real MI355X, kernel level, on synthetic blocks (tests/blocks.py, no fit): ``A[r][c] !=
A[c][r]``, both signs, and padding that holds a finite sentinel above every value, so a wrong transposed read or a read
of padding becomes a wrong core similarity.

The select gives ``hdbscan_ref``'s core similarities bit for bit, as float64 and in the compare type, in all four
layouts, with the strides and bases of ``blocks.variants``, with ``ids = NULL`` and with a permutation that has a few ids
out of range, at n on both sides of the 64 x 64 tile (one tile, a diagonal tile plus pairs, a ragged last tile), at the
ranks 1, 2, 4, n - 1 and n.  Guard words after every array survive, the counters are left at 0 and a second run gives
the same bits; the entries driven one by one give what ``simrank_hdbscan_select`` gives.  Planted cases: the k-th value
only below the diagonal; the k-th and (k + 1)-th values one unit in the last place apart and a sign bit apart; negative
values with zeros of both signs and NaN in one and in both directions; an all-equal block.

The clamped pick: with ``core = +inf`` its slots are ``simrank_linkage_pick``'s word for word; with the reference's core
similarities the forest through ``simrank_linkage_hook`` / ``_flatten`` and ``_linkage.canonical`` is ``hdbscan_ref``'s
table, also accumulated over two column blocks and under a floor; the status word stays 0."""
import numpy as np
import pytest

from simrank_amd import _hdbscan, _linkage
from tests import blocks as B
from tests import hdbscan_ref as HR
from tests import linkage_ref as LR
from tests.test_gpu_cluster import GUARD, dev, device  # noqa: F401 (fixtures)
from tests.test_gpu_density import id_cases, put
from tests.test_gpu_linkage import GUARD64, floor_ref, rows_of, same

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 127, 129, 200)


def ranks_of(n):
    return sorted({1, 2, 4, max(1, n - 1), n})


def cmp_type(layout):
    return np.float64 if layout == B.ROWMAJOR_F64 else np.float32


def run_select(dev, S, layout, stride, n, ids, rank, stepwise=False):
    """The select on the square block -> (core float64 [n], core in the compare type [n]).  Every array carries a guard
    word that must survive; the counters are 0 afterwards."""
    lib, st = _hdbscan.load(), dev.ops.stream
    ct = cmp_type(layout)
    prefix_h, rem_h = np.full(n + 1, GUARD64, dtype=np.uint64), np.full(n + 1, GUARD, dtype=np.int32)
    hist_h = np.full(_hdbscan.BINS * n + 1, GUARD, dtype=np.int32)
    c64_h = np.full(n + 1, GUARD64, dtype=np.uint64)
    cc_h = np.full(n + 1, GUARD64 if ct == np.float64 else GUARD, dtype=np.uint64 if ct == np.float64 else np.uint32)
    prefix, rem, hist, c64, cc = (dev.put(x) for x in (prefix_h, rem_h, hist_h, c64_h, cc_h))
    if stepwise:
        _hdbscan.check(lib.simrank_hdbscan_select_init(prefix, rem, hist, n, rank, st), "init")
        passes = lib.simrank_hdbscan_select_passes(layout)
        assert passes == _hdbscan.select_passes(layout)
        for p in range(passes):
            _hdbscan.check(lib.simrank_hdbscan_select_count(S, layout, stride, n, ids, p, prefix, hist, st), "count")
            _hdbscan.check(lib.simrank_hdbscan_select_step(layout, p, prefix, rem, hist, n, st), "step")
        _hdbscan.check(lib.simrank_hdbscan_select_finish(layout, prefix, rem, n, c64, cc, st), "finish")
    else:
        _hdbscan.check(lib.simrank_hdbscan_select(S, layout, stride, n, ids, rank, prefix, rem, hist, c64, cc, st), "select")
    got = [dev.get(p, h) for p, h in ((prefix, prefix_h), (rem, rem_h), (hist, hist_h), (c64, c64_h), (cc, cc_h))]
    assert got[0][-1] == GUARD64 and got[1][-1] == GUARD and got[2][-1] == GUARD and got[3][-1] == GUARD64
    assert got[4][-1] == cc_h[-1] and not got[2][:-1].any()
    return got[3][:n].view(np.float64).copy(), got[4][:n].view(ct).copy()


def check(dev, S, layout, stride, n, ids, A, ranks, what):
    """Every rank twice: both outputs equal the reference and each other, bit for bit.  -> {rank: core}."""
    ids_dev = None if ids is None else dev.put(np.asarray(ids, dtype=np.int32))
    out = {}
    for i, rank in enumerate(ranks):
        want = HR.block_core(A, ids, n, rank)
        c64, cc = run_select(dev, S, layout, stride, n, ids_dev, rank)
        assert np.array_equal(B.bits(c64), B.bits(want)), (what, rank, c64, want)
        assert np.array_equal(B.bits(cc.astype(np.float64)), B.bits(want)), (what, rank)
        again = run_select(dev, S, layout, stride, n, ids_dev, rank, stepwise=i == 0)
        assert np.array_equal(B.bits(again[0]), B.bits(c64)) and np.array_equal(B.bits(again[1]), B.bits(cc)), (what, rank)
        out[rank] = c64
    return out


# ---- 1. the select against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_the_select_equals_the_reference(dev, layout, n):
    finite = 0
    for i, (tag, stride, base) in enumerate(B.variants(layout, n, n)):
        blk = B.make_block(layout, n, n, stride, 120 + i, kind=("dyadic", "wide")[i % 2])
        S = dev.put(blk.raw, base)
        for ids in id_cases(n, np.random.default_rng([i, layout, n])):
            got = check(dev, S, layout, stride, n, ids, blk.A, ranks_of(n), (layout, n, tag, ids is None))
            finite += sum(int(np.isfinite(c).sum()) for c in got.values())
            assert np.isneginf(got[n]).all()                              # nobody has n pairs
        dev.release()
    assert n < 2 or finite > 0
    # rank 0 (min_samples = 1): +inf without a sweep
    S, stride = put(dev, layout, np.zeros((n, n)))
    assert np.isposinf(run_select(dev, S, layout, stride, n, None, 0)[0]).all()


# ---- 2. planted cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_the_kth_value_only_below_the_diagonal(dev, layout):
    n = 130
    A = np.full((n, n), -1.0)
    A[5, 2] = 1.0                                             # S[5][2] alone: w(2, 5) = 1
    A[100, 3] = 0.5                                           # tile (1, 0) alone
    A[129, 70], A[70, 129] = 0.25, -0.5                       # tiles (2, 1) and (1, 2), the ragged last tile: the larger
    A[64, 63] = 0.75                                          # next to the corner of two diagonal tiles
    S, stride = put(dev, layout, A)
    got = check(dev, S, layout, stride, n, None, A, [1, 2], layout)
    want = np.full(n, -1.0)
    want[[2, 5]], want[[3, 100]], want[[70, 129]], want[[63, 64]] = 1.0, 0.5, 0.25, 0.75
    assert np.array_equal(got[1], want) and (got[2] == -1.0).all()


def neighbours_in_the_stored_type(layout):
    """(x, the next value above x) as float64, both exactly storable: one unit in the last place of the stored type apart."""
    if layout == B.PANEL_F16:
        h = np.array([1.0], dtype=np.float16)
        return float(h[0]) / B.HALF_SCALE, float(np.nextafter(h, np.float16(2))[0]) / B.HALF_SCALE
    t = B.STORED[layout]
    return 1.0, float(np.nextafter(t(1.0), t(2.0)))


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_values_one_bit_apart(dev, layout):
    """The k-th and the (k + 1)-th value differ only in the LOWEST bit of the stored type (the last pass decides) and only
    in the HIGHEST (the sign: the first pass decides): a wrong pass order or digit shift exchanges them."""
    n = 70
    x, y = neighbours_in_the_stored_type(layout)
    assert x < y
    A = np.full((n, n), -0.75)
    A[0, 1], A[2, 0] = x, y                                   # node 0: y, x, then -0.75
    A[10, 66], A[67, 10] = 0.5, -0.5                          # node 10: 0.5, -0.5 (one sign bit apart), then -0.75
    A[20, 21], A[20, 22], A[23, 20] = y, y, x                 # node 20: y twice, then x: a tie above the k-th
    S, stride = put(dev, layout, A)
    got = check(dev, S, layout, stride, n, None, A, [1, 2, 3, 4], layout)
    assert [got[r][0] for r in (1, 2, 3)] == [y, x, -0.75]
    assert [got[r][10] for r in (1, 2, 3)] == [0.5, -0.5, -0.75]
    assert [got[r][20] for r in (1, 2, 3, 4)] == [y, y, x, -0.75]


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_negative_values_zeros_of_both_signs_and_nan(dev, layout):
    n = 129
    _, stride, base = B.variants(layout, n, n)[0]
    rng = np.random.default_rng(layout)
    A = -(rng.integers(1, 1000, size=(n, n)) * 2.0 ** -10)
    stored = B.encode(layout, A, stride, B.SENTINEL[(layout, "dyadic")])
    at = B.offsets(layout, n, n, stride)
    rr, cc = rng.integers(0, n, size=520), rng.integers(0, n, size=520)
    for lo, hi, v in ((0, 200, np.nan), (200, 330, -0.0), (330, 460, 0.0), (460, 520, 0.25)):
        A[rr[lo:hi], cc[lo:hi]] = v
        stored[at[rr[lo:hi], cc[lo:hi]]] = v if np.isnan(v) else B.store(layout, v)
    # NaN in both directions of a few pairs, and a node with nothing but NaN around it
    for a, b in ((3, 90), (64, 65), (128, 0)):
        A[a, b] = A[b, a] = np.nan
        stored[at[a, b]] = stored[at[b, a]] = np.nan
    A[77, :] = A[:, 77] = np.nan
    stored[at[77, :]] = np.nan
    stored[at[:, 77]] = np.nan
    assert np.array_equal(B.bits(B.decode(layout, stored, n, n, stride)), B.bits(A))
    S = dev.put(stored.tobytes(), base)
    got = check(dev, S, layout, stride, n, None, A, [1, 2, 3, 5, 64, 126, 127, 128], layout)
    allc = np.concatenate(list(got.values()))
    assert not (np.signbit(allc) & (allc == 0)).any() and (allc == 0).any() and (allc == 0.25).any() and (allc < 0).any()
    assert all(np.isneginf(c[77]) for c in got.values())                  # no pair exists
    assert np.isfinite(got[126]).any() and np.isneginf(got[128]).all()


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_an_all_equal_block(dev, layout):
    n = 257
    S, stride = put(dev, layout, np.ones((n, n)))
    for rank, want in ((1, 1.0), (5, 1.0), (n - 1, 1.0), (n, -np.inf)):
        c64, cc = run_select(dev, S, layout, stride, n, None, rank)
        assert (c64 == want).all() and (cc == want).all(), rank


# ---- 3. the clamped pick -----------------------------------------------------------------------------------------------------
def pick_with(lib_pick, core):
    """One pick call on a block tuple, by ``simrank_linkage_pick`` (core None) or ``simrank_hdbscan_pick``."""
    def call(block, layout, fl, phase, comp, best, n, status, st):
        S, stride, n_rows, n_cols, row_ids, col_ids = block
        if core is None:
            _linkage.check(lib_pick(S, layout, stride, n_rows, n_cols, row_ids, col_ids, fl, phase, comp, best, n, status, st),
                           "linkage pick")
        else:
            _hdbscan.check(lib_pick(S, layout, stride, n_rows, n_cols, row_ids, col_ids, fl, phase, core, comp, best, n, status,
                                    st), "hdbscan pick")
    return call


def forest(dev, blocks, n, layout, core, floor=None, first_slots=False):
    """test_gpu_linkage.forest with the pick replaced: ``core`` None runs ``simrank_linkage_pick``, a device array in the
    compare type runs ``simrank_hdbscan_pick`` -> (hook_other, hook_value) or, with ``first_slots``, the slots after the
    picks of the first round."""
    L, H, st = _linkage.load(), _hdbscan.load(), dev.ops.stream
    pick = pick_with(L.simrank_linkage_pick if core is None else H.simrank_hdbscan_pick, core)
    wide = layout == B.ROWMAJOR_F64
    comp_h, other_h = np.full(n + 1, GUARD, dtype=np.int32), np.full(n + 1, GUARD, dtype=np.int32)
    best_h, value_h = np.full(2 * n + 1, GUARD64, dtype=np.uint64), np.full(n + 1, GUARD64, dtype=np.uint64)
    state_h = np.full(3, GUARD, dtype=np.int32)
    comp, other, best, value, state = (dev.put(x) for x in (comp_h, other_h, best_h, value_h, state_h))
    status = state + 4
    _linkage.check(L.simrank_linkage_init(comp, best, other, value, n, state, status, st), "init")
    fl = floor_ref(layout, floor)
    rounds = total = 0
    while True:
        rounds += 1
        assert rounds <= _linkage.max_rounds(n), (rounds, n)
        for phase in range(2 if wide else 1):
            for block in blocks:
                pick(block, layout, fl, phase, comp, best, n, status, st)
        if first_slots:
            words, slots = dev.get(state, state_h), dev.get(best, best_h)
            assert words[1] == 0 and slots[-1] == GUARD64
            return slots[:-1]
        _linkage.check(L.simrank_linkage_hook(best, 64 if wide else 32, comp, other, value, n, state, status, st), "hook")
        _linkage.check(L.simrank_linkage_flatten(comp, best, n, status, st), "flatten")
        words = dev.get(state, state_h)
        assert words[1] == 0 and words[2] == GUARD, words                  # the status word stays 0
        if words[0] == total or words[0] == n - 1:
            total = int(words[0])
            break
        total = int(words[0])
    got_other, got_best, got_value = dev.get(other, other_h), dev.get(best, best_h), dev.get(value, value_h)
    assert got_other[-1] == GUARD and got_best[-1] == GUARD64 and got_value[-1] == GUARD64 and not got_best[:-1].any()
    assert int((got_other[:n] >= 0).sum()) == total
    return got_other[:n].copy(), got_value[:n].view(np.float64).copy()


def node_matrix(A, ids, n):
    """float64 [n, n] over the node ids: the square block A when position p is node ids[p]; NaN where no position is."""
    pid = np.arange(len(A)) if ids is None else np.asarray(ids, dtype=np.int64)
    ok = np.flatnonzero((pid >= 0) & (pid < n))
    S = np.full((n, n), np.nan)
    S[np.ix_(pid[ok], pid[ok])] = A[np.ix_(ok, ok)]
    return S


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_with_an_infinite_core_the_slots_are_the_plain_picks(dev, layout):
    for i, (n_rows, n_cols) in enumerate(((9, 65), (129, 257), (64, 700))):
        for tag, stride, base in B.variants(layout, n_rows, n_cols):
            blk = B.make_block(layout, n_rows, n_cols, stride, 140 + i)
            S = dev.put(blk.raw, base)
            n = max(n_rows, n_cols)
            inf = dev.put(np.full(n, np.inf, dtype=cmp_type(layout)))
            block = [(S, stride, n_rows, n_cols, None, None)]
            for floor in (None, 0.0):
                plain = forest(dev, block, n, layout, None, floor, first_slots=True)
                clamped = forest(dev, block, n, layout, inf, floor, first_slots=True)
                assert plain.any() and np.array_equal(plain, clamped), (layout, n_rows, n_cols, tag, floor)
        dev.release()


@pytest.mark.parametrize("n", (65, 129, 200))
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_the_forest_of_the_clamped_picks_is_the_reference_table(dev, layout, n):
    clamped = 0
    for i, (tag, stride, base) in enumerate(B.variants(layout, n, n)):
        blk = B.make_block(layout, n, n, stride, 150 + i, kind=("dyadic", "wide")[i % 2])
        S = dev.put(blk.raw, base)
        for ids in id_cases(n, np.random.default_rng([i, layout, n, 1])):
            ids_dev = None if ids is None else dev.put(np.asarray(ids, dtype=np.int32))
            M = node_matrix(blk.A, ids, n)
            for m in (2, 5, n // 2):
                core = HR.core(M, m)
                want = HR.linkage(M, m)
                core_dev = dev.put(core.astype(cmp_type(layout)))
                block = [(S, stride, n, n, ids_dev, ids_dev)]
                got = rows_of(n, *forest(dev, block, n, layout, core_dev))
                assert same(got, want), (layout, n, tag, ids is None, m)
                assert same(rows_of(n, *forest(dev, block, n, layout, core_dev)), got)          # a second run
                clamped += not same(want, LR.linkage(M))
                # the binding's own path: select and rounds in one call
                b = dict(ptr=S, layout=layout, stride=stride, rows=n, cols=n, row_ids=ids_dev, col_ids=ids_dev)
                c2, a2, b2, v2, _ = _hdbscan.forest_blocks(dev.ops, b, [b], n, m - 1, None)
                assert np.array_equal(B.bits(c2), B.bits(core)) and same(_linkage.canonical(n, a2, b2, v2), want)
        dev.release()
    assert clamped >= 3                                       # the clamp does change the table


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_the_clamped_picks_over_two_column_blocks_and_under_a_floor(dev, layout):
    rng = np.random.default_rng(3)
    n = 96
    A = rng.integers(-500, 500, size=(n, n)) * 2.0 ** -8
    A[rng.random((n, n)) < 0.6] = -2.0                        # sparse above -2: core similarities that differ
    blocks = []
    for lo, hi in ((0, 64), (64, 96)):
        part = np.ascontiguousarray(A[:, lo:hi])
        _, stride, base = B.variants(layout, n, hi - lo)[0]
        S = dev.put(B.encode(layout, part, stride, B.SENTINEL[(layout, "dyadic")]).tobytes(), base)
        blocks.append((S, stride, n, hi - lo, None, dev.put(np.arange(lo, hi, dtype=np.int32))))
    for m in (3, 8):
        core = HR.core(A, m)
        core_dev = dev.put(core.astype(cmp_type(layout)))
        want = HR.linkage(A, m)
        assert same(rows_of(n, *forest(dev, blocks, n, layout, core_dev)), want), m
        assert not same(rows_of(n, *forest(dev, blocks[:1], n, layout, core_dev)), want)        # one block alone is not it
        hs = np.unique(want[2])
        for floor in (float(hs[hs.size // 2]), float(hs[hs.size // 2] + hs[hs.size // 2 + 1]) / 2):
            under = HR.linkage(A, m, floor)
            assert 0 < len(under[0]) < len(want[0])
            assert same(rows_of(n, *forest(dev, blocks, n, layout, core_dev, floor)), under), (m, floor)
