"""The companion libraries' block-reading entry points past 2^31 and 2^32 elements: the 70 x 1100 block of tests/far.py
in its four far geometries (the offsets of the last rows and panels of a kept model of N = 65536), in ONE arena of
2 x 17.5 GiB whose every other byte is a filler that is finite and above every value.  An index computed in 32 bits reads
the filler (or another row) and the comparison, bit for bit against the NumPy statements of tests/blocks.py,
tests/profile_ref.py, tests/cluster_ref.py and tests/rank_ref.py, fails.  Conventions are those of
tests/test_gpu_companion_blocks.py: outputs pre-filled, over-wide, followed by a guard row; positions outside the block;
queries, sets and lists name rows and columns on each side of every boundary, and the last ones.

Far outputs and bands live in the same arena and are read back at their live parts and margins only:
``simrank_query_rows`` with ld_out = 2^28 (output row 8 starts at 2^31 doubles), the ``simrank_sets_score`` band with
ld = 2^28 read again by ``simrank_sets_topk`` and ``simrank_rank_gather`` / ``_count``, and ``simrank_model_pack`` from a
far source into a far destination.  2^31 still fits 32 UNSIGNED bits, so both far-output tests run again with ld = 2^32
and two rows.  From the main library: ``simrank_handback_f64`` in both forms and ``simrank_permute_layout`` both ways on a PANEL_F32 matrix of n = 1100 with rows_pad = 2^22."""
import ctypes as C
import types

import numpy as np
import pytest

from simrank_amd import _f64, _foldin, _model, _neighbors, _profile, _query, _rank, _select, _sets
from simrank_amd.engine import HipOps
from tests import blocks as B
from tests import cluster_ref as CR
from tests import far as F
from tests import profile_ref as PR
from tests import rank_ref as K
from tests.test_gpu_cluster import check_levels
from tests.test_gpu_cluster import id_cases as cluster_ids
from tests.test_gpu_cluster import levels_of
from tests.test_gpu_companion_blocks import INVALID, PAIRS, Dev, out_of, run_select, same_bits
from tests.test_gpu_profile import device_sweep, interval_counts, thresholds_of
from tests.test_gpu_profile import id_cases as profile_ids

pytestmark = pytest.mark.gpu

KINDS = ("dyadic", "wide")
# A far output or band: (ld in doubles, rows, bytes into the arena at which it starts).
# ld = 2^28, nine rows: row 8 starts at 2^31 doubles.  It starts 2^34 bytes and 1 MiB in, so that row 8 wrapped to -2^31
# doubles is still inside (at 1 MiB) and a guard row 9 fits before the end.
# ld = 2^32, two rows: row 1 starts at 2^32 doubles, which 32 bits of either sign turn into row 0.  (Seventeen rows of
# 2^28 would reach 2^32 as well, but their rows 8 .. 15 wrapped to a negative offset need 16 GiB below the start and
# row 16 needs 32 GiB above it: more than the arena.)  It starts 1 MiB in and has no guard row.
FAR_OUTPUTS = [(1 << 28, 9, (1 << 34) + (1 << 20)), (1 << 32, 2, 1 << 20)]
FAR_IDS = ["ld=2^28", "ld=2^32"]
SHIFT = 1 << 20                                    # a far destination starts this many bytes after the source's base


@pytest.fixture(scope="module")
def device():
    d = Dev()
    yield d
    d.close()


@pytest.fixture(scope="module")
def arena(device):
    free, total = C.c_int64(0), C.c_int64(0)
    _f64.check(_f64.load().simrank_f64_mem_info(C.byref(free), C.byref(total)), "simrank_f64_mem_info")
    if free.value < F.ARENA + F.HEADROOM:
        pytest.skip(f"the device reports {free.value / 2 ** 30:.1f} GiB free, the arena needs {F.ARENA / 2 ** 30:.1f} GiB "
                    f"plus {F.HEADROOM / 2 ** 30:.0f} GiB of headroom")
    a = F.Arena(device.ops)
    yield a
    a.free()
    HipOps.trim_pool(0)


@pytest.fixture
def dev(device):
    yield device
    device.release()


def far_blocks(arena, layout, kinds=KINDS, seed=0, overflow=0):
    """(block, geometry, S, label) over the layout's far geometries and the kinds; the arena holds nothing else."""
    arena.fill(layout)
    for g in F.geometries(layout):
        for kind in kinds:
            blk = F.block(layout, kind, seed, overflow if kind == "wide" else 0)
            S = arena.place(g, blk.A, blk.sentinel)
            yield blk, g, S, (layout, g.tag, kind)
            arena.clear()


def edge_rows(rng, n_q):
    """Row positions: both sides of every boundary, the last row, a row twice, one outside the block."""
    rows = list(F.EDGE_ROWS) + [F.EDGE_ROWS[2], F.N_ROWS] + list(rng.integers(0, F.N_ROWS, size=n_q))
    return np.array(rows[:n_q], dtype=np.int32)


# ---- query -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_query_rows_pairs_topk(dev, arena, layout):
    lib, st = _query.load(), dev.ops.stream
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        A, rng = blk.A, np.random.default_rng(i)
        n_q = 10
        row_pos = edge_rows(rng, n_q)
        rp = dev.put(row_pos)
        cmap = rng.permutation(n_cols).astype(np.int32)
        cmap[n_cols // 2] = n_cols
        for col_pos in (None, cmap):
            ld = n_cols + 3
            out, host = out_of(dev, (n_q + 1, ld), np.float64, 1e300)
            _query.check(lib.simrank_query_rows(S, layout, g.stride, n_rows, n_cols, rp, n_q,
                                                None if col_pos is None else dev.put(col_pos), n_cols, out, ld, st), "rows")
            host[:n_q, :n_cols] = B.ref_rows(A, row_pos, col_pos, n_cols)
            same_bits(dev.get(out, host), host, ("rows", what, col_pos is None))
        # pairs: every edge row with every edge column, and positions outside
        a = np.array([r for r in F.EDGE_ROWS for _ in F.EDGE_COLS] + [n_rows, 3], dtype=np.int32)
        b = np.array([c for _ in F.EDGE_ROWS for c in F.EDGE_COLS] + [5, n_cols], dtype=np.int32)
        out, host = out_of(dev, a.size + 4, np.float64, 1e300)
        _query.check(lib.simrank_query_pairs(S, layout, g.stride, n_rows, n_cols, dev.put(a), dev.put(b), a.size, out, st), "pairs")
        host[:a.size] = B.ref_pairs(A, a, b)
        same_bits(dev.get(out, host), host, ("pairs", what))
        col_ids = (rng.permutation(n_cols + 7)[:n_cols] * 3 + 1).astype(np.int32)
        own = col_ids[(row_pos.astype(np.int64) * 5 + 1) % n_cols].astype(np.int32)
        for ids, row_ids in ((col_ids, own), (None, row_pos)):
            for k in (10, 1024):
                idx, hi = out_of(dev, (n_q + 1, k), np.int32, -9)
                val, hv = out_of(dev, (n_q + 1, k), np.float64, 1e300)
                _query.check(lib.simrank_query_topk(S, layout, g.stride, n_rows, n_cols, rp, dev.put(row_ids), n_q,
                                                    None if ids is None else dev.put(ids), k, idx, val, st), "topk")
                hi[:n_q], hv[:n_q] = B.ref_topk(A, row_pos, row_ids, ids, k)
                same_bits(dev.get(idx, hi), hi, ("topk ids", what, ids is None, k))
                same_bits(dev.get(val, hv), hv, ("topk values", what, ids is None, k))
        dev.release()


def far_rows(arena, far, n_cols, fill):
    """A far output (ld, rows, start) of n_cols doubles per row in the arena, each row over-wide by 3, a guard row after
    the last where the arena has room for one, pre-filled -> (device pointer, host image [rows (+ 1), n_cols + 3])."""
    ld, n, at = far
    guard = at + 8 * (n * ld + n_cols + 3) <= F.ARENA
    out = arena.ptr + at
    host = np.full((n + guard, n_cols + 3), fill, dtype=np.float64)
    for q in range(n + guard):
        arena.write(out + 8 * q * ld, host[q].tobytes())
    return out, host


def read_far_rows(dev, far, out, host):
    got = np.empty_like(host)
    for q in range(host.shape[0]):
        dev.ops.d2h(got[q], out + 8 * q * far[0])
    dev.ops.synchronize()
    return got


def check_far_output(far):
    """The last row starts at 2^31 or 2^32 doubles; its offset wrapped to 32 bits of either sign stays inside the arena."""
    ld, n, at = far
    last = (n - 1) * ld
    assert last in (1 << 31, 1 << 32) and at + 8 * (last + F.N_COLS + 3) <= F.ARENA
    for wrapped in (int(np.int64(last).astype(np.int32)), last & 0xffffffff):
        assert 0 <= at + 8 * wrapped and at + 8 * (wrapped + F.N_COLS + 3) <= F.ARENA


@pytest.mark.parametrize("far", FAR_OUTPUTS, ids=FAR_IDS)
def test_query_rows_into_a_far_output(dev, arena, far):
    """Read back: the rows, three doubles past each, the guard row."""
    lib, st = _query.load(), dev.ops.stream
    layout, n = B.ROWMAJOR_F32, far[1]
    check_far_output(far)
    for blk, g, S, what in far_blocks(arena, layout, kinds=("dyadic",)):
        if g.tag != "aligned":
            continue
        row_pos = np.array((list(F.EDGE_ROWS) + [F.N_ROWS, 5, F.N_ROWS - 1])[-n:], dtype=np.int32)
        assert row_pos.size == n and 0 <= row_pos[n - 1] < F.N_ROWS
        out, host = far_rows(arena, far, F.N_COLS, 1e300)
        _query.check(lib.simrank_query_rows(S, layout, g.stride, F.N_ROWS, F.N_COLS, dev.put(row_pos), n, None, F.N_COLS,
                                            out, far[0], st), "rows")
        host[:n, :F.N_COLS] = B.ref_rows(blk.A, row_pos, None, F.N_COLS)
        same_bits(read_far_rows(dev, far, out, host), host, ("far rows", what))


# ---- select ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [B.PANEL_F32, B.ROWMAJOR_F32, B.PANEL_F16])
def test_select_count_emit(dev, arena, layout):
    lib = _select.load()
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        A, rng = blk.A, np.random.default_rng(100 + i)
        view = types.SimpleNamespace(A=A, stride=g.stride)
        pos = np.sort(A[A > 0].astype(np.float32))
        n_ids = n_cols + 3
        col_ids = rng.permutation(n_ids)[:n_cols].astype(np.int32)
        row_ids = rng.permutation(n_ids)[:n_rows].astype(np.int32)
        row_ids[0] = col_ids[n_cols - 1]
        stored = pos[(3 * pos.size) // 4]
        kept = run_select(dev, lib, view, S, layout, row_ids, col_ids, float(stored), what)
        plain = run_select(dev, lib, view, S, layout, None, None, float(pos[pos.size // 2]), what)
        assert kept.sum() > 0 and plain[list(F.EDGE_ROWS)].min() > 0          # hits in the rows on each side of each boundary
        up = np.nextafter(pos[-1], np.float32(np.inf))
        assert run_select(dev, lib, view, S, layout, row_ids, None, float(up), what).sum() == 0 and up < blk.sentinel
        dev.release()


def test_select_refuses_a_float64_block(dev, arena):
    """What the library does today: select reads no float64 block, far or near; nothing is written."""
    lib, layout = _select.load(), B.ROWMAJOR_F64
    for blk, g, S, what in far_blocks(arena, layout, kinds=("dyadic",)):
        cnt, hc = out_of(dev, F.N_ROWS + 1, np.int32, -9)
        rc = lib.simrank_select_count(S, layout, g.stride, F.N_ROWS, F.N_COLS, None, None, C.c_float(0.5), cnt, dev.ops.stream)
        assert rc == INVALID and b"layout" in lib.simrank_select_last_error(), what
        offs = dev.put(np.zeros(F.N_ROWS + 1, dtype=np.int64))
        ids, hi = out_of(dev, 8, np.int32, -9)
        vals, hv = out_of(dev, 8, np.float32, 9e30)
        rc = lib.simrank_select_emit(S, layout, g.stride, F.N_ROWS, F.N_COLS, None, None, C.c_float(0.5), offs, 8, ids, vals,
                                     dev.ops.stream)
        assert rc == INVALID, what
        same_bits(dev.get(cnt, hc), hc, what)
        same_bits(dev.get(ids, hi), hi, what)
        dev.release()


# ---- fold-in -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_foldin_gather(dev, arena, layout):
    lib, st = _foldin.load(), dev.ops.stream
    t_dtype = B.acc_type(layout)
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout, kinds=("dyadic",))):
        rng = np.random.default_rng(200 + i)
        n_tile = (32, 5, 31)[i % 3]
        ptr, pos, w = B.gather_case(n_rows, n_tile, i)
        pos[:len(F.EDGE_ROWS)] = F.EDGE_ROWS                                 # list 0 (37 entries) names every edge row
        pos[ptr[2]] = n_rows - 1                                             # the list of one entry: the last row alone
        assert ptr[1] >= len(F.EDGE_ROWS) and ptr[3] - ptr[2] == 1 and w[0] != 0 and w[2] != 0
        pd, posd, wd = dev.put(ptr), dev.put(pos), dev.put(w)
        n_src = n_cols + 6
        ids = rng.permutation(n_src)[:n_cols].astype(np.int32)
        ids[1], ids[n_cols - 2] = n_src, -1
        for col_ids, col_base in ((ids, 0), (None, 4)):
            T, host = out_of(dev, (n_src + 1, B.TILE), t_dtype, 77.0)
            _foldin.check(lib.simrank_foldin_gather(S, layout, g.stride, n_rows, n_cols, None if col_ids is None else dev.put(col_ids),
                                                    col_base, pd, posd, wd, n_tile, T, n_src, st), "gather")
            host[:n_src] = B.ref_gather(blk.A, layout, col_ids, col_base, ptr, pos, w, n_tile, host[:n_src])
            same_bits(dev.get(T, host), host, ("gather", what, n_tile, col_ids is None))
        dev.release()


# ---- model -------------------------------------------------------------------------------------------------------------------
DST_ROWS = 66                                     # destination rows: past row 64 (2^32 elements), SHIFT below the arena's end


def pack_case(rng, j):
    """(row_map, col_dst, col_src, n_list, dst_cols) with each map on and off; the row map names the edge rows and one
    row outside the source, the column maps the edge columns."""
    n_list = F.N_COLS - 1 - (j % 3)
    dst_cols = n_list + 2
    row_map = col_dst = col_src = None
    if j % 4 in (1, 3):
        row_map = rng.integers(0, F.N_ROWS, size=DST_ROWS).astype(np.int32)
        row_map[[0, 31, 32, 63, 64, 65]] = F.EDGE_ROWS[::-1]
        row_map[40] = (F.N_ROWS, -1)[j % 2]
        rest = np.setdiff1d(np.arange(F.N_COLS), F.EDGE_COLS)
        col_src = rng.permutation(np.concatenate([F.EDGE_COLS, rng.permutation(rest)[:n_list - len(F.EDGE_COLS)]])).astype(np.int32)
    if j % 4 in (2, 3):
        col_dst = np.sort(rng.permutation(dst_cols)[:n_list]).astype(np.int32)
    return row_map, col_dst, col_src, n_list, dst_cols


@pytest.mark.parametrize("src_layout,dst_layout", PAIRS)
def test_model_pack_far_to_far(dev, arena, src_layout, dst_layout):
    """Source and destination both far, in the one arena; the destination holds 0xA5 where it is read back (its rows or
    panels and their margins) and the filler elsewhere."""
    lib, st = _model.load(), dev.ops.stream
    converts = B.STORED[src_layout] != B.STORED[dst_layout]
    dtype = B.STORED[dst_layout]
    fill = np.frombuffer(bytes([B.PACK_FILL]) * dtype().itemsize, dtype=dtype)[0]
    j = 0
    for blk, g, S, what in far_blocks(arena, src_layout, kinds=("wide",), seed=50, overflow=6 if converts else 0):
        if converts:
            assert len(blk.special["overflow"]) == 6
        for gd, case in [(gd, case) for gd in F.geometries(dst_layout)[:2] for case in range(4)]:
            j = 4 * (j // 4) + case                                          # every map case for every pair of geometries
            rng = np.random.default_rng(300 + j)
            row_map, col_dst, col_src, n_list, dst_cols = pack_case(rng, j)
            D = arena.base + SHIFT
            assert SHIFT + F.extent(gd, DST_ROWS, dst_cols) <= F.HALF
            before = F.stored_pieces(gd, np.full((DST_ROWS, dst_cols), fill, dtype=dtype), fill)
            mark = len(arena.placed)
            for at, raw in before:
                arena.write(D + at, raw)
            over = dev.put(np.array([1000], dtype=np.int64)) if converts else None
            _model.check(lib.simrank_model_pack(
                S, src_layout, g.stride, F.N_ROWS, F.N_COLS, None if row_map is None else dev.put(row_map),
                None if col_dst is None else dev.put(col_dst), None if col_src is None else dev.put(col_src), n_list, D,
                dst_layout, gd.stride, DST_ROWS, dst_cols, over, st), "pack")
            # the statement on a near destination of the same shape, then laid out as the far one is
            near = F.geometries(dst_layout, DST_ROWS + 3 if dst_layout in B.PANEL else dst_cols + 8)[0]
            flat = np.full(B.n_elems(dst_layout, DST_ROWS, dst_cols, near.stride), fill, dtype=dtype)
            flat, n_over = B.ref_pack(blk, dst_layout, near.stride, DST_ROWS, dst_cols, row_map, col_dst, col_src, n_list, flat)
            want = F.stored_pieces(gd, flat[B.offsets(dst_layout, DST_ROWS, dst_cols, near.stride)], fill)
            for (at, raw), (at0, raw0) in zip(want, before):
                assert at == at0 and len(raw) == len(raw0)
                got = np.empty(len(raw), dtype=np.uint8)
                dev.ops.d2h(got, D + at)
                dev.ops.synchronize()
                same_bits(got, np.frombuffer(raw, dtype=np.uint8), ("pack", what, gd.tag, j % 4, at))
            if converts:
                assert dev.get(over, np.zeros(1, dtype=np.int64))[0] == 1000 + n_over
                assert n_over >= 1 or row_map is not None
            # the destination gives way to the next one: the filler again
            dev.ops.synchronize()
            for at, n in arena.placed[mark:]:
                dev.ops.h2d(at, F.filler(src_layout, n // F.itemsize(src_layout)).view(np.uint8))
            del arena.placed[mark:]
            j += case == 3                                                   # (the next pair draws other maps and n_list)
        dev.release()


# ---- sets, and the rank library on the band --------------------------------------------------------------------------------------
def far_baskets(rng):
    """test_gpu_companion_blocks' baskets with members on each side of every boundary: empty, one member (the last row),
    a member twice, 19 members with every edge row, 8 members, one with a position outside the block."""
    n_rows = F.N_ROWS
    lists = [rng.integers(0, n_rows, size=m).astype(np.int32) for m in (0, 1, 3, 19, 8, 4)]
    lists[1][0] = n_rows - 1
    lists[2][2] = lists[2][0] = 64
    lists[3][:len(F.EDGE_ROWS)] = F.EDGE_ROWS
    lists[4][:2] = (32, 63)
    lists[5][1] = n_rows
    ptr, pos = _sets.join(lists)
    w = rng.choice([-1.0, 1.0], size=pos.size) * 10.0 ** rng.uniform(-9, 6, size=pos.size)
    return ptr, pos, w


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_sets_score(dev, arena, layout):
    lib, st = _sets.load(), dev.ops.stream
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        rng = np.random.default_rng(400 + i)
        ptr, pos, w = far_baskets(rng)
        n_sets = ptr.size - 1
        pd, posd, wd = dev.put(ptr), dev.put(pos), dev.put(w)
        cmap = rng.permutation(n_cols).astype(np.int32)
        cmap[n_cols // 3] = n_cols
        ex = [np.array(x, dtype=np.int32) for x in ([0], [n_cols - 1], [512, 515], [1023, 1023], [n_cols, -1], [0, n_cols - 1, 1024])]
        xp, xc = _sets.join(ex)
        xpd, xcd = dev.put(xp), dev.put(xc)
        for col_pos in (None, cmap):
            for excl in (False, True):
                want = B.ref_score(blk.A, col_pos, n_cols, ptr, pos, w, xp if excl else None, xc if excl else None)
                order = (_sets.BASKET_MAJOR, _sets.CHUNK_LABEL)[(i + excl) % 2]
                ld = n_cols + 3
                out, host = out_of(dev, (n_sets + 1, ld), np.float64, 1e300)
                _sets.check(lib.simrank_sets_score(S, layout, g.stride, n_rows, n_cols, None if col_pos is None else dev.put(col_pos),
                                                   n_cols, pd, posd, wd, n_sets, xpd if excl else None, xcd if excl else None, out, ld,
                                                   order, st), "score")
                host[:n_sets, :n_cols] = want
                same_bits(dev.get(out, host), host, ("score", what, col_pos is None, excl, order))
                # the band's k best, on the near band
                for k in (10, n_cols + 5):
                    idx, hi = out_of(dev, (n_sets + 1, k), np.int32, -9)
                    val, hv = out_of(dev, (n_sets + 1, k), np.float64, 1e300)
                    _sets.check(lib.simrank_sets_topk(out, ld, n_sets, n_cols, None, k, idx, val, st), "sets_topk")
                    hi[:n_sets], hv[:n_sets] = B.ref_band_topk(want, None, k)
                    same_bits(dev.get(idx, hi), hi, ("band ids", what, k))
                    same_bits(dev.get(val, hv), hv, ("band values", what, k))
        dev.release()


@pytest.mark.parametrize("far", FAR_OUTPUTS, ids=FAR_IDS)
def test_a_far_band_scored_ranked_and_counted(dev, arena, far):
    """The score band in the arena (nine baskets with ld = 2^28, or two with ld = 2^32): written by simrank_sets_score,
    read by simrank_sets_topk, simrank_rank_gather and simrank_rank_count."""
    slib, rlib, st = _sets.load(), _rank.load(), dev.ops.stream
    layout, n_cols = B.PANEL_F32, F.N_COLS
    LD_FAR, N_FAR = far[0], far[1]
    pick = list(range(9))[-N_FAR:] if N_FAR == 9 else [3, 8]
    check_far_output(far)
    for blk, g, S, what in far_blocks(arena, layout, kinds=("dyadic",)):
        rng = np.random.default_rng(77)
        lists = [rng.integers(0, F.N_ROWS, size=m).astype(np.int32) for m in (3, 1, 0, 19, 8, 4, 2, 5, 6)]
        lists[3][:len(F.EDGE_ROWS)] = F.EDGE_ROWS
        lists[8][:3] = (F.N_ROWS - 1, 64, 31)
        lists = [lists[q] for q in pick]
        ptr, pos = _sets.join(lists)
        w = rng.choice([-1.0, 1.0], size=pos.size) * 2.0 ** rng.integers(-6, 6, size=pos.size)
        ex = [np.array(x, dtype=np.int32) for x in ([0], [], [5], [n_cols - 1], [], [512], [], [], [0, 1023, n_cols - 1])]
        xp, xc = _sets.join([ex[q] for q in pick])
        want = B.ref_score(blk.A, None, n_cols, ptr, pos, w, xp, xc)
        band, host = far_rows(arena, far, n_cols, np.inf)                  # (+inf in the padding would be counted first)
        for order in (_sets.CHUNK_LABEL, _sets.BASKET_MAJOR):
            host[:] = np.inf                                                 # the pre-fill again: each order writes every value
            for q in range(host.shape[0]):
                dev.ops.h2d(band + 8 * q * LD_FAR, host[q])
            _sets.check(slib.simrank_sets_score(S, layout, g.stride, F.N_ROWS, n_cols, None, n_cols, dev.put(ptr), dev.put(pos),
                                                dev.put(w), N_FAR, dev.put(xp), dev.put(xc), band, LD_FAR, order, st), "score")
            host[:N_FAR, :n_cols] = want
            same_bits(read_far_rows(dev, far, band, host), host, ("far band", what, order))
        ids = (rng.permutation(n_cols + 7)[:n_cols] * 3 + 1).astype(np.int32)
        for col_ids in (None, ids):
            for k in (10, n_cols + 5):
                idx, hi = out_of(dev, (N_FAR + 1, k), np.int32, -9)
                val, hv = out_of(dev, (N_FAR + 1, k), np.float64, 1e300)
                _sets.check(slib.simrank_sets_topk(band, LD_FAR, N_FAR, n_cols, None if col_ids is None else dev.put(col_ids), k,
                                                   idx, val, st), "sets_topk")
                hi[:N_FAR], hv[:N_FAR] = B.ref_band_topk(want, col_ids, k)
                same_bits(dev.get(idx, hi), hi, ("far band ids", what, col_ids is None, k))
                same_bits(dev.get(val, hv), hv, ("far band values", what, col_ids is None, k))
            # targets per basket: edge columns, an excluded one, a column of another block (-1), none for basket 1
            targets = [list(F.EDGE_COLS), [], [5, 7], [n_cols - 1, 3], [-1, 9], [512, 513], [1], [2, 2], [0, 1023, n_cols - 1, 600]]
            targets = [targets[q] for q in pick]
            tptr = np.zeros(N_FAR + 1, dtype=np.int64)
            np.cumsum([len(t) for t in targets], out=tptr[1:])
            tcol = np.concatenate([np.asarray(t, dtype=np.int32) for t in targets])
            col_id = np.arange(n_cols, dtype=np.int32) if col_ids is None else col_ids
            tid = np.where(tcol >= 0, col_id[np.maximum(tcol, 0)], 5).astype(np.int32)
            score0 = np.where(tcol >= 0, 123.0, 0.25)
            basket = np.repeat(np.arange(N_FAR), np.diff(tptr))
            want_score = np.where(tcol >= 0, want[basket, np.maximum(tcol, 0)], score0)
            tptr_dev, score_dev, tid_dev = dev.put(tptr), dev.put(score0), dev.put(tid)
            _rank.check(rlib.simrank_rank_gather(band, LD_FAR, N_FAR, n_cols, tptr_dev, dev.put(tcol), score_dev, st), "gather")
            score = dev.get(score_dev, score0)
            same_bits(score, want_score, ("far gather", what))
            before0, cand0 = 1000 + np.arange(tcol.size, dtype=np.int64), 77 + np.arange(N_FAR + 1, dtype=np.int64)
            want_before, want_cand = before0.copy(), cand0.copy()
            for q in range(N_FAR):
                for x in range(tptr[q], tptr[q + 1]):
                    b, c = K.count(want[q], col_id, want_score[x], tid[x])
                    want_before[x] += b
                    want_cand[q] = cand0[q] + c
            before_dev, cand_dev = dev.put(before0), dev.put(cand0)
            _rank.check(rlib.simrank_rank_count(band, LD_FAR, N_FAR, n_cols, None if col_ids is None else dev.put(col_ids), tptr_dev,
                                                score_dev, tid_dev, before_dev, cand_dev, st), "count")
            assert np.array_equal(dev.get(before_dev, before0), want_before), (what, col_ids is None)
            assert np.array_equal(dev.get(cand_dev, cand0), want_cand), (what, col_ids is None)
            assert want_cand[N_FAR - 1] - cand0[N_FAR - 1] == n_cols - 3    # the far row: all but its excluded columns
        dev.release()


# ---- neighbors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_neighbors_select(dev, arena, layout):
    lib, st = _neighbors.load(), dev.ops.stream
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        rng = np.random.default_rng(500 + i)
        n_q = 10
        row_pos = edge_rows(rng, n_q)
        rp = dev.put(row_pos)
        col_ids = (rng.permutation(n_cols + 7)[:n_cols] * 3 + 1).astype(np.int32)
        own = col_ids[(row_pos.astype(np.int64) * 5 + 1) % n_cols].astype(np.int32)
        for ids, row_ids in ((col_ids, own), (None, row_pos)):
            for k in (10, 65, n_cols):
                idx, hi = out_of(dev, (n_q + 1, k), np.int32, -9)
                val, hv = out_of(dev, (n_q + 1, k), np.float64, 1e300)
                _neighbors.check(lib.simrank_neighbors_select(S, layout, g.stride, n_rows, n_cols, rp, dev.put(row_ids), n_q,
                                                              None if ids is None else dev.put(ids), k, idx, val, st), "select")
                hi[:n_q], hv[:n_q] = B.ref_topk(blk.A, row_pos, row_ids, ids, k)
                same_bits(dev.get(idx, hi), hi, ("ids", what, ids is None, k))
                same_bits(dev.get(val, hv), hv, ("values", what, ids is None, k))
        dev.release()


# ---- profile -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_profile_count_and_digits(dev, arena, layout):
    lib, st = _profile.load(), dev.ops.stream
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        A, rng = blk.A, np.random.default_rng([i, layout])
        ts = thresholds_of(A, rng)
        order = np.argsort(ts, kind="stable")
        edges = ts[order] if layout == B.ROWMAJOR_F64 else _profile.edges_f32(ts[order])
        edges_dev = dev.put(edges)
        for row_ids, col_ids, skip in profile_ids(n_rows, n_cols, rng):
            rid, cid = None if row_ids is None else dev.put(row_ids), None if col_ids is None else dev.put(col_ids)
            v = A[~skip]
            host = np.zeros(ts.size + 2, dtype=np.uint64)
            host[-1] = 77
            counts = dev.put(host)
            _profile.check(lib.simrank_profile_count(S, layout, g.stride, n_rows, n_cols, rid, cid, edges_dev, ts.size, counts, st),
                           "count")
            got = dev.get(counts, host)
            assert got[-1] == 77 and np.array_equal(got[:-1], interval_counts(v, edges.astype(np.float64))), (what, row_ids is None)
            at_least = np.empty(ts.size, dtype=np.int64)
            at_least[order] = np.cumsum(got[:-1][::-1].astype(np.int64))[::-1][1:]
            assert np.array_equal(at_least, PR.count_pairs(A, ts, skip)), (what, row_ids is None)
            assert int(got[:-1].sum()) == v.size                            # every entry once: no filler, no padding
            # the digit sweeps, driven by the host half of the select
            entries = int((~skip).sum())
            for m in (1, entries // 3, entries):
                sweep, calls = device_sweep(dev, (S, layout, g.stride, n_rows, n_cols, rid, cid), layout)
                assert _profile.radix_select(sweep, _profile.key_bits(layout), m) == PR.threshold_for(A, m, skip), (what, m)
        dev.release()


# ---- cluster -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_cluster_union(dev, arena, layout):
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        A, rng = blk.A, np.random.default_rng([i, layout, 9])
        ts = levels_of(A)
        for n, row_ids, col_ids in cluster_ids(n_rows, n_cols, rng):
            block = (S, g.stride, n_rows, n_cols, None if row_ids is None else dev.put(row_ids),
                     None if col_ids is None else dev.put(col_ids))
            got = check_levels(dev, [block], n, layout, ts, lambda t: CR.block_edges(A, row_ids, col_ids, n, t),
                               (what, row_ids is None))
            # level 7 is above every value: nothing joins.  (It is below the filler too, but for a wide binary16 block, whose
            # largest value + 1 passes 65504 / 2^14: there the other seven levels are what a wrong address changes.)
            assert np.array_equal(got[7], np.arange(n)), what
        dev.release()


# ---- the main library's two layout kernels -------------------------------------------------------------------------------------
N_SQ, ROWS_PAD = 1100, 1 << 22


def square_far(arena, sym):
    """A PANEL_F32 matrix of n = 1100 with rows_pad = 2^22 in the arena -> (A, device pointer).  ``sym``: mirror-equal, what
    the symmetric form of the hand-back asks for."""
    blk = B.make_block(B.PANEL_F32, N_SQ, N_SQ, N_SQ + 3, 21, kind="dyadic")
    A = np.triu(blk.A) + np.triu(blk.A, 1).T if sym else blk.A
    g = F.Geometry(B.PANEL_F32, "panel", ROWS_PAD, 0)
    assert F.extent(g, N_SQ, N_SQ) <= F.HALF
    arena.fill(B.PANEL_F32)
    return A, arena.place(g, A, blk.sentinel)


@pytest.mark.parametrize("mode", [0, 1])
def test_handback_f64_from_far_panels(dev, arena, mode):
    """Panel 16 of the source starts at 2^31 floats, panel 32 at 2^32.  Expected: the values widened, in the caller's order."""
    ops = dev.ops
    A, S = square_far(arena, sym=mode == 1)
    rng = np.random.default_rng(mode)
    inv = rng.permutation(N_SQ).astype(np.int32)
    from simrank_amd._lib import check
    for idx in (None, inv):
        ld = N_SQ + 4
        out = np.full((N_SQ + 1, ld), 1e300)
        check(ops.lib.simrank_handback_f64(out.ctypes.data, ld, S, 32, ROWS_PAD, N_SQ, None if idx is None else dev.put(idx), mode,
                                           ops.stream), "simrank_handback_f64")
        ops.synchronize()
        want = np.full_like(out, 1e300)
        want[:N_SQ, :N_SQ] = A if idx is None else A[np.ix_(idx, idx)]
        same_bits(out, want, ("handback", mode, idx is None))
    arena.clear()


def test_permute_layout_from_far_panels_and_back(dev, arena):
    ops = dev.ops
    from simrank_amd._lib import check
    A, S = square_far(arena, sym=False)
    rng = np.random.default_rng(5)
    ri, ci = rng.permutation(N_SQ).astype(np.int32), rng.permutation(N_SQ).astype(np.int32)
    ld = N_SQ + 4
    flat, host = out_of(dev, (N_SQ + 1, ld), np.float32, 9e30)
    check(ops.lib.simrank_permute_layout(S, 32, ROWS_PAD, flat, ld, 0, N_SQ, N_SQ, dev.put(ri), dev.put(ci), 4, ops.stream),
          "simrank_permute_layout")
    host[:N_SQ, :N_SQ] = A[np.ix_(ri, ci)].astype(np.float32)
    same_bits(dev.get(flat, host), host, "far panels to row-major")
    # and back into far panels, SHIFT bytes on: the inverse maps restore the matrix
    g = F.Geometry(B.PANEL_F32, "panel", ROWS_PAD, 0)
    D = arena.base + SHIFT
    before = F.stored_pieces(g, np.full((N_SQ, N_SQ), np.float32(9e30)), np.float32(9e30))
    for at, raw in before:
        arena.write(D + at, raw)
    rinv, cinv = np.argsort(ri).astype(np.int32), np.argsort(ci).astype(np.int32)
    check(ops.lib.simrank_permute_layout(flat, ld, 0, D, 32, ROWS_PAD, N_SQ, N_SQ, dev.put(rinv), dev.put(cinv), 4, ops.stream),
          "simrank_permute_layout")
    want = F.stored_pieces(g, A.astype(np.float32), np.float32(9e30))
    for (at, raw), (_, raw0) in zip(want, before):
        got = np.empty(len(raw), dtype=np.uint8)
        ops.d2h(got, D + at)
        ops.synchronize()
        same_bits(got, np.frombuffer(raw, dtype=np.uint8), ("row-major to far panels", at))
    arena.clear()
