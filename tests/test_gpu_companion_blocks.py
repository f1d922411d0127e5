"""The five companion libraries at their C interface, on blocks the test built itself (tests/blocks.py): asymmetric, no
two values of a row or column equal, both signs, every element of padding a sentinel that would pass any threshold and
win any top-k, strides and bases that lead onto the vector and the non-vector paths.  Every comparison is BIT FOR BIT
against the plain NumPy statement of the entry point (a NaN counts as a NaN whatever its payload); tests/test_blocks_cpu.py
shows why that is a fair demand of the fold-in sums too.  Every output is pre-filled with a sentinel, has a leading
dimension larger than needed and a guard row after the last: whatever the header does not promise must still hold the
sentinel afterwards."""
import ctypes as C

import numpy as np
import pytest

from simrank_amd import _foldin, _model, _query, _select, _sets
from simrank_amd.engine import HipOps
from tests import blocks as B

pytestmark = pytest.mark.gpu

INVALID = -1                                     # SIMRANK_*_ERR_INVALID of the five headers


class Dev:
    """Device memory of one test through HipOps: freed together at the end."""

    def __init__(self):
        self.ops, self.held = HipOps(0), []

    def put(self, host, base=0):
        """A device copy of the host array (or bytes) starting ``base`` bytes into its allocation."""
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

    def close(self):
        self.release()
        self.ops.close()


@pytest.fixture(scope="module")
def device():
    d = Dev()
    yield d
    d.close()


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


def blocks_of(layout, kinds=("dyadic", "wide"), shapes=B.SHAPES, tags=None, seed=0):
    """(block, base bytes, label) over the shared shapes and the layout's strides / bases."""
    for i, (n_rows, n_cols) in enumerate(shapes):
        for tag, stride, base in B.variants(layout, n_rows, n_cols):
            if tags is None or tag in tags:
                kind = kinds[i % len(kinds)]
                yield B.make_block(layout, n_rows, n_cols, stride, seed + i, kind=kind), base, (layout, n_rows, n_cols, tag, kind)


def out_of(dev, shape, dtype, fill):
    host = np.full(shape, fill, dtype=dtype)
    return dev.put(host), host


# ---- query ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_query_rows_pairs_topk(dev, layout):
    lib, st = _query.load(), dev.ops.stream
    for i, (blk, base, what) in enumerate(blocks_of(layout)):
        A, (n_rows, n_cols) = blk.A, blk.A.shape
        rng = np.random.default_rng(i)
        S = dev.put(blk.raw, base)
        n_q = (1, 8, 9, 50)[i % 4]
        row_pos = rng.integers(0, n_rows, size=n_q).astype(np.int32)
        if n_q > 1:
            row_pos[1] = row_pos[0]                                       # a row asked for twice
            row_pos[n_q // 2 + 1] = (n_rows, -1)[i % 2]                   # one position outside the block
        elif i % 8 == 0:                                                  # (n_q = 1 comes at i = 0, 4, 8, ...: the single row
            row_pos[0] = n_rows                                           # is outside the block in every other such call)
        rp = dev.put(row_pos)
        # rows: the block's own columns, and a column map with one entry outside
        cmap = rng.permutation(n_cols).astype(np.int32)
        if n_cols > 1:
            cmap[n_cols // 2] = n_cols
        for col_pos in (None, cmap):
            ld = n_cols + 3
            out, host = out_of(dev, (n_q + 1, ld), np.float64, 1e300)
            _query.check(lib.simrank_query_rows(S, layout, blk.stride, n_rows, n_cols, rp, n_q,
                                                None if col_pos is None else dev.put(col_pos), n_cols, out, ld, st), "rows")
            host[:n_q, :n_cols] = B.ref_rows(A, row_pos, col_pos, n_cols)
            same_bits(dev.get(out, host), host, ("rows", what, col_pos is None))
        # pairs
        n_p = 2 * n_q + 1
        a, b = rng.integers(0, n_rows, size=n_p).astype(np.int32), rng.integers(0, n_cols, size=n_p).astype(np.int32)
        a[0], b[n_p - 1] = n_rows, n_cols
        out, host = out_of(dev, n_p + 4, np.float64, 1e300)
        _query.check(lib.simrank_query_pairs(S, layout, blk.stride, n_rows, n_cols, dev.put(a), dev.put(b), n_p, out, st), "pairs")
        host[:n_p] = B.ref_pairs(A, a, b)
        same_bits(dev.get(out, host), host, ("pairs", what))
        # top-k: ids that are a permutation (the own node is excluded by ID), and positions
        col_ids = (rng.permutation(n_cols + 7)[:n_cols] * 3 + 1).astype(np.int32)
        own = col_ids[(row_pos.astype(np.int64) * 5 + 1) % n_cols].astype(np.int32)      # the id of some OTHER column
        for ids, row_ids in ((col_ids, own), (None, row_pos)):
            for k in sorted({1, 10, min(n_cols, 1024), min(n_cols + 5, 1024)}):
                idx, hi = out_of(dev, (n_q + 1, k), np.int32, -9)
                val, hv = out_of(dev, (n_q + 1, k), np.float64, 1e300)
                _query.check(lib.simrank_query_topk(S, layout, blk.stride, n_rows, n_cols, rp, dev.put(row_ids), n_q,
                                                    None if ids is None else dev.put(ids), k, idx, val, st), "topk")
                hi[:n_q], hv[:n_q] = B.ref_topk(A, row_pos, row_ids, ids, k)
                same_bits(dev.get(idx, hi), hi, ("topk ids", what, ids is None, k))
                same_bits(dev.get(val, hv), hv, ("topk values", what, ids is None, k))
                if k > n_cols:
                    assert (hi[:n_q, n_cols:] == -1).all()                  # the empty-slot fill was exercised
        dev.release()


# ---- select ---------------------------------------------------------------------------------------------------------------
def run_select(dev, lib, blk, S, layout, row_ids, col_ids, t32, what):
    A, (n_rows, n_cols) = blk.A, blk.A.shape
    st = dev.ops.stream
    rid = None if row_ids is None else dev.put(row_ids)
    cid = None if col_ids is None else dev.put(col_ids)
    cnt, hc = out_of(dev, n_rows + 1, np.int32, -9)
    _select.check(lib.simrank_select_count(S, layout, blk.stride, n_rows, n_cols, rid, cid, C.c_float(t32), cnt, st), "count")
    counts, rows = B.ref_select(A, row_ids, col_ids, t32)
    hc[:n_rows] = counts
    got = dev.get(cnt, hc)
    same_bits(got, hc, ("counts", what, t32))
    offs, total = np.full(n_rows + 2, -5, dtype=np.int64), C.c_int64(-1)
    _select.check(lib.simrank_select_offsets(got.ctypes.data, n_rows, offs.ctypes.data, C.byref(total)), "offsets")
    want_off, want_total = B.ref_offsets(counts)
    assert np.array_equal(offs[:n_rows + 1], want_off) and offs[n_rows + 1] == -5 and total.value == want_total
    od = dev.put(want_off)
    for capacity in (want_total + 3, want_total // 2):
        ids, hi = out_of(dev, want_total + 5, np.int32, -9)
        vals, hv = out_of(dev, want_total + 5, np.float32, 9e30)
        _select.check(lib.simrank_select_emit(S, layout, blk.stride, n_rows, n_cols, rid, cid, C.c_float(t32), od, capacity,
                                              ids, vals, st), "emit")
        wi, wv = B.ref_emit(rows, want_off, capacity, hi, hv)
        same_bits(dev.get(ids, hi), wi, ("emit ids", what, t32, capacity))
        same_bits(dev.get(vals, hv), wv, ("emit values", what, t32, capacity))
        assert (wi[min(capacity, want_total):] == -9).all()
    return counts


@pytest.mark.parametrize("layout", [B.PANEL_F32, B.ROWMAJOR_F32, B.PANEL_F16])
def test_select_count_offsets_emit(dev, layout):
    lib = _select.load()
    for i, (blk, base, what) in enumerate(blocks_of(layout)):
        A, (n_rows, n_cols) = blk.A, blk.A.shape
        rng = np.random.default_rng(100 + i)
        S = dev.put(blk.raw, base)
        pos = np.sort(A[A > 0].astype(np.float32))
        n_ids = max(n_rows, n_cols) + 3
        col_ids = rng.permutation(n_ids)[:n_cols].astype(np.int32)
        row_ids = rng.permutation(n_ids)[:n_rows].astype(np.int32)
        row_ids[0] = col_ids[n_cols - 1]                                  # an own node that is not on the diagonal
        up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
        if pos.size:
            # equal to a stored value (>= keeps it) and the next float above it (it is none any more)
            stored = pos[pos.size // 2]
            kept = run_select(dev, lib, blk, S, layout, row_ids, col_ids, float(stored), what)
            lost = run_select(dev, lib, blk, S, layout, row_ids, col_ids, float(up(stored)), what)
            plain = run_select(dev, lib, blk, S, layout, None, None, float(stored), what)
            assert kept.sum() >= lost.sum() and plain.sum() >= B.ref_select(A, None, None, float(up(stored)))[0].sum()
            # the largest value, and just above every value: no hit, though the padding's sentinel would be one
            top = pos[-1]
            assert run_select(dev, lib, blk, S, layout, None, col_ids, float(top), what).sum() <= n_rows + len(blk.repeats)
            assert run_select(dev, lib, blk, S, layout, row_ids, None, float(up(top)), what).sum() == 0 and up(top) < blk.sentinel
        # a small positive threshold: every value > 0 and no zero, no negative value
        run_select(dev, lib, blk, S, layout, row_ids, col_ids, 2.0 ** -100, what)
        # a threshold that is not positive is refused (simrank_select.h: t > 0) and nothing is written
        cnt, hc = out_of(dev, n_rows + 1, np.int32, -9)
        rc = lib.simrank_select_count(S, layout, blk.stride, n_rows, n_cols, None, None, C.c_float(-0.25), cnt, dev.ops.stream)
        assert rc == INVALID and b"threshold" in lib.simrank_select_last_error()
        same_bits(dev.get(cnt, hc), hc, ("refused", what))
        dev.release()


@pytest.mark.parametrize("layout", [B.PANEL_F32, B.ROWMAJOR_F32, B.PANEL_F16])
def test_select_dense_hits_in_one_row_of_a_wave(dev, layout):
    """Every column of rows 3 and 8 is a hit and no column of their wave-mates: the ballot ranks of a full row."""
    lib = _select.load()
    for n_rows, n_cols in ((9, 257), (70, 129), (9, 1025)):
        for tag, stride, base in B.variants(layout, n_rows, n_cols):
            blk = B.make_block(layout, n_rows, n_cols, stride, 41, kind="dyadic")
            step = np.abs(blk.A[blk.A != 0]).min()
            A = -np.abs(blk.A)
            A[[3, 8]] = np.maximum(np.abs(blk.A[[3, 8]]), step)
            dense = B.Block(layout, A, stride, blk.sentinel, np.argwhere(A == 0), blk.repeats[:0], {})
            S = dev.put(dense.raw, base)
            ids = np.random.default_rng(n_cols).permutation(n_cols + n_rows).astype(np.int32)
            counts = run_select(dev, lib, dense, S, layout, ids[n_cols:], ids[:n_cols], float(step), (layout, n_rows, n_cols, tag))
            assert counts[3] == counts[8] == n_cols and counts.sum() == 2 * n_cols
            dev.release()


# ---- fold-in --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_foldin_gather_and_member(dev, layout):
    lib, st = _foldin.load(), dev.ops.stream
    t_dtype = B.acc_type(layout)
    for i, (blk, base, what) in enumerate(blocks_of(layout, kinds=("dyadic",))):
        A, (n_rows, n_cols) = blk.A, blk.A.shape
        rng = np.random.default_rng(200 + i)
        n_tile = (1, 5, 31, 32)[i % 4]
        ptr, pos, w = B.gather_case(n_rows, n_tile, i)
        S, pd, wd = dev.put(blk.raw, base), dev.put(ptr), dev.put(w)
        posd = dev.put(pos if pos.size else np.zeros(1, dtype=np.int32))
        n_src = n_cols + 6
        assert lib.simrank_foldin_t_bytes(layout, n_src) == n_src * 32 * np.dtype(t_dtype).itemsize
        ids = rng.permutation(n_src)[:n_cols].astype(np.int32)
        if n_cols > 2:
            ids[1], ids[n_cols - 1] = n_src, -1                           # ids outside the source nodes: not written
        for col_ids, col_base in ((ids, 0), (None, 4)):
            T, host = out_of(dev, (n_src + 1, B.TILE), t_dtype, 77.0)
            _foldin.check(lib.simrank_foldin_gather(S, layout, blk.stride, n_rows, n_cols,
                                                    None if col_ids is None else dev.put(col_ids), col_base, pd, posd, wd, n_tile,
                                                    T, n_src, st), "gather")
            host[:n_src] = B.ref_gather(A, layout, col_ids, col_base, ptr, pos, w, n_tile, host[:n_src])
            same_bits(dev.get(T, host), host, ("gather", what, n_tile, col_ids is None))
            assert (host[n_src] == 77.0).all() and (host[:n_src] == 77.0).all(axis=1).sum() >= 6 - 2 * (col_ids is None)
        # member: the lists as source ids
        list_ids = ids[pos % n_cols] if pos.size else pos
        mem, hm = out_of(dev, n_src + 1, np.uint32, 0xDEADBEEF)
        _foldin.check(lib.simrank_foldin_member(pd, dev.put(list_ids if pos.size else np.zeros(1, dtype=np.int32)), wd, n_tile,
                                                mem, n_src, st), "member")
        hm[:n_src] = B.ref_member(ptr, list_ids, w, n_tile, n_src)
        same_bits(dev.get(mem, hm), hm, ("member", what, n_tile))
        dev.release()


@pytest.mark.parametrize("t_layout", [B.PANEL_F32, B.ROWMAJOR_F64])
def test_foldin_apply_on_a_small_csr(dev, t_layout):
    """Row lengths 0 .. 600 around SIMRANK_FOLDIN_LONG_ROW, through the half-wave kernel alone and with the long rows on
    their own kernel; evidence and prior on and off; a scale of 0; counts that reach 255 and pass it."""
    lib, st = _foldin.load(), dev.ops.stream
    c = B.apply_case(B.acc_type(t_layout))
    n_out, n_src = c["n_out"], c["n_src"]
    ld_prior = n_out + 2
    prior = np.full((B.TILE, ld_prior), 1e300)
    prior[:, :n_out] = c["prior"]
    d = {k: dev.put(c[k]) for k in ("rowptr", "col", "scale", "T", "member", "long_rows")}
    pr = dev.put(prior)
    for n_tile in (32, 5):
        for member in (c["member"], None):
            for pri in (c["prior"], None):
                for n_long in (len(c["long_rows"]), 0):
                    ld = n_out + 3
                    out, host = out_of(dev, (n_tile + 1, ld), np.float64, -55.0)
                    _foldin.check(lib.simrank_foldin_apply(
                        d["rowptr"], d["col"], d["scale"], n_out, n_src, d["long_rows"] if n_long else None, n_long, d["T"],
                        t_layout, None if member is None else d["member"], c["coef"], c["lbd"], None if pri is None else pr,
                        ld_prior, n_tile, out, ld, st), "apply")
                    want = B.ref_apply(c["rowptr"], c["col"], c["scale"], c["T"], member, c["coef"], c["lbd"], pri, n_tile, host)
                    same_bits(dev.get(out, host), want, ("apply", t_layout, n_tile, member is None, pri is None, n_long))
                    assert (want[n_tile] == -55.0).all() and (want[:, n_out:] == -55.0).all()


# ---- model ----------------------------------------------------------------------------------------------------------------
PAIRS = [(B.PANEL_F32, B.ROWMAJOR_F32), (B.ROWMAJOR_F32, B.ROWMAJOR_F32), (B.PANEL_F16, B.PANEL_F16),
         (B.ROWMAJOR_F64, B.ROWMAJOR_F64), (B.PANEL_F32, B.PANEL_F16), (B.ROWMAJOR_F32, B.PANEL_F16)]
PACK_SHAPES = [(7, 1), (8, 33), (9, 63), (70, 129), (7, 255), (9, 1023), (8, 1025), (7, 2050)]     # 512 / 1024 / 2048 per chunk


def pack_maps(rng, blk, j):
    """(dst_rows, dst_cols, row_map, col_dst, col_src, n_list): each map on and off; n_list below both column counts; a
    row_map entry outside the source (its destination row keeps the fill)."""
    n_rows, n_cols = blk.A.shape
    n_list = max(1, n_cols - 1 - (j % 3))
    dst_cols = n_list + 2
    if j % 4 == 0:
        return n_rows, dst_cols, None, None, None, n_list
    dst_rows = n_rows + 2
    row_map = rng.integers(0, n_rows, size=dst_rows).astype(np.int32)
    row_map[dst_rows // 2] = (n_rows, -1)[j % 2]
    col_src = rng.permutation(n_cols)[:n_list].astype(np.int32)
    if j % 4 == 1:
        return dst_rows, dst_cols, row_map, None, col_src, n_list
    col_dst = np.sort(rng.permutation(dst_cols)[:n_list]).astype(np.int32)
    if j % 4 == 2:
        return n_rows, dst_cols, None, col_dst, None, n_list
    return dst_rows, dst_cols, row_map, col_dst, col_src, n_list


@pytest.mark.parametrize("src_layout,dst_layout", PAIRS)
def test_model_pack(dev, src_layout, dst_layout):
    lib, st = _model.load(), dev.ops.stream
    converts = B.STORED[src_layout] != B.STORED[dst_layout]
    j = 0
    for i, (n_rows, n_cols) in enumerate(PACK_SHAPES):
        for tag, stride, base in B.variants(src_layout, n_rows, n_cols):
            rng = np.random.default_rng(300 + j)
            planted = 6 if converts and n_rows * n_cols > 500 else 0
            blk = B.make_block(src_layout, n_rows, n_cols, stride, 50 + i, kind="wide", overflow=planted)
            if planted:
                assert len(blk.special["overflow"]) == planted
            S = dev.put(blk.raw, base)
            dst_rows, dst_cols, row_map, col_dst, col_src, n_list = pack_maps(rng, blk, j)
            # destination strides that allow and that forbid the 16-byte store (panels: always allowed)
            for dtag, dst_stride, _ in B.variants(dst_layout, dst_rows, dst_cols)[:2]:
                n = B.n_elems(dst_layout, dst_rows, dst_cols, dst_stride) + 32              # (a guard after the block)
                before = np.frombuffer(bytes([B.PACK_FILL]) * (n * np.dtype(B.STORED[dst_layout]).itemsize), dtype=B.STORED[dst_layout])
                D = dev.put(before)
                over = dev.put(np.array([1000], dtype=np.int64)) if converts else None
                _model.check(lib.simrank_model_pack(
                    S, src_layout, blk.stride, n_rows, n_cols, None if row_map is None else dev.put(row_map),
                    None if col_dst is None else dev.put(col_dst), None if col_src is None else dev.put(col_src), n_list, D,
                    dst_layout, dst_stride, dst_rows, dst_cols, over, st), "pack")
                want, n_over = B.ref_pack(blk, dst_layout, dst_stride, dst_rows, dst_cols, row_map, col_dst, col_src, n_list, before)
                same_bits(B.bits(dev.get(D, before)), B.bits(want), ("pack", src_layout, dst_layout, n_rows, n_cols, tag, dtag, j % 4))
                if converts:
                    assert dev.get(over, np.zeros(1, dtype=np.int64))[0] == 1000 + n_over       # ADDED, each value once
                    if planted and row_map is None and col_src is None:
                        assert n_over >= planted - 3                           # (n_list drops at most three columns)
            j += 1
            dev.release()


def test_model_pack_counts_once_across_the_bands_of_a_multi_launch_pack(dev):
    """2^23 + 16 destination rows of one chunk are two launches (model.hip cuts the rows into bands of 2^23 workgroup rows).
    Nearly every row_map entry is -1 (such a row is neither read nor written), a few rows at both ends of each band
    point at source rows that hold planted values binary16 cannot hold.  The 1 GiB destination is not filled and is
    read back only around the live rows; it is the one block of this module above 1 MB, because the shipped band size is
    the one to test.  The counter must hold 1000 + the overflows read, each once, and both bands the right bits."""
    lib, st = _model.load(), dev.ops.stream
    blk = B.make_block(B.ROWMAJOR_F32, 70, 129, 132, 77, kind="wide", overflow=9)
    planted = blk.special["overflow"]
    assert len(planted) == 9
    rng = np.random.default_rng(78)
    band, n_list = 1 << 23, 40
    dst_rows, dst_cols, dst_stride = band + 16, n_list, band + 16
    over_cols = sorted({c for _, c in planted})
    rest = [c for c in rng.permutation(129) if c not in over_cols][:n_list - len(over_cols)]
    col_src = rng.permutation(np.array(over_cols + rest, dtype=np.int32))
    src_rows = [r for r, _ in planted]
    live = {0: src_rows[0], 5: src_rows[1], band - 2: src_rows[2], band - 1: src_rows[3],          # the first launch
            band: src_rows[4], band + 1: src_rows[5], band + 9: 70, band + 14: src_rows[6], band + 15: src_rows[7]}
    row_map = np.full(dst_rows, -1, dtype=np.int32)
    for r, sr in live.items():
        row_map[r] = sr
    # the rows read back: every live row and its neighbours, which hold the fill before the call
    look = sorted({r + d for r in live for d in (-1, 0, 1) if 0 <= r + d < dst_rows})
    fill = np.frombuffer(bytes([B.PACK_FILL]) * (len(look) * 128), dtype=np.float16).reshape(len(look), 64)
    D = dev.ops._malloc(B.n_elems(B.PANEL_F16, dst_rows, dst_cols, dst_stride) * 2)
    dev.held.append(D)
    for r in look:
        dev.ops.h2d(D + 128 * r, fill[0])
    over = dev.put(np.array([1000], dtype=np.int64))
    _model.check(lib.simrank_model_pack(dev.put(blk.raw), B.ROWMAJOR_F32, blk.stride, 70, 129, dev.put(row_map), None,
                                        dev.put(col_src), n_list, D, B.PANEL_F16, dst_stride, dst_rows, dst_cols, over, st), "pack")
    # the same rows as a destination of their own: one 64-column panel, so a row is the same 128 bytes in both
    want, n_over = B.ref_pack(blk, B.PANEL_F16, len(look), len(look), dst_cols, row_map[look], None, col_src, n_list, fill.ravel())
    per_band = [B.ref_pack(blk, B.PANEL_F16, len(look), len(look), dst_cols, np.where(keep, row_map[look], -1), None, col_src,
                           n_list, fill.ravel())[1] for keep in (np.array(look) < band, np.array(look) >= band)]
    assert min(per_band) >= 4 and sum(per_band) == n_over                  # both launches read values that overflow
    got = np.empty_like(fill)
    for i, r in enumerate(look):
        dev.ops.d2h(got[i], D + 128 * r)
    dev.ops.synchronize()
    same_bits(B.bits(got), B.bits(want.reshape(len(look), 64)), "rows around the seam of the two launches")
    assert dev.get(over, np.zeros(1, dtype=np.int64))[0] == 1000 + n_over
    untouched = [i for i, r in enumerate(look) if row_map[r] < 0 or row_map[r] >= 70]
    assert len(untouched) >= 8 and (B.bits(got[untouched]) == 0xA5A5).all()
    dev.release()
    HipOps.trim_pool(0)                                                    # (the 1 GiB block goes back to the driver)


def test_model_pack_refuses_the_other_pairs(dev):
    lib = _model.load()
    blk = B.make_block(B.ROWMAJOR_F64, 9, 63, 64, 1)                           # (512 bytes per row: room for every layout)
    S, D = dev.put(blk.raw), dev.put(np.full(9 * 64, 5.0))
    over = dev.put(np.zeros(1, dtype=np.int64))
    refused = 0
    for s in B.LAYOUTS:
        for d in B.LAYOUTS:
            if (s, d) in PAIRS:
                continue
            rc = lib.simrank_model_pack(S, s, 16, 9, 16, None, None, None, 8, D, d, 16, 9, 16, over, dev.ops.stream)
            msg = lib.simrank_model_last_error().decode()
            assert rc == INVALID and f"layout {s} to layout {d}" in msg, (s, d, rc, msg)
            refused += 1
    assert refused == 10
    assert (dev.get(D, np.zeros(9 * 64)) == 5.0).all() and dev.get(over, np.zeros(1, dtype=np.int64))[0] == 0


# ---- sets -----------------------------------------------------------------------------------------------------------------
SETS_SHAPES = [(7, 1), (8, 33), (70, 129), (9, 1023), (8, 1025), (7, 2050)]       # the ragged last quad at 1023, 1025, 2050


def baskets(rng, n_rows):
    """Empty, one member, a member twice, 19 members (above the unroll factor of 8, no multiple of it), 8 members, one with a
    position outside the block; weights of both signs over many decades."""
    lists = [rng.integers(0, n_rows, size=m).astype(np.int32) for m in (0, 1, 3, 19, 8, 4)]
    lists[2][2] = lists[2][0]
    lists[5][1] = n_rows
    ptr, pos = _sets.join(lists)
    w = rng.choice([-1.0, 1.0], size=pos.size) * 10.0 ** rng.uniform(-9, 6, size=pos.size)
    return ptr, pos, w


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_sets_score(dev, layout):
    lib, st = _sets.load(), dev.ops.stream
    tags = ("offset",) if layout == B.ROWMAJOR_F32 else None                 # (row-major f32 has its own test: only the new case)
    for i, (blk, base, what) in enumerate(blocks_of(layout, kinds=("wide", "dyadic"), shapes=SETS_SHAPES, tags=tags)):
        A, (n_rows, n_cols) = blk.A, blk.A.shape
        rng = np.random.default_rng(400 + i)
        S = dev.put(blk.raw, base)
        ptr, pos, w = baskets(rng, n_rows)
        n_sets = ptr.size - 1
        pd, posd, wd = dev.put(ptr), dev.put(pos), dev.put(w)
        cmap = rng.permutation(n_cols).astype(np.int32)
        if n_cols > 1:
            cmap[n_cols // 3] = n_cols                                    # a mapped column outside the block
        # excluded OUTPUT columns: the first, the last, a lane's first and fourth, one twice, one outside
        lane = 4 * (n_cols // 8)
        ex = [np.array(x, dtype=np.int32) for x in ([0], [n_cols - 1], [lane, min(lane + 3, n_cols - 1)], [n_cols // 2] * 2, [n_cols, -1],
                                                    [0, n_cols - 1, lane])]
        xp, xc = _sets.join(ex)
        xpd, xcd = dev.put(xp), dev.put(xc)
        for col_pos in (None, cmap):
            for excl in (False, True):
                want = B.ref_score(A, col_pos, n_cols, ptr, pos, w, xp if excl else None, xc if excl else None)
                for order in (_sets.BASKET_MAJOR, _sets.CHUNK_LABEL):
                    ld = n_cols + 3
                    out, host = out_of(dev, (n_sets + 1, ld), np.float64, 1e300)
                    _sets.check(lib.simrank_sets_score(S, layout, blk.stride, n_rows, n_cols,
                                                       None if col_pos is None else dev.put(col_pos), n_cols, pd, posd, wd, n_sets,
                                                       xpd if excl else None, xcd if excl else None, out, ld, order, st), "score")
                    host[:n_sets, :n_cols] = want
                    same_bits(dev.get(out, host), host, ("score", what, col_pos is None, excl, order))
        assert np.isnan(want[5]).sum() >= n_cols - 3 and (want[0][np.isfinite(want[0])] == 0).all()
        dev.release()


def test_sets_topk_on_a_band_of_its_own(dev):
    """NaN, -inf, +inf, repeated values, rows with fewer than k candidates and with none; ids a permutation; the band's
    padding holds a value that would win."""
    lib, st = _sets.load(), dev.ops.stream
    rng = np.random.default_rng(9)
    n_sets, n_out, ld = 6, 300, 303
    band = np.full((n_sets + 1, ld), 1e300)
    body = rng.integers(-40, 40, size=(n_sets, n_out)) * 0.125             # few distinct values: ties everywhere
    body[0, rng.permutation(n_out)[:40]] = np.nan
    body[1, rng.permutation(n_out)[:40]] = -np.inf
    body[2, 7], body[2, 200] = np.inf, np.inf
    body[3, :] = -np.inf
    body[3, [5, 299, 64]] = [1.0, 1.0, np.nan]                             # two candidates
    body[4, :] = np.nan                                                    # none
    body[5, :] = 0.0
    body[5, 63], body[5, 64] = -0.0, np.nan
    band[:n_sets, :n_out] = body
    bd = dev.put(band)
    ids = (rng.permutation(n_out + 9)[:n_out] * 2).astype(np.int32)
    for col_ids in (ids, None):
        for k in (1, 10, n_out + 5):
            idx, hi = out_of(dev, (n_sets + 1, k), np.int32, -9)
            val, hv = out_of(dev, (n_sets + 1, k), np.float64, 1e300)
            _sets.check(lib.simrank_sets_topk(bd, ld, n_sets, n_out, None if col_ids is None else dev.put(col_ids), k, idx, val, st),
                        "sets_topk")
            hi[:n_sets], hv[:n_sets] = B.ref_band_topk(body, col_ids, k)
            same_bits(dev.get(idx, hi), hi, ("band ids", col_ids is None, k))
            same_bits(dev.get(val, hv), hv, ("band values", col_ids is None, k))
    assert (hi[4] == -1).all() and (hi[3, 2:] == -1).all() and hi[3, :2].tolist() == [5, 299] and (hi[0, n_out - 40:] == -1).all()
