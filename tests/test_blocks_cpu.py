"""tests/blocks.py pinned on the CPU: the generator keeps its promises at every layout, shape and stride the GPU module
uses, the addressing round-trips, the references do what a hand-made case says, and, for the dyadic kind, the fold-in
reference gives the SAME BITS with float64 sums, float32 sums, reversed summation order and an epilogue whose last line is
contracted into one multiply-add either way.  That is why tests/test_gpu_companion_blocks.py may ask the device for bit
equality: nothing in it depends on an order or on a contraction the compiler is free to choose."""
import numpy as np
import pytest

from tests import blocks as B


@pytest.mark.parametrize("kind", ["dyadic", "wide"])
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_blocks_round_trip_and_keep_their_promises(layout, kind):
    for n_rows, n_cols in B.SHAPES:
        for tag, stride, _ in B.variants(layout, n_rows, n_cols):
            blk = B.make_block(layout, n_rows, n_cols, stride, 3, kind=kind)          # (asserts its promises itself)
            A, raw = blk
            assert A.dtype == np.float64 and A.shape == (n_rows, n_cols)
            assert len(raw) == B.n_elems(layout, n_rows, n_cols, stride) * np.dtype(B.STORED[layout]).itemsize
            back = B.decode(layout, raw, n_rows, n_cols, stride)
            assert np.array_equal(B.bits(back), B.bits(A)), (tag, n_rows, n_cols)
            assert np.array_equal(B.bits(B.encode(layout, back, stride, blk.sentinel)), B.bits(blk.stored))
            assert not (A == blk.sentinel).any() and (np.abs(A) < blk.sentinel).all()
            at = B.offsets(layout, n_rows, n_cols, stride)
            assert np.unique(at).size == at.size and at.max() < blk.stored.size        # an injective addressing
            assert len(blk.zeros) == (A == 0).sum()
            if n_rows * n_cols >= 200:
                assert len(blk.zeros) and len(blk.repeats)
            same = B.make_block(layout, n_rows, n_cols, stride, 3, kind=kind)
            assert same.raw == raw                                                      # the seed decides everything
    assert B.make_block(layout, 9, 63, 70, 4, kind=kind).raw != B.make_block(layout, 9, 63, 70, 5, kind=kind).raw


LONG = [(65545, 40), (24577, 40), (20, 33000), (8300, 40), (5, 4200)]      # the tall and long shapes of the GPU tests


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_long_blocks_round_trip_and_keep_their_promises(layout):
    """``make_long`` at the shapes ``make_block`` cannot reach: decode(encode(A)) == A bit for bit, padding holds the
    sentinel, every value exactly storable, both signs, about 4 % zeros, the seed decides everything."""
    for n_rows, n_cols in LONG:
        for tag, stride, _ in B.variants(layout, n_rows, n_cols)[-2:]:
            blk = B.make_long(layout, n_rows, n_cols, stride, 3)                       # (asserts its promises itself)
            A = blk.A
            assert A.dtype == np.float64 and A.shape == (n_rows, n_cols)
            assert len(blk.raw) == B.n_elems(layout, n_rows, n_cols, stride) * np.dtype(B.STORED[layout]).itemsize
            back = B.decode(layout, blk.raw, n_rows, n_cols, stride)
            assert np.array_equal(B.bits(back), B.bits(A)), (tag, n_rows, n_cols)
            assert np.array_equal(B.bits(B.encode(layout, back, stride, blk.sentinel)), B.bits(blk.stored))
            assert np.array_equal(B.bits(B.store(layout, A).astype(np.float64)),
                                  B.bits(A * (B.HALF_SCALE if layout == B.PANEL_F16 else 1.0)))
            pad = np.ones(blk.stored.size, dtype=bool)
            pad[B.offsets(layout, n_rows, n_cols, stride).ravel()] = False
            assert pad.any() and (B.widen(layout, blk.stored[pad]) == blk.sentinel).all()
            assert blk.sentinel == B.SENTINEL[(layout, "dyadic")] and (np.abs(A) < blk.sentinel).all()
            steps = A * 1024.0
            assert np.array_equal(steps, np.round(steps)) and np.abs(A).max() < 16     # what operator_ref.assert_exact needs
            assert (A > 0).mean() > 0.4 and (A < 0).mean() > 0.4
            assert 0.03 < (A == 0).mean() < 0.05 and len(blk.zeros) == (A == 0).sum()
            # every stretch of 8 rows (a wave of a panel sweep) and every column holds both signs
            if n_cols >= 40:
                assert (A > 0).any(axis=1).all() and (A < 0).any(axis=1).all()
    same = B.make_long(layout, 8197, 40, B.variants(layout, 8197, 40)[0][1], 4)
    again = B.make_long(layout, 8197, 40, same.stride, 4)
    other = B.make_long(layout, 8197, 40, same.stride, 5)
    assert same.raw == again.raw and same.raw != other.raw


def test_the_addressing_is_the_headers():
    """Hand-computed offsets of include/simrank_query.h's formulas."""
    assert B.offsets(B.PANEL_F32, 5, 70, 9)[4, 69] == ((69 >> 5) * 9 + 4) * 32 + (69 & 31) == (2 * 9 + 4) * 32 + 5
    assert B.offsets(B.PANEL_F16, 5, 70, 9)[4, 69] == ((69 >> 6) * 9 + 4) * 64 + (69 & 63) == (9 + 4) * 64 + 5
    assert B.offsets(B.ROWMAJOR_F32, 5, 70, 75)[4, 69] == B.offsets(B.ROWMAJOR_F64, 5, 70, 75)[4, 69] == 4 * 75 + 69
    assert B.n_elems(B.PANEL_F32, 5, 70, 9) == 3 * 9 * 32 and B.n_elems(B.PANEL_F16, 5, 70, 9) == 2 * 9 * 64
    # the fp16-held form: value x 2^14 in binary16, widened through float
    raw = B.encode(B.PANEL_F16, np.array([[0.5, -2.0 ** -38]]), 1, 3.0)
    assert raw[0] == np.float16(8192.0) and B.bits(raw[1:2])[0] == 0x8001 and raw[2] == np.float16(49152.0)


def test_wide_blocks_hold_what_narrowing_has_to_get_right():
    blk = B.make_block(B.ROWMAJOR_F32, 70, 129, 132, 1, kind="wide", overflow=9)
    A = blk.A
    h = B.narrow(A)
    hb = B.bits(h).astype(np.int64)
    at = lambda name: [hb[r, c] for r, c in blk.special[name]]
    assert at("tie_down") == [0x6800, 0xe800] and at("tie_up") == [0x6802, 0xe802]      # 2048 and 2052, never 2050
    assert at("sub_tie_zero") == [0x0000] and at("sub_tie_up") == [0x0002]
    assert at("sub_exact") == [0x0001, 0x03ff] and at("sub_round") == [0x0005, 0x8000 | 778]
    assert at("neg_zero") == [0x8000] and at("pos_zero") == [0x0000]
    assert at("largest") == [0x7bff, 0x7bff, 0xfbff]
    assert len(blk.special["overflow"]) == 9 and all((b & 0x7c00) == 0x7c00 for b in at("overflow"))
    assert int(((hb & 0x7c00) == 0x7c00).sum()) == 9                                   # the planted ones and no other
    sub = (hb & 0x7c00) == 0
    assert sub.sum() > 100 and ((hb & 0x7fff) == 0).sum() > 20                          # subnormal and flushed results
    # truncation would differ: the rounding mode is visible in this block
    toward_zero = np.where(np.abs(h.astype(np.float64)) > np.abs(A * B.HALF_SCALE), 1, 0)
    assert toward_zero.sum() > 100
    plain = B.make_block(B.PANEL_F32, 70, 129, 75, 1, kind="wide")
    assert np.isfinite(plain.A).all() and not ((B.bits(B.narrow(plain.A)) & 0x7c00) == 0x7c00).any()
    assert (np.abs(plain.A) < 2.0 ** -28).any() and (plain.A == 65504.0 / B.HALF_SCALE).any()


def test_query_and_select_references_on_a_hand_made_block():
    A = np.array([[0.5, -1.0, 0.5, 0.0, 2.0],
                  [0.25, 0.25, 0.25, -3.0, 0.125]])
    rows = B.ref_rows(A, [1, 2, 0, 0], [4, 0, 7], 3)
    assert np.array_equal(rows[0], [0.125, 0.25, np.nan], equal_nan=True) and np.isnan(rows[1]).all()
    assert np.array_equal(rows[2][:2], [2.0, 0.5]) and np.isnan(rows[2][2]) and np.array_equal(rows[2], rows[3], equal_nan=True)
    assert np.array_equal(B.ref_pairs(A, [0, 1, 2, 0], [4, 3, 0, 5]), [2.0, -3.0, np.nan, np.nan], equal_nan=True)
    ids = np.array([10, 7, 3, 9, 4])
    idx, val = B.ref_topk(A, [0, 1, 5], [4, 7, 0], ids, 6)
    assert idx[0].tolist() == [3, 10, 9, 7, -1, -1] and val[0].tolist() == [0.5, 0.5, 0.0, -1.0, 0.0, 0.0]   # id 4 is its own
    assert idx[1].tolist() == [3, 10, 4, 9, -1, -1] and val[1].tolist() == [0.25, 0.25, 0.125, -3.0, 0.0, 0.0]
    assert (idx[2] == -1).all() and (val[2] == 0).all()
    idx, val = B.ref_topk(A, [0], [99], None, 2)
    assert idx[0].tolist() == [4, 0] and val[0].tolist() == [2.0, 0.5]
    band = np.array([[1.0, np.nan, -np.inf, 1.0, np.inf, -2.0]])
    idx, val = B.ref_band_topk(band, np.array([5, 4, 3, 2, 1, 0]), 5)
    assert idx[0].tolist() == [1, 2, 5, 0, -1] and val[0].tolist() == [np.inf, 1.0, 1.0, -2.0, 0.0]
    counts, hits = B.ref_select(A, [3, 7], ids, 0.25)
    assert counts.tolist() == [2, 2] and hits[0][0].tolist() == [10, 4] and hits[1][0].tolist() == [10, 3]   # >= keeps 0.25
    counts, hits = B.ref_select(A, [3, 7], ids, np.nextafter(np.float32(0.25), np.float32(1)))
    assert counts.tolist() == [2, 0] and hits[0][1].tolist() == [0.5, 2.0]
    counts, hits = B.ref_select(A, None, None, 0.25)
    off, total = B.ref_offsets(counts)
    assert off.tolist() == [0, 2, 4] and total == 4                                     # (0, 0) and (1, 1) are their own
    i, v = B.ref_emit(hits, off, 3, np.full(6, -7, dtype=np.int32), np.full(6, 9.0, dtype=np.float32))
    assert i.tolist() == [2, 4, 0, -7, -7, -7] and v.tolist() == [0.5, 2.0, 0.25, 9.0, 9.0, 9.0]


def test_pack_reference_on_a_hand_made_block():
    src = B.make_block(B.PANEL_F32, 3, 40, 5, 2, kind="wide")
    fill = np.frombuffer(bytes([B.PACK_FILL]) * (4 * 4 * 8), dtype=np.float32)
    out, over = B.ref_pack(src, B.ROWMAJOR_F32, 8, 4, 6, [2, 0, 9, 1], [5, 0, 7, 3], [39, 1, 2, 40], 4, fill)
    got = out.reshape(4, 8)
    assert over == 0
    assert np.array_equal(got[0, [5, 0]], src.A[2, [39, 1]].astype(np.float32))         # col_dst 7 and col_src 40: skipped
    assert np.array_equal(got[3, [5, 0]], src.A[1, [39, 1]].astype(np.float32))
    untouched = np.ones((4, 8), dtype=bool)
    untouched[[0, 0, 1, 1, 3, 3], [5, 0, 5, 0, 5, 0]] = False
    assert (B.bits(got)[untouched] == 0xA5A5A5A5).all()                                 # row 2 (row_map 9) too
    over_src = B.make_block(B.ROWMAJOR_F32, 70, 129, 129, 1, kind="wide", overflow=5)
    fill16 = np.frombuffer(bytes([B.PACK_FILL]) * (2 * B.n_elems(B.PANEL_F16, 70, 129, 72)), dtype=np.float16)
    out, over = B.ref_pack(over_src, B.PANEL_F16, 72, 70, 129, None, None, None, 129, fill16)
    assert over == 5
    assert np.array_equal(B.bits(out[B.offsets(B.PANEL_F16, 70, 129, 72)]), B.bits(B.narrow(over_src.A)))


def test_score_reference_is_the_sets_statement():
    from tests import sets_ref
    blk = B.make_block(B.ROWMAJOR_F64, 9, 63, 64, 2, kind="wide")
    ptr, pos, w = np.array([0, 0, 3, 5]), np.array([1, 8, 1, 9, 2]), np.array([0.5, -3.0, 1e-7, 1.0, 2.0])
    out = B.ref_score(blk.A, None, 63, ptr, pos, w, np.array([0, 1, 1, 3]), np.array([5, 0, 62]))
    want = sets_ref.scores(blk.A, [[], [1, 8, 1]], [[], w[:3]])
    assert out[0, 5] == -np.inf and (np.delete(out[0], 5) == 0).all()
    assert np.array_equal(B.bits(out[1]), B.bits(want[1]))
    assert np.isnan(np.delete(out[2], [0, 62])).all() and out[2, 0] == out[2, 62] == -np.inf
    perm = np.arange(63)[::-1].copy()
    perm[4] = 63
    mapped = B.ref_score(blk.A, perm, 63, ptr, pos, w, None, None)
    assert np.isnan(mapped[1, 4]) and np.array_equal(B.bits(np.delete(mapped[1], 4)), B.bits(np.delete(want[1][::-1], 4)))


# ---- why the fold-in may be held to bit equality ----------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_dyadic_gather_is_order_free_and_exact_in_f32(layout):
    for (n_rows, n_cols), n_tile in zip([(70, 129), (9, 257), (7, 31), (8, 33)], [32, 31, 5, 1]):
        stride = B.variants(layout, n_rows, n_cols)[0][1]
        blk = B.make_block(layout, n_rows, n_cols, stride, 11, kind="dyadic")
        ptr, pos, w = B.gather_case(n_rows, n_tile, 11)
        assert (np.diff(ptr) == 0).any() or n_tile == 1
        assert set(np.log2(w[w > 0]) % 1) == {0.0}
        n_src = n_cols + 6
        ids = np.random.default_rng(1).permutation(n_src)[:n_cols]
        for t_dtype in (np.float32, np.float64):
            T0 = np.full((n_src, B.TILE), 77.0, dtype=t_dtype)
            want = B.ref_gather(blk.A, layout, ids, 0, ptr, pos, w, n_tile, T0, acc=np.float64)
            for kw in (dict(acc=np.float32), dict(acc=np.float32, reverse=True), dict(acc=np.float64, reverse=True)):
                got = B.ref_gather(blk.A, layout, ids, 0, ptr, pos, w, n_tile, T0, **kw)
                assert np.array_equal(B.bits(got), B.bits(want)), (layout, n_tile, kw)
            assert np.array_equal(want.astype(np.float64), B.ref_gather(blk.A, layout, ids, 0, ptr, pos, w, n_tile,
                                                                        T0.astype(np.float64), acc=np.float64))
            untouched = np.setdiff1d(np.arange(n_src), ids)
            assert (want[untouched] == 77.0).all() and (want[ids][:, n_tile:] == 0).all()
            # exact: the float64 sums are integers of 2^-10 steps, far below 2^24 of them
            dense = np.zeros((n_tile, n_rows))
            for q in range(n_tile):
                np.add.at(dense[q], pos[ptr[q]:ptr[q + 1]], 1.0)
            assert np.array_equal(want[ids][:, :n_tile].astype(np.float64), (dense @ blk.A).T * w[None, :])
    member = B.ref_member(ptr, pos, w, n_tile, n_rows)
    assert member.dtype == np.uint32 and member.max() <= 1


@pytest.mark.parametrize("t_dtype", [np.float32, np.float64])
def test_dyadic_apply_is_order_free_and_contraction_free(t_dtype):
    c = B.apply_case(t_dtype)
    assert sorted(set(c["lens"]) & set(B.APPLY_ROWS)) == B.APPLY_ROWS and c["n_out"] > 32
    assert c["long_rows"].size == 2 and (c["scale"] == 0).sum() == 1
    n_tile = 32
    out0 = np.full((n_tile + 1, c["n_out"] + 3), -55.0)
    for member in (c["member"], None):
        for prior in (c["prior"], None):
            args = (c["rowptr"], c["col"], c["scale"], c["T"], member, c["coef"], c["lbd"], prior, n_tile, out0)
            want = B.ref_apply(*args, acc=np.float64)
            for kw in (dict(acc=np.float32), dict(acc=np.float32, reverse=True), dict(acc=np.float64, reverse=True),
                       dict(fused="head"), dict(fused="prior")):
                got = B.ref_apply(*args, **kw)
                assert np.array_equal(B.bits(got), B.bits(want)), (member is None, prior is None, kw)
            assert (want[n_tile] == -55.0).all() and (want[:, c["n_out"]:] == -55.0).all()
            assert np.isfinite(want).all() and (want[:n_tile, :c["n_out"]] != 0).mean() > 0.5
    # the counts of new node 3 are the row lengths: 255 is reached and passed, and both saturate to E = 1
    cnt3 = np.array([sum((int(c["member"][j]) >> 3) & 1 for j in c["col"][c["rowptr"][b]:c["rowptr"][b + 1]])
                     for b in range(c["n_out"])])
    assert cnt3.tolist() == c["lens"] and 255 in cnt3 and cnt3.max() == 600
    # one dropped partial sum or one evidence count off shows in the bits
    assert B.finish(1.0, 3, 1.0, 0.75, 0.25, True, None) != B.finish(1.0, 4, 1.0, 0.75, 0.25, True, None)
    assert B.finish(1.0, 254, 1.0, 0.75, 0.25, True, None) == B.finish(1.0, 255, 1.0, 0.75, 0.25, True, None) == 0.5625
    assert B.finish(2.5, 9, 0.0, 0.75, 0.25, True, 8.0) == 2.0
