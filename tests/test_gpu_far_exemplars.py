"""libsimrank_exemplars.so past 2^31 and 2^32 elements: ``simrank_exemplars_gains`` and ``simrank_exemplars_cover`` on the
70 x 1100 block of tests/far.py in its four far geometries, in the arena of tests/test_gpu_far_blocks.py, whose every
other byte is a filler that is finite and above every value.  ``gains`` addresses the block at three sites (the vector
load of a quad, the single element, ``cover + c``) and ``cover`` at one; an element offset narrowed to 32 bits reads the
filler, which lies above every cover used here (asserted: tests/far_cases.py) and so changes every gain, raises every
cover and counts.  tests/test_far_cpu.py evaluates the same references on the narrowed matrix and shows that they differ.

The rows name both sides of every boundary, the last row, a row twice and rows outside; the gains are compared bit for
bit with ``exemplars_ref.exact_sum`` on the dyadic block and with ``ordered_sum`` (inside the header's bound) on the wide
one, the cover bit for bit and the counters exactly with ``block_cover``; every call runs twice.  ``cover`` and ``gain``
are also placed in the arena, 2^34 bytes and 1 MiB in, and read back at their live parts and margins."""
import numpy as np
import pytest

from simrank_amd import _exemplars
from tests import blocks as B
from tests import exemplars_ref as ER
from tests import far as F
from tests import far_cases as FC
from tests.test_gpu_companion_blocks import same_bits
from tests.test_gpu_exemplars import GUARD_F64, GUARD_U32, run_cover, run_gains, want_gains
from tests.test_gpu_far_blocks import FAR_OUTPUTS, arena, dev, device, far_blocks  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

FAR_AT = FAR_OUTPUTS[0][2]                          # 2^34 bytes + 1 MiB into the arena
MARGIN = 16                                         # bytes read back on either side of a far vector


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_gains(dev, arena, layout):  # noqa: F811
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        kind = what[2]
        assert i == FC.counter(g, kind)
        inp = FC.exemplar_inputs(blk, i)
        want, _ = FC.exemplar_outputs(blk.A, inp)
        for name, c in inp["covers"].items():
            # (the "offset" geometry also moves the cover off 16 bytes: the element-by-element path reads it)
            cover_dev = dev.put(np.append(c, GUARD_F64), 8 if g.tag == "offset" else 0)
            for rows in inp["gain_rows"]:
                w = want[(name, rows is None)]
                same_bits(w, want_gains(blk.A, rows, c, kind), "the shared reference is the block test's")
                got = run_gains(dev, S, layout, g.stride, n_rows, n_cols, rows, cover_dev)
                same_bits(got, np.append(w, GUARD_F64), (what, name, rows is None))
                again = run_gains(dev, S, layout, g.stride, n_rows, n_cols, rows, cover_dev)
                assert np.array_equal(B.bits(got), B.bits(again)), (what, name)
            same_bits(dev.get(cover_dev, np.append(c, GUARD_F64)), np.append(c, GUARD_F64), (what, name, "cover"))
        assert want[("a row", True)][inp["r0"]] == 0.0 and np.isnan(want[("zeros", False)]).sum() == 3
        assert (want[("mixed", True)][list(F.EDGE_ROWS)] > 0).all()          # the far rows gain
        dev.release()


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_cover(dev, arena, layout):  # noqa: F811
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        inp = FC.exemplar_inputs(blk, i)
        _, want = FC.exemplar_outputs(blk.A, inp)
        for (rows, start, first), (want_c, want_r) in zip(inp["cover_runs"], want):
            label = (what, rows.tolist(), start)
            got_c, got_r = run_cover(dev, S, layout, g.stride, n_rows, n_cols, rows, inp["covers"][start], first)
            same_bits(got_c, np.append(want_c, GUARD_F64), label + ("cover",))
            assert got_r.tolist() == want_r.tolist() + [GUARD_U32], label
            again_c, again_r = run_cover(dev, S, layout, g.stride, n_rows, n_cols, rows, inp["covers"][start], first)
            assert np.array_equal(B.bits(got_c), B.bits(again_c)) and np.array_equal(got_r, again_r), label
            assert (want_r - first).sum() > 0 and (first > 0).all()
        dev.release()


def far_vector(arena, dev, at, host):  # noqa: F811
    """``host`` (its last element a guard word) at the device address ``at`` in the arena -> how to read it back with
    MARGIN bytes of the arena's filler on either side."""
    arena.write(at, host.tobytes())
    arena.touch(at - MARGIN, MARGIN)
    arena.touch(at + host.nbytes, MARGIN)

    def read():
        raw = np.empty(host.nbytes + 2 * MARGIN, dtype=np.uint8)
        dev.ops.d2h(raw, at - MARGIN)
        dev.ops.synchronize()
        return raw
    return read


def with_margins(arena, host):  # noqa: F811
    pad = F.filler(arena.filled, MARGIN // F.itemsize(arena.filled)).view(np.uint8)
    return np.concatenate([pad, np.ascontiguousarray(host).view(np.uint8), pad])


@pytest.mark.parametrize("layout", [B.PANEL_F32, B.ROWMAJOR_F32])
def test_cover_and_gain_placed_far(dev, arena, layout):  # noqa: F811
    """``cover`` (read by gains, written by cover) and ``gain``, each in its turn 2^34 bytes + 1 MiB into the arena, where
    the first far output of tests/test_gpu_far_blocks.py starts; the other one lies near.  Read back: the vector, its
    guard word and 16 bytes of the arena on either side."""
    lib, st = _exemplars.load(), dev.ops.stream
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    at = arena.ptr + FAR_AT
    assert FAR_AT % 16 == 0 and FAR_AT + 8 * (n_cols + 1) + MARGIN <= F.ARENA
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout, kinds=("dyadic",))):
        if g.tag == "crooked":
            continue
        inp = FC.exemplar_inputs(blk, FC.counter(g, "dyadic"))
        rows, c = inp["gain_rows"][1], inp["covers"]["mixed"]
        want = ER.block_gains(blk.A, rows, c, total=ER.exact_sum)
        rows_dev = dev.put(rows.astype(np.int32))
        # ---- gain far, cover near ----
        gain_h = np.full(rows.size + 1, GUARD_F64)
        read = far_vector(arena, dev, at, gain_h)
        _exemplars.check(lib.simrank_exemplars_gains(S, layout, g.stride, n_rows, n_cols, rows_dev, rows.size, dev.put(c), at,
                                                     st), "gains")
        got = read()
        want_raw = with_margins(arena, np.append(want, GUARD_F64))
        nan = np.isnan(np.append(want, GUARD_F64))
        same_bits(np.isnan(got[MARGIN:-MARGIN].view(np.float64)), nan, (what, "far gain: NaN"))
        keep = np.repeat(np.concatenate([[True] * (MARGIN // 8), ~nan, [True] * (MARGIN // 8)]), 8)
        same_bits(got[keep], want_raw[keep], (what, "far gain"))
        arena.clear()
        S = arena.place(g, blk.A, blk.sentinel)                             # (clear put the filler over the block too)
        # ---- cover far: read by gains, then written by cover ----
        cover_h = np.append(c, GUARD_F64)
        read = far_vector(arena, dev, at, cover_h)
        near = run_gains(dev, S, layout, g.stride, n_rows, n_cols, rows, at)
        same_bits(near, np.append(want, GUARD_F64), (what, "gains of a far cover"))
        same_bits(read(), with_margins(arena, cover_h), (what, "far cover after gains"))
        run_rows, _, first = inp["cover_runs"][2]
        want_c, want_r = ER.block_cover(blk.A, run_rows, c, first)
        raised_h = np.append(first.astype(np.uint32), np.uint32(GUARD_U32))
        raised = dev.put(raised_h)
        _exemplars.check(lib.simrank_exemplars_cover(S, layout, g.stride, n_rows, n_cols, dev.put(run_rows.astype(np.int32)),
                                                     run_rows.size, at, raised, st), "cover")
        same_bits(read(), with_margins(arena, np.append(want_c, GUARD_F64)), (what, "far cover"))
        assert dev.get(raised, raised_h).tolist() == want_r.tolist() + [GUARD_U32], what
        assert (want_r - first).sum() > 0
        dev.release()
