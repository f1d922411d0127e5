"""tests/far.py without a device: the far geometries reach the offsets their table states, the scatter plan stays inside
the arena and does not overlap, the filler beats every value of every block, and at a small stride the plan applied to a
filler-filled host buffer is ``blocks.encode`` wherever the plan wrote.  And the inputs of the exemplars and candidates
far tests (tests/far_cases.py) are sensitive: evaluated on the matrix a narrowed address would read, their references
give other gains, another cover and other top-k ids."""
import numpy as np
import pytest

from tests import blocks as B
from tests import far as F
from tests import far_cases as FC

KINDS = ("dyadic", "wide")
P31, P32 = 1 << 31, 1 << 32


def first_at(values, bound):
    """Index of the first entry >= bound (entries ascend)."""
    return int(np.searchsorted(np.asarray(values, dtype=np.int64), bound, side="left"))


@pytest.mark.parametrize("g", F.ALL, ids=lambda g: f"{g.layout}-{g.tag}")
def test_offsets_fall_on_the_stated_sides(g):
    off = F.live_offsets(g)
    assert off.dtype == np.int64 and off.min() == 0
    size = F.itemsize(g.layout)
    if g.layout in B.PANEL:
        w = B.PANEL[g.layout]
        starts = off[0, ::w]                                            # where each panel starts
        assert starts.size == {B.PANEL_F32: 35, B.PANEL_F16: 18}[g.layout]
        want31, want32 = {B.PANEL_F32: (16, 32), B.PANEL_F16: (8, 16)}[g.layout]
        assert first_at(starts, P31) == want31 and starts[want31] == P31
        assert first_at(starts, P32) == want32 and starts[want32] == P32
        ends = off[-1, w - 1::w]                                        # the last live element of each whole panel
        assert ends[want31 - 1] < P31 and ends[want32 - 1] < P32
        assert off.max() >= P32                                         # live values past 2^32 elements
        assert off.max() * size >= (1 << 33)
    else:
        starts, ends = off[:, 0], off[:, -1]
        if g.layout == B.ROWMAJOR_F32:
            assert first_at(starts, P31) == 32 and ends[31] < P31
            assert first_at(starts, P32) == 64 and ends[63] < P32
            assert off.max() >= P32
        else:
            assert first_at(starts, P31) == 64 and ends[63] < P31
            assert starts[64] * size >= (1 << 34) and ends[63] * size < (1 << 34)
            assert off.max() < P32
    # bytes: values on both sides of 2^32 bytes in every geometry
    assert (off * size < P32).any() and (off * size >= P32).any()
    # the rows and columns the GPU tests name lie on both sides of every boundary that exists
    edge = off[np.ix_(F.EDGE_ROWS, F.EDGE_COLS)]
    for bound in (P31, P32):
        if off.max() >= bound:
            assert (edge < bound).any() and (edge >= bound).any()
    assert edge.max() == off.max()                                      # the last row and column


@pytest.mark.parametrize("g", F.ALL, ids=lambda g: f"{g.layout}-{g.tag}")
def test_the_plan_stays_inside_the_arena(g):
    blk = F.block(g.layout, "dyadic")
    plan = F.pieces(g, blk.A, blk.sentinel)
    E = F.extent(g)
    assert len(plan) == (-(-F.N_COLS // B.PANEL[g.layout]) if g.layout in B.PANEL else F.N_ROWS)
    end = 0
    for at, raw in plan:
        assert at >= end and at + len(raw) <= E                        # ascending, disjoint, inside [0, E)
        end = at + len(raw)
    if g.layout in B.PANEL:
        assert all(len(raw) == (F.N_ROWS + F.GUARD_ROWS) * 128 for _, raw in plan) and plan[1][0] % 16 == 0
    else:
        size = F.itemsize(g.layout)
        assert len(plan[0][1]) == F.N_COLS * size + F.MARGIN and all(len(raw) == F.N_COLS * size + 2 * F.MARGIN for _, raw in plan[1:])
    # the base in the middle: a sign-wrapped offset (down to -2^31 elements) and a zero-extended one stay inside
    base = F.HALF + g.base
    assert base - F.HALF >= 0 and base + E <= F.ARENA and F.ARENA == 2 * F.HALF
    size = F.itemsize(g.layout)
    off = F.live_offsets(g)
    wrapped = off.astype(np.int32).astype(np.int64)                     # what an int32 keeps of the offset
    zero_extended = off & (P32 - 1)                                     # what a uint32 keeps
    for o in (wrapped, zero_extended):
        assert (base + o * size >= 0).all() and (base + (o + 1) * size <= F.ARENA).all()
    assert (wrapped != off).any()                                       # and narrowing does move some element
    assert F.ARENA + F.HEADROOM < 48 << 30


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_the_filler_is_finite_and_above_every_value(layout):
    fill = B.widen(layout, F.filler(layout, 4))
    assert np.isfinite(fill).all() and (fill == fill[0]).all()
    for kind in KINDS:
        blk = F.block(layout, kind)
        assert blk.A.shape == (F.N_ROWS, F.N_COLS) and np.isfinite(blk.A).all()
        assert fill[0] > blk.A.max() and fill[0] > np.abs(blk.A).max() and fill[0] >= blk.sentinel
    raw = F.filler(layout, 16 // F.itemsize(layout)).tobytes()
    assert len(raw) == 16 and raw * 2 == F.filler(layout, 32 // F.itemsize(layout)).tobytes()


@pytest.mark.parametrize("layout", B.LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_plan_reproduces_encode_at_a_small_stride(layout, kind):
    blk = F.block(layout, kind)
    small = F.N_ROWS + 11 if layout in B.PANEL else F.N_COLS + 40
    for g in F.geometries(layout, small):
        want = B.encode(layout, blk.A, g.stride, blk.sentinel)
        buf = F.filler(layout, want.size)
        raw, wrote = buf.view(np.uint8), np.zeros(buf.nbytes, dtype=bool)
        for at, piece in F.pieces(g, blk.A, blk.sentinel):
            assert not wrote[at:at + len(piece)].any()
            raw[at:at + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
            wrote[at:at + len(piece)] = True
        live = F.live_offsets(g).ravel()
        elem = wrote.reshape(-1, F.itemsize(layout)).all(axis=1)
        assert elem[live].all()                                         # every live element was written
        assert np.array_equal(B.bits(buf[elem]), B.bits(want[elem]))    # values and margins are encode's
        margins = elem.copy()
        margins[live] = False
        assert margins.sum() >= (F.N_ROWS if layout not in B.PANEL else 0) and \
            (B.bits(buf[margins]) == B.bits(B.store(layout, blk.sentinel).reshape(1))[0]).all()
        assert np.array_equal(B.bits(buf[~elem]), B.bits(F.filler(layout, int((~elem).sum()))))
        assert np.array_equal(B.bits(B.decode(layout, buf, F.N_ROWS, F.N_COLS, g.stride)), B.bits(blk.A))


# ---- the far exemplars and candidates tests could fail -----------------------------------------------------------------------
def differ(a, b):
    return not np.array_equal(B.bits(np.asarray(a)), B.bits(np.asarray(b)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("g", F.ALL, ids=lambda g: f"{g.layout}-{g.tag}")
def test_a_narrowed_address_changes_what_the_far_tests_expect(g, kind):
    """The references of tests/test_gpu_far_exemplars.py and tests/test_gpu_far_candidates.py on the rows, lists, covers
    and k those tests use, on ``A`` and on ``A'``: an element whose offset changes when cut to int32 or to uint32 holds
    the widened filler.  Wherever narrowing moves an element, the gains (for every cover, with and without a list), the
    cover and the counters of every run, and the ids of every top-k differ."""
    blk = F.block(g.layout, kind)
    i = FC.counter(g, kind)
    ex, ca = FC.exemplar_inputs(blk, i), FC.candidate_inputs(blk, i)
    gains, covers = FC.exemplar_outputs(blk.A, ex)
    topk = FC.candidate_outputs(blk.A, ca)
    for bits in ("int32", "uint32"):
        A2, moved = FC.narrowed(g, blk.A, bits)
        if bits == "uint32" and g.layout == B.ROWMAJOR_F64:
            assert moved == 0 and F.live_offsets(g).max() < P32           # it stays below 2^32 elements
            continue
        assert moved > 0
        gains2, covers2 = FC.exemplar_outputs(A2, ex)
        for key in gains:
            assert differ(gains[key], gains2[key]), (bits, "gains", key)
        for run, (c, r), (c2, r2) in zip(ex["cover_runs"], covers, covers2):
            assert differ(c, c2) and differ(r, r2), (bits, "cover", run[0].tolist())
        for run, (idx, _), (idx2, _) in zip(ca["runs"], topk, FC.candidate_outputs(A2, ca)):
            assert differ(idx, idx2), (bits, "top-k ids", run[0], run[2] is None, run[4])


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_the_long_lists_tie_at_rank_k(layout):
    """Every run of a not-staged list has, in every geometry, a row whose values at ranks k and k + 1 of the full order
    are equal: the index passes of the selection decide."""
    for g in F.geometries(layout):
        for kind in KINDS:
            blk = F.block(layout, kind)
            inp = FC.candidate_inputs(blk, FC.counter(g, kind))
            long = [run for run in inp["runs"] if run[0] == "long"]
            assert len(long) == 2 * len(FC.LONG_KS) and all(run[1].size == FC.STAGED[layout] + 1 for run in long)
            for run in long:
                assert set(F.EDGE_COLS) <= set(run[1][F.N_COLS:].tolist())
                assert FC.ties_at_k(blk.A, inp, run) >= 1, (g.tag, kind, run[2] is None, run[4])
