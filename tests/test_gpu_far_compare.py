"""libsimrank_compare.so past 2^31 and 2^32 elements: the 70 x 1100 block of tests/far.py in far geometries, in the arena
of tests/test_gpu_far_blocks.py, whose every other byte is a filler that is finite and above every value.  Both sides of
a pair live in the ONE arena: B starts a little before A (2048 columns before a row-major A, 1024 rows before a panel A),
in the gaps the far stride leaves, so an element offset of either side narrowed to 32 bits, sign-wrapped or
zero-extended, still lands in the arena and reads the filler (or another row), which is no value of either block: the
differences change, and the comparison, bit for bit against tests/compare_ref.py, fails.  Row-major f32 in its three
geometries (vector path, scalar path, a base 4 bytes in: rows past 2^31 and 2^32 elements, where the rows of a compact
f32 model of N = 65536 lie) and the binary16 panels (panel 8 starts at 2^31 elements, panel 16 at 2^32)."""
import numpy as np
import pytest

from tests import blocks as B
from tests import compare_ref as R
from tests import far as F
from tests.test_gpu_compare import NAMES, TOLS, cast, expected, pair, run_sweep
from tests.test_gpu_companion_blocks import same_bits
from tests.test_gpu_far_blocks import arena, dev, device  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

# bytes B starts before A: 2048 f32 columns of a row (the row's 1100 live columns and margins end before), or 1024 rows of
# a binary16 panel (its 70 rows and 8 guard rows end before); both keep the alignment of A's base
BEFORE = {B.ROWMAJOR_F32: 2048 * 4, B.PANEL_F16: 1024 * 64 * 2}


@pytest.mark.parametrize("layout", [B.ROWMAJOR_F32, B.PANEL_F16])
def test_sweep_of_two_far_blocks(dev, arena, layout):  # noqa: F811
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    MA, MB, twice_row = pair(layout, layout, n_rows, n_cols, 0)
    A, Bm = B.widen(layout, MA), B.widen(layout, MB)
    floor = 2.0 ** -20
    refs = {n_tol: R.sweep(A, Bm, TOLS[n_tol], floor) for n_tol in (0, 8)}
    d = R.distance(A, Bm)
    assert refs[8][5].sum() == n_rows * n_cols
    differs = np.flatnonzero((d > 0).any(axis=1))
    assert set(F.EDGE_ROWS) <= set(differs.tolist())                     # rows on each side of 2^31 and 2^32 elements say something
    # What a narrowed offset changes.  On one side alone: the filler is no value of either block, so an element that
    # agrees (most do) would differ.  On both sides alike: filler against filler agrees, so an element that differs would
    # not.  Both kinds lie past 2^31 and past 2^32 elements: rows 32 .. 63 and 64 .. of a row-major block, columns 512 ..
    # 1023 and 1024 .. of the binary16 panels.
    filler = float(B.widen(layout, F.filler(layout))[0])
    assert not (A == filler).any() and not (Bm == filler).any()
    for far in ([d[32:64], d[64:]] if layout == B.ROWMAJOR_F32 else [d[:, 512:1024], d[:, 1024:]]):
        assert (far > 0).any() and (far == 0).any()
    pad = cast(layout, B.SENTINEL[(layout, "wide")])
    arena.fill(layout)
    for g in F.geometries(layout):
        SA = arena.base + g.base
        SB = SA - BEFORE[layout]
        for S, M in ((SA, MA), (SB, MB)):
            for off, raw in F.stored_pieces(g, M, pad):
                arena.write(S + off, raw)
        for n_tol in (8, 0):
            got = run_sweep(dev, SA, layout, g.stride, SB, layout, g.stride, n_rows, n_cols, TOLS[n_tol], floor)
            for x, w, name in zip(got, expected(refs[n_tol], n_rows, n_tol), NAMES):
                same_bits(x, w, (layout, g.tag, n_tol, name))
        arena.clear()
        dev.release()
