"""libsimrank_density.so past 2^31 and 2^32 elements, in the geometries and the arena of tests/far.py, whose every other
byte is a filler that is finite and above every value.  The degrees sweep takes a SQUARE block: the row-major layouts at
n = 70 (rows 32 and 64 start past 2^31 and 2^32 elements), the panel layouts at n = 1100 (18 and 35 panels: the later
ones start past 2^31 and 2^32).  A 32-bit offset in the tile-pair addressing, of tile (I, J) or of its partner (J, I),
reads the filler, which passes every threshold: the counts, the core flags and the roots no longer equal
``density_ref``'s.  Every layout, with ids and without."""
import functools

import numpy as np
import pytest

from tests import blocks as B
from tests import far as F
from tests.test_gpu_density import check, id_cases, levels_of
from tests.test_gpu_far_blocks import arena, dev, device  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


def far_size(layout):
    return 1100 if layout in B.PANEL else F.N_ROWS


@functools.lru_cache(maxsize=None)
def square(layout, kind):
    """The n x n block of (layout, kind) at a small stride: its ``A`` and sentinel are those of every far geometry."""
    n = far_size(layout)
    stride = n + 3 if layout in B.PANEL else n + 4
    return B.make_block(layout, n, n, stride, 7, kind=kind, zero_fraction=0.04 if n < 100 else 0.002)


def test_the_far_geometry_of_a_square_block():
    """What the test below relies on: the block's last rows (panels) lie past 2^31 and 2^32 elements and inside the arena."""
    for g in F.ALL:
        n = far_size(g.layout)
        at = F.live_offsets(g, n, n)
        assert (at < 2 ** 31).any() and ((at >= 2 ** 31) & (at < 2 ** 32)).any()
        assert at.max() >= 2 ** 32 or g.layout == B.ROWMAJOR_F64           # (float64: 2^31 elements are 2^34 bytes)
        assert g.base + F.extent(g, n, n) <= F.HALF


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_degrees_union_labels(dev, arena, layout):  # noqa: F811
    n = far_size(layout)
    arena.fill(layout)
    for i, g in enumerate(F.geometries(layout)):
        for kind in ("dyadic", "wide") if n < 100 else ("dyadic",):
            blk = square(layout, kind)
            A = blk.A
            S = arena.place(g, A, blk.sentinel)
            ts = levels_of(A)
            assert max(ts) < B.widen(layout, F.filler(layout))[0]          # the filler passes every level
            if n >= 100:                                                    # clusters where the graph is sparse: 2 and 5 neighbours a node
                v = np.sort(A[~np.eye(n, dtype=bool)])
                ts[0], ts[4] = float(v[-n]), float(v[-(5 * n) // 2])
            for ids in id_cases(n, np.random.default_rng([i, layout, 11])):
                check(dev, S, layout, g.stride, n, ids, A, ts, (0, 4), (layout, g.tag, kind, ids is None))
            arena.clear()
            dev.release()
