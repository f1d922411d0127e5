"""libsimrank_hdbscan.so past 2^31 and 2^32 elements, in the geometries and the arena of tests/far.py, whose every other
byte is a filler that is finite and above every value.

The count sweep takes a SQUARE block, as ``test_gpu_far_density`` places it: the row-major layouts at n = 70 (rows 32 and
64 start past 2^31 and 2^32 elements), the panel layouts at n = 1100 (the later panels start past them).  A 32-bit
offset in the tile-pair addressing, of tile (I, J) or of its partner (J, I), reads the filler, which is above every
value: the largest pair height of a node is then the filler and no longer ``hdbscan_ref``'s.

The clamped pick takes the 70 x 1100 block of ``test_gpu_far_linkage``: an offset narrowed to 32 bits reads the filler,
a weight that only the two core similarities still clamp, and the canonical rows change.  Every layout, with ids and
without."""
import numpy as np
import pytest

from tests import blocks as B
from tests import far as F
from tests import linkage_ref as LR
from tests.test_gpu_cluster import id_cases as block_ids
from tests.test_gpu_density import id_cases
from tests.test_gpu_far_blocks import arena, dev, device, far_blocks  # noqa: F401 (fixtures)
from tests.test_gpu_far_density import far_size, square
from tests.test_gpu_hdbscan import check, cmp_type, forest
from tests.test_gpu_linkage import rows_of, same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_the_count_sweeps(dev, arena, layout):  # noqa: F811
    n = far_size(layout)
    arena.fill(layout)
    top = B.widen(layout, F.filler(layout))[0]
    for i, g in enumerate(F.geometries(layout)):
        for kind in ("dyadic", "wide") if n < 100 else ("dyadic",):
            blk = square(layout, kind)
            S = arena.place(g, blk.A, blk.sentinel)
            for ids in id_cases(n, np.random.default_rng([i, layout, 13])):
                got = check(dev, S, layout, g.stride, n, ids, blk.A, [1, 4], (layout, g.tag, kind, ids is None))
                assert np.isfinite(got[1]).any() and np.nanmax(got[1][np.isfinite(got[1])]) < top      # the filler would win
            arena.clear()
            dev.release()


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_the_clamped_pick(dev, arena, layout):  # noqa: F811
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        A, rng = blk.A, np.random.default_rng([i, layout, 17])
        for n, row_ids, col_ids in block_ids(n_rows, n_cols, rng):
            # any clamp serves: values of the block's upper half, and a few nodes at +inf and at -inf
            upper = np.sort(A[~np.isnan(A)])[A.size // 2:]
            core = rng.choice(upper, size=n)
            core[rng.integers(0, n, size=n // 8)] = np.inf
            core[rng.integers(0, n, size=n // 16)] = -np.inf
            a, b, v = LR.block_edges(A, row_ids, col_ids, n)
            v = np.minimum(v, np.minimum(core[a], core[b]))
            keep = ~np.isneginf(v)
            want = LR.rows_of_edges(n, a[keep], b[keep], v[keep])
            block = (S, g.stride, n_rows, n_cols, None if row_ids is None else dev.put(row_ids),
                     None if col_ids is None else dev.put(col_ids))
            core_dev = dev.put(core.astype(cmp_type(layout)))
            got = rows_of(n, *forest(dev, [block], n, layout, core_dev))
            assert same(got, want), (what, row_ids is None)
            assert len(want[0]) > 0 and want[2][0] < B.widen(layout, F.filler(layout))[0]
            assert not same(want, LR.rows_of_edges(n, a, b, LR.block_edges(A, row_ids, col_ids, n)[2]))    # the clamp matters
        dev.release()
