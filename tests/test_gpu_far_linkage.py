"""libsimrank_linkage.so past 2^31 and 2^32 elements: the 70 x 1100 block of tests/far.py in its four far geometries, in
the arena of tests/test_gpu_far_blocks.py, whose every other byte is a filler that is finite and above every value.  An
element offset narrowed to 32 bits reads the filler (or another row): a weight above every real one, which changes the
first merge, and the canonical rows no longer equal ``linkage_ref``'s.  Every layout, with id arrays and without."""
import numpy as np
import pytest

from simrank_amd import _linkage
from tests import blocks as B
from tests import far as F
from tests import linkage_ref as LR
from tests.test_gpu_cluster import id_cases
from tests.test_gpu_far_blocks import arena, dev, device, far_blocks  # noqa: F401 (fixtures)
from tests.test_gpu_linkage import check_forest, same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_linkage_pick(dev, arena, layout):  # noqa: F811
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        A, rng = blk.A, np.random.default_rng([i, layout, 11])
        for n, row_ids, col_ids in id_cases(n_rows, n_cols, rng):
            block = (S, g.stride, n_rows, n_cols, None if row_ids is None else dev.put(row_ids),
                     None if col_ids is None else dev.put(col_ids))
            want = LR.rows_of_edges(n, *LR.block_edges(A, row_ids, col_ids, n))
            check_forest(dev, [block], n, layout, want, (what, row_ids is None))
            # the first merge is at the block's largest value between two nodes, below the filler
            assert want[2][0] < B.widen(layout, F.filler(layout))[0] and want[2][0] == np.nanmax(LR.block_edges(A, row_ids, col_ids, n)[2])
            b = dict(ptr=S, layout=layout, stride=g.stride, rows=n_rows, cols=n_cols, row_ids=block[4], col_ids=block[5])
            a2, b2, v2, _ = _linkage.forest_blocks(dev.ops, [b], n, None)
            assert same(_linkage.canonical(n, a2, b2, v2), want), what
        dev.release()
