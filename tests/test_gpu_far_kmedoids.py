"""libsimrank_kmedoids.so past 2^31 and 2^32 elements: ``simrank_kmedoids_assign`` on the 70 x 1100 block of tests/far.py in
its four far geometries, in the arena of tests/test_gpu_far_blocks.py, whose every other byte is a filler that is finite
and above every value.  The medoid rows include ``far.EDGE_ROWS``: rows that start past 2^31 and 2^32 elements.  An
element offset narrowed to 32 bits reads the filler, which wins every column it enters: the comparison with
``kmedoids_ref.block_assign``, bit for bit on the dyadic and on the wide block (nothing is added), fails."""
import numpy as np
import pytest

from tests import blocks as B
from tests import far as F
from tests import kmedoids_ref as KR
from tests.test_gpu_far_blocks import arena, dev, device, far_blocks  # noqa: F401 (fixtures)
from tests.test_gpu_kmedoids import check_assign, currents_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_kmedoids_assign(dev, arena, layout):  # noqa: F811
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    filler = float(B.widen(layout, F.filler(layout))[0])
    rng = np.random.default_rng([layout, 29])                              # (the same medoids for every geometry)
    # every edge row, one of them twice, a row outside, and seven more; the edge rows' own columns are edge columns
    med_row = np.array(list(F.EDGE_ROWS) + [F.EDGE_ROWS[3], n_rows] + rng.integers(0, n_rows, size=7).tolist(), dtype=np.int32)
    med_col = np.full(med_row.size, -1, dtype=np.int32)
    med_col[:len(F.EDGE_COLS)] = F.EDGE_COLS
    k = med_row.size
    refs = {}
    for blk, g, S, what in far_blocks(arena, layout):
        A, kind = blk.A, what[2]
        assert np.isfinite(filler) and filler > A.max()                     # a filler that entered a column would win it
        if kind not in refs:
            first = KR.block_assign(A, med_row, med_col)
            current = currents_of(np.random.default_rng([layout, 31]), first[0], k)
            refs[kind] = (first, current, KR.block_assign(A, med_row, med_col, current))
            assert len(set(first[0].tolist())) >= len(F.EDGE_ROWS)           # the far rows win columns of their own
        first, current, second = refs[kind]
        check_assign(dev, S, layout, g.stride, A, med_row, med_col, None, first, what, moved=0)
        check_assign(dev, S, layout, g.stride, A, med_row, med_col, current, second, (what, "stay"), moved=3)
        dev.release()
