"""libsimrank_explain.so past 2^31 and 2^32 elements: ``simrank_explain_gather`` on the 70 x 1100 block of tests/far.py in
its four far geometries, in the arena of tests/test_gpu_far_blocks.py, whose every other byte is a filler that is finite
and above every value.  The row lists include ``far.EDGE_ROWS`` (rows that start past 2^31 and 2^32 elements) and the column
lists ``far.EDGE_COLS`` (panels that do).  An element offset narrowed to 32 bits reads the filler: the comparison with
``explain_ref.block_gather``, bit for bit on the dyadic and on the wide block (nothing is added), fails."""
import numpy as np
import pytest

from tests import blocks as B
from tests import explain_ref as ER
from tests import far as F
from tests.test_gpu_companion_blocks import same_bits
from tests.test_gpu_explain import Case, Run, flat
from tests.test_gpu_far_blocks import arena, dev, device, far_blocks  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_explain_gather(dev, arena, layout):  # noqa: F811
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    filler = float(B.widen(layout, F.filler(layout))[0])
    rng = np.random.default_rng([layout, 41])                              # (the same lists for every geometry)
    edge_r, edge_c = np.array(F.EDGE_ROWS), np.array(F.EDGE_COLS)
    # the edges against the edges; every row against a spread of columns; a long pair; one with a row and a column outside
    lists_a = [edge_r, np.arange(n_rows), rng.integers(0, n_rows, size=300), np.append(edge_r[::-1], n_rows), np.empty(0)]
    lists_b = [edge_c, np.concatenate([edge_c, rng.integers(0, n_cols, size=90)]), rng.integers(0, n_cols, size=257),
               np.append(edge_c, -1), edge_c]
    case = Case(lists_a, lists_b)
    want = {}
    for blk, g, S, what in far_blocks(arena, layout):
        A, kind = blk.A, what[2]
        assert np.isfinite(filler) and filler > A.max()                     # a filler that was read would show
        if kind not in want:
            want[kind] = flat([ER.block_gather(A, a, b) for a, b in zip(case.lists_a, case.lists_b)])
            assert not (want[kind] == filler).any() and np.isnan(want[kind]).any()
        same_bits(Run(dev, case).gather(S, layout, g.stride, n_rows, n_cols), want[kind], what)
        dev.release()
