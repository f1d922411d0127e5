"""libsimrank_diverse.so past 2^31 and 2^32 elements: ``simrank_diverse_pick`` on the 70 x 1100 block of tests/far.py in its
four far geometries, in the arena of tests/test_gpu_far_blocks.py, whose every other byte is a filler that is finite and
above every value.  The band is built so that the first picks fall on candidates whose ``row_pos`` are ``far.EDGE_ROWS``
(31 | 32 and 63 | 64: the rows on each side of 2^31 and 2^32 elements, and the last row) and which sit at
``far.EDGE_COLS`` (each side of 512 and 1024); the later picks are decided by the penalties those rows left.  An element
offset narrowed to 32 bits reads the filler, which passes every pen it meets: the penalties and the picks change and the
comparison with tests/diverse_ref.py, bit for bit on the dyadic and on the wide block, fails."""
import numpy as np
import pytest

from simrank_amd import _diverse
from tests import blocks as B
from tests import diverse_ref as D
from tests import far as F
from tests.test_gpu_diverse_blocks import call_pick, check_outputs
from tests.test_gpu_far_blocks import arena, dev, device, far_blocks  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

K, DIVERSITY = 14, 0.25


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_pick_reads_far_rows(dev, arena, layout):  # noqa: F811
    lib = _diverse.load()
    n_rows, n_out = F.N_ROWS, F.N_COLS
    filler = float(B.widen(layout, F.filler(layout))[0])
    rng = np.random.default_rng([layout, 41])                              # (the same case for every geometry)
    edge = np.array(F.EDGE_COLS)
    rows = rng.integers(0, n_rows, size=n_out).astype(np.int32)
    rows[edge] = F.EDGE_ROWS
    # two baskets: the edge candidates far above the others (no penalty reaches 1000 x 0.75), in both orders
    band = rng.integers(-32, 33, size=(2, n_out)) / 8.0
    band[0, edge] = 2000.0 - 100.0 * np.arange(edge.size)
    band[1, edge] = 1000.0 + 100.0 * np.arange(edge.size)
    band[:, rng.choice(np.setdiff1d(np.arange(n_out), edge), size=40, replace=False)] = -np.inf
    perm = rng.permutation(n_out).astype(np.int32)
    band_dev = dev.put(band)
    refs = {}
    for blk, g, S, what in far_blocks(arena, layout):
        A, kind = blk.A, what[2]
        assert np.isfinite(filler) and filler > A.max()                     # a filler that is read passes every pen
        far = type("Far", (), dict(layout=layout, stride=g.stride, n_rows=n_rows, n_cols=n_out))
        for col_pos in (None, perm):
            key = (kind, col_pos is None)
            if key not in refs:
                M = A if col_pos is None else A[:, col_pos]
                refs[key] = want = D.band_picks(band, lambda b: M[rows[b]], K, DIVERSITY)
                assert want[0][0, :edge.size].tolist() == edge.tolist() and want[0][1, :edge.size].tolist() == edge[::-1].tolist()
                assert (want[0] >= 0).all() and (want[2] > 0).sum() >= K   # the later picks carry the far rows' penalties
            got = call_pick(dev, lib, S, far, rows, col_pos, band_dev, n_out, 2, n_out, K, DIVERSITY, what)
            check_outputs(got, refs[key], 2, K, (what, col_pos is None))
