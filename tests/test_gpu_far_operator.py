"""libsimrank_operator.so past 2^31 and 2^32 elements: ``simrank_operator_apply`` in both directions on the 70 x 1100 block
of tests/far.py in its four far geometries, in the arena of tests/test_gpu_far_blocks.py, whose every other byte is a
filler that is finite and above every value.  Every output row of ``S @ X`` sums a whole far row (rows 31 | 32 and 63 | 64
lie on each side of 2^31 and 2^32 elements), every output row of ``S.T @ X`` sums a column over all of them.  The values
are dyadic and X holds small integers times powers of two, so every sum is exact in any order: an element offset
narrowed to 32 bits reads the filler and the comparison with the NumPy product, bit for bit, fails."""
import numpy as np
import pytest

from simrank_amd import _operator
from tests import blocks as B
from tests import far as F
from tests import operator_ref as R
from tests.test_gpu_companion_blocks import same_bits
from tests.test_gpu_far_blocks import arena, dev, device, far_blocks  # noqa: F401 (fixtures)
from tests.test_gpu_operator_blocks import call_apply, effective

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_apply_reads_far_rows_in_both_directions(dev, arena, layout):  # noqa: F811
    lib = _operator.load()
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    filler = float(B.widen(layout, F.filler(layout))[0])
    rng = np.random.default_rng([layout, 43])                              # (the same case for every geometry)
    perms = (rng.permutation(n_rows).astype(np.int32), rng.permutation(n_cols).astype(np.int32))
    Xs = [R.exact_operand(rng, n_cols, 33, layout), R.exact_operand(rng, n_rows, 33, layout)]
    for blk, g, S, what in far_blocks(arena, layout, kinds=("dyadic",)):
        assert np.isfinite(filler) and filler > np.abs(blk.A).max()
        far = type("Far", (), dict(layout=layout, stride=g.stride, n_rows=n_rows, n_cols=n_cols))
        for transpose in (0, 1):
            X = Xs[transpose]
            n_out = n_cols if transpose else n_rows
            for maps in ((None, None), perms):
                E = effective(blk.A, maps[0], maps[1], transpose)
                R.assert_exact(E, X)
                assert (np.abs(E) @ np.abs(X) > 0).all()                   # every far row and column takes part in a sum
                for d, alpha, beta in ((33, 1.0, 0.0), (3, 0.5, 1.0), (8, 1.0, 0.0)):
                    out0 = np.full((n_out, d), np.nan) if beta == 0.0 else rng.integers(-64, 65, size=(n_out, d)) / 4.0
                    want = alpha * (E @ X[:, :d]) + (0.0 if beta == 0.0 else beta * out0)
                    got = call_apply(dev, lib, S, far, maps[0], maps[1], transpose, X, d, alpha, beta, out0, what)
                    same_bits(got, want, (what, transpose, maps[0] is None, d))
        dev.release()
