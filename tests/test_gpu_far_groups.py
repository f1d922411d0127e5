"""libsimrank_groups.so past 2^31 and 2^32 elements: the 70 x 1100 block of tests/far.py in its four far geometries, in
the arena of tests/test_gpu_far_blocks.py, whose every other byte is a filler that is finite and above every value.  An
element offset narrowed to 32 bits reads the filler (or another row), which changes any sum it enters by far more than
the bound: the dyadic block is compared bit for bit with ``groups_ref.block_means``, the wide one (many binades: its sums
round) within the bound of a float64 sum in any order.  Every layout; K = 1 (1100 positions: the workgroup sums), five
clusters (a wave each), 300 small ones (a lane each)."""
import numpy as np
import pytest

from tests import blocks as B
from tests import far as F
from tests import groups_ref as GR
from tests.test_gpu_companion_blocks import same_bits
from tests.test_gpu_far_blocks import arena, dev, device, far_blocks  # noqa: F401 (fixtures)
from tests.test_gpu_groups import check_call, lists_of, rows_of, run_means

pytestmark = pytest.mark.gpu


def far_labellings(rng):
    n = F.N_COLS
    five = rng.choice(5, size=n, p=[0.4, 0.3, 0.15, 0.1, 0.05])
    five[rng.permutation(n)[:5]] = np.arange(5)
    return {"one": np.zeros(n, dtype=np.int64), "five": five, "small": rng.permutation(n) % 300}


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_groups_means(dev, arena, layout):  # noqa: F811
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    filler = float(B.widen(layout, F.filler(layout))[0])
    refs = {}
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        A, kind = blk.A, what[2]
        rng = np.random.default_rng([layout, 23])                          # (the same labellings for every geometry)
        for name, gidx in far_labellings(rng).items():
            col_pos, ptr = lists_of(gidx, rng)
            case = rows_of(n_rows, n_cols, gidx) + (col_pos, ptr)
            assert set(F.EDGE_ROWS) - {n_rows // 2} <= set(np.flatnonzero(case[0] >= 0).tolist())
            if (kind, name) not in refs:
                refs[(kind, name)] = GR.block_means(A, *case)
            ref = refs[(kind, name)]
            own, other, near, table, tol = ref
            # a filler that entered a sum in place of a value would move the mean by far more than the bound
            counts = np.maximum(np.diff(ptr), 1)[None, :]
            assert np.abs(filler - A).min() / counts.max() > 1024 * tol.max(), (what, name)
            if kind == "dyadic":
                check_call(dev, S, layout, g.stride, A, case, ref, (what, name))
                continue
            k = len(ptr) - 1
            got_own, got_other, got_near, got_means = run_means(dev, S, layout, g.stride, n_rows, n_cols, *case, k + 3)
            live = near != -2
            body = got_means[:n_rows * (k + 3)].reshape(n_rows, k + 3)
            assert (body[:, k:] == 1e300).all() and got_means[-1] == 1e300 and (body[~live] == 1e300).all()
            assert got_own[-1] == 1e300 and got_other[-1] == 1e300 and (got_own[:n_rows][~live] == 1e300).all()
            same_bits(np.isnan(body[live][:, :k]), np.isnan(table[live]), (what, name, "nan"))
            ok = live[:, None] & ~np.isnan(table)
            assert np.all(np.abs(body[:, :k][ok] - table[ok]) <= tol[ok]), (what, name, "means")
            rows = np.flatnonzero(live)
            assert not np.isnan(own[rows]).any()                               # (no cluster is a single node here)
            assert np.all(np.abs(got_own[rows] - own[rows]) <= tol[rows, case[0][rows]]), (what, name, "own")
            has = rows[near[rows] >= 0]
            picked = got_near[has]
            assert (picked >= 0).all() and (picked != case[0][has]).all(), (what, name)
            assert np.all(table[has, picked] >= other[has] - 2 * tol[has, picked]), (what, name, "nearest")
            assert np.all(np.abs(got_other[has] - table[has, picked]) <= tol[has, picked]), (what, name, "other")
            again = run_means(dev, S, layout, g.stride, n_rows, n_cols, *case, None)
            for a, b in zip((got_own, got_other, got_near), again[:3]):
                assert np.array_equal(B.bits(a), B.bits(b)), (what, name)          # a second run: the same bits
        dev.release()
