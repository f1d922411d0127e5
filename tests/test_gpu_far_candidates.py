"""libsimrank_candidates.so past 2^31 and 2^32 elements: ``simrank_candidates_topk`` on the 70 x 1100 block of tests/far.py
in its four far geometries, in the arena of tests/test_gpu_far_blocks.py, whose every other byte is a filler that is
finite and above every value.  The kernel gathers single elements at scattered (row, column); an element offset narrowed
to 32 bits reads the filler, which wins every top-k it enters.  tests/test_far_cpu.py evaluates the reference on the
narrowed matrix for the very lists, rows and k used here (tests/far_cases.py) and shows that the ids differ.

Staged lists: every column in ascending-id order, which must equal ``simrank_neighbors_select`` on the same far block,
and the edge columns plus 40 others with -1 and n_cols inside the list.  Not staged: the far panels hold 1 100 columns,
so the LIST is long instead of the block, one entry more than the staging cap: every column once, then columns drawn
with repeats.  A candidate is a list index, so every value meets about fifteen exact ties, the k-th value ties and both
index passes decide; the reference's tie rule is the list index.  With ids and without, every call twice, outputs
pre-filled and one guard row longer, compared bit for bit with ``candidates_ref.ref_topk``."""
import numpy as np
import pytest

from simrank_amd import _candidates, _neighbors
from tests import blocks as B
from tests import far as F
from tests import far_cases as FC
from tests.test_gpu_candidates import topk
from tests.test_gpu_companion_blocks import out_of, same_bits
from tests.test_gpu_far_blocks import arena, dev, device, far_blocks  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_candidates_topk(dev, arena, layout):  # noqa: F811
    nlib, st = _neighbors.load(), dev.ops.stream
    n_rows, n_cols = F.N_ROWS, F.N_COLS
    assert _candidates.staged(layout) == FC.STAGED[layout]
    filler = FC.widened_filler(layout)
    for i, (blk, g, S, what) in enumerate(far_blocks(arena, layout)):
        assert i == FC.counter(g, what[2]) and filler > blk.A.max()         # a filler that entered a list would lead it
        inp = FC.candidate_inputs(blk, i)
        want = FC.candidate_outputs(blk.A, inp)
        row_pos = inp["row_pos"]
        where = (S, layout, g.stride, n_rows, n_cols)
        rp = dev.put(row_pos)
        tied = 0
        for run, (want_i, want_v) in zip(inp["runs"], want):
            name, pos, ids, row_ids, k = run
            label = (what, name, ids is None, k)
            rows = (rp, dev.put(np.ascontiguousarray(row_ids, dtype=np.int32)), row_pos.size)
            got_i, got_v = topk(dev, where, rows, pos, ids, k)
            same_bits(got_i, want_i, ("ids", label))
            same_bits(got_v, want_v, ("values", label))
            again_i, again_v = topk(dev, where, rows, pos, ids, k)
            assert np.array_equal(got_i, again_i) and np.array_equal(B.bits(got_v), B.bits(again_v)), label
            if name == "all":                                                # what the unfiltered selection returns
                idx, hi = out_of(dev, (row_pos.size + 1, k), np.int32, -9)
                val, hv = out_of(dev, (row_pos.size + 1, k), np.float64, 1e300)
                _neighbors.check(nlib.simrank_neighbors_select(*where, *rows, None if ids is None else dev.put(inp["col_ids"]),
                                                               k, idx, val, st), "select")
                same_bits(got_i, dev.get(idx, hi)[:row_pos.size], ("ids against neighbors_select", label))
                same_bits(got_v, dev.get(val, hv)[:row_pos.size], ("values against neighbors_select", label))
            if name == "long":
                assert pos.size == _candidates.staged(layout) + 1
                tied += FC.ties_at_k(blk.A, inp, run) > 0
        assert tied == 2 * len(FC.LONG_KS), what                             # every long run has a row that ties at rank k
        dev.release()
