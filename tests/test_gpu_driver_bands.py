"""The two band walks of ``_driver.bands`` that no other test cuts into several bands, on a real MI355X: the rows of a
pruned model and the float64 pairs of a compacted one.  Both compare the same code across band sizes, bit for bit."""
import numpy as np
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _query, synth

pytestmark = pytest.mark.gpu

N = 300


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.fixture(scope="module")
def graph():
    df = synth.er_directed(N, 0.03, seed=9)
    assert len(set(df["from"]) | set(df["to"])) == N
    return df


def test_rows_of_a_pruned_model_are_banded(graph, monkeypatch):
    with SRA.SimRankPP().fit(graph, verbose=False, keep=True) as model:
        model.prune(5)
        solver, j, _ = model._kept()
        reader, ids = solver._reader(j), np.arange(N, dtype=np.int32)
        whole, ms = reader.rows(ids).copy(), []
        reader.rows(ids, timing=ms)
        assert len(ms) == 1 and np.count_nonzero(whole) > N          # (one band; the lists and the diagonal are there)
        for slab, rows_per_band in ((7 * 8 * N, 7), (1, 1)):
            monkeypatch.setattr(_query, "SLAB_BYTES", slab)
            _same_bits(reader.rows(ids), whole)
            ms = []
            _same_bits(reader.rows(ids, timing=ms), whole)
            assert len(ms) == -(-N // rows_per_band)                  # (one kernel per band)


def test_float64_pairs_of_a_compacted_model_are_banded(graph, monkeypatch):
    with SRA.SimRank().fit(graph, verbose=False, keep=True, storage_precision="f64") as model:
        model.compact()
        solver, j, _ = model._kept()
        dense = solver.result(j)
        assert dense.dtype == np.float64 and dense.shape == (N, N)
        t = float(np.median(dense[dense > 0]))
        whole = solver.pairs(j, t, None)
        assert 0 < whole[1].size < N * (N - 1)
        reader, asked = solver._reader(j), []
        rows = reader.rows
        monkeypatch.setattr(reader, "rows", lambda ids, *a, **kw: (asked.append(len(ids)), rows(ids, *a, **kw))[1])
        monkeypatch.setattr(_query, "SLAB_BYTES", 11 * 8 * N)
        banded = solver.pairs(j, t, None)
        assert asked == [11] * (N // 11) + [N % 11]
        for got, want in zip(banded, whole):
            _same_bits(got, want)
