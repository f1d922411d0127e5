"""``simrank_amd._driver``: what the companion drivers share on the host, on a machine without a GPU and without a
library.  ``Ops`` is a recording double of the engine's ``HipOps``: it hands out numbered blocks and logs every call, so
the tests read the order of synchronise and free straight off the log."""
import itertools
import os

import numpy as np
import pandas as pd
import pytest

from simrank_amd import _driver, _query
from simrank_amd._driver import Scratch, bands, id_lists, join, scatter_blocks, stage


class Ops:
    def __init__(self, sync_error=None):
        self.log, self.sync_error, self._next = [], sync_error, 0x1000

    def _malloc(self, nbytes):
        self._next += 0x100
        self.log.append(("_malloc", self._next, int(nbytes)))
        return self._next

    def _free(self, ptr):
        self.log.append(("_free", ptr))

    def h2d(self, ptr, host):
        assert host.flags.c_contiguous
        self.log.append(("h2d", ptr, host.nbytes))

    def put(self, host):
        ptr = self._malloc(host.nbytes)
        self.h2d(ptr, host)
        return ptr

    def synchronize(self):
        self.log.append(("synchronize",))
        if self.sync_error is not None:
            raise self.sync_error

    def timed(self, launch):
        self.log.append(("timed",))
        launch()
        return 1.5

    def names(self):
        return [e[0] for e in self.log]


# ---- Scratch -----------------------------------------------------------------------------------------------------------
def _use(scratch):
    """Three blocks, one of them from a host array that is not C-contiguous -> their pointers in the order handed out."""
    return [scratch.malloc(64), scratch.put(np.arange(12, dtype=np.int32).reshape(3, 4).T), scratch.malloc(8)]


def _assert_synced_then_freed_in_reverse(ops, ptrs):
    names = ops.names()
    assert names.count("synchronize") == 1
    assert names.index("synchronize") < names.index("_free")
    assert [e[1] for e in ops.log if e[0] == "_free"] == ptrs[::-1]        # each once, last first


def test_scratch_synchronises_then_frees_in_reverse():
    ops = Ops()
    with Scratch(ops) as scratch:
        ptrs = _use(scratch)
        assert len(set(ptrs)) == 3 and "_free" not in ops.names()
    _assert_synced_then_freed_in_reverse(ops, ptrs)


def test_scratch_exits_the_same_way_under_an_exception():
    ops, ptrs = Ops(), []
    with pytest.raises(KeyError, match="the caller's"):
        with Scratch(ops) as scratch:
            ptrs += _use(scratch)
            raise KeyError("the caller's")
    _assert_synced_then_freed_in_reverse(ops, ptrs)


def test_scratch_frees_and_keeps_the_first_exception_when_the_synchronise_fails_too():
    ops, ptrs = Ops(sync_error=RuntimeError("the stream's")), []
    with pytest.raises(KeyError, match="the caller's"):
        with Scratch(ops) as scratch:
            ptrs += _use(scratch)
            raise KeyError("the caller's")
    _assert_synced_then_freed_in_reverse(ops, ptrs)
    # with nothing pending the stream's error is the caller's to see, after the frees
    ops = Ops(sync_error=RuntimeError("the stream's"))
    with pytest.raises(RuntimeError, match="the stream's"):
        with Scratch(ops) as scratch:
            ptrs = _use(scratch)
    _assert_synced_then_freed_in_reverse(ops, ptrs)


# ---- stage -------------------------------------------------------------------------------------------------------------
def test_stage_times_into_a_list_or_a_dict_and_not_at_all_without_one():
    ops, ran = Ops(), []
    stage(ops, None, "a_ms", lambda: ran.append(0))
    assert ran == [0] and ops.log == []
    ms = []
    stage(ops, ms, "a_ms", lambda: ran.append(1))
    stage(ops, ms, "b_ms", lambda: ran.append(2))
    assert ms == [1.5, 1.5]
    stages = {"other_ms": 4.0}
    stage(ops, stages, "a_ms", lambda: ran.append(3))
    stage(ops, stages, "a_ms", lambda: ran.append(4))
    assert stages == {"other_ms": 4.0, "a_ms": 3.0}
    assert ran == [0, 1, 2, 3, 4] and ops.names() == ["timed"] * 4


# ---- bands -------------------------------------------------------------------------------------------------------------
TILE, MAX_BLOCKS = 32, 1 << 24          # _foldin.TILE; _sets.MAX_BLOCKS = _neighbors.MAX_BLOCKS


def _parent_bands(n, width, SLAB_BYTES, cap):
    """The five band sizes as the drivers wrote them out before ``bands``: ``n`` items over rows of ``width`` float64."""
    return {
        "Reader.rows": int(max(1, min(n, SLAB_BYTES // (8 * width)))),
        "_sets.run": int(max(1, min(n, SLAB_BYTES // (8 * width), MAX_BLOCKS // cap))),
        "NeighborReader.rows": int(max(1, min(n, SLAB_BYTES // (8 * width), MAX_BLOCKS // cap))),
        "Folder.run": int(max(TILE, min(-(-n // TILE) * TILE, SLAB_BYTES // (8 * width) // TILE * TILE))),
        "DetachedSolver.pairs": int(max(1, min(n, SLAB_BYTES // (8 * max(1, width))))),
    }


@pytest.mark.parametrize("slab", [1, 8 * 300 - 1, 7 * 8 * 300, 64 * 8 * 300 + 5, 256 << 20])
def test_bands_are_the_five_formulas_and_tile_the_items(monkeypatch, slab):
    monkeypatch.setattr(_query, "SLAB_BYTES", slab)
    for n, width, cap in itertools.product([1, 2, 31, 32, 33, 70, 1000], [1, 300], [8, MAX_BLOCKS // 3, 2 * MAX_BLOCKS]):
        want = _parent_bands(n, width, slab, cap)
        walks = {
            "Reader.rows": bands(n, 8 * width),
            "_sets.run": bands(n, 8 * width, MAX_BLOCKS // cap),
            "NeighborReader.rows": bands(n, 8 * width, MAX_BLOCKS // cap),
            "Folder.run": bands(n, 8 * width, unit=TILE),
            "DetachedSolver.pairs": bands(n, 8 * max(1, width)),
        }
        for name, walk in walks.items():
            assert walk.size == want[name], (name, n, width, cap)
            got = list(walk)
            assert got == list(walk), "a walk can be iterated again"
            assert [q0 for q0, _ in got] == list(range(0, n, walk.size)), (name, n, width, cap)
            assert all(1 <= m <= walk.size for _, m in got) and sum(m for _, m in got) == n
            assert all(q0 + m == nxt for (q0, m), (nxt, _) in zip(got, got[1:]))


def test_bands_of_nothing_and_the_slab_read_at_the_call(monkeypatch):
    assert list(bands(0, 8)) == [] and bands(0, 8).size == 1 and bands(0, 8, unit=TILE).size == TILE
    monkeypatch.setattr(_query, "SLAB_BYTES", 9 * 8 * 50)
    assert bands(70, 8 * 50).size == 9 and list(bands(70, 8 * 50))[-1] == (63, 7)
    monkeypatch.setattr(_query, "SLAB_BYTES", 1)
    assert list(bands(3, 8 * 50)) == [(0, 1), (1, 1), (2, 1)]


# ---- scatter_blocks ----------------------------------------------------------------------------------------------------
def test_scatter_blocks_is_a_fancy_index_per_block():
    rng = np.random.default_rng(0)
    widths, m, band = [5, 1, 3], 4, 6                        # three uneven blocks; the stage buffer holds 6 rows, 4 are used
    n = sum(widths)
    caller = rng.permutation(n).astype(np.int32)             # caller id of every column, block after block
    col_ids = np.split(caller, np.cumsum(widths)[:-1])
    pieces = [rng.random((m, w)) for w in widths]
    staged = np.full((band, n), np.nan)
    staged.reshape(-1)[:m * n] = np.concatenate([p.reshape(-1) for p in pieces])
    out = np.full((10, n), -1.0)
    scatter_blocks(out[2:2 + m], staged, m, [dict(cols=w) for w in widths], lambda i: col_ids[i])
    want = np.full((10, n), -1.0)
    for p, ids in zip(pieces, col_ids):
        want[2:2 + m, ids] = p
    np.testing.assert_array_equal(out, want)
    assert not np.isnan(out).any()


# ---- id_lists / join ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [pd.Index(["a", "b", "c", "d"], dtype=object), pd.Index([10, 20, 30, 40])])
def test_id_lists_and_join(index):
    a, b, c, d = index
    lists = id_lists("sets", [[c, a, c], [], (d,)], index)
    assert [x.tolist() for x in lists] == [[2, 0, 2], [], [3]] and all(x.dtype == np.int32 for x in lists)
    ptr, ids = join(lists)
    assert ptr.dtype == np.int64 and ptr.tolist() == [0, 3, 3, 4]
    assert ids.dtype == np.int32 and ids.flags.c_contiguous and ids.tolist() == [2, 0, 2, 3]
    ptr, ids = join(id_lists("sets", [[], []], index))
    assert ptr.tolist() == [0, 0, 0] and ids.dtype == np.int32 and ids.size == 0
    ptr, ids = join([])
    assert ptr.tolist() == [0] and ids.size == 0
    # repeats: kept, or refused where a list is a node's edges
    assert [x.tolist() for x in id_lists("neighbors", [[b], [a, d]], index, unique=True)] == [[1], [0, 3]]
    with pytest.raises(ValueError, match=r"neighbors\[1\] repeats a label: a node has one edge per neighbour"):
        id_lists("neighbors", [[a], [c, a, c]], index, unique=True)
    # the first unknown label, by name
    unknown = ["x", "y"] if index.dtype == object else [77, 88]
    with pytest.raises(KeyError) as e:
        id_lists("sets", [[a], [b, unknown[0], unknown[1]]], index)
    assert e.value.args == (unknown[0],)
    with pytest.raises(ValueError, match="^sets must be a sequence with one sequence of labels per basket$"):
        id_lists("sets", "ab", index)
    with pytest.raises(ValueError, match="^neighbors must be a sequence with one sequence of labels per new node$"):
        id_lists("neighbors", iter([[a]]), index, unique=True, each="new node")
    with pytest.raises(ValueError, match=r"^targets\[1\] must be a sequence of labels, not 7$"):
        id_lists("targets", [[a], 7], index)


# ---- merge_topk's shortcut ---------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(_query.LIB_PATH), reason="libsimrank_query.so is not built")
def test_one_piece_of_width_k_comes_back_as_the_library_merges_it():
    """One block's k best, in the order (value descending, id ascending) with ties and empty slots as the selection
    kernels leave them: ``merge_topk`` hands the piece back, which is what the library's merge makes of it (asked here
    through two pieces: the one, and one of empty slots)."""
    rng = np.random.default_rng(1)
    n_q, k = 23, 6
    ids, vals = np.full((n_q, k), -1, dtype=np.int32), np.zeros((n_q, k))
    for q in range(n_q):
        have = int(rng.integers(0, k + 1))
        cand = sorted((-float(rng.integers(1, 4)) / 4, int(i)) for i in rng.choice(50, size=have, replace=False))
        ids[q, :have], vals[q, :have] = [c[1] for c in cand], [-c[0] for c in cand]
    got = _query.merge_topk([(ids, vals)], k)
    want = _query.merge_topk([(ids, vals), (np.full((n_q, 1), -1, dtype=np.int32), np.zeros((n_q, 1)))], k)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        np.testing.assert_array_equal(g, w)
    # a narrower or wider single piece still goes through the library
    idx, val = _query.merge_topk([(ids[:, :4], vals[:, :4])], k)
    assert idx.shape == (n_q, k) and (idx[:, 4:] == -1).all() and (val[:, 4:] == 0).all()


def test_driver_imports_nothing_of_the_product():
    import ast
    with open(_driver.__file__) as f:
        tree = ast.parse(f.read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert [getattr(n, "module", None) or n.names[0].name for n in top] == ["__future__", "numpy"]
