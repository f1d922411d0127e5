"""libsimrank_query.so (include/simrank_query.h) and ``fit(keep=True)`` on a machine without a GPU: header, binding and
exports agree, the header is plain C99 and stands alone, argument checks need no device, the host merge of per-block
top-k candidates orders as a NumPy sort does, and ``fit(keep=True)`` refuses what it does not serve before any device
work.  The main library's ABI stays at version 8 with 117 entry points."""
import re

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _query
from tests import companion_abi as A

CLASSES = ["SimRank", "SimRankPP", "AprioriSimRank", "BipartiteSimRank", "BipartiteSimRankPP", "BipartitleAprioriSimRank"]


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_query) == _query.VERSION == 1
    A.assert_header_stands_alone(_query)


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_query)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_query)


def test_layout_codes_agree_across_headers_and_bindings():
    """One set of layout codes: ``engine._iterate_block`` hands a plan's "iterate_layout" to every library that reads a
    block alike, and ``_foldin.Folder`` passes a query code to fold-in calls (csrc/companion.h asserts the same of the
    headers when the libraries are compiled)."""
    from simrank_amd import _cluster, _companion, _foldin, _model, _neighbors, _profile, _select, _sets
    want = {"PANEL_F32": 0, "ROWMAJOR_F32": 1, "PANEL_F16": 2, "ROWMAJOR_F64": 3}
    # _query, _model, _profile and _cluster define all four names.  _sets and _neighbors define no layout name at all:
    # their callers pass them a block's code, so only their headers can be checked.
    named = (_query, _model, _profile, _cluster)
    for mod in named + (_foldin, _sets, _neighbors):
        assert A.layout_codes(mod) == want, mod.__name__
    three = {k: v for k, v in want.items() if k != "ROWMAJOR_F64"}            # (select reads no float64 iterate)
    assert A.layout_codes(_select) == three
    for mod, names in [(_companion, want), (_select, three), (_foldin, ["ROWMAJOR_F64"])] + [(m, want) for m in named]:
        for name in names:
            assert getattr(mod, name) == getattr(_companion, name) == want[name], (mod.__name__, name)


def test_main_library_abi_is_unchanged():
    version, names, exports = A.main_library(_query)
    assert version == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_a_c_program_links(tmp_path):
    assert "query 1 ok" in A.run_c99(_query, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_query.h"
int main(void) {
    int32_t ids0[4] = {7, 3, -1, -1}, ids1[2] = {5, 1};
    double v0[4] = {0.5, 0.25, 0.0, 0.0}, v1[2] = {0.5, 0.25};
    const int32_t* ids[2];
    const double* vals[2];
    int32_t ks[2] = {2, 1}, idx[6];
    double val[6];
    ids[0] = ids0; ids[1] = ids1; vals[0] = v0; vals[1] = v1;
    if (simrank_query_version() != SIMRANK_QUERY_VERSION) return 1;
    if (simrank_query_rows(NULL, 9, 8, 4, 4, NULL, 1, NULL, 4, NULL, 4, NULL) != SIMRANK_QUERY_ERR_INVALID) return 2;
    if (!strlen(simrank_query_last_error())) return 3;
    if (simrank_query_rows(NULL, SIMRANK_QUERY_PANEL_F32, 8, 4, 4, NULL, 1, NULL, 4, NULL, 4, NULL)
        != SIMRANK_QUERY_ERR_INVALID) return 4;                                   /* S is NULL */
    if (simrank_query_rows(NULL, SIMRANK_QUERY_ROWMAJOR_F64, 4, 0, 4, NULL, 0, NULL, 4, NULL, 4, NULL)
        != SIMRANK_QUERY_OK) return 5;                                            /* nothing asked: no device touched */
    if (simrank_query_pairs(NULL, SIMRANK_QUERY_PANEL_F16, 2, 4, 4, NULL, NULL, 1, NULL, NULL)
        != SIMRANK_QUERY_ERR_INVALID) return 6;                                   /* stride below the rows */
    if (simrank_query_topk(ids0, SIMRANK_QUERY_ROWMAJOR_F32, 4, 4, 4, NULL, NULL, 1, NULL, 0, NULL, NULL, NULL)
        != SIMRANK_QUERY_ERR_INVALID) return 7;                                   /* k = 0 */
    if (simrank_query_topk(ids0, SIMRANK_QUERY_ROWMAJOR_F32, 4, 4, 4, NULL, NULL, 1, NULL, 1025, NULL, NULL, NULL)
        != SIMRANK_QUERY_ERR_INVALID) return 8;
    /* two rows, piece 0 with k = 2, piece 1 with k = 1: row 0 = {(.5,7),(.25,3)} + {(.5,5)}, row 1 = {} + {(.25,1)} */
    if (simrank_query_merge_topk(2, ids, vals, ks, 2, 3, idx, val) != SIMRANK_QUERY_OK) return 9;
    if (idx[0] != 5 || idx[1] != 7 || idx[2] != 3 || idx[3] != 1 || idx[4] != -1 || val[3] != 0.25 || val[5] != 0.0) return 10;
    printf("query %d ok\n", simrank_query_version());
    return 0;
}
''')


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_merge_of_per_block_candidates_is_a_numpy_sort(seed):
    """Per-rank candidates (each block's own k best, already in the order, -1 padded) merged = the k best of the row's
    union by (value descending, id ascending), on data with many ties."""
    rng = np.random.default_rng(seed)
    n_q, P, k = 37, 3, 9
    widths = [11, 4, 16]                                  # a block narrower than k hands fewer candidates
    values = rng.integers(0, 4, size=(n_q, sum(widths))).astype(np.float64) / 4          # four distinct values: ties
    ids = rng.permutation(sum(widths)).astype(np.int32)
    pieces, lo = [], 0
    for w in widths:
        kk = min(k, w)
        pi, pv = np.full((n_q, kk), -1, dtype=np.int32), np.zeros((n_q, kk))
        for q in range(n_q):
            cand = [(-(values[q, c]), int(ids[c])) for c in range(lo, lo + w) if ids[c] != q]    # the row's own id is out
            cand.sort()
            cand = cand[:kk]
            pi[q, :len(cand)] = [c[1] for c in cand]
            pv[q, :len(cand)] = [-c[0] for c in cand]
        pieces.append((pi, pv))
        lo += w
    idx, val = _query.merge_topk(pieces, k)
    assert idx.dtype == np.int32 and val.dtype == np.float64 and idx.shape == (n_q, k)
    for q in range(n_q):
        keep = ids != q
        order = np.lexsort((ids[keep], -values[q][keep]))[:k]
        np.testing.assert_array_equal(idx[q], ids[keep][order])
        np.testing.assert_array_equal(val[q], values[q][keep][order])
    # fewer candidates than k: -1 / 0 past them
    idx, val = _query.merge_topk([(np.array([[4, -1]]), np.array([[0.5, 0.0]]))], 3)
    assert idx.tolist() == [[4, -1, -1]] and val.tolist() == [[0.5, 0.0, 0.0]]


EDGES = pd.DataFrame({"from": [0, 1, 2, 2], "to": [1, 2, 0, 1], "user": [0, 1, 2, 2], "item": [1, 2, 0, 1]})


def _fit(cls, **kw):
    est = getattr(SRA, cls)()
    prior = [np.eye(3)] * (2 if cls == "BipartitleAprioriSimRank" else 1 if cls == "AprioriSimRank" else 0)
    return est, lambda: est.fit(EDGES, *prior, verbose=False, **kw)


@pytest.mark.parametrize("cls", CLASSES)
def test_keep_argument_checks_need_no_device(cls, monkeypatch):
    from simrank_amd import estimators
    monkeypatch.setattr(estimators, "_make_solver", lambda *a, **k: pytest.fail("device work before the checks"))
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="keep must be True or False"):
            _fit(cls, keep=bad)[1]()
    with pytest.raises(ValueError, match="keep=True hands nothing back"):
        _fit(cls, keep=True, top_k=3)[1]()
    with pytest.raises(ValueError, match="keep=True hands nothing back"):
        _fit(cls, keep=True, min_similarity=0.1)[1]()
    with pytest.raises(ValueError, match="behind the C ABI"):
        _fit(cls, keep=True, mode="dense")[1]()
    with pytest.raises(ValueError, match="behind the C ABI"):
        _fit(cls, keep=True, _ops_factory=lambda r: None)[1]()
    with pytest.raises(ValueError, match="behind the C ABI"):                 # (checked for every storage alike)
        _fit(cls, keep=True, storage_precision="f64", mode="hybrid")[1]()


def test_keep_is_keyword_only_and_defaults_to_false():
    import inspect
    for cls in CLASSES:
        p = inspect.signature(getattr(SRA, cls).fit).parameters["keep"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_keep_on_a_torch_world_is_refused(tmp_path, monkeypatch):
    """A TorchWorld (one gloo rank is enough to make one) is refused with the reason, before any device work."""
    import torch.distributed as dist
    from simrank_amd import estimators
    from simrank_amd.driver import TorchWorld
    monkeypatch.setattr(estimators, "_make_solver", lambda *a, **k: pytest.fail("device work before the checks"))
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        world = TorchWorld()
        with pytest.raises(ValueError, match="collective call on all ranks"):
            SRA.SimRank().fit(EDGES, verbose=False, world=world, keep=True)
    finally:
        dist.destroy_process_group()


def test_f64_library_reports_its_iterate_additively_at_version_1():
    """``simrank_f64_plan_get`` (what a kept float64 model is read through) is declared, bound and exported; the f64
    library stays at version 1 and its argument checks need no device."""
    import ctypes
    from simrank_amd import _f64
    text = open(_f64.HEADER_PATH).read()
    assert re.search(r"^SIMRANK_F64_API int simrank_f64_plan_get\(", text, flags=re.M)
    assert "simrank_f64_plan_get" in _f64.PROTOTYPES
    lib = _f64.load()
    assert lib.simrank_f64_version() == 1
    v = ctypes.c_int64(7)
    assert lib.simrank_f64_plan_get(None, 0, b"iterate", ctypes.byref(v)) == _f64.ERR_INVALID


def test_queries_without_a_kept_model_raise():
    est = SRA.SimRank()
    for call in (lambda: est.rows([0]), lambda: est.similarity([0], [1]), lambda: est.most_similar([0], 2),
                 lambda: est.frame(), lambda: est.top_k(2), lambda: est.pairs(0.1)):
        with pytest.raises(RuntimeError, match="no kept model"):
            call()
    est.release()                     # nothing kept: a no-op
    with est:
        pass


class _FakeSolver:
    """Stands in for a kept solver: what the argument checks of the query methods reach is never the device."""
    mode, released = "sparse", 0

    def release(self):
        self.released += 1

    def rows(self, j, ids):
        return np.zeros((len(ids), 3))

    def pair_values(self, j, a, b):
        return np.zeros(len(a))

    def topk_of(self, j, ids, k):
        return np.full((len(ids), min(k, 2)), -1, dtype=np.int32), np.zeros((len(ids), min(k, 2)))


def test_query_argument_checks_and_lifetime_on_the_host():
    est, solver = SRA.SimRank(), _FakeSolver()
    est._keep(solver, [(0, ["a", "b", "c"])])
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="k must be a positive integer"):
            est.most_similar(["a"], bad)
        with pytest.raises(ValueError, match="k must be a positive integer"):
            est.top_k(bad)
    with pytest.raises(ValueError, match="same length"):
        est.similarity(["a", "b"], ["a"])
    with pytest.raises(KeyError, match="zz"):
        est.rows(["a", "zz"])
    with pytest.raises(KeyError, match="7"):
        est.similarity(["a"], [7])
    with pytest.raises(ValueError, match="group"):
        est.rows(["a"], group=2)
    got = est.rows([])
    assert got.shape == (0, 3) and list(got.columns) == ["a", "b", "c"]
    assert est.similarity([], []).shape == (0,)
    assert list(est.most_similar([], 2).columns) == ["node", "rank", "neighbor", "similarity"]
    assert list(est.rows(["c", "a", "c"]).index) == ["c", "a", "c"]
    with est as same:
        assert same is est
    assert solver.released == 1
    est.release()
    assert solver.released == 1
    with pytest.raises(RuntimeError, match="released"):
        est.rows(["a"])
    two = SRA.BipartiteSimRank()
    two._keep(_FakeSolver(), [(0, [1, 2, 3]), (1, ["x", "y", "z"])])
    with pytest.raises(ValueError, match="group must be 1 or 2"):
        two.rows([1])
    assert list(two.rows(["y"], group=2).columns) == ["x", "y", "z"]
    kept = two._model[0]
    del two
    assert kept.released == 1
