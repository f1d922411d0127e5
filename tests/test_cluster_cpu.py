"""libsimrank_cluster.so (include/simrank_cluster.h) and ``components`` on a machine without a GPU: header, binding and
exports agree, the header is plain C99 and stands alone, every entry point refuses bad arguments without a device, the
argument checks of ``components`` run before any device work, and the host path of a pruned model equals ``cluster_ref``
on hand-made tables."""
import re

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _cluster, _lib, _neighbors, _query
from tests import cluster_ref as CR
from tests import companion_abi as A


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_cluster) == _cluster.VERSION == 1
    text = A.header(_cluster)
    assert re.search(r"#define SIMRANK_CLUSTER_MAX_LEVELS %d\b" % _cluster.MAX_LEVELS, text) and _cluster.MAX_LEVELS == 8
    assert re.search(r"SIMRANK_CLUSTER_BAD_PARENT = %d\b" % _cluster.BAD_PARENT, text)
    assert re.search(r"SIMRANK_CLUSTER_CAP_REACHED = %d\b" % _cluster.CAP_REACHED, text)
    A.assert_header_stands_alone(_cluster)


def test_the_layout_codes_are_the_shared_ones():
    assert A.layout_codes(_cluster) == A.layout_codes(_query) and len(A.layout_codes(_cluster)) == 4


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_cluster)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_cluster)


def test_the_main_library_is_unchanged():
    version, names, exports = A.main_library(_cluster)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_every_entry_refuses_bad_arguments_without_a_device(tmp_path):
    assert "cluster 1 ok" in A.run_c99(_cluster, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_cluster.h"
#define BAD(call, code) do { if ((call) != SIMRANK_CLUSTER_ERR_INVALID) return code; \
                             if (!strlen(simrank_cluster_last_error())) return 100 + code; } while (0)
int main(void) {
    /* 16-byte aligned stand-ins for device memory: nothing below may reach a device */
    static int32_t mem[8] __attribute__((aligned(16)));
    int32_t* one = mem;
    int32_t* other = mem + 4;
    float e[1] = {0.5f};
    const int32_t f32 = SIMRANK_CLUSTER_ROWMAJOR_F32;
    const int32_t big = SIMRANK_CLUSTER_MAX_LEVELS + 1;
    if (simrank_cluster_version() != SIMRANK_CLUSTER_VERSION) return 1;
    /* init: NULL parent, negative or huge n, levels 0 and 9, NULL status */
    BAD(simrank_cluster_init(NULL, 4, 1, one, NULL), 2);
    BAD(simrank_cluster_init(one, -1, 1, one, NULL), 3);
    BAD(simrank_cluster_init(one, (int64_t)1 << 31, 1, one, NULL), 4);
    BAD(simrank_cluster_init(one, 4, 0, one, NULL), 5);
    BAD(simrank_cluster_init(one, 4, big, one, NULL), 6);
    if (!strstr(simrank_cluster_last_error(), "8")) return 7;
    BAD(simrank_cluster_init(one, 4, 1, NULL, NULL), 8);
    /* union: layout, NULL block, stride, shape, alignment of a panel block, NULL edges / parent / status, levels, n */
    BAD(simrank_cluster_union(one, 9, 4, 4, 4, NULL, NULL, e, 1, one, 4, one, NULL), 10);
    BAD(simrank_cluster_union(NULL, f32, 4, 4, 4, NULL, NULL, e, 1, one, 4, one, NULL), 11);
    BAD(simrank_cluster_union(one, f32, 3, 4, 4, NULL, NULL, e, 1, one, 4, one, NULL), 12);
    BAD(simrank_cluster_union(one, SIMRANK_CLUSTER_PANEL_F16, 2, 4, 4, NULL, NULL, e, 1, one, 4, one, NULL), 13);
    BAD(simrank_cluster_union(one, f32, 4, -1, 4, NULL, NULL, e, 1, one, 4, one, NULL), 14);
    BAD(simrank_cluster_union(one + 1, SIMRANK_CLUSTER_PANEL_F32, 4, 4, 4, NULL, NULL, e, 1, one, 4, one, NULL), 15);
    BAD(simrank_cluster_union(one, f32, 4, 4, 4, NULL, NULL, NULL, 1, one, 4, one, NULL), 16);
    BAD(simrank_cluster_union(one, f32, 4, 4, 4, NULL, NULL, e, 1, NULL, 4, one, NULL), 17);
    BAD(simrank_cluster_union(one, f32, 4, 4, 4, NULL, NULL, e, 1, one, 4, NULL, NULL), 18);
    BAD(simrank_cluster_union(one, f32, 4, 4, 4, NULL, NULL, e, 0, one, 4, one, NULL), 19);
    BAD(simrank_cluster_union(one, f32, 4, 4, 4, NULL, NULL, e, big, one, 4, one, NULL), 20);
    BAD(simrank_cluster_union(one, f32, 4, 4, 4, NULL, NULL, e, 1, one, -4, one, NULL), 21);
    /* an empty block or no nodes: nothing to queue */
    if (simrank_cluster_union(NULL, f32, 4, 0, 4, NULL, NULL, e, 1, one, 4, one, NULL) != SIMRANK_CLUSTER_OK) return 22;
    if (simrank_cluster_union(one, f32, 4, 4, 4, NULL, NULL, e, 1, NULL, 0, one, NULL) != SIMRANK_CLUSTER_OK) return 23;
    /* labels: NULL parent / labels / status, labels == parent, levels */
    BAD(simrank_cluster_labels(NULL, 4, 1, other, one, NULL), 30);
    BAD(simrank_cluster_labels(one, 4, 1, NULL, one, NULL), 31);
    BAD(simrank_cluster_labels(one, 4, 1, other, NULL, NULL), 32);
    BAD(simrank_cluster_labels(one, 4, 1, one, one, NULL), 33);
    BAD(simrank_cluster_labels(one, 4, 0, other, one, NULL), 34);
    BAD(simrank_cluster_labels(one, 4, big, other, one, NULL), 35);
    BAD(simrank_cluster_labels(one, -1, 1, other, one, NULL), 36);
    if (simrank_cluster_labels(NULL, 0, 1, NULL, one, NULL) != SIMRANK_CLUSTER_OK) return 37;
    printf("cluster %d ok\n", simrank_cluster_version());
    return 0;
}
''')


# ---- argument checks: no device --------------------------------------------------------------------------------------
def boom(*a, **k):
    raise AssertionError("the device was touched")


class _Csr:
    rowptr, col = np.array([0, 2, 2, 3], dtype=np.int32), np.array([2, 0, 1], dtype=np.int32)


class _Spec:
    csr, rowscale, storage, apriori, evidence_from = _Csr, np.array([0.5, 0.0, 1.0]), "f32", None, None


class _Tables:
    n, k, ids, nbytes = 3, 2, 1, 3 * 2 * 12 + 3 * 8

    def host(self):
        boom()

    def free(self):
        self.ids = None


def guarded_estimator():
    """An estimator holding a model whose device (and whose lists) no argument check may reach."""
    est = SRA.SimRank()
    solver = _neighbors.NeighborSolver(None, [_Spec], [_Tables()])
    solver._make_reader = boom
    est._keep(solver, [(0, ["a", "b", "c"])])
    return est


BAD_THRESHOLDS = [True, False, np.True_, float("nan"), float("inf"), -float("inf"), "0.5", b"1", None, [], (), [0.1] * 9,
                  [0.5, float("nan")], [0.5, True], [0.5, "x"], [[0.5]], {"t": 0.5}.items(), 1 + 2j,
                  10 ** 400, [0.5, -10 ** 400], np.array(True), np.array(float("nan")), np.array("x")]


def test_components_argument_checks_need_no_device(monkeypatch):
    monkeypatch.setattr(_cluster, "roots", boom)
    monkeypatch.setattr(_cluster, "load", boom)
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().components(0.5)
    est = guarded_estimator()
    for bad in BAD_THRESHOLDS:
        with pytest.raises(ValueError, match="threshold"):
            est.components(bad)
        with pytest.raises(ValueError, match="threshold"):
            SRA.SimRank().components(bad)                   # (the argument is judged before the model)
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.components(0.5)
    with pytest.raises(RuntimeError, match="released"):
        est.components([0.5, 0.1])


def test_what_the_threshold_check_accepts():
    for good in (0.5, -3, 0, -0.0, np.float32(0.25), np.int64(2), np.array(0.125), np.array(3)):
        ts, scalar = _cluster.check_thresholds(good)
        assert scalar and ts.dtype == np.float64 and ts.tolist() == [float(good)]
    ts, scalar = _cluster.check_thresholds([0.5, 0.1, 0.5, -1, np.float64(0.01), 3, 2, 1])
    assert not scalar and ts.tolist() == [0.5, 0.1, 0.5, -1.0, 0.01, 3.0, 2.0, 1.0]
    ts, scalar = _cluster.check_thresholds(np.array([0.25]))
    assert not scalar and ts.tolist() == [0.25]
    ts, scalar = _cluster.check_thresholds(x for x in (1, 2))
    assert not scalar and ts.tolist() == [1.0, 2.0]


# ---- the host half: numbering, and the lists of a pruned model -------------------------------------------------------------
def test_numbering_is_by_first_member():
    roots = np.array([[0, 1, 0, 3, 1, 3], [0, 0, 0, 0, 0, 0], [0, 1, 2, 3, 4, 5]])
    assert _cluster.number(roots).tolist() == [[0, 1, 0, 2, 1, 2], [0] * 6, [0, 1, 2, 3, 4, 5]]
    assert _cluster.number(np.empty((2, 0), dtype=np.int64)).shape == (2, 0)


def test_roots_of_edges_on_a_path_a_star_and_loose_nodes():
    rng = np.random.default_rng(1)
    n = 300
    ids = rng.permutation(n)
    path = ids[:200]                                          # a path through shuffled ids: labels travel far
    star = ids[200:260]
    a = np.concatenate([path[:-1], np.full(star.size - 1, star[0])])
    b = np.concatenate([path[1:], star[1:]])
    got = _cluster.roots_of_edges(n, a, b)
    want = CR.labels_of_edges(n, zip(a, b))
    assert np.array_equal(_cluster.number(got[None])[0], want)
    assert got[path].tolist() == [path.min()] * 200 and got[star].tolist() == [star.min()] * 60   # a root is the smallest id
    assert np.array_equal(got[ids[260:]], ids[260:])
    assert _cluster.roots_of_edges(4, [], []).tolist() == [0, 1, 2, 3]


def lists_case():
    """Hand-made lists of 6 nodes, 3 slots: node 2 lists nobody; (4, 1) is listed in one direction only; 0 <-> 3 are
    listed in both with different values; a NaN, a -0.0 and a negative value are kept."""
    ids = np.array([[3, 1, -1], [0, 2, 5], [-1, -1, -1], [5, 4, 0], [1, -1, -1], [2, 0, 4]], dtype=np.int32)
    vals = np.array([[0.5, 0.25, 0], [0.75, np.nan, 0.0], [0, 0, 0], [1.0, 0.5, 0.125], [-0.0, 0, 0], [0.125, -0.5, 1e-9]])
    return ids, vals


THRESHOLDS = [0.75, 0.5, 0.3, 0.125, 1e-9, 1e-300, 0.0, -0.0, -0.25, -0.5, -1.0, 2.0]


def test_the_host_path_of_pruned_lists_equals_the_reference():
    ids, vals = lists_case()
    P = CR.matrix_of_lists(ids, vals)
    for lo in range(0, len(THRESHOLDS), 8):
        ts = THRESHOLDS[lo:lo + 8]
        got = _cluster.number(_cluster.roots_of_lists(ids, vals, ts))
        assert got.dtype == np.int64 and np.array_equal(got, CR.components(P, ts)), ts
    one = lambda t: _cluster.number(_cluster.roots_of_lists(ids, vals, [t]))[0].tolist()
    # 0.3: 0 - 3 (0.5 one way, 0.125 the other), 1 - 0, 3 - 5, 3 - 4; node 2 is alone (a NaN and a 0.125 point at it)
    assert one(0.3) == [0, 0, 1, 0, 0, 0] and one(0.75) == [0, 0, 1, 2, 3, 2] and one(0.125) == [0] * 6
    # 1e-9 is listed by 5 alone: 5 - 4 holds there; (4, 1) holds -0.0 one way and is absent the other: joined from 0.0 down
    assert one(0.6) == [0, 0, 1, 2, 3, 2] and one(0.6)[4] != one(0.6)[1]
    assert one(2.0) == [0, 1, 2, 3, 4, 5] and one(0.0) == [0] * 6 and one(-1.0) == [0] * 6


def test_at_or_below_zero_only_pairs_kept_in_both_directions_can_stay_apart():
    """Three nodes that list each other completely (k = n - 1) with negative values: at t = 0 nobody is joined, just
    below the largest value one pair is; a fourth node that lists nobody is absent everywhere and joins everything."""
    ids = np.array([[1, 2], [0, 2], [0, 1]], dtype=np.int32)
    vals = np.array([[-0.5, -0.25], [-0.75, -0.25], [-1.0, -2.0]])
    P = CR.matrix_of_lists(ids, vals)
    ts = [0.0, -0.25, -0.3, -0.5, -0.75, -1.0, -3.0]
    got = _cluster.number(_cluster.roots_of_lists(ids, vals, ts))
    assert np.array_equal(got, CR.components(P, ts))
    assert got[0].tolist() == [0, 1, 2] and got[1].tolist() == [0, 0, 0] and got[-1].tolist() == [0, 0, 0]
    ids4 = np.array([[1, 2], [0, 2], [0, 1], [-1, -1]], dtype=np.int32)
    vals4 = np.vstack([vals, [0.0, 0.0]])
    got = _cluster.number(_cluster.roots_of_lists(ids4, vals4, ts + [1e-30]))
    assert np.array_equal(got, CR.components(CR.matrix_of_lists(ids4, vals4), ts + [1e-30]))
    assert got[0].tolist() == [0, 0, 0, 0] and got[-1].tolist() == [0, 1, 2, 3]
    # more nodes than twice the slots: one component at t <= 0 without an n x n table
    rng = np.random.default_rng(2)
    n, k = 41, 5
    ids = np.array([rng.permutation(np.delete(np.arange(n), i))[:k] for i in range(n)], dtype=np.int32)
    vals = -rng.random((n, k)) - 0.1
    got = _cluster.number(_cluster.roots_of_lists(ids, vals, [0.0, -0.3, -5.0]))
    assert np.array_equal(got, CR.components(CR.matrix_of_lists(ids, vals), [0.0, -0.3, -5.0])) and not got.any()


# ---- components() of a pruned model on a stand-in for the device ----------------------------------------------------------
class HostOps:
    """``HipOps``'s memory calls on host memory: what ``Tables`` does besides launching kernels."""
    stream = None

    def __init__(self):
        self.live = {}

    def _malloc(self, nbytes):
        buf = np.zeros(max(16, int(nbytes)), dtype=np.uint8)
        self.live[buf.ctypes.data] = buf
        return buf.ctypes.data

    def _free(self, ptr):
        del self.live[ptr]

    def h2d(self, ptr, host):
        import ctypes
        ctypes.memmove(ptr, host.ctypes.data, host.nbytes)

    def d2h(self, host, ptr, nbytes=None):
        import ctypes
        ctypes.memmove(host.ctypes.data, ptr, host.nbytes if nbytes is None else nbytes)

    def put(self, host):
        ptr = self._malloc(host.nbytes)
        self.h2d(ptr, host)
        return ptr

    def synchronize(self):
        pass


class _FullSpec:
    def __init__(self, n):
        from simrank_amd.ingest import CSR
        rowptr = np.arange(n + 1, dtype=np.int32)
        self.csr = CSR(n, n, rowptr, ((np.arange(n) + 1) % n).astype(np.int32), np.ones(n))
        self.rowscale, self.coef, self.lbd = np.ones(n), 0.8, 0.0
        self.evidence_from, self.apriori, self.storage = None, None, "f32"


def test_components_of_a_pruned_model(monkeypatch):
    monkeypatch.setattr(_cluster, "load", boom)              # (a pruned model needs no library)
    ops = HostOps()
    ids, vals = lists_case()
    solver = _neighbors.NeighborSolver(ops, [_FullSpec(6)], [_neighbors.Tables.from_host(ops, ids, vals, np.ones(6))])
    est = SRA.SimRank()._keep(solver, [(0, list("abcdef"))])
    P = CR.matrix_of_lists(ids, vals)
    one = est.components(0.3)
    assert isinstance(one, pd.Series) and one.name == "component" and one.dtype == np.int64
    assert one.index.tolist() == list("abcdef") and one.tolist() == CR.components(P, [0.3])[0].tolist() == [0, 0, 1, 0, 0, 0]
    ts = [0.5, 0.0, 0.75, 0.5, -1, 2.0, 1e-9, 0.3]
    many = est.components(ts)
    assert isinstance(many, pd.DataFrame) and many.index.tolist() == list("abcdef")
    assert many.columns.tolist() == [float(t) for t in ts] and (many.dtypes == np.int64).all()
    assert np.array_equal(many.to_numpy().T, CR.components(P, ts))
    assert np.array_equal(many.iloc[:, 7].to_numpy(), one.to_numpy())
    assert est.kept_neighbors == 3                            # the model is as it was
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.components(0.3)
    assert not ops.live
