"""libsimrank_neighbors.so (include/simrank_neighbors.h) and ``prune`` on a machine without a GPU: header, binding and
exports agree, the header is plain C99 and stands alone, every entry point refuses bad arguments without a device, the
"form": "neighbors" header of a saved model round-trips and a damaged pruned file is refused before any device work, and
``prune``'s argument checks run before any device work."""
import io
import re

import numpy as np
import pytest

import simrank_amd
import simrank_amd.SimRank as SRA
from simrank_amd import _lib, _model, _neighbors, _query
from tests import companion_abi as A


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_neighbors) == _neighbors.VERSION == 1
    text = A.header(_neighbors)
    assert re.search(r"#define SIMRANK_NEIGHBORS_MAX_K %d\b" % _neighbors.MAX_K, text) and _neighbors.MAX_K >= 1024
    assert re.search(r"#define SIMRANK_NEIGHBORS_CHUNK %d\b" % _neighbors.CHUNK, text)
    assert re.search(r"#define SIMRANK_NEIGHBORS_MAX_BLOCKS \(1 << 24\)", text) and _neighbors.MAX_BLOCKS == 1 << 24
    A.assert_header_stands_alone(_neighbors)


def test_the_layout_codes_are_the_shared_ones():
    assert A.layout_codes(_neighbors) == A.layout_codes(_query)


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_neighbors)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_neighbors)


def test_the_main_library_is_unchanged():
    version, names, exports = A.main_library(_neighbors)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_every_entry_refuses_bad_arguments_without_a_device(tmp_path):
    assert "neighbors 1 ok" in A.run_c99(_neighbors, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_neighbors.h"
#define BAD(call, code) do { if ((call) != SIMRANK_NEIGHBORS_ERR_INVALID) return code; \
                             if (!strlen(simrank_neighbors_last_error())) return 100 + code; } while (0)
int main(void) {
    int64_t ptr[2] = {0, 0};
    int32_t one[1] = {0};
    double w[1] = {1.0};
    const int32_t f32 = SIMRANK_NEIGHBORS_ROWMAJOR_F32;
    const int32_t big = SIMRANK_NEIGHBORS_MAX_K + 1;
    if (simrank_neighbors_version() != SIMRANK_NEIGHBORS_VERSION) return 1;
    /* select: layout, NULL block, stride, k = 0, k above the maximum, NULL outputs */
    BAD(simrank_neighbors_select(one, 9, 4, 4, 4, one, one, 1, NULL, 1, one, w, NULL), 2);
    BAD(simrank_neighbors_select(NULL, f32, 4, 4, 4, one, one, 1, NULL, 1, one, w, NULL), 3);
    BAD(simrank_neighbors_select(one, SIMRANK_NEIGHBORS_PANEL_F16, 2, 4, 4, one, one, 1, NULL, 1, one, w, NULL), 4);
    BAD(simrank_neighbors_select(one, f32, 4, 4, 4, one, one, 1, NULL, 0, one, w, NULL), 5);
    BAD(simrank_neighbors_select(one, f32, 4, 4, 4, one, one, 1, NULL, big, one, w, NULL), 6);
    if (!strstr(simrank_neighbors_last_error(), "4096")) return 7;
    BAD(simrank_neighbors_select(one, f32, 4, 4, 4, NULL, one, 1, NULL, 1, one, w, NULL), 8);
    BAD(simrank_neighbors_select(one, f32, 4, 4, 4, one, one, 1, NULL, 1, NULL, w, NULL), 9);
    BAD(simrank_neighbors_select(one, f32, 4, 4, 4, one, one, -1, NULL, 1, one, w, NULL), 10);
    if (simrank_neighbors_select(one, f32, 4, 4, 4, NULL, NULL, 0, NULL, 1, NULL, NULL, NULL) != SIMRANK_NEIGHBORS_OK) return 11;
    /* rows */
    BAD(simrank_neighbors_rows(NULL, w, w, 4, 1, one, 1, w, 4, NULL), 20);
    BAD(simrank_neighbors_rows(one, w, w, 4, 0, one, 1, w, 4, NULL), 21);
    BAD(simrank_neighbors_rows(one, w, w, 4, big, one, 1, w, 4, NULL), 22);
    BAD(simrank_neighbors_rows(one, w, w, 4, 1, one, 1, w, 3, NULL), 23);            /* ld_out below n */
    BAD(simrank_neighbors_rows(one, w, w, 4, 1, NULL, 1, w, 4, NULL), 24);
    BAD(simrank_neighbors_rows(one, w, w, 4, 1, one, 1, NULL, 4, NULL), 25);
    BAD(simrank_neighbors_rows(one, w, w, 2000000000, 1, one, 20000, w, 2000000000, NULL), 26);
    if (!strstr(simrank_neighbors_last_error(), "bands")) return 27;
    if (simrank_neighbors_rows(one, w, w, 4, 1, NULL, 0, NULL, 4, NULL) != SIMRANK_NEIGHBORS_OK) return 28;
    /* pairs */
    BAD(simrank_neighbors_pairs(one, NULL, w, 4, 1, one, one, 1, w, NULL), 30);
    BAD(simrank_neighbors_pairs(one, w, w, 4, 0, one, one, 1, w, NULL), 31);
    BAD(simrank_neighbors_pairs(one, w, w, 4, big, one, one, 1, w, NULL), 32);
    BAD(simrank_neighbors_pairs(one, w, w, 4, 1, one, NULL, 1, w, NULL), 33);
    BAD(simrank_neighbors_pairs(one, w, w, 4, 1, one, one, 1, NULL, NULL), 34);
    BAD(simrank_neighbors_pairs(one, w, w, 4, 1, one, one, -1, w, NULL), 35);
    if (simrank_neighbors_pairs(one, w, w, 4, 1, NULL, NULL, 0, NULL, NULL) != SIMRANK_NEIGHBORS_OK) return 36;
    /* score */
    BAD(simrank_neighbors_score(one, w, NULL, 4, 1, ptr, one, w, 1, NULL, NULL, w, 4, NULL), 40);
    BAD(simrank_neighbors_score(one, w, w, 4, 0, ptr, one, w, 1, NULL, NULL, w, 4, NULL), 41);
    BAD(simrank_neighbors_score(one, w, w, 4, big, ptr, one, w, 1, NULL, NULL, w, 4, NULL), 42);
    BAD(simrank_neighbors_score(one, w, w, 4, 1, ptr, one, w, 1, NULL, NULL, w, 3, NULL), 43);
    BAD(simrank_neighbors_score(one, w, w, 4, 1, ptr, one, w, 1, ptr, NULL, w, 4, NULL), 44);   /* excl_ptr alone */
    BAD(simrank_neighbors_score(one, w, w, 4, 1, NULL, one, w, 1, NULL, NULL, w, 4, NULL), 45);
    BAD(simrank_neighbors_score(one, w, w, 4, 1, ptr, one, w, 1, NULL, NULL, NULL, 4, NULL), 46);
    BAD(simrank_neighbors_score(one, w, w, 2000000000, 1, ptr, one, w, 20000, NULL, NULL, w, 2000000000, NULL), 47);
    if (simrank_neighbors_score(one, w, w, 4, 1, ptr, one, w, 0, NULL, NULL, NULL, 4, NULL) != SIMRANK_NEIGHBORS_OK) return 48;
    printf("neighbors %d ok\n", simrank_neighbors_version());
    return 0;
}
''')


# ---- the file ------------------------------------------------------------------------------------------------------------
def pruned_file(n=5, k=2, **changes):
    """(bytes of a pruned model's file with zeroed arrays, its meta): SimRank, n nodes, k kept."""
    side = dict(n=n, n_src=n, nnz=3, k=k, C=0.8, lbd=0.0, evidence=False, prior=False, labels=list(range(n)), label_kind="py")
    meta = {"class": "SimRank", "weighted": False, "strict": False, "storage": "f32", "form": "neighbors", "sides": [side]}
    arrays = {"nbr_ids0": ("<i4", [n, k]), "nbr_vals0": ("<f8", [n, k]), "diag0": ("<f8", [n]), "rowptr0": ("<i4", [n + 1]),
              "col0": ("<i4", [3]), "rowscale0": ("<f8", [n])}
    for name, change in changes.items():
        if change is None:
            del arrays[name]
        else:
            arrays[name] = change
    f = io.BytesIO()
    where = _model.write_header(f, meta, [(name, d, s) for name, (d, s) in arrays.items()])
    end = max(o + b for o, b in where.values())
    f.write(b"\0" * (end - f.tell()))
    return f.getvalue(), meta


def parse(data):
    return _model.parse_header(io.BytesIO(data), file_size=len(data))


def test_the_neighbors_header_round_trips():
    data, meta = pruned_file()
    got, arrays = parse(data)
    assert got["form"] == "neighbors" and got["format"] == _model.FORMAT_VERSION == 1 and got["sides"][0]["k"] == 2
    assert arrays["nbr_ids0"]["dtype"] == "<i4" and arrays["nbr_ids0"]["shape"] == [5, 2]
    assert arrays["nbr_vals0"]["dtype"] == "<f8" and arrays["diag0"]["shape"] == [5]
    _model.check_meta(got, arrays)
    # a file without "form" is the dense form: it asks for iterate0, as before
    dense = {k: v for k, v in got.items() if k != "form"}
    with pytest.raises(ValueError, match="iterate0|layout"):
        _model.check_meta(dense, arrays)
    layout, stride, nbytes = _model.block_shape("f32", 5)
    dense["sides"] = [dict(got["sides"][0], layout=layout, stride=stride)]
    f = io.BytesIO()
    _model.write_header(f, {k: v for k, v in dense.items() if k not in ("format", "arrays")},
                        [("iterate0", "<f4", [nbytes // 4]), ("rowptr0", "<i4", [6]), ("col0", "<i4", [3]), ("rowscale0", "<f8", [5])])
    f.write(b"\0" * (nbytes + 256))
    m, a = parse(f.getvalue())
    assert "form" not in m
    _model.check_meta(m, a)
    with pytest.raises(ValueError, match="unknown form"):
        _model.check_meta(dict(got, form="lists"), arrays)


def boom(*a, **k):
    raise AssertionError("the device was touched")


@pytest.mark.parametrize("what,changes,message", [
    ("missing", {"nbr_vals0": None}, "no array 'nbr_vals0'"),
    ("dtype", {"nbr_ids0": ("<f4", [5, 2])}, "nbr_ids0"),
    ("shape", {"nbr_vals0": ("<f8", [5, 3])}, "nbr_vals0"),
    ("diag", {"diag0": ("<f8", [4])}, "diag0"),
])
def test_a_damaged_pruned_file_is_refused_before_any_device_work(what, changes, message, tmp_path, monkeypatch):
    monkeypatch.setattr(SRA, "_default_ops_factory", boom, raising=False)
    import simrank_amd.estimators as E
    monkeypatch.setattr(E, "_default_ops_factory", boom)
    data, _ = pruned_file(**changes)
    path = tmp_path / "bad.bin"
    path.write_bytes(data)
    with pytest.raises(ValueError, match=message):
        simrank_amd.load_model(path)


def test_a_truncated_or_disagreeing_pruned_file_is_refused(tmp_path, monkeypatch):
    import simrank_amd.estimators as E
    monkeypatch.setattr(E, "_default_ops_factory", boom)
    data, meta = pruned_file()
    path = tmp_path / "cut.bin"
    path.write_bytes(data[:len(data) - 30])
    with pytest.raises(ValueError, match="truncated"):
        simrank_amd.load_model(path)
    for k in (0, 5, _neighbors.MAX_K + 1, "2", None):          # (5 nodes keep at most 4)
        got, arrays = parse(data)
        got["sides"][0]["k"] = k
        with pytest.raises(ValueError, match="kept neighbours|nbr_"):
            _model.check_meta(got, arrays)
    # an id outside the nodes: found on the host, before the device
    ids = np.zeros((5, 2), dtype="<i4")
    ids[3, 1] = 5
    _, arrays = parse(data)
    data = bytearray(data)
    for name, host in (("nbr_ids0", ids), ("rowptr0", np.array([0, 1, 2, 3, 3, 3], dtype="<i4"))):
        at = arrays[name]["offset"]
        data[at:at + host.nbytes] = host.tobytes()
    path.write_bytes(bytes(data))
    with pytest.raises(ValueError, match="neighbour id outside"):
        simrank_amd.load_model(path)


# ---- argument checks: no device --------------------------------------------------------------------------------------
class _Csr:
    rowptr, col = np.array([0, 2, 2, 3], dtype=np.int32), np.array([2, 0, 1], dtype=np.int32)


class _Spec:
    csr, rowscale, storage, apriori, evidence_from = _Csr, np.array([0.5, 0.0, 1.0]), "f32", None, None


class _Tables:
    n, k, ids, nbytes = 3, 2, 1, 3 * 2 * 12 + 3 * 8

    def free(self):
        self.ids = None


def pruned_estimator():
    """An estimator holding a ``NeighborSolver`` whose device is never reached by what the argument checks do."""
    est = SRA.SimRank()
    solver = _neighbors.NeighborSolver(None, [_Spec], [_Tables()])
    solver._make_reader = boom
    solver.truncated = boom
    est._keep(solver, [(0, ["a", "b", "c"])])
    return est


def test_prune_argument_checks_need_no_device(monkeypatch):
    monkeypatch.setattr(_neighbors, "prune", boom)
    monkeypatch.setattr(_neighbors, "select", boom)
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().prune(3)
    assert SRA.SimRank().kept_neighbors is None
    est = pruned_estimator()
    assert est.kept_neighbors == 2 and est.device_bytes == 3 * 2 * 12 + 3 * 8
    for bad in (0, -1, 2.5, True, "3", None):
        with pytest.raises(ValueError, match="k must be a positive integer"):
            est.prune(bad)
        with pytest.raises(ValueError, match="k must be a positive integer"):
            SRA.SimRank().prune(bad)
    assert est.prune(2) is est and est.prune(7) is est           # (7 clamps to the N - 1 = 2 the model keeps)
    assert est.compact() is est
    with pytest.raises(ValueError, match="pruned model holds float64"):
        est.compact(precision="fp16")
    with pytest.raises(ValueError, match="precision must be"):
        est.compact(precision="bf16")
    with pytest.raises(ValueError, match="fold in before"):
        est.fold_in([["a"]])
    # a model of more nodes than it keeps neighbours of: asking for more names what is kept
    wide = pruned_estimator()
    wide._model[0].n = [9]
    wide._model = (wide._model[0], [(0, list("abcdefghi"))])
    for call in (lambda: wide.prune(3), lambda: wide.most_similar(["a"], 3), lambda: wide.top_k(3)):
        with pytest.raises(ValueError, match="kept_neighbors = 2"):
            call()
    with pytest.raises(ValueError, match="at most 4096"):
        _neighbors.check_prune_k(5000, [100, 6000])
    assert _neighbors.check_prune_k(5000, [100, 4097]) == 5000
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.prune(1)


# ---- the host half of a pruned model, on a stand-in for the device -------------------------------------------------------
class HostOps:
    """``HipOps``'s memory calls on host memory: what ``Tables``, ``NeighborSolver.pairs`` / ``topk_of`` / ``truncated`` and
    ``save`` / ``load_file`` do besides launching kernels."""
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


def test_the_host_half_of_a_pruned_model(tmp_path, monkeypatch):
    import simrank_amd.estimators as E
    ops = HostOps()
    monkeypatch.setattr(E, "_default_ops_factory", lambda device: lambda rank: ops)
    n, k = 6, 3
    ids = np.array([[3, 1, -1], [0, 2, 5], [-1, -1, -1], [5, 4, 0], [1, -1, -1], [2, 0, 4]], dtype=np.int32)
    vals = np.array([[0.5, 0.25, 0], [0.75, 0.75, 0.0], [0, 0, 0], [1.0, 0.5, 0.5], [-0.0, 0, 0], [0.125, 0.125, 1e-9]])
    diag = np.arange(1.0, n + 1)
    solver = _neighbors.NeighborSolver(ops, [_FullSpec(n)], [_neighbors.Tables.from_host(ops, ids, vals, diag)])
    est = SRA.SimRank()._keep(solver, [(0, list("abcdef"))])
    assert est.kept_neighbors == 3 and est.device_bytes == n * k * 12 + n * 8
    # the first k2 entries of the lists, a few nodes (row copies) and all of them (one copy of the tables)
    got = est.most_similar(["d", "c"], 2)
    assert got["node"].tolist() == ["d", "d"] and got["neighbor"].tolist() == ["f", "e"] and got["similarity"].tolist() == [1.0, 0.5]
    top = est.top_k(1)
    assert top["node"].tolist() == list("abdef") and top["neighbor"].tolist() == list("dafbc")
    assert np.signbit(top["similarity"].to_numpy()[3])                 # (-0.0 keeps its bits)
    # pairs: kept entries >= t, neighbours ascending by position within a node
    pairs = est.pairs(0.5)
    assert pairs["node"].tolist() == list("abbddd") and pairs["neighbor"].tolist() == list("dacaef")
    assert pairs["similarity"].tolist() == [0.5, 0.75, 0.75, 0.5, 0.5, 1.0]
    with pytest.raises(ValueError, match="max_pairs=2"):
        est.pairs(0.5, max_pairs=2)
    # save -> load: the same tables, the same header facts
    path = tmp_path / "pruned.bin"
    est.save(path)
    loaded = simrank_amd.load_model(path)
    assert type(loaded) is SRA.SimRank and loaded.kept_neighbors == 3
    li, lv, ld = loaded._model[0].tables[0].host()
    assert np.array_equal(li, ids) and np.array_equal(lv.view(np.uint64), vals.view(np.uint64)) and np.array_equal(ld, diag)
    with pytest.raises(AttributeError, match="loaded from a file, not fitted"):
        loaded.Graph
    with open(path, "rb") as f:
        meta, arrays = _model.parse_header(f)
    assert meta["form"] == "neighbors" and meta["sides"][0]["k"] == 3 and "iterate0" not in arrays
    # pruning again cuts the lists; more than is kept is refused
    assert loaded.prune(2) is loaded and loaded.kept_neighbors == 2
    ci, cv, _ = loaded._model[0].tables[0].host()
    assert np.array_equal(ci, ids[:, :2]) and np.array_equal(cv, vals[:, :2])
    with pytest.raises(ValueError, match="kept_neighbors = 2"):
        loaded.prune(3)
    tables = loaded._model[0].tables
    loaded.release()
    est.release()
    assert all(t.ids is None for t in tables) and not ops.live            # everything was freed
