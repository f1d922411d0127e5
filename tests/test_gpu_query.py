"""``fit(keep=True)`` on a real MI355X: a kept model answers ``rows`` / ``similarity`` / ``most_similar`` through
libsimrank_query.so BIT-EQUAL to the dense frame / ``top_k`` frame of an identical fit without ``keep``, on every class,
f32 and fp16-held matrices, asymmetric priors, both ``strict_reference`` values, ``LocalWorld(2 | 3)``, odd sizes, banded
requests, and at BASELINE's full sizes; ``frame`` / ``top_k`` / ``pairs`` are the plain fit's hand-backs; lifetime rules.
Tolerances against the reference are the dense frame's own: ``tests/helpers.RTOL`` as in test_gpu_parity.py for f32, and
for ``storage_precision="f64"`` those of test_gpu_f64.py (goldens within 1e-12, the oracle within 1e-11, absolute)."""
import contextlib
import ctypes as C
import io

import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

import simrank_amd.SimRank as SRA
from oracle import simrank_oracle as O
from simrank_amd import _query, synth
from simrank_amd.driver import LocalWorld
from tests.conftest import Golden
from tests.graphs import bipartite_random
from tests.helpers import RTOL, TIME_RE, assert_close

pytestmark = pytest.mark.gpu


def _fit(g, **extra):
    est = getattr(SRA, g.cls)()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = est.fit(g.frame, *g.args, **g.kwargs, **extra)
    return est, res, TIME_RE.sub("Finished in <t>s!", buf.getvalue())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape
    np.testing.assert_array_equal(_bits(got), _bits(want))


def _check_side(kept, dense, topk, group, seed=0, k=None):
    """One side of a kept model against the dense frame and the top-k frame of the identical plain fit."""
    rng = np.random.default_rng(seed)
    labels = list(dense.index)
    n = len(labels)
    kw = {} if group is None else {"group": group}
    # rows: every label, shuffled, some repeated
    pick = list(rng.permutation(n)) + list(rng.integers(0, n, size=min(n, 5)))
    nodes = [labels[i] for i in pick]
    got = kept.rows(nodes, **kw)
    assert list(got.index) == nodes and list(got.columns) == labels
    _same_bits(got.values, dense.values[pick])
    one = kept.rows([labels[-1]], **kw)
    _same_bits(one.values, dense.values[[n - 1]])
    assert kept.rows([], **kw).shape == (0, n)
    # similarity: random pairs, a == b among them
    a = rng.integers(0, n, size=64)
    b = rng.integers(0, n, size=64)
    b[::7] = a[::7]
    sim = kept.similarity([labels[i] for i in a], [labels[i] for i in b], **kw)
    _same_bits(sim, dense.values[a, b])
    assert np.all(sim[::7] == 1.0)
    # most_similar on a subset, in the subset's order
    sub = [labels[i] for i in rng.permutation(n)[:max(1, n // 3)]]
    ms = kept.most_similar(sub, k, **kw)
    want = pd.concat([topk[topk["node"] == s] for s in sub]).reset_index(drop=True) if len(topk) else topk
    assert_frame_equal(ms, want, check_exact=True)
    _same_bits(ms["similarity"].to_numpy(), want["similarity"].to_numpy())
    return got


def _compare_fits(g, k=3, t=0.05, **extra):
    plain, dense, text = _fit(g, **extra)
    _, topk, _ = _fit(g, top_k=k, **extra)
    _, pairs, _ = _fit(g, min_similarity=t, **extra)
    kept, ret, ktext = _fit(g, keep=True, **extra)
    assert ret is kept and ktext == text and kept.converged_at == plain.converged_at
    assert kept.engine_mode == plain.engine_mode
    if isinstance(dense, tuple):
        rows = [_check_side(kept, dense[s], topk[s], s + 1, seed=s, k=k) for s in (0, 1)]
        for f, w in zip(kept.frame(), dense):
            assert_frame_equal(f, w, check_exact=True)
        for f, w in zip(kept.pairs(t), pairs):
            assert_frame_equal(f, w, check_exact=True)
        for f, w in zip(kept.top_k(k), topk):
            assert_frame_equal(f, w, check_exact=True)
        for s in (0, 1):                                                   # again, after the hand-backs
            _check_side(kept, dense[s], topk[s], s + 1, seed=7 + s, k=k)
    else:
        rows = [_check_side(kept, dense, topk, None, k=k)]
        assert_frame_equal(kept.pairs(t), pairs, check_exact=True)
        assert_frame_equal(kept.frame(), dense, check_exact=True)
        assert_frame_equal(kept.top_k(k), topk, check_exact=True)
        assert_frame_equal(kept.frame(), dense, check_exact=True)          # again, after the other hand-backs
        _check_side(kept, dense, topk, None, seed=7, k=k)
    kept.release()
    return kept, text, rows


GOLDENS = ["SimRank_er128", "SimRank_toy5", "SimRank_bts300", "SimRankPP_quirky", "SimRankPP_pl256", "AprioriSimRank_er64",
           "AprioriSimRank_er64_asym", "AprioriSimRank_quirky_asym", "BipartiteSimRank_b5030", "BipartiteSimRank_k10",
           "BipartiteSimRankPP_b40", "BipartitleAprioriSimRank_b40", "BipartitleAprioriSimRank_b40_asym"]


@pytest.mark.parametrize("name", GOLDENS)
def test_kept_model_on_the_goldens(name):
    g = Golden(name)
    kept, text, rows = _compare_fits(g)
    assert text == g.stdout
    if g.kwargs.get("verbose", True):
        assert (kept.converged_at if kept.converged_at is not None else -1) == g.k
    # the reference's own matrix, at the dense frame's tolerance (tests/test_gpu_parity.py: helpers.RTOL)
    for r, key in zip(rows, ("S",) if "S" in g.out else ("S1", "S2")):
        lab = list(g.out["labels" if key == "S" else "labels" + key[1]])
        want = pd.DataFrame(g.out[key], index=lab, columns=lab).loc[list(r.index)]
        assert_close(r.values, want.values, RTOL)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["SimRank_er128", "SimRankPP_quirky", "AprioriSimRank_er64_asym", "BipartiteSimRank_b5030",
                                  "BipartiteSimRankPP_b40"])
def test_kept_model_on_logical_shards(name, world):
    """Against the SHARDED fit's own dense / top-k results (a sharded loop sums in another order than one GPU's)."""
    _compare_fits(Golden(name), world=LocalWorld(world), mode="sparse")


@pytest.mark.parametrize("name", ["SimRank_er128", "SimRankPP_pl256", "SimRankPP_quirky"])
def test_kept_model_on_fp16_held_matrices(name):
    _compare_fits(Golden(name), storage_precision="fp16")


def _close_abs(got, want, tol):
    """tests/test_gpu_f64.py's ``close``: largest absolute error."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max()) if got.size else 0.0
    print("max abs err", err)
    assert err <= tol, err


@pytest.mark.parametrize("name", GOLDENS)
def test_kept_model_in_f64_on_the_goldens(name):
    """``storage_precision="f64"``: the same bit-equalities against the f64 fit's own frames, the golden's console text and
    convergence index, and the golden's matrix within test_gpu_f64.py's 1e-12."""
    g = Golden(name)
    kept, text, rows = _compare_fits(g, storage_precision="f64")
    assert text == g.stdout
    if g.kwargs.get("verbose", True):
        assert (kept.converged_at if kept.converged_at is not None else -1) == g.k
    for r, key in zip(rows, ("S",) if "S" in g.out else ("S1", "S2")):
        lab = list(g.out["labels" if key == "S" else "labels" + key[1]])
        want = pd.DataFrame(g.out[key], index=lab, columns=lab).loc[list(r.index)]
        _close_abs(r.values, want.values, 1e-12)


def test_mid_size_graph_in_f64_against_the_oracle():
    """test_gpu_f64.py's mid-size SimRank++ case and its bound (1e-11) on ``rows`` / ``similarity`` of a kept f64 model."""
    df = synth.powerlaw_directed(1200, 8, 3)
    want = O.fit_simrank_pp(df, verbose=False)
    frame = pd.DataFrame(want["S"], index=want["labels"], columns=want["labels"])
    nodes = [want["labels"][i] for i in np.random.default_rng(0).integers(0, len(frame), 200)]
    with SRA.SimRankPP().fit(df, verbose=False, keep=True, storage_precision="f64") as kept:
        assert kept.converged_at == want["k"]
        got = kept.rows(nodes)
        sim = kept.similarity(nodes, nodes[::-1])
        ms = kept.most_similar(nodes[:50], 12)
    _close_abs(got.values, frame.loc[nodes].values, 1e-11)
    _close_abs(sim, frame.values[frame.index.get_indexer(nodes), frame.index.get_indexer(nodes[::-1])], 1e-11)
    topk = SRA.SimRankPP().fit(df, verbose=False, top_k=12, storage_precision="f64")
    by_node = dict(tuple(topk.groupby("node", sort=False)))
    assert_frame_equal(ms, pd.concat([by_node[s] for s in nodes[:50]]).reset_index(drop=True), check_exact=True)


def test_kept_model_on_fp16_held_shards():
    df = synth.er_directed(256, 0.03, seed=5)
    for world in (2,):
        dense = SRA.SimRankPP().fit(df, verbose=False, storage_precision="fp16", world=LocalWorld(world), iterations=5)
        topk = SRA.SimRankPP().fit(df, verbose=False, storage_precision="fp16", world=LocalWorld(world), iterations=5, top_k=40)
        with SRA.SimRankPP().fit(df, verbose=False, storage_precision="fp16", world=LocalWorld(world), iterations=5,
                                 keep=True) as kept:
            _check_side(kept, dense, topk, None, k=40)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("cls", ["BipartiteSimRank", "BipartiteSimRankPP"])
def test_bipartite_groups_of_different_sizes(cls, strict):
    """n1 != n2, both labelings.  (BipartiteSimRankPP in strict mode raises NumPy's broadcast error there, kept or not.)"""
    df = bipartite_random(70, 45, 0.12, seed=2)
    make = lambda **kw: getattr(SRA, cls)().fit(df, verbose=False, strict_reference=strict, iterations=6, **kw)
    if cls == "BipartiteSimRankPP" and strict:
        with pytest.raises(ValueError, match="broadcast"):
            make(keep=True)
        return
    dense, topk = make(), make(top_k=33)
    kept = make(keep=True)
    for s in (0, 1):
        _check_side(kept, dense[s], topk[s], s + 1, seed=s, k=33)
    kept.release()


@pytest.mark.parametrize("n", [1, 2, 33, 65, 100, 257])
@pytest.mark.parametrize("storage", ["f32", "fp16", "f64"])
def test_sizes_that_stress_the_layouts(n, storage):
    rng = np.random.default_rng(n)
    if n == 1:
        df = pd.DataFrame({"from": [0], "to": [0]})
    else:
        m = 4 * n
        df = pd.DataFrame({"from": rng.integers(0, n, m), "to": rng.integers(0, n, m)})
        df = pd.concat([df, pd.DataFrame({"from": np.arange(n), "to": (np.arange(n) + 1) % n})]).drop_duplicates()
    fit = lambda **kw: SRA.SimRank().fit(df, verbose=False, iterations=5, eps=0, storage_precision=storage, **kw)
    dense = fit()
    assert len(dense) == n
    kept = fit(keep=True)
    for k in sorted({1, max(1, n - 1), 40, n + 5}):
        _check_side(kept, dense, fit(top_k=k), None, seed=k, k=k)
    kept.release()


def test_a_request_larger_than_one_slab_is_banded(monkeypatch):
    df = synth.er_directed(300, 0.03, seed=9)
    dense = SRA.SimRankPP().fit(df, verbose=False)
    labels = list(dense.index)
    with SRA.SimRankPP().fit(df, verbose=False, keep=True) as kept:
        whole = kept.rows(labels)
        monkeypatch.setattr(_query, "SLAB_BYTES", 7 * 8 * 300)        # seven query rows per band
        banded = kept.rows(labels)
        monkeypatch.setattr(_query, "SLAB_BYTES", 1)                  # one row per band
        single = kept.rows(labels[:9])
    _same_bits(whole.values, dense.values)
    _same_bits(banded.values, dense.values)
    _same_bits(single.values, dense.values[:9])
    with SRA.SimRankPP().fit(df, verbose=False, keep=True, world=LocalWorld(3), mode="sparse") as kept:
        want = SRA.SimRankPP().fit(df, verbose=False, world=LocalWorld(3), mode="sparse")
        monkeypatch.setattr(_query, "SLAB_BYTES", 11 * 8 * 300)
        _same_bits(kept.rows(labels).values, want.values)


def test_mid_size_graph_against_the_oracle():
    df = synth.er_directed(1500, 0.004, seed=11)
    want = O.fit_simrank_pp(df, verbose=False)
    frame = pd.DataFrame(want["S"], index=want["labels"], columns=want["labels"])
    rng = np.random.default_rng(0)
    nodes = [want["labels"][i] for i in rng.integers(0, len(frame), 200)]
    with SRA.SimRankPP().fit(df, verbose=False, keep=True) as kept:
        assert kept.converged_at == want["k"]
        got = kept.rows(nodes)
        sim = kept.similarity(nodes, nodes[::-1])
    assert list(got.columns) == want["labels"]
    assert_close(got.values, frame.loc[nodes].values, RTOL)
    assert_close(sim, frame.values[frame.index.get_indexer(nodes), frame.index.get_indexer(nodes[::-1])], RTOL)


def test_float64_row_major_layout_at_the_c_interface():
    """Layout 3 (what a float64 solver holds): rows with a column map, pairs and top-k by id on a device matrix."""
    from simrank_amd.engine import HipOps, check
    ops = HipOps(0)
    rng = np.random.default_rng(4)
    n, ld, k = 70, 72, 40
    host = np.zeros((n, ld))
    host[:, :n] = rng.integers(0, 6, size=(n, n)) / 8 + rng.random((n, n)) * (rng.random((n, n)) < 0.3)
    rows = rng.integers(0, n, 50).astype(np.int32)
    cmap = rng.permutation(n).astype(np.int32)
    ids = rng.permutation(n).astype(np.int32)                    # position -> id
    got = np.full((50, n + 3), -1.0)
    pv, ti, tv = np.empty(50), np.empty((50, k), dtype=np.int32), np.empty((50, k))
    held = []

    def dev(a):
        a = np.ascontiguousarray(a)
        ptr = ops._malloc(a.nbytes)
        held.append(ptr)
        check(ops.lib.simrank_memcpy_h2d(C.c_void_p(ptr), a.ctypes.data, a.nbytes, ops.stream), "simrank_memcpy_h2d")
        return ptr

    def back(a, ptr):
        check(ops.lib.simrank_memcpy_d2h(a.ctypes.data, C.c_void_p(ptr), a.nbytes, ops.stream), "simrank_memcpy_d2h")

    lib, st = _query.load(), ops.stream
    try:
        S, d_rows, d_cmap, d_ids, d_rid = dev(host), dev(rows), dev(cmap), dev(ids), dev(ids[rows])
        d_out, d_pv, d_ti, d_tv = dev(got), dev(pv), dev(ti), dev(tv)
        _query.check(lib.simrank_query_rows(S, 3, ld, n, n, d_rows, 50, d_cmap, n, d_out, n + 3, st), "rows")
        _query.check(lib.simrank_query_pairs(S, 3, ld, n, n, d_rows, d_cmap, 50, d_pv, st), "pairs")
        _query.check(lib.simrank_query_topk(S, 3, ld, n, n, d_rows, d_rid, 50, d_ids, k, d_ti, d_tv, st), "topk")
        back(got, d_out), back(pv, d_pv), back(ti, d_ti), back(tv, d_tv)
        ops.synchronize()
    finally:
        for ptr in held:
            ops._free(ptr)
    _same_bits(got[:, :n].copy(), host[rows][:, cmap])
    assert np.all(got[:, n:] == -1.0)                              # nothing past n_out
    _same_bits(pv, host[rows, cmap[:50]])
    for q, r in enumerate(rows):
        keep = ids != ids[r]
        order = np.lexsort((ids[keep], -host[r, :n][keep]))[:k]
        np.testing.assert_array_equal(ti[q], ids[keep][order])
        np.testing.assert_array_equal(tv[q], host[r, :n][keep][order])


def _device_bytes_in_use():
    from simrank_amd import _f64
    from simrank_amd.engine import HipOps
    HipOps.trim_pool(0)
    free, total = C.c_int64(0), C.c_int64(0)
    _f64.check(_f64.load().simrank_f64_mem_info(C.byref(free), C.byref(total)), "simrank_f64_mem_info")
    return total.value - free.value


def test_lifetime_of_a_kept_model():
    df = synth.er_directed(2048, 0.004, seed=3)
    SRA.SimRankPP().fit(df, verbose=False, top_k=1)                 # (warm: code objects, the engine of this thread,
    with SRA.SimRankPP().fit(df, verbose=False, keep=True) as warm:  # the query library's kernels)
        lab0 = sorted(warm.Nodes)[:2]
        warm.rows(lab0), warm.similarity(lab0, lab0), warm.most_similar(lab0, 2)
    del warm
    before = _device_bytes_in_use()
    est = SRA.SimRankPP()
    assert est.fit(df, verbose=False, keep=True) is est
    labels = sorted(est.Nodes)
    held = _device_bytes_in_use()
    assert held - before >= 3 * 2048 * 2048 * 4                    # the whole plan stays: three N x N matrices and more
    a = est.rows(labels[:40])
    t = est.most_similar(labels[:40], 5)
    s = est.similarity(labels[:40], labels[40:80])
    f = est.frame()
    _same_bits(est.rows(labels[:40]).values, a.values)             # repeated, interleaved: the same bits
    assert_frame_equal(est.most_similar(labels[:40], 5), t, check_exact=True)
    _same_bits(est.similarity(labels[:40], labels[40:80]), s)
    _same_bits(a.values, f.loc[labels[:40]].values)
    first = est._model[0]
    est.fit(df, verbose=False, keep=True, iterations=2)            # a second fit releases the first model
    assert first.plan.get("iterate") == 0
    assert est.converged_at is None
    est.release()
    for call in (lambda: est.rows(labels[:1]), lambda: est.similarity(labels[:1], labels[:1]),
                 lambda: est.most_similar(labels[:1], 1), lambda: est.frame(), lambda: est.top_k(1), lambda: est.pairs(0.5)):
        with pytest.raises(RuntimeError, match="released"):
            call()
    assert est.Evidence.shape == (2048, 2048)                      # the lazy attributes keep working
    with SRA.SimRank().fit(df, verbose=False, keep=True, world=LocalWorld(2), mode="sparse") as w:
        w.rows(labels[:3])
    with pytest.raises(RuntimeError, match="released"):
        w.rows(labels[:3])
    del est, first, w, f
    after = _device_bytes_in_use()
    # back to the value before the fit: the pool is trimmed in both readings, so nothing of a size class is at rest, and
    # the smallest thing a model could leave behind that matters is one N x N block (u8 counts 4 MiB, f32 matrix 16 MiB);
    # the bound is the counts' 4 MiB, which is also twice the driver's 2 MiB allocation granule
    print("device bytes in use: before", before, "held", held, "after", after)
    assert abs(after - before) < 2048 * 2048, (before, held, after)


# ---- full size --------------------------------------------------------------------------------------------------------
def test_config4_rows_and_most_similar_of_1024_nodes():
    """BASELINE.json config 4 (N = 32768): 1024 random nodes of a kept fit against the same rows of a plain fit's dense
    frame and its ``top_k=10`` frame."""
    df = synth.WORKLOADS["pl32768"][0]()
    rng = np.random.default_rng(7)
    dense = SRA.SimRank().fit(df, verbose=False, iterations=4, eps=0)
    labels = list(dense.index)
    pick = rng.integers(0, len(labels), 1024)
    nodes = [labels[i] for i in pick]
    want_rows = dense.values[pick].copy()
    del dense
    topk = SRA.SimRank().fit(df, verbose=False, iterations=4, eps=0, top_k=10)
    with SRA.SimRank().fit(df, verbose=False, iterations=4, eps=0, keep=True) as kept:
        got = kept.rows(nodes)
        ms = kept.most_similar(nodes, 10)
    _same_bits(got.values, want_rows)
    by_node = dict(tuple(topk.groupby("node", sort=False)))
    want = pd.concat([by_node[s] for s in nodes]).reset_index(drop=True)
    assert_frame_equal(ms, want, check_exact=True)


@pytest.mark.parametrize("storage", ["f32", "fp16"])
def test_config5_rows_of_256_nodes_against_the_sampler(storage):
    """BASELINE.json config 5 (SimRank++, N = 65536): no dense frame is ever built; ``rows`` against
    ``simrank_plan_rows_f32`` (an independent route: float32 rows copied to the host, widened there)."""
    df = synth.WORKLOADS["pl65536"][0]()
    with SRA.SimRankPP().fit(df, verbose=False, iterations=3, eps=0, storage_precision=storage, keep=True) as kept:
        labels = list(kept._model[1][0][1])
        assert len(labels) == 65536
        pick = np.random.default_rng(5).integers(0, 65536, 256)
        got = kept.rows([labels[i] for i in pick])
        want = kept._model[0].plan.rows(pick.astype(np.int32)).astype(np.float64)
        sim = kept.similarity([labels[i] for i in pick], [labels[i] for i in pick[::-1]])
    _same_bits(got.values, want)
    _same_bits(sim, want[np.arange(256), pick[::-1]])
    assert np.all(got.values[np.arange(256), pick] == 1.0)
