"""``compact()``, ``save()`` and ``load_model()`` on a real MI355X: a kept model cut down to one matrix per side
(libsimrank_model.so) answers every query BIT-EQUAL to the kept model it came from and to the identical fit without
``keep`` — every class, weighted fits, asymmetric priors, fp16-held and float64 storage, ``LocalWorld(2 | 3)``, sizes at
the edges of the 32- and 64-column panels and of a workgroup's run, and one size past 2^31 elements; the f32 -> fp16
narrowing is the NumPy statement of its rounding, with binary16's error bound; a saved model comes back with the same
answers and the same label types."""
import contextlib
import io

import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

import simrank_amd
import simrank_amd.SimRank as SRA
from simrank_amd import _model, engine
from simrank_amd.driver import LocalWorld
from tests.conftest import Golden
from tests.graphs import bipartite_random

pytestmark = pytest.mark.gpu

UPDATES = 3


def ring(n, extra, seed, weighted=False, label=lambda i: i):
    """A directed graph on EXACTLY n nodes: a ring (a self-loop for n = 1) and ``extra`` random edges."""
    rng = np.random.default_rng(seed)
    e = {(i, (i + 1) % n) for i in range(n)}
    for a, b in zip(rng.integers(0, n, size=extra), rng.integers(0, n, size=extra)):
        e.add((int(a), int(b)))
    e = sorted(e)
    order = rng.permutation(len(e))
    df = pd.DataFrame({"from": [label(e[i][0]) for i in order], "to": [label(e[i][1]) for i in order]})
    if weighted:
        df["weight"] = rng.integers(1, 6, size=len(e))
    return df


def prior(n, seed, symmetric=True, scale=0.5):
    a = np.random.default_rng(seed).random((n, n)) * scale
    return (a + a.T) / 2 if symmetric else a


def fit(cls, df, *args, **kw):
    est = getattr(SRA, cls)()
    with contextlib.redirect_stdout(io.StringIO()):
        res = est.fit(df, *args, iterations=UPDATES, eps=1e-30, verbose=False, **kw)
    return est, res


def fold_args(model, bip, weighted, group):
    """Three new nodes joining ``group``: neighbour lists of fitted labels of the side the update reads."""
    frames = model.frame()
    src = (frames[2 - group] if bip else frames)
    labels = list(src.index)
    rng = np.random.default_rng(11 + group)
    lists = [[labels[i] for i in rng.permutation(len(labels))[:min(len(labels), m)]] for m in (1, 3, 0)]
    kw = {"weights": [list(rng.integers(1, 5, size=len(one)).astype(float)) for one in lists]} if weighted else {}
    if bip:
        kw["group"] = group
    return lists, kw


def snapshot(model, bip, weighted=False, k=3, t=0.01):
    """Every query of a kept model, on fixed arguments."""
    out = {}
    frames = model.frame()
    for s, frame in enumerate(frames if bip else (frames,)):
        kw = {"group": s + 1} if bip else {}
        labels = list(frame.index)
        n = len(labels)
        rng = np.random.default_rng(5 + s)
        out["rows", s] = model.rows(labels, **kw)
        a, b = rng.integers(0, n, size=64), rng.integers(0, n, size=64)
        out["similarity", s] = model.similarity([labels[i] for i in a], [labels[i] for i in b], **kw)
        sub = [labels[i] for i in rng.permutation(n)[:max(1, n // 3)]]
        out["most_similar", s] = model.most_similar(sub, k, **kw)
        lists, fkw = fold_args(model, bip, weighted, s + 1)
        try:
            out["fold_in", s] = model.fold_in(lists, **fkw)
            out["fold_in_top_k", s] = model.fold_in(lists, top_k=2, **fkw)
        except ValueError as e:                 # (strict_reference=True has no fold_in(group=2): the same refusal both times)
            assert bip and s == 1 and "strict_reference" in str(e)
            out["fold_in", s] = str(e)
    out["frame"], out["top_k"], out["pairs"] = frames, model.top_k(k), model.pairs(t)
    return out


def same(got, want, what=""):
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and len(got) == len(want)
        for g, w in zip(got, want):
            same(g, w, what)
    elif isinstance(want, pd.DataFrame):
        assert_frame_equal(got, want, check_exact=True, obj=str(what))
        for c in want.columns:
            if want[c].dtype == np.float64:
                assert np.array_equal(got[c].to_numpy().view(np.uint64), want[c].to_numpy().view(np.uint64)), what
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and np.array_equal(got, want), what
    else:
        assert got == want, what


def same_snapshots(got, want):
    assert got.keys() == want.keys()
    for key in want:
        same(got[key], want[key], key)


def block_bytes(storage, sizes):
    """N x stride x itemsize summed over sides: f32 rows padded to 16 bytes, fp16-held 64-column panels of N rows."""
    if storage == "fp16":
        return sum(-(-n // 64) * 64 * n * 2 for n in sizes)
    item = 8 if storage == "f64" else 4
    unit = 16 // item
    return sum(n * (-(-n // unit) * unit) * item for n in sizes)


def check_compact(cls, df, *args, weighted=False, storage="f32", **kw):
    bip = "ipartit" in cls
    if weighted:
        kw["weighted"] = True
    if storage != "f32":
        kw["storage_precision"] = storage
    _, dense = fit(cls, df, *args, **kw)
    model, ret = fit(cls, df, *args, keep=True, **kw)
    assert ret is model
    before = snapshot(model, bip, weighted)
    same(before["frame"], dense, "kept frame against the fit without keep")
    old = model._model[0]
    assert model.compact() is model
    solver = model._model[0]
    assert isinstance(solver, _model.DetachedSolver) and solver is not old
    same_snapshots(snapshot(model, bip, weighted), before)
    same(model.frame(), dense, "compact frame against the fit without keep")
    sizes = [len(f) for f in (dense if bip else (dense,))]
    assert model.device_bytes == block_bytes(storage, sizes)
    assert model.compact() is model and model._model[0] is solver          # a second compact() is a no-op
    model.release()
    with pytest.raises(RuntimeError, match="released"):
        model.rows([])
    with pytest.raises(RuntimeError, match="released"):
        model.compact()
    return model, old


# ---- every class ---------------------------------------------------------------------------------------------------------
def test_compact_simrank_releases_the_plan():
    model, old = check_compact("SimRank", ring(65, 130, 1))
    with pytest.raises(ValueError, match="released"):
        engine._iterate_block(old.plan.get)


def test_compact_simrank_pp_keeps_the_evidence():
    df = ring(65, 130, 2)
    plain, _ = fit("SimRankPP", df)
    want = plain.Evidence
    model, _ = fit("SimRankPP", df, keep=True)
    model.compact()
    same(model.Evidence, want)
    model.release()
    check_compact("SimRankPP", df)


def test_compact_apriori():
    check_compact("AprioriSimRank", ring(64, 130, 3), prior(64, 3))


def test_compact_apriori_with_an_asymmetric_prior():
    check_compact("AprioriSimRank", ring(65, 130, 4), prior(65, 4, symmetric=False))


@pytest.mark.parametrize("cls", ["BipartiteSimRank", "BipartiteSimRankPP"])
@pytest.mark.parametrize("strict", [True, False])
def test_compact_bipartite(cls, strict):
    if cls == "BipartiteSimRankPP" and strict:
        df = bipartite_random(33, 33, 0.15, 5)      # (the reference's quirk Q2 needs sides of equal size)
    else:
        df = bipartite_random(33, 65, 0.15, 5)
    check_compact(cls, df, strict_reference=strict)


def test_compact_bipartite_apriori_with_asymmetric_priors():
    df = bipartite_random(33, 65, 0.15, 6)
    check_compact("BipartitleAprioriSimRank", df, prior(33, 6, symmetric=False), prior(65, 7), strict_reference=False)


def test_compact_weighted_fits():
    check_compact("SimRankPP", ring(33, 70, 8, weighted=True), weighted=True)
    check_compact("BipartiteSimRankPP", bipartite_random(33, 65, 0.15, 9), weighted=True, strict_reference=False)


# ---- storage, worlds, sizes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "fp16", "f64"])
@pytest.mark.parametrize("n", [1, 2, 31, 33, 64, 65, 257, 1025])
def test_compact_at_the_edges_of_panels_and_runs(n, storage):
    check_compact("SimRankPP", ring(n, 2 * n, 100 + n), storage=storage)


def test_compact_float64_bipartite_and_prior():
    check_compact("BipartiteSimRankPP", bipartite_random(33, 65, 0.15, 12), storage="f64", strict_reference=False)
    check_compact("AprioriSimRank", ring(65, 130, 13), prior(65, 13, symmetric=False), storage="f64")


@pytest.mark.parametrize("world", [2, 3])
def test_compact_on_logical_shards(world):
    """The result is a one-block model: one pack per rank's column block into the same destination."""
    check_compact("SimRank", ring(65, 130, 14), world=LocalWorld(world), mode="sparse")
    check_compact("SimRankPP", ring(257, 600, 15), world=LocalWorld(world), mode="sparse")
    check_compact("BipartiteSimRankPP", bipartite_random(33, 65, 0.15, 16), world=LocalWorld(world), mode="sparse",
                  strict_reference=False)
    check_compact("AprioriSimRank", ring(65, 130, 17), prior(65, 17, symmetric=False), world=LocalWorld(world), mode="sparse")


def test_compact_on_fp16_held_shards():
    check_compact("SimRankPP", ring(384, 900, 18), storage="fp16", world=LocalWorld(2), mode="sparse")
    check_compact("SimRankPP", ring(384, 900, 18), storage="fp16", world=LocalWorld(3), mode="sparse")


# ---- f32 -> fp16 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [None, 2])
def test_compact_to_fp16_is_the_numpy_rounding(world):
    """rows(all) after ``compact(precision="fp16")`` of an f32 model, bit for bit: binary16 of x * 2^14 (round to nearest
    even), widened as every fp16-held value is.  binary16 has 11 significant bits and its smallest subnormal is 2^-24, so
    with the 2^14 scale the relative error is at most 2^-11 from 2^-28 up and the absolute error at most 2^-39 below."""
    kw = {} if world is None else {"world": LocalWorld(world), "mode": "sparse"}
    model, _ = fit("SimRankPP", ring(257, 600, 19), keep=True, **kw)
    labels = list(model.frame().index)
    x64 = model.rows(labels).to_numpy()
    x = x64.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), x64)
    assert model.compact(precision="fp16") is model
    assert model._model[0].storage == "fp16" and model.device_bytes == block_bytes("fp16", [257])
    got = model.rows(labels).to_numpy()
    want = (np.float16(x * np.float32(16384)).astype(np.float32) * np.float32(2 ** -14)).astype(np.float64)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    big = np.abs(x64) >= 2.0 ** -28
    err = np.abs(got - x64)
    print("max rel err", float((err[big] / np.abs(x64[big])).max()), "max abs err below 2^-28",
          float(err[~big].max()) if (~big).any() else 0.0)
    assert np.all(err[big] <= np.abs(x64[big]) * 2.0 ** -11)
    assert np.all(err[~big] <= 2.0 ** -39)
    assert model.compact(precision="fp16") is model                         # idempotent
    same(model.frame().to_numpy(), want)
    model.release()


def test_compact_to_fp16_refuses_float64_and_overflow():
    model, _ = fit("SimRank", ring(33, 70, 20), keep=True, storage_precision="f64")
    before = model.rows(list(model.frame().index))
    with pytest.raises(ValueError, match="float64"):
        model.compact(precision="fp16")
    same(model.rows(list(before.index)), before)
    model.release()
    # prior entries of 8 at lbd = 0.9: similarities near 7.2, past the fp16-held form's 3.998
    n = 33
    model, _ = fit("AprioriSimRank", ring(n, 70, 21), np.full((n, n), 8.0), 0.8, 0.9, keep=True)
    labels = list(model.frame().index)
    before = model.rows(labels)
    assert before.to_numpy().max() > 4
    count = int((np.abs(before.to_numpy()) * 16384 >= 65520).sum())
    old = model._model[0]
    with pytest.raises(ValueError, match=rf"\b{count} values"):
        model.compact(precision="fp16")
    assert model._model[0] is old
    same(model.rows(labels), before)
    model.release()


# ---- save / load ---------------------------------------------------------------------------------------------------------
def check_save_load(model, path, bip, weighted=False, compact_first=False):
    if compact_first:
        model.compact()
    kept = model._model[0]
    want = snapshot(model, bip, weighted)
    model.save(path)
    assert model._model[0] is kept                                           # saving does not change the model
    same_snapshots(snapshot(model, bip, weighted), want)
    with simrank_amd.load_model(path) as loaded:
        assert type(loaded) is type(model) and isinstance(loaded._model[0], _model.DetachedSolver)
        for (_, a), (_, b) in zip(loaded._model[1], model._model[1]):
            assert a == b and [type(x) for x in a] == [type(x) for x in b]
        same_snapshots(snapshot(loaded, bip, weighted), want)
        assert loaded.converged_at == model.converged_at
        for name in ("Graph", "Evidence", "Weight", "Graph_N1_N2", "Evidence_N1", "Weight_N2"):
            if hasattr(type(loaded), name):
                with pytest.raises(AttributeError, match="loaded"):
                    getattr(loaded, name)
    with pytest.raises(RuntimeError, match="released"):
        loaded.rows([])
    model.release()


@pytest.mark.parametrize("compact_first", [False, True])
def test_save_and_load_a_directed_pp_fit(tmp_path, compact_first):
    model, _ = fit("SimRankPP", ring(65, 130, 22), keep=True)
    check_save_load(model, tmp_path / "pp.simrank", False, compact_first=compact_first)


def test_save_and_load_a_bipartite_fit_with_str_labels(tmp_path):
    df = bipartite_random(33, 65, 0.15, 23)
    df["user"] = ["u%d" % u for u in df["user"]]
    df["item"] = ["item-%d" % i for i in df["item"]]
    model, _ = fit("BipartiteSimRankPP", df, keep=True, strict_reference=False)
    assert all(type(x) is str for _, lab in model._model[1] for x in lab)
    check_save_load(model, tmp_path / "bip.simrank", True)


def test_save_and_load_the_bigints_golden_and_python_big_ints(tmp_path):
    g = Golden("BipartiteSimRankPP_bigints")
    est = getattr(SRA, g.cls)()
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(g.frame, *g.args, **g.kwargs, keep=True)
    check_save_load(est, tmp_path / "golden.simrank", True, weighted=bool(g.kwargs.get("weighted", False)))
    df = ring(33, 70, 24, label=lambda i: 2 ** 70 + 977 * i)
    assert df["from"].dtype == object
    model, _ = fit("SimRank", df, keep=True, storage_precision="fp16")
    assert all(type(x) is int for x in model._model[1][0][1])
    check_save_load(model, tmp_path / "big.simrank", False)


def test_a_loaded_model_folds_in_with_weights_and_prior(tmp_path):
    n = 65
    model, _ = fit("AprioriSimRank", ring(n, 130, 25, weighted=True), prior(n, 25), weighted=True, keep=True,
                   storage_precision="f64")
    labels = list(model.frame().index)
    lists = [labels[:3], labels[10:11], labels[20:29]]
    weights = [[1.0, 2.0, 0.5], [3.0], list(np.arange(1.0, 10.0))]
    pr = prior(n, 26)[:3]
    want = model.fold_in(lists, weights=weights, prior=pr, names=["x", "y", "z"])
    want_k = model.fold_in(lists, weights=weights, prior=pr, top_k=4)
    model.save(tmp_path / "m.simrank")
    model.release()
    with simrank_amd.load_model(tmp_path / "m.simrank") as loaded:
        same(loaded.fold_in(lists, weights=weights, prior=pr, names=["x", "y", "z"]), want)
        same(loaded.fold_in(lists, weights=weights, prior=pr, top_k=4), want_k)
        with pytest.raises(ValueError, match="weights"):
            loaded.fold_in(lists)


def test_save_refuses_labels_it_cannot_write(tmp_path):
    df = ring(9, 12, 27, label=lambda i: i + 0.5)
    model, _ = fit("SimRank", df, keep=True)
    with pytest.raises(ValueError, match="float"):
        model.save(tmp_path / "no.simrank")
    assert not (tmp_path / "no.simrank").exists()
    model.rows([])                                                            # still usable
    model.release()


# ---- 64-bit offsets ------------------------------------------------------------------------------------------------------
def test_compact_past_two_to_the_31_elements():
    """N = 47104: N^2 = 2.2e9 elements, so a 32-bit element offset wraps in the last rows (from row 45591 on)."""
    n = 47104
    rng = np.random.default_rng(28)
    src = np.concatenate([np.arange(n), rng.integers(0, n, size=3 * n)])
    dst = np.concatenate([(np.arange(n) + 1) % n, rng.integers(0, n, size=3 * n)])
    df = pd.DataFrame({"from": src, "to": dst}).drop_duplicates()
    est = SRA.SimRank()
    est.fit(df, iterations=2, eps=1e-30, verbose=False, keep=True)
    labels = est._model[1][0][1]
    assert len(labels) == n
    nodes = [labels[i] for i in rng.integers(0, n, size=56)] + labels[-8:]
    a = [labels[i] for i in rng.integers(0, n, size=1000)]
    b = [labels[i] for i in rng.integers(n - 1500, n, size=1000)]
    rows, sim = est.rows(nodes), est.similarity(a, b)
    est.compact()
    assert est.device_bytes == 4 * n * n
    same(est.rows(nodes), rows)
    same(est.similarity(a, b), sim)
    est.release()
