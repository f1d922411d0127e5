"""``fold_in`` on a real MI355X: rows of nodes that were NOT in the fitted graph, from a kept model, through
libsimrank_foldin.so.

Two yardsticks.  (a) The model's OWN iterate: ``fold_in_ref`` (tests/foldin_ref.py, float64 NumPy, proven against the
reference's loop in tests/test_foldin_cpu.py) on ``model.frame()``.  Every term is non-negative, so a sum of them in any
order is within (number of additions) x u relative of the exact value: the bound asserted per new node is
``(|I_q| + max_b |I(b)| + 8) * u``, u = 2^-24 for f32 / fp16-held iterates (against the widened values ``frame()`` returns),
2^-53 for float64 ones; the 8 covers the multiplications of the epilogue.  (b) The REFERENCE: a fit stopped after 3 updates
folds in every node's own list and must give the oracle's 4-update matrix off the diagonal at ``helpers.RTOL`` (1e-5, the
project's bar for every f32 comparison with the reference), in float64 at test_gpu_f64.py's 1e-11 absolute."""
import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

import simrank_amd.SimRank as SRA
from simrank_amd import _query, synth
from simrank_amd.driver import LocalWorld
from simrank_amd.engine import HipOps
from tests import foldin_ref as R
from tests.conftest import Golden
from tests.helpers import RTOL

pytestmark = pytest.mark.gpu

U32, U64 = 2.0 ** -24, 2.0 ** -53

GOLDENS = ["SimRank_er128", "SimRank_toy5", "SimRank_bts300", "SimRankPP_quirky", "SimRankPP_pl256", "AprioriSimRank_er64",
           "AprioriSimRank_er64_asym", "AprioriSimRank_quirky_asym", "BipartiteSimRank_b5030", "BipartiteSimRank_k10",
           "BipartiteSimRankPP_b40", "BipartitleAprioriSimRank_b40", "BipartitleAprioriSimRank_b40_asym"]   # test_gpu_query.py's
WEIGHTED = ["SimRank_er64_weighted", "SimRankPP_er64_cols", "BipartiteSimRankPP_b40_weighted"]


def _keep(g, **extra):
    est = getattr(SRA, g.cls)()
    kw = dict(g.kwargs, verbose=False, keep=True)
    kw.update(extra)
    return est.fit(g.frame, *g.args, **kw)


def _sides(g, model, kwargs=None):
    """``foldin_ref.sides_of`` on the model's own iterate and the estimator's own dense attributes (caller's order), with
    each side's labels."""
    pp = g.cls not in ("SimRank", "BipartiteSimRank")
    frames = model.frame()
    if isinstance(frames, tuple):
        r = dict(S1=frames[0].values, S2=frames[1].values, G12=model.Graph_N1_N2.values, G21=model.Graph_N2_N1.values)
        if pp:
            r.update(W1=np.asarray(model.Weight_N1), W2=np.asarray(model.Weight_N2))
        labels = {1: (list(frames[1].index), list(frames[0].index)), 2: (list(frames[0].index), list(frames[1].index))}
    else:
        r = dict(S=frames.values, G=model.Graph.values)
        if pp:
            r.update(W=np.asarray(model.Weight))
        labels = {None: (list(frames.index), list(frames.index))}
    out = R.sides_of(g, r, kwargs)
    for sd in out:
        sd["S"] = r[sd["reads"]]
        sd["src_labels"], sd["out_labels"] = labels[sd["group"]]
    return out


def _weights_for(lists, w):
    """Weights whose sum gives the row scale ``w`` back (own lists of a weighted fit): len(list) equal parts."""
    return [np.full(len(l), (1.0 / (w[q] * len(l))) if w[q] > 0 else 0.0) for q, l in enumerate(lists)]


def _lists_for(sd, rng, weighted):
    """Every fitted node's own list, random lists of 1, 2, 33 and N labels, an empty one, and random ones up to at least 70
    new nodes (three tiles).  -> (position lists, row scales, weights or None)."""
    lists, w = R.own_lists(sd["G"])
    n_src = sd["S"].shape[0]
    own = len(lists)
    extra = [min(n, n_src) for n in (1, 2, 33, n_src)] + [0]
    while own + len(extra) < 70:
        extra.append(int(rng.integers(1, min(n_src, 40) + 1)))
    extra_lists = [rng.permutation(n_src)[:n] for n in extra]
    if weighted:
        weights = _weights_for(lists, w) + [rng.uniform(0.5, 2.0, len(l)) for l in extra_lists]
        lists = lists + extra_lists
        w = R.row_scales([len(l) for l in lists], weights)
    else:
        weights = None
        lists = lists + extra_lists
        w = R.row_scales([len(l) for l in lists])
    return lists, w, weights


def _assert_within(got, want, tol, what=""):
    """|got - want| <= tol[q] * |want| + 1e-30 per new node q (``helpers.assert_close``'s atol)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want != 0, err / np.abs(want), np.where(err > 1e-30, np.inf, 0.0))
    worst = rel.max(axis=1) if rel.size else np.zeros(len(tol))
    print(f"{what} worst relative error {worst.max() if worst.size else 0:.3e} (bound of that node "
          f"{tol[int(np.argmax(worst / np.maximum(tol, 1e-300)))] if worst.size else 0:.3e})")
    bad = err > tol[:, None] * np.abs(want) + 1e-30
    assert not bad.any(), (what, int(bad.sum()), float(rel[bad].max()))


def _check_model_against_its_iterate(g, model, u, seed=0, kwargs=None):
    rng = np.random.default_rng(seed)
    weighted = bool(dict(g.kwargs, **(kwargs or {})).get("weighted", False))
    strict = dict(g.kwargs, **(kwargs or {})).get("strict_reference", True)
    for sd in _sides(g, model, kwargs):
        kw = {} if sd["group"] is None else {"group": sd["group"]}
        if sd["group"] == 2 and sd["pattern"] is not None and strict:
            with pytest.raises(ValueError, match="Evidence_N1"):
                model.fold_in([[]], **kw)
            continue
        lists, w, weights = _lists_for(sd, rng, weighted)
        prior = rng.uniform(0.0, 1.0, (len(lists), sd["W"].shape[0])) if sd["lbd"] is not None else None
        names = [f"new{q}" for q in range(len(lists))]
        got = model.fold_in([[sd["src_labels"][i] for i in l] for l in lists], weights=weights, prior=prior, names=names, **kw)
        assert list(got.index) == names and list(got.columns) == sd["out_labels"] and got.values.dtype == np.float64
        want = R.fold_in_ref(lists, sd["S"], sd["W"], sd["coef"], w, sd["pattern"], sd["lbd"], prior)
        _assert_within(got.values, want, R.tolerance(lists, sd["W"], u), f"{g.name} group {sd['group']}")
        empty = [q for q, l in enumerate(lists) if len(l) == 0]
        if prior is None:
            assert empty and not got.values[empty].any()
        if sd["lbd"] is not None:                          # prior omitted = zeros
            some = list(range(min(5, len(lists))))
            got0 = model.fold_in([[sd["src_labels"][i] for i in lists[q]] for q in some],
                                 weights=None if weights is None else [weights[q] for q in some], **kw)
            want0 = R.fold_in_ref([lists[q] for q in some], sd["S"], sd["W"], sd["coef"], w[some], sd["pattern"], sd["lbd"])
            _assert_within(got0.values, want0, R.tolerance([lists[q] for q in some], sd["W"], u), "no prior")


@pytest.mark.parametrize("name", GOLDENS + WEIGHTED)
def test_against_the_models_own_iterate(name):
    g = Golden(name)
    with _keep(g) as model:
        _check_model_against_its_iterate(g, model, U32)


def test_bipartite_pp_with_its_own_group_2_evidence():
    g = Golden("BipartiteSimRankPP_b40")
    with _keep(g, strict_reference=False) as model:
        _check_model_against_its_iterate(g, model, U32, kwargs=dict(strict_reference=False))
    g = Golden("BipartitleAprioriSimRank_b40_asym")
    with _keep(g, strict_reference=False) as model:
        _check_model_against_its_iterate(g, model, U32, kwargs=dict(strict_reference=False))


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["SimRank_er128", "SimRankPP_quirky", "AprioriSimRank_er64_asym", "BipartiteSimRank_b5030",
                                  "BipartiteSimRankPP_b40", "SimRankPP_er64_cols", "BipartiteSimRankPP_b40_weighted",
                                  "BipartitleAprioriSimRank_b40", "BipartitleAprioriSimRank_b40_asym"])
def test_on_logical_shards(name, world):
    g = Golden(name)
    with _keep(g, world=LocalWorld(world), mode="sparse") as model:
        _check_model_against_its_iterate(g, model, U32, seed=world)


@pytest.mark.parametrize("name", ["SimRank_er128", "SimRankPP_pl256", "SimRankPP_quirky"])
def test_on_fp16_held_matrices(name):
    g = Golden(name)
    with _keep(g, storage_precision="fp16") as model:
        _check_model_against_its_iterate(g, model, U32)


@pytest.mark.parametrize("cls", ["SimRank", "SimRankPP"])
def test_on_fp16_held_shards(cls):
    """fp16-held column blocks of two virtual ranks (64-column panels with block-local columns); the sharded fp16 loop
    takes node counts that are multiples of 64 x ranks and the one-matrix classes without a prior."""
    g = _Plain(synth.er_directed(256, 0.03, seed=5), iterations=5)
    g.cls = cls
    with _keep(g, storage_precision="fp16", world=LocalWorld(2)) as model:
        _check_model_against_its_iterate(g, model, U32, seed=2)


@pytest.mark.parametrize("name", GOLDENS + WEIGHTED)
def test_in_f64(name):
    g = Golden(name)
    with _keep(g, storage_precision="f64") as model:
        _check_model_against_its_iterate(g, model, U64)


class _Plain:
    """A stand-in golden for a synthetic SimRank input."""
    cls, args, name = "SimRank", (), "synthetic"

    def __init__(self, frame, **kwargs):
        self.frame, self.kwargs = frame, kwargs


@pytest.mark.parametrize("n", [1, 2, 33, 65, 257])
@pytest.mark.parametrize("storage", ["f32", "fp16", "f64"])
def test_sizes_that_stress_the_layouts(n, storage):
    rng = np.random.default_rng(n)
    if n == 1:
        df = pd.DataFrame({"from": [0], "to": [0]})
    else:
        m = 4 * n
        df = pd.DataFrame({"from": rng.integers(0, n, m), "to": rng.integers(0, n, m)})
        df = pd.concat([df, pd.DataFrame({"from": np.arange(n), "to": (np.arange(n) + 1) % n})]).drop_duplicates()
    g = _Plain(df, iterations=5, eps=0)
    with _keep(g, storage_precision=storage) as model:
        assert len(model.frame()) == n
        _check_model_against_its_iterate(g, model, U64 if storage == "f64" else U32, seed=n)


def test_a_row_longer_than_the_half_wave_limit():
    """A hub with more in-neighbours than SIMRANK_FOLDIN_LONG_ROW: its column is summed by the workgroup-per-row kernel."""
    from simrank_amd import _foldin
    n = 700
    rng = np.random.default_rng(3)
    hub = pd.DataFrame({"from": np.arange(1, 601), "to": np.zeros(600, dtype=np.int64)})
    rest = pd.DataFrame({"from": rng.integers(0, n, 3000), "to": rng.integers(1, n, 3000)})
    df = pd.concat([hub, rest]).drop_duplicates()
    for cls in ("SimRank", "SimRankPP"):
        g = _Plain(df, iterations=4, eps=0)
        g.cls = cls
        for storage in ("f32", "f64"):
            with _keep(g, storage_precision=storage) as model:
                assert int((model.Graph.values != 0).sum(axis=1).max()) > _foldin.LONG_ROW
                _check_model_against_its_iterate(g, model, U64 if storage == "f64" else U32)


# ---- against the reference -------------------------------------------------------------------------------------------
# the inputs tests/test_foldin_cpu.py qualifies for the same identity in NumPy, all of them
REFERENCE_CASES = ["SimRank_er128", "SimRank_er64_weighted", "SimRank_quirky", "SimRankPP_pl256", "SimRankPP_er64_cols",
                   "AprioriSimRank_er64", "AprioriSimRank_er64_asym", "AprioriSimRank_quirky_asym", "BipartiteSimRank_b5030",
                   "BipartiteSimRank_b40_weighted", "BipartiteSimRank_k10", "BipartiteSimRankPP_b40",
                   "BipartiteSimRankPP_b40_weighted", "BipartiteSimRankPP_bigints", "BipartitleAprioriSimRank_b40",
                   "BipartitleAprioriSimRank_b40_asym"]


def _gated(name):
    return name.split("_")[0] in ("BipartiteSimRankPP", "BipartitleAprioriSimRank")


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("name,strict", [(n, s) for n in REFERENCE_CASES for s in ((True, False) if _gated(n) else (True,))])
def test_against_the_reference_after_one_more_update(name, strict, storage):
    """A fit stopped after 3 updates folds in every node's own list (and its own row of the prior): the oracle's matrix after
    4 updates, off the diagonal.  Group 2 of the bipartite classes: the oracle's own S2 after 3 updates."""
    g = Golden(name)
    over = dict(iterations=3, eps=1e-12)
    if _gated(name):
        over["strict_reference"] = strict
    r3 = R.run_oracle(g, verbose=False, **over)
    r4 = R.run_oracle(g, verbose=False, **dict(over, iterations=4))
    assert r3["k"] is None and r4["k"] is None
    weighted = bool(g.kwargs.get("weighted", False))
    with _keep(g, storage_precision=storage, **over) as model:
        assert model.converged_at is None
        for sd in _sides(g, model, over):
            if sd["group"] == 2 and _gated(name) and strict:
                continue
            kw = {} if sd["group"] is None else {"group": sd["group"]}
            lists, w = R.own_lists(sd["G"])
            got = model.fold_in([[sd["src_labels"][i] for i in l] for l in lists],
                                weights=_weights_for(lists, w) if weighted else None,
                                prior=sd["prior"] if sd["lbd"] is not None else None, **kw).values
            want = (r3 if sd["group"] == 2 else r4)[sd["writes"]]
            off = ~np.eye(len(want), dtype=bool)
            err = np.abs(got - want)[off]
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(want[off] != 0, err / np.abs(want[off]), np.where(err > 1e-30, np.inf, 0.0))
            print(f"{name} strict={strict} {storage} group {sd['group']}: max rel {rel.max():.3e} max abs {err.max():.3e}")
            if storage == "f64":
                assert err.max() <= 1e-11, err.max()
            else:
                np.testing.assert_allclose(got[off], want[off], rtol=RTOL, atol=1e-30)


# ---- top_k, determinism, lifetime ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SimRank_er128", "SimRankPP_pl256", "AprioriSimRank_er64_asym", "BipartiteSimRankPP_b40"])
@pytest.mark.parametrize("world", [1, 2])
def test_top_k_is_a_numpy_selection_on_the_dense_fold_in(name, world):
    g = Golden(name)
    rng = np.random.default_rng(1)
    with _keep(g, world=LocalWorld(world), mode="sparse") as model:
        for sd in _sides(g, model)[:1]:
            kw = {} if sd["group"] is None else {"group": sd["group"]}
            lists, _, _ = _lists_for(sd, rng, False)
            labels = [[sd["src_labels"][i] for i in l] for l in lists]
            names = [f"n{q}" for q in range(len(lists))]
            dense = model.fold_in(labels, names=names, **kw)
            n_out = dense.shape[1]
            for k in (1, 10, n_out, n_out + 5):
                got = model.fold_in(labels, names=names, top_k=k, **kw)
                idx, val = R.topk_ref(dense.values, k)
                kk = idx.shape[1]
                assert kk == min(k, n_out)
                want = pd.DataFrame({"node": np.repeat(names, kk), "rank": np.tile(np.arange(1, kk + 1), len(names)),
                                     "neighbor": pd.Index(sd["out_labels"]).take(idx.ravel()), "similarity": val.ravel()})
                assert_frame_equal(got, want, check_exact=True)


def test_more_new_nodes_than_one_band(monkeypatch):
    g = Golden("SimRankPP_pl256")
    rng = np.random.default_rng(2)
    with _keep(g) as model:
        (sd,) = _sides(g, model)
        lists, _, _ = _lists_for(sd, rng, False)
        labels = [[sd["src_labels"][i] for i in l] for l in lists]
        whole, whole_k = model.fold_in(labels), model.fold_in(labels, top_k=7)
        monkeypatch.setattr(_query, "SLAB_BYTES", 64 * 8 * 256)          # two tiles per band
        assert_frame_equal(model.fold_in(labels), whole, check_exact=True)
        assert_frame_equal(model.fold_in(labels, top_k=7), whole_k, check_exact=True)
        monkeypatch.setattr(_query, "SLAB_BYTES", 1)                     # one tile per band
        assert_frame_equal(model.fold_in(labels), whole, check_exact=True)
        assert_frame_equal(model.fold_in(labels, top_k=7), whole_k, check_exact=True)


@pytest.mark.parametrize("storage", ["f32", "fp16", "f64"])
def test_two_calls_give_the_same_bits_and_the_iterate_is_only_read(storage):
    g = Golden("SimRankPP_pl256")
    rng = np.random.default_rng(4)
    HipOps.trim_pool()
    with _keep(g, storage_precision=storage) as never:              # the same queries, but no fold_in
        _sides(g, never)
        never.rows(list(never.frame().index))
        never.rows(list(never.frame().index))
    idle = HipOps.pool_stats()
    HipOps.trim_pool()
    model = _keep(g, storage_precision=storage)
    (sd,) = _sides(g, model)
    lists, _, _ = _lists_for(sd, rng, False)
    labels = [[sd["src_labels"][i] for i in l] for l in lists]
    before = model.rows(sd["src_labels"])
    a = model.fold_in(labels)
    b = model.fold_in(labels)
    np.testing.assert_array_equal(a.values.view(np.uint64), b.values.view(np.uint64))
    assert_frame_equal(model.fold_in(labels, top_k=5), model.fold_in(labels, top_k=5), check_exact=True)
    after = model.rows(sd["src_labels"])
    np.testing.assert_array_equal(before.values.view(np.uint64), after.values.view(np.uint64))
    model.release()
    assert HipOps.pool_stats() == idle
    with pytest.raises(RuntimeError, match="released"):
        model.fold_in(labels)


def test_config4_fold_in_of_256_new_nodes():
    """BASELINE.json config 4 (N = 32768): 256 new nodes whose list lengths are drawn from the graph's own degree
    distribution, on a sample of columns against a float64 recomputation from ``model.rows(union of their neighbours)``."""
    df = synth.WORKLOADS["pl32768"][0]()
    rng = np.random.default_rng(11)
    with SRA.SimRank().fit(df, verbose=False, iterations=4, eps=0, keep=True) as model:
        labels = list(model._model[1][0][1])
        n = len(labels)
        csr = model._csr
        deg = np.diff(csr.rowptr)
        lens = np.maximum(1, rng.choice(deg, 256))
        lists = [rng.permutation(n)[:l] for l in lens]
        got = model.fold_in([[labels[i] for i in l] for l in lists])
        union = np.unique(np.concatenate(lists))
        rows = model.rows([labels[i] for i in union]).values
    where = {int(u): i for i, u in enumerate(union)}
    cols = np.concatenate([rng.integers(0, n, 500), np.argsort(-deg)[:12]])           # the longest rows among them
    want = np.zeros((256, cols.size))
    for q, l in enumerate(lists):
        t = rows[[where[int(i)] for i in l]].sum(axis=0) * (1.0 / len(l))
        for c, b in enumerate(cols):
            nb = csr.col[csr.rowptr[b]:csr.rowptr[b + 1]]
            want[q, c] = 0.8 * (csr.rowscale[b] * t[nb].sum())
    tol = np.array([(len(l) + int(deg.max()) + 8) * U32 for l in lists])
    _assert_within(got.values[:, cols], want, tol, "config 4")
