"""SimRank++ leg 2 restricted to supp(E) (SimRank.py:315-316, :361; gather3_kernel's RESTRICT instantiations: a lane group
whose 32 evidence counts are all zero skips its gathers) through the SHIPPED loops — plan.hip, biplan.hip, shardplan.hip —
against the float64 oracle.  Every case reads the plan's choice back through the C ABI (simrank_plan_get / _biplan_get /
_shardplan_get "restrict_support"), so a plan that stopped restricting fails here instead of passing unnoticed."""
import contextlib

import numpy as np
import pytest

import simrank_amd.SimRank as SRA
from oracle import simrank_oracle as O
from simrank_amd import ingest, synth
from tests.graphs import bipartite_random, relabel_big_ints
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

DEFAULTS = dict(restrict_support=-1, fuse_sym=-1, ids16=1, addr32=1, dense_sym=-1)


@pytest.fixture(scope="module")
def ops():
    from simrank_amd.engine import HipOps
    return HipOps(0)


@contextlib.contextmanager
def knobs(ops, **kw):
    ops.set_tuning(**kw)
    try:
        yield
    finally:
        ops.set_tuning(**DEFAULTS)


# ---- graphs (sparse evidence: fewer than half of the 32-column segments of E are live) and their oracle results, once
def _er4096():
    return synth.er_directed(4096, 0.001, seed=11)


def _er2100():
    # ragged (not a multiple of 32 or 128), labels that are large sparse ints
    return relabel_big_ints(synth.er_directed(2100, 0.002, seed=5), ("from", "to"), seed=5)


def _powerlaw():
    # sparse power-law: rows of >= 512 entries (phase A0, "huge" rows split over the waves) beside the restricted phases
    return synth.powerlaw_directed(4096, 3, seed=5, exponent=1.8)


def _dense_corner():
    # dense sets in many 128-row blocks (tests/test_gpu_parity.py:_dense_corner_graph)
    return synth.powerlaw_directed(4096, 32, seed=21)


def _bip():
    return bipartite_random(1500, 900, 0.0015, seed=4)


def _bip_square():
    return bipartite_random(1200, 1200, 0.002, seed=6)


GRAPHS = {"er4096": _er4096, "er2100": _er2100, "powerlaw": _powerlaw, "dense_corner": _dense_corner, "bip": _bip,
          "bip_square": _bip_square}
_frames, _oracle = {}, {}


def frame(name):
    if name not in _frames:
        _frames[name] = GRAPHS[name]()
    return _frames[name]


def prior_for(name, n, seed=0):
    """A dense symmetric prior in [0, 1): where E is zero, S is non-zero through it alone."""
    rng = np.random.default_rng(n + seed)
    p = rng.random((n, n))
    return (p + p.T) / 2


def oracle(name, cls, **kw):
    key = (name, cls, tuple(sorted(kw.items())))
    if key not in _oracle:
        df = frame(name)
        if cls == "SimRankPP":
            _oracle[key] = O.fit_simrank_pp(df, verbose=False)
        elif cls == "AprioriSimRank":
            n = len(O.directed_graph(df)[0])
            _oracle[key] = O.fit_simrank_pp(df, verbose=False, apriori=prior_for(name, n), lbd=0.3)
        elif cls == "BipartitleAprioriSimRank":
            n1, n2 = df["user"].nunique(), df["item"].nunique()
            _oracle[key] = O.fit_bipartite_pp(df, verbose=False, strict_reference=False, apriori1=prior_for(name, n1),
                                              apriori2=prior_for(name, n2, 1), lbd1=0.3, lbd2=0.3)
        else:
            _oracle[key] = O.fit_bipartite_pp(df, verbose=False, **kw)
    return _oracle[key]


@pytest.fixture
def seen(monkeypatch):
    """What every solver the fits build chose at creation: ("plan" | "shards", [restrict_support per side / rank],
    the single plan's graph handle or None, the solver — kept alive with the handle it owns)."""
    import simrank_amd.cplan as cplan
    import simrank_amd.cshard as cshard
    out = []
    orig_plan, orig_shard = cplan.PlanSolver.__init__, cshard.CShardSolver.__init__

    def plan_spy(self, *a, **k):
        orig_plan(self, *a, **k)
        if self.bipartite:
            out.append(("plan", [self.plan.get(1, "restrict_support"), self.plan.get(2, "restrict_support")], None, self))
        else:
            out.append(("plan", [self.plan.get("restrict_support")], self.plan.graph_handle(), self))

    def shard_spy(self, *a, **k):
        orig_shard(self, *a, **k)
        p = self.plans
        if self.bipartite:
            got = [p.side_info(g, i)["restrict_support"] for g in (1, 2) for i in range(len(p.pairs))]
        else:
            got = [p.info(i)["restrict_support"] for i in range(len(p.plans))]
        out.append(("shards", got, None, self))

    monkeypatch.setattr(cplan.PlanSolver, "__init__", plan_spy)
    monkeypatch.setattr(cshard.CShardSolver, "__init__", shard_spy)
    return out


def fit_directed(name, cls, **kw):
    df = frame(name)
    est = getattr(SRA, cls)()
    if cls == "AprioriSimRank":
        n = len(O.directed_graph(df)[0])
        got = est.fit(df, prior_for(name, n), lbd=0.3, verbose=False, **kw)
    else:
        got = est.fit(df, verbose=False, **kw)
    return est, got


def check_directed(name, cls, est, got):
    want = oracle(name, cls)
    assert list(got.index) == want["labels"]
    assert_close(got.values, want["S"])
    assert est.converged_at == want["k"]
    assert np.array_equal(np.asarray(est.Evidence), want["E"])


def fit_bipartite(name, cls, **kw):
    df = frame(name)
    est = getattr(SRA, cls)()
    if cls == "BipartitleAprioriSimRank":
        n1, n2 = df["user"].nunique(), df["item"].nunique()
        s1, s2 = est.fit(df, prior_for(name, n1), prior_for(name, n2, 1), lbd1=0.3, lbd2=0.3, verbose=False,
                         strict_reference=False, **kw)
        want = oracle(name, cls)
    else:
        s1, s2 = est.fit(df, verbose=False, **kw)
        want = oracle(name, cls, strict_reference=kw.get("strict_reference", True))
    strict = kw.get("strict_reference", True) and cls != "BipartitleAprioriSimRank"
    assert list(s1.index) == list(want["labels1" if strict else "sorted1"])
    assert list(s2.index) == list(want["labels2" if strict else "sorted2"])
    assert_close(s1.values, want["S1"])
    assert_close(s2.values, want["S2"])
    assert est.converged_at == want["k"]
    assert np.array_equal(np.asarray(est.Evidence_N1), want["E1"])
    assert np.array_equal(np.asarray(est.Evidence_N2), want["E2"])
    return s1, s2


# ---------------------------------------------------------------------------------------------------------------------
# 1-2: the automatic choice, with and without a prior
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["er4096", "er2100", "powerlaw"])
def test_plans_restrict_sparse_evidence_by_themselves(name, seen, ops):
    if name == "powerlaw":
        _, csr = ingest.directed(frame(name), False, "from", "to", "weight")
        assert np.diff(csr.rowptr).max() >= ops.get_tuning("huge")          # (phase A0 runs beside the restricted phases)
    est, got = fit_directed(name, "SimRankPP")
    assert [s[:2] for s in seen] == [("plan", [1])]
    check_directed(name, "SimRankPP", est, got)


@pytest.mark.parametrize("name", ["er4096", "er2100"])
def test_apriori_with_sparse_evidence_emits_the_rows_it_skips(name, seen):
    """AprioriSimRank (SimRank.py:453): (1 - lbd) E.C.prod + lbd.prior — non-zero exactly where E is zero, so every row whose
    gathers the restricted leg skips must still be emitted with its prior term."""
    est, got = fit_directed(name, "AprioriSimRank")
    assert [s[:2] for s in seen] == [("plan", [1])]
    check_directed(name, "AprioriSimRank", est, got)
    assert np.all(got.values > 0)                                         # (the prior reaches every element)


def test_bipartite_apriori_with_sparse_evidence(seen):
    fit_bipartite("bip", "BipartitleAprioriSimRank")
    assert [s[:2] for s in seen] == [("plan", [1, 1])]


# ---------------------------------------------------------------------------------------------------------------------
# 3: forced restriction is bit-exact (gather3 either way: fuse_sym = 0)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls", [("er4096", "SimRankPP"), ("er2100", "SimRankPP"), ("powerlaw", "SimRankPP"),
                                      ("er4096", "AprioriSimRank"), ("er2100", "AprioriSimRank")])
def test_forced_restriction_is_bit_exact(name, cls, seen, ops):
    out = {}
    for rs in (0, 1, -1):
        seen.clear()
        with knobs(ops, fuse_sym=0, restrict_support=rs):
            est, got = fit_directed(name, cls)
        assert [s[:2] for s in seen] == [("plan", [1 if rs else 0])]
        out[rs] = (got.values, est.converged_at)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][0], out[-1][0])
    assert out[0][1] == out[1][1] == out[-1][1] == oracle(name, cls)["k"]
    assert_close(out[1][0], oracle(name, cls)["S"])


def test_forced_restriction_is_bit_exact_bipartite_apriori(seen, ops):
    out = {}
    for rs in (0, 1, -1):
        seen.clear()
        with knobs(ops, fuse_sym=0, restrict_support=rs):
            out[rs] = fit_bipartite("bip", "BipartitleAprioriSimRank")
        assert [s[:2] for s in seen] == [("plan", [1, 1] if rs else [0, 0])]
    for j in (0, 1):
        assert np.array_equal(out[0][j].values, out[1][j].values) and np.array_equal(out[0][j].values, out[-1][j].values)


# ---------------------------------------------------------------------------------------------------------------------
# 4-5: every restricted kSym instantiation on the plan, and the one-launch leg 2 on a restricted plan
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids16", [1, 0])
@pytest.mark.parametrize("addr32", [1, 0])
@pytest.mark.parametrize("dense", [1, 0])
def test_every_restricted_instantiation_on_the_plan(ids16, addr32, dense, seen, ops):
    """gather3_kernel<kSym, IDS16, RESTRICT, DENSE, A32>: {16, 32-bit ids} x {with, without dense partial sums} x {32, 64-bit
    operand addressing}, forced on the plan of a graph with dense sets; each against the oracle and bit-equal to the same
    variant unrestricted."""
    class G:                                     # (the plan's graph object, for the statistics entry points)
        def __init__(self, h):
            self.handle = h
    got = {}
    for rs in (1, 0):
        seen.clear()
        with knobs(ops, restrict_support=rs, fuse_sym=0, ids16=ids16, addr32=addr32, dense_sym=dense):
            est, S = fit_directed("dense_corner", "SimRankPP")
            kind, restricted, gh, _ = seen[0]
            assert (kind, restricted) == ("plan", [rs])
            g = G(gh)
            assert ops.graph_get(g, "gather_ids16") == ids16
            blocks, cols, covered = ops.dense_stats(g)
            assert (blocks > 0 and covered > 0) if dense else blocks == 0
        got[rs] = (S.values, est.converged_at)
    check_directed("dense_corner", "SimRankPP", est, S)
    assert np.array_equal(got[1][0], got[0][0]) and got[1][1] == got[0][1]


def test_one_launch_leg2_on_a_restricted_plan(seen, ops):
    """restrict_support = 1 with fuse_sym = 1: leg 2 is the one-launch kernel all the same (spmm.hip, the fuse_sym > 0 rule)."""
    with knobs(ops, restrict_support=1, fuse_sym=1):
        est, got = fit_directed("dense_corner", "SimRankPP")
        assert [s[:2] for s in seen] == [("plan", [1])]
        assert ops.graph_get(seen[0][2], "fused_ids16") == 1
    check_directed("dense_corner", "SimRankPP", est, got)


# ---------------------------------------------------------------------------------------------------------------------
# 6-7: bipartite and sharded
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,strict", [("bip", False), ("bip_square", True)])
def test_bipartite_pp_restricts_both_sides(name, strict, seen):
    """strict_reference = True: side 2 is gated by Evidence_N1 (quirk Q2), whose live segments decide its restriction."""
    fit_bipartite(name, "BipartiteSimRankPP", strict_reference=strict)
    assert [s[:2] for s in seen] == [("plan", [1, 1])]


@pytest.mark.parametrize("half", [True, False])
def test_sharded_simrank_pp_restricts_on_every_rank(half, seen):
    from simrank_amd.driver import LocalWorld
    est, got = fit_directed("er4096", "SimRankPP", world=LocalWorld(4, symmetric_shards=half))
    assert [s[:2] for s in seen] == [("shards", [1, 1, 1, 1])]
    check_directed("er4096", "SimRankPP", est, got)


def test_sharded_bipartite_pp_restricts_on_every_rank(seen):
    from simrank_amd.driver import LocalWorld
    fit_bipartite("bip", "BipartiteSimRankPP", strict_reference=False, world=LocalWorld(3))
    assert [s[:2] for s in seen] == [("shards", [1] * 6)]


# ---------------------------------------------------------------------------------------------------------------------
# the getters on live handles
# ---------------------------------------------------------------------------------------------------------------------
def test_getters_refuse_unknown_keys_on_live_handles(ops):
    from simrank_amd._lib import SimRankHipError
    from simrank_amd.engine import BiPlan, Plan, ShardPlans, _shardplan_get
    df = synth.er_directed(256, 0.02, seed=3)
    _, csr = ingest.directed(df, False, "from", "to", "weight")
    p = Plan(ops, csr, evidence=True)
    sp = ShardPlans(ops, csr, world=2, evidence=True)
    _, _, _, _, g12, g21 = ingest.bipartite(bipartite_random(90, 70, 0.05, seed=2), False, "user", "item", "weight")
    bp = BiPlan(ops, g12, g12.rowscale, g21.rowscale, evidence=True)
    try:
        assert p.get("restrict_support") in (0, 1) and bp.get(2, "restrict_support") in (0, 1)
        assert sp.info(1)["restrict_support"] in (0, 1)
        assert ops.graph_get(p.graph_handle(), "fused_ids16") in (-1, 0, 1)
        for call in (lambda: p.get("no_such_key"), lambda: bp.get(1, "no_such_key"),
                     lambda: _shardplan_get(ops.lib, sp.plans[0], "no_such_key"),
                     lambda: ops.graph_get(p.graph_handle(), "no_such_key")):
            with pytest.raises(SimRankHipError, match="no_such_key"):
                call()
        with pytest.raises(SimRankHipError, match="group"):
            bp.get(3, "restrict_support")
    finally:
        p.free()
        sp.free()
        bp.free()
