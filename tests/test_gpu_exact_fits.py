"""Whole loops on graphs whose iterates stay EXACT (tests/exact.py: regular_graph, C = 0.5), bit for bit against the oracle.

Every node has d in-neighbours (d a power of two) and C = 0.5, so the float64 oracle's iterates live on a dyadic grid;
exact_updates says for how many updates U every term and every sum of both legs fits the format's mantissa.  Within U
there is no rounding anywhere, in any summation order, so every way the project runs the loop — fit() in its modes, the
plan stepped update by update, virtual ranks in the full and the half form with staged exchanges, the sharded plans behind
the C ABI, float64 storage, fp16 storage and the fp16 wire — must return the oracle's frame exactly, with the oracle's
`converged_at`.  Ties: with eps = a difference that occurs in the run, the loop stops where the oracle's strict > stops.
SimRank.py:124-141, :346-363 and the two-matrix loop :280-302."""
import contextlib

import numpy as np
import pytest

import simrank_amd.SimRank as SRA
from oracle import simrank_oracle as O
from simrank_amd import ingest
from simrank_amd.driver import LocalWorld
from tests import exact as X
from tests.leg2_rule import short_groups

pytestmark = pytest.mark.gpu

GRAPHS = [(300, 2), (300, 4), (1031, 4), (2100, 8)]
HALF_FORM = (512, 4)            # a node count the half form of a sharded leg 2 takes (a multiple of 32 x ranks) at 2, 4, 8 ranks
TINY = 1e-30                    # an eps no difference of these runs is below, but zero
# Leg 2's short path (tuning "leg2_short"): every row of regular_graph(n, d) has d entries and every tile is whole, so every
# group of four tiles is short at every width >= d and none below.  GRAPHS (d <= 8) are short at 8 and at 16; the graph with
# d = 16 is general at 8 and short at 16, the one whole loop in which the two widths differ (plain SimRank only: its exact
# updates are 2 plain and 1 for SimRank++, too few for these tests).
LEG2_WIDTHS = (0, 8, 16)
SHORT_AT_16_ONLY = (520, 16)
# the two-launch upper-triangle leg 2 on the plain pattern, whatever a plan would choose by itself on these graphs (the
# one-launch leg 2 and the dense part are other kernels): as BASE of tests/leg2_short_worker.py
TWO_LAUNCH = dict(fuse_sym=0, dense_sym=0, ids16=1, restrict_support=0, balance=2)


@contextlib.contextmanager
def leg2_width(ops, width):
    """The process-wide tuning with the two-launch leg 2 forced and leg2_short = width; restored."""
    kw = dict(TWO_LAUNCH, leg2_short=width)
    saved = {k: ops.get_tuning(k) for k in kw}
    ops.set_tuning(**kw)
    try:
        yield
    finally:
        ops.set_tuning(**saved)


def leg2_rule(c, width):
    """Short groups of regular_graph(n, d) at `width`, from the rule in NumPy (the order of equal-length rows is immaterial)."""
    return short_groups([c.d] * c.n, width)


class Case:
    """A regular graph, its oracle matrices and (lazily, once) the exact update counts and the oracle's iterates."""

    def __init__(self, n, d):
        self.n, self.d = n, d
        self.df = X.regular_graph(n, d, seed=n + d)
        self.labels, self.G = O.directed_graph(self.df)
        self.E = None
        self._u, self._its = {}, {}

    def evidence(self):
        if self.E is None:
            self.E = O.evidence(self.G)
        return self.E

    def updates(self, pp=False, mantissa=24):
        key = (pp, mantissa)
        if key not in self._u:
            self._u[key] = X.exact_updates(self.G, 0.5, self.evidence() if pp else None, mantissa=mantissa,
                                           limit=8 if mantissa < 53 else 10)
            print(f"regular_graph({self.n}, {self.d}) {'++' if pp else 'plain'} mantissa {mantissa}: {self._u[key]}")
        return self._u[key].updates

    def iterates(self, pp, updates):
        have = self._its.setdefault(pp, [np.eye(self.n)])
        while len(have) <= updates:
            have.append(O.update(self.G, have[-1], 0.5, self.evidence() if pp else None))
        return have[:updates + 1]

    def oracle(self, pp, iterations, eps):
        """(S, k) of the oracle's loop, from the cached iterates (the loop of oracle.iterate_directed)."""
        its = self.iterates(pp, iterations)
        old = np.zeros((self.n, self.n))
        for k in range(iterations):
            if O.converged(old, its[k], eps):
                return its[k], k
            old = its[k]
        return its[iterations], None


_cases = {}


def case(n, d):
    if (n, d) not in _cases:
        _cases[(n, d)] = Case(n, d)
    return _cases[(n, d)]


def same_frame(got, want_S, labels):
    assert list(got.index) == labels and list(got.columns) == labels
    a = got.values
    assert a.dtype == np.float64 and a.shape == want_S.shape
    if not np.array_equal(a, want_S):
        bad = np.argwhere(a != want_S)
        r, c = bad[0]
        raise AssertionError(f"{len(bad)} elements differ from the oracle, first at ({r}, {c}): {a[r, c]!r} != {want_S[r, c]!r}")


def fit(cls, c, iterations, eps, **kw):
    est = getattr(SRA, cls)()
    got = est.fit(c.df, C=0.5, iterations=iterations, eps=eps, verbose=False, **kw)
    return est, got


@pytest.fixture(scope="module")
def ops():
    from simrank_amd.engine import HipOps
    return HipOps(0)


# ---- fit() ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", GRAPHS + [HALF_FORM])
@pytest.mark.parametrize("cls", ["SimRank", "SimRankPP"])
@pytest.mark.parametrize("mode", ["auto", "sparse"])
def test_fit_is_the_oracle(n, d, cls, mode):
    c = case(n, d)
    pp = cls == "SimRankPP"
    U = c.updates(pp)
    assert U >= 2
    S, k = c.oracle(pp, U, TINY)
    est, got = fit(cls, c, U, TINY, mode=mode)
    same_frame(got, S, c.labels)
    assert est.converged_at == k
    if pp:
        assert np.array_equal(np.asarray(est.Evidence), c.evidence())


def _stops_on_a_tie(c, cls):
    pp = cls == "SimRankPP"
    U, eps, step = X.tie_eps(c.iterates(pp, c.updates(pp)))
    S, k = c.oracle(pp, U, eps)
    assert k == U - 1
    est, got = fit(cls, c, U, eps)
    assert est.converged_at == k
    same_frame(got, S, c.labels)
    S, k = c.oracle(pp, U, eps - step)
    assert k is None
    est, got = fit(cls, c, U, eps - step)
    assert est.converged_at is None
    same_frame(got, S, c.labels)


@pytest.mark.parametrize("n,d", GRAPHS)
@pytest.mark.parametrize("cls", ["SimRank", "SimRankPP"])
def test_fit_stops_on_a_tie_where_the_oracle_stops(n, d, cls):
    """eps = max |S_{U-1} - S_{U-2}|: the test at loop index U - 1 passes only under strict >; one grid step less and it
    does not pass, and the loop applies all U updates."""
    _stops_on_a_tie(case(n, d), cls)


@pytest.mark.parametrize("n,d", GRAPHS + [SHORT_AT_16_ONLY])
@pytest.mark.parametrize("width", LEG2_WIDTHS)
def test_fit_stops_on_a_tie_on_each_path_of_leg2(ops, monkeypatch, n, d, width):
    """The same (SimRank) with the two-launch leg 2 forced and leg2_short = 0, 8, 16: the general path, and the short path
    where the rule says so — read from the plan of every fit ("leg2_short_groups" after its run)."""
    from simrank_amd import cplan
    c = case(n, d)
    assert c.updates(False) >= 2
    seen = []
    run = cplan.PlanSolver.run

    def spy(self, *a, **kw):
        out = run(self, *a, **kw)
        seen.append(self.plan.get("leg2_short_groups"))
        return out
    monkeypatch.setattr(cplan.PlanSolver, "run", spy)
    with leg2_width(ops, width):
        _stops_on_a_tie(c, "SimRank")
    rule = leg2_rule(c, width)
    assert seen == [rule, rule] and rule == (0 if width < d else ((n + 31) // 32 + 3) // 4), (seen, rule)


# ---- the plan, update by update ------------------------------------------------------------------------------------
def _stepped(ops, c, pp, groups=None):
    """simrank_plan_step, update by update; `groups`: what "leg2_short_groups" must say after every update."""
    from simrank_amd.engine import Plan
    n = c.n
    U = c.updates(pp)
    assert U >= 2
    its = c.iterates(pp, U)
    nodes, csr = ingest.directed(c.df, False, "from", "to", "weight")
    assert nodes == c.labels
    rowscale = csr.rowscale
    if pp:
        assert np.array_equal(ingest.spread(csr), np.ones(n))              # equal entries in every row: no spread
        rowscale = ingest.spread(csr) * csr.rowscale
    plan = Plan(ops, csr, rowscale, coef=0.5, evidence=pp)
    try:
        plan.reset()
        for u in range(1, U + 1):
            diff = np.abs(its[u] - its[u - 1])
            top = float(diff.max())
            if top == 0:
                eps, want = 0.0, 0
            else:
                below = diff[diff < top]
                eps = float(below.max()) if below.size else 0.0             # a difference that occurs: not counted itself
                want = int((diff > eps).sum())
                assert want == int((diff == top).sum())
            assert plan.step(eps, exact_count=True) == want, (u, eps)
            assert groups is None or plan.get("leg2_short_groups") == groups, (u, plan.get("leg2_short_groups"), groups)
            assert np.array_equal(plan.result(), its[u]), u
    finally:
        plan.free()


@pytest.mark.parametrize("n,d", GRAPHS)
@pytest.mark.parametrize("pp", [False, True])
@pytest.mark.parametrize("identity_leg1", ["1", "0"])
def test_plan_stepped_update_by_update(ops, monkeypatch, n, d, pp, identity_leg1):
    """simrank_plan_step: after every update the oracle's iterate, and the count of that update on a tie — eps = the largest
    difference of the update but one grid step: exactly the elements that moved by the largest difference count."""
    monkeypatch.setenv("SIMRANK_IDENTITY_LEG1", identity_leg1)
    _stepped(ops, case(n, d), pp)


@pytest.mark.parametrize("n,d,pp", [(n, d, pp) for n, d in GRAPHS for pp in (False, True)] + [SHORT_AT_16_ONLY + (False,)])
@pytest.mark.parametrize("width", LEG2_WIDTHS)
def test_plan_stepped_on_each_path_of_leg2(ops, monkeypatch, n, d, pp, width):
    """The same with the two-launch upper-triangle leg 2 forced (TWO_LAUNCH: a plan may choose the one-launch leg 2 or the
    dense part by itself, and the rule speaks about neither) and leg2_short = 0, 8, 16: at 0 the general gather3 kSym leg
    runs the whole loop, at 8 and 16 every group is short on GRAPHS, on the d = 16 graph at 16 only.  After every update the
    plan's "leg2_short_groups" is the rule's number, the iterate and the count on a tie are the oracle's."""
    monkeypatch.setenv("SIMRANK_IDENTITY_LEG1", "1")
    c = case(n, d)
    rule = leg2_rule(c, width)
    assert rule == (0 if width < d else ((n + 31) // 32 + 3) // 4)            # every group of four 32-row tiles, or none
    with leg2_width(ops, width):
        _stepped(ops, c, pp, groups=rule)


# ---- virtual ranks --------------------------------------------------------------------------------------------------
def _worlds():
    out = []
    for P in (2, 4, 8):
        for stages in (1, 2, 4):
            out.append((P, True, stages))
        out.append((P, False, 1))
    return out


@pytest.mark.parametrize("n,d", GRAPHS + [HALF_FORM])
@pytest.mark.parametrize("P,half,stages", _worlds())
def test_virtual_ranks_are_the_oracle(n, d, P, half, stages):
    """LocalWorld(P, loop="c"): the sharded loop on P virtual ranks, leg 2 in its half form (where the node count is a multiple
    of 32 P: the last graph) and in its full form, the half form's exchange in 1, 2 and 4 stages."""
    c = case(n, d)
    pp = (P + stages) % 2 == 1                                             # both classes over the grid
    cls = "SimRankPP" if pp else "SimRank"
    U = c.updates(pp)
    S, k = c.oracle(pp, U, TINY)
    est, got = fit(cls, c, U, TINY, mode="sparse",
                   world=LocalWorld(P, symmetric_shards=half, leg2_stages=stages, loop="c"))
    same_frame(got, S, c.labels)
    assert est.converged_at == k


@pytest.mark.parametrize("P", [2, 4, 8])
@pytest.mark.parametrize("stages", [1, 2])
def test_half_form_ranks_stop_on_a_tie(P, stages):
    """The half form counts a mirrored element twice; the loop's decision on a tie is the oracle's all the same."""
    c = case(*HALF_FORM)
    U, eps, step = X.tie_eps(c.iterates(False, c.updates(False)))
    for e, k_want in ((eps, U - 1), (eps - step, None)):
        S, k = c.oracle(False, U, e)
        assert k == k_want
        est, got = fit("SimRank", c, U, e, mode="sparse", world=LocalWorld(P, symmetric_shards=True, leg2_stages=stages))
        assert est.converged_at == k
        same_frame(got, S, c.labels)


@pytest.mark.parametrize("n,d", GRAPHS + [HALF_FORM])
@pytest.mark.parametrize("leg2_form,stages", [(0, 1), (0, 3), (1, 1), (1, 3)])
def test_shard_plans_are_the_oracle(ops, n, d, leg2_form, stages):
    """engine.ShardPlans (simrank_shardplan_*) on four virtual ranks: full and half form (the half form where the node count
    allows it), one stage and three; stepped, with the count of every update from the oracle."""
    from simrank_amd.engine import ShardPlans
    if leg2_form == 1 and n % 128:
        leg2_form = 0                                                      # (the half form needs whole tiles on every rank)
        stages += 1                                                        # (still a case of its own: another cut of leg 1)
    c = case(n, d)
    U = c.updates(False)
    its = c.iterates(False, U)
    _, csr = ingest.directed(c.df, False, "from", "to", "weight")
    sp = ShardPlans(ops, csr, world=4, coef=0.5, leg2_form=leg2_form, stages=stages)
    try:
        assert sp.info(0)["half_form"] == bool(leg2_form)
        sp.reset()
        for u in range(1, U + 1):
            diff = np.abs(its[u] - its[u - 1])
            top = float(diff.max())
            below = diff[diff < top]
            eps = float(below.max()) if below.size else 0.0
            assert sp.step(eps, exact_count=True) == int((diff > eps).sum()), (u, eps)
        assert np.array_equal(sp.result(), its[U])
        S, k = c.oracle(False, U, TINY)
        sp.reset()
        assert sp.run(U, TINY) == (U if k is None else k, k)
        assert np.array_equal(sp.result(), S)
    finally:
        sp.free()


# ---- the two-matrix loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2,d1", [(256, 256, 2), (384, 192, 2)])
@pytest.mark.parametrize("cls", ["BipartiteSimRank", "BipartiteSimRankPP"])
def test_bipartite_pair_is_the_oracle(n1, n2, d1, cls):
    df = X.biregular_graph(n1, n2, d1, seed=n1 + n2)
    pp = cls.endswith("PP")
    kw = dict(strict_reference=False) if pp else {}
    ref = O.fit_bipartite_pp if pp else O.fit_bipartite
    base = ref(df, C1=0.5, C2=0.5, iterations=0, verbose=False, **kw)
    if pp:
        assert np.array_equal(base["W1"], base["G12"]) and np.array_equal(base["W2"], base["G21"])
    U = X.exact_updates_bipartite(base["G12"], base["G21"], 0.5, base.get("E1"), base.get("E2")).updates
    print(f"biregular_graph({n1}, {n2}, {d1}) {cls}: {U} exact updates")
    assert U >= 2
    want = ref(df, C1=0.5, C2=0.5, iterations=U, eps=TINY, verbose=False, **kw)
    est = getattr(SRA, cls)()
    s1, s2 = est.fit(df, C1=0.5, C2=0.5, iterations=U, eps=TINY, verbose=False, **kw)
    lab1, lab2 = ("sorted1", "sorted2") if pp else ("labels1", "labels2")
    assert list(s1.index) == list(want[lab1]) and list(s2.index) == list(want[lab2])
    assert np.array_equal(s1.values, want["S1"]) and np.array_equal(s2.values, want["S2"])
    assert est.converged_at == want["k"]


# ---- the other formats ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", GRAPHS)
@pytest.mark.parametrize("cls", ["SimRank", "SimRankPP"])
def test_f64_storage_is_the_oracle(n, d, cls):
    """storage_precision="f64": 53 bits, so many more exact updates (its own count), the same bits as the oracle's float64."""
    c = case(n, d)
    pp = cls == "SimRankPP"
    U = c.updates(pp, mantissa=53)
    assert U > c.updates(pp) or U >= 8
    S, k = c.oracle(pp, U, TINY)
    est, got = fit(cls, c, U, TINY, storage_precision="f64")
    same_frame(got, S, c.labels)
    assert est.converged_at == k
    U, eps, step = X.tie_eps(c.iterates(pp, U), fmt=np.float64)
    S, k = c.oracle(pp, U, eps)
    est, got = fit(cls, c, U, eps, storage_precision="f64")                 # f64.hip's own count, on a tie
    assert est.converged_at == k == U - 1
    same_frame(got, S, c.labels)


@pytest.mark.parametrize("n,d", [(300, 2), (512, 2)])
@pytest.mark.parametrize("how", ["storage", "storage-ranks", "wire-full", "wire-half"])
def test_fp16_storage_and_wire_are_the_oracle_within_11_bits(n, d, how):
    """exact_updates(mantissa=11): while every term fits fp16's 11 bits, matrices held in fp16 and exchanges over the fp16
    wire round nothing."""
    c = case(n, d)
    U = c.updates(False, mantissa=11)
    assert U >= 2
    S, k = c.oracle(False, U, TINY)
    if how == "storage":
        kw = dict(storage_precision="fp16")
    elif how == "storage-ranks":
        if n % 64:
            kw = dict(storage_precision="fp16", world=LocalWorld(1))
        else:
            kw = dict(storage_precision="fp16", world=LocalWorld(4))
    else:
        kw = dict(mode="sparse", world=LocalWorld(4, symmetric_shards=how == "wire-half", exchange_precision="fp16"))
    est, got = fit("SimRank", c, U, TINY, **kw)
    same_frame(got, S, c.labels)
    assert est.converged_at == k
