"""Whole TWO-MATRIX loops on graphs whose node reorder is a real permutation on BOTH sides, bit for bit against the oracle.

tests/exact.py pow2_bidegree_graph: mixed power-of-two degrees among the users AND among the items, so the stable length
order of each group (planprep.hip length_order) is neither the identity nor — for n1 = n2 — the other group's.  What only
a bipartite plan does then shows in the bits: the columns of group w's pattern renamed by the OTHER group's order, one
(ord, inv) pair and one prior upload per group, the group-1 counts taken in group 2's order under strict_reference, the
dealt order per group on shards.  Row scales are powers of two and C1 = C2 = 0.5, so for U updates (exact_updates_bipartite
on the oracle's matrices, pinned in tests/test_exact_cpu.py) no summation order rounds: np.array_equal against the oracle,
integer equality for every count, and the leg-2 path of every update held against the rule of tests/leg2_rule.py.  No
tolerance anywhere.  SimRank.py:280-302, :402-424, :470-492."""
import ctypes as C

import numpy as np
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import ingest
from simrank_amd.driver import LocalWorld
from tests import evidence_ref as E
from tests import exact as X
from tests import test_gpu_exact_priors as P
from tests.leg2_rule import short_groups
from tests.test_gpu_exact_priors import ops  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TINY = P.TINY
MIXED = ("mixed384", "mixed512")
# (graph, class, strict_reference): SimRank and SimRank++ on both mixed graphs, the reference's Evidence_N1 on both updates where
# n1 = n2 allows it
FITS = [(g, cls, False) for g in MIXED for cls in ("BipartiteSimRank", "BipartiteSimRankPP")] + [("mixed384", "BipartiteSimRankPP", True)]
KINDS = {"sym-sym": (True, True), "asym-sym": (False, True), "asym-asym": (False, False)}


def _fit_id(v):
    return v if isinstance(v, str) else ("strict" if v else "corrected")


def loop_of(graph, cls, strict, mantissa=24):
    return X.bi_loop(graph, pp=cls.endswith("PP"), strict=strict, mantissa=mantissa)


def same2(got, c, u, what):
    """Both matrices after update u of loop c."""
    P.same(got[0], c.pairs[u - 1][0], f"{what}: S1 after update {u}")
    P.same(got[1], c.pairs[u - 1][1], f"{what}: S2 after update {u}")


def fit(c, cls, iterations, eps, **kw):
    est = getattr(SRA, cls)()
    args = (c.A1, c.A2) if c.kinds is not None else ()
    if c.kinds is not None:
        kw.update(lbd1=c.lbd, lbd2=c.lbd)
    got = est.fit(c.df, *args, C1=0.5, C2=0.5, iterations=iterations, eps=eps, verbose=False, strict_reference=c.strict, **kw)
    return est, got


def check_frames(got, c, want, what):
    s1, s2 = got
    for s, lab, col in ((s1, c.lab1, "user"), (s2, c.lab2, "item")):
        if c.strict:                      # (the reference's labels: set order on arrays that are in sorted order, quirk Q1)
            lab = list(set(c.df[col].unique()))
        assert list(s.index) == lab and list(s.columns) == lab
    P.same(s1.values, want[0], what + ": S1")
    P.same(s2.values, want[1], what + ": S2")


def csrs(c):
    _, _, lab1, lab2, g12, g21 = ingest.bipartite(c.df, False, "user", "item", "weight")
    assert list(lab1) == c.lab1 and list(lab2) == c.lab2
    return g12, g21


def biplan(ops, c, **kw):
    from simrank_amd.engine import BiPlan
    g12, g21 = csrs(c)
    prior = dict(apriori1=c.A1, apriori2=c.A2, lbd1=c.lbd, lbd2=c.lbd) if c.kinds is not None else {}
    return BiPlan(ops, g12, g12.rowscale, g21.rowscale, c1=0.5, c2=0.5, evidence=c.pp, strict_reference=c.strict, **prior, **kw)


def orders(ops, bp):
    return [P.solver_order(ops, lambda k, g=g: bp.get(g, k)) for g in (1, 2)]


def check_orders(c, got, reorder=True):
    """Both groups' "ids": the stable length order restated in NumPy — real permutations that differ from each other, or
    (reorder = 0) the identity."""
    for g, o in zip((1, 2), got):
        want = X.stable_length_order(c.lengths(g)) if reorder else np.arange(len(o))
        assert np.array_equal(o, want), f"group {g}: not the stable length order"
        assert P.is_identity(o) == (not reorder)
    if reorder:
        assert len(got[0]) != len(got[1]) or not np.array_equal(got[0], got[1])


def stepped(bp, c, runs, check=None):
    """simrank_biplan_step with exact_count = 1, once per entry (group, kind) of `runs` after reset(): ONE eps for both
    half-updates of a step — X.count_eps of that group's update: below every difference (0), on a difference that occurs (1),
    one grid step below it (2) — and each side's count from the oracle's iterates in NumPy."""
    for g, kind in runs:
        bp.reset()
        old = (np.eye(c.n1), np.eye(c.n2))
        for u, new in enumerate(c.pairs, 1):
            eps = X.count_eps(new[g], old[g])[kind][0]
            wants = tuple(int((np.abs(new[j] - old[j]) > eps).sum()) for j in (0, 1))
            got = bp.step(eps, exact_count=True)
            assert got == wants, (g, kind, u, eps, got, wants)
            if check is not None:
                check(bp, u)
            same2((bp.result_group(1), bp.result_group(2)), c, u, f"eps of group {g + 1}, kind {kind}")
            old = new


ALL_RUNS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2))


# ---- fit() ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,cls,strict", FITS, ids=_fit_id)
@pytest.mark.parametrize("mode", ["auto", "sparse"])
def test_fit_is_the_oracle(graph, cls, strict, mode):
    c = loop_of(graph, cls, strict)
    U = c.updates
    assert U >= 2
    s1, s2, k = c.oracle(U, TINY)
    est, got = fit(c, cls, U, TINY, mode=mode)
    check_frames(got, c, (s1, s2), f"{cls} {mode}")
    assert est.converged_at == k
    if c.pp:
        from oracle import simrank_oracle as O
        assert np.array_equal(np.asarray(est.Evidence_N1), c.E1)
        assert np.array_equal(np.asarray(est.Evidence_N2), O.evidence(c.G21))
    if mode == "sparse":
        assert est.engine_mode == "sparse"


@pytest.mark.parametrize("graph,cls,strict", FITS, ids=_fit_id)
def test_fit_stops_on_a_tie_where_the_oracle_stops(graph, cls, strict):
    """eps = the largest difference of either group at loop index U - 1: the test there passes only under strict > in BOTH
    groups' counts; one grid step less and the loop applies all U updates."""
    c = loop_of(graph, cls, strict)
    U, eps, step = c.tie_eps()
    s1, s2, k = c.oracle(U, eps)
    assert k == U - 1
    est, got = fit(c, cls, U, eps)
    assert est.converged_at == k
    check_frames(got, c, (s1, s2), "eps on the tie")
    s1, s2, k = c.oracle(U, eps - step)
    assert k is None
    est, got = fit(c, cls, U, eps - step)
    assert est.converged_at is None
    check_frames(got, c, (s1, s2), "eps one step below the tie")


# ---- the plan, update by update -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,cls,strict", FITS, ids=_fit_id)
@pytest.mark.parametrize("identity_leg1", ["1", "0"])
@pytest.mark.parametrize("reorder", [1, 0])
def test_biplan_stepped_update_by_update(ops, monkeypatch, graph, cls, strict, identity_leg1, reorder):
    """engine.BiPlan: both iterates and both counts of every update, with and without the identity's leg 1, in the solver's
    order and in the caller's; the node orders read back and held against the rule; the counts that gate each group."""
    monkeypatch.setenv("SIMRANK_IDENTITY_LEG1", identity_leg1)
    c = loop_of(graph, cls, strict)
    assert c.updates >= 2
    bp = biplan(ops, c, reorder=bool(reorder))
    try:
        check_orders(c, orders(ops, bp), bool(reorder))
        if c.pp:
            g12, g21 = csrs(c)
            want1 = E.counts(g12).toarray().astype(np.uint8)
            assert np.array_equal(bp.evidence_counts(1), want1)
            # strict_reference: group 2's counts are group 1's, position by position in the caller's order
            assert np.array_equal(bp.evidence_counts(2), want1 if strict else E.counts(g21).toarray().astype(np.uint8))
            assert not strict or not np.array_equal(want1, E.counts(g21).toarray().astype(np.uint8))
        stepped(bp, c, ALL_RUNS if identity_leg1 == "1" and reorder else ((0, 1), (1, 2)))
    finally:
        bp.free()


# ---- which leg 2 ran ------------------------------------------------------------------------------------------------------
def _taken(ops, bp, g):
    return ops.graph_get(bp.graph_handle(g), "leg2_short_taken")


@pytest.mark.parametrize("graph", MIXED)
@pytest.mark.parametrize("width", P.LEG2_WIDTHS)
def test_two_launch_leg2_takes_the_path_the_rule_says(ops, graph, width):
    """The two-launch upper-triangle leg 2 forced, leg2_short = 0, 8, 16: after every update each group's
    "leg2_short_groups" — and "leg2_short_taken" of the group's own graph object, through the plan's "graph" key — is the
    rule on that group's row lengths IN THE SOLVER'S ORDER."""
    c = X.bi_loop(graph)
    with P.knobs(ops, leg2_short=width, **P.TWO_LAUNCH):
        bp = biplan(ops, c)
        try:
            order = orders(ops, bp)
            rules = [short_groups(c.lengths(g)[order[g - 1]].tolist(), width) for g in (1, 2)]
            assert all((r > 0) == (width >= int(c.lengths(g).max())) for g, r in zip((1, 2), rules)), rules

            def check(bp, u):
                for g in (1, 2):
                    assert bp.get(g, "leg2_short_groups") == rules[g - 1] == _taken(ops, bp, g), (u, g, rules)
                    assert ops.graph_get(bp.graph_handle(g), "leg2_short_groups") == rules[g - 1]
            stepped(bp, c, ((0, 1), (1, 2)), check=check)
        finally:
            bp.free()


def _covered(ops, handle):
    """-> (entries on the matrix cores, all entries) of simrank_graph_fused_stats."""
    steps, cov, rem = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert ops.lib.simrank_graph_fused_stats(handle, C.byref(steps), C.byref(cov), C.byref(rem)) == 0
    return cov.value, cov.value + rem.value


HUB_KNOBS = {"fuse_min 2": dict(fuse_min=2, fuse_steps=1),
             "split blocks": dict(fuse_min=2, fuse_steps=1, fuse_unit=4, fuse_rows=64)}


@pytest.mark.parametrize("kind", ["plain", "prior without evidence"])
@pytest.mark.parametrize("form", list(HUB_KNOBS))
@pytest.mark.parametrize("fuse_sym", [1, 0])
def test_hub_graph_runs_the_one_launch_leg2_inside_the_loop(ops, kind, form, fuse_sym):
    """"hub512": 48 items that 8 users each reference — dense sets in group 1's pattern, whose COLUMNS the hub items are
    (asserted through the plan's "graph" key: entries covered by matrix-core steps > 0).  With fuse_sym = 1 that group's leg 2
    is the one-launch kernel; with fuse_sym = 0 the two-launch leg runs, on its short path, as the rule says.  Which of the
    two ran is INFERRED (no key names the kernel of a launch): the graph holds its short image with the rule's groups in both
    runs, the two-launch leg takes all of them ("leg2_short_taken" == rule > 0), and the only other launch spmm.hip has for a
    panel-blocked triangle form with dense_sym = 0 — the one-launch leg, chosen by fuse_sym = 1 wherever the graph has a
    one-launch plan — takes none.  "split blocks": a block whose gathered remainder exceeds fuse_rows entries is cut into
    gather units (fused.hip) — asserted from the statistics: the gathered entries exceed fuse_rows x the number of 128-row
    blocks, so some block is split; under the first knob set they stay below fuse_rows and none is.  Bits and counts are the
    oracle's either way."""
    c = X.bi_loop("hub512", kinds=(True, True)) if kind != "plain" else X.bi_loop("hub512")
    assert c.updates >= 1
    with P.knobs(ops, fuse_sym=fuse_sym, dense_sym=0, ids16=1, restrict_support=0, balance=2, leg2_short=16, **HUB_KNOBS[form]):
        bp = biplan(ops, c)
        try:
            order = orders(ops, bp)
            check_orders(c, order)
            rules = [short_groups(c.lengths(g)[order[g - 1]].tolist(), 16) for g in (1, 2)]
            assert min(rules) > 0
            cov = [_covered(ops, bp.graph_handle(g)) for g in (1, 2)]
            print(f"hub512 {form}: entries on the matrix cores {cov}")
            # (group 2's pattern has the hubs as ROWS of 8 entries; at fuse_min 2 the users that two of a block's rows share
            # make its dense sets)
            assert cov[0][0] > 0 and cov[1][0] > 0 and cov[0][1] == cov[1][1] == len(c.df), "no dense set on the hub graph"
            fuse_rows = ops.get_tuning("fuse_rows")
            for (covered, entries), n in zip(cov, (c.n1, c.n2)):
                blocks = (n + 127) // 128
                if form == "split blocks":
                    assert fuse_rows == 64 and entries - covered > fuse_rows * blocks, "no block is split"
                else:
                    assert entries - covered <= fuse_rows and ops.get_tuning("fuse_unit") >= 48, "a block is split"

            def check(bp, u):
                for g in (1, 2):
                    assert ops.graph_get(bp.graph_handle(g), "leg2_short_groups") == rules[g - 1]
                    assert bp.get(g, "leg2_short_groups") == _taken(ops, bp, g) == (0 if fuse_sym == 1 else rules[g - 1]), (u, g)
            stepped(bp, c, ((0, 0), (0, 1), (1, 2)), check=check)
        finally:
            bp.free()


# ---- priors, through two real reorders ------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", MIXED)
@pytest.mark.parametrize("kinds", list(KINDS))
def test_priors_on_a_mixed_graph(ops, graph, kinds):
    """BipartitleAprioriSimRank.fit and engine.BiPlan stepped, 2-bit loop_priors, lbd 0.5: each group's prior is uploaded as
    A[ord][:, ord] with ITS group's order — an ord / inv mix-up or a group mix-up cannot pass (asserted: the two
    permutations of each prior differ, and so do the groups' orders)."""
    c = X.bi_loop(graph, pp=True, kinds=KINDS[kinds])
    U = c.updates
    assert U >= 1
    s1, s2, k = c.oracle(U, TINY)
    est, got = fit(c, "BipartitleAprioriSimRank", U, TINY)
    check_frames(got, c, (s1, s2), f"priors {kinds}")
    assert est.converged_at == k
    bp = biplan(ops, c)
    try:
        order = orders(ops, bp)
        check_orders(c, order)
        for A, o in ((c.A1, order[0]), (c.A2, order[1])):
            inv = np.argsort(o)
            assert not np.array_equal(A[np.ix_(o, o)], A[np.ix_(inv, inv)])
        if c.n1 == c.n2:
            o, other = order
            assert not np.array_equal(c.A2[np.ix_(other, other)], c.A2[np.ix_(o, o)])
        stepped(bp, c, ALL_RUNS)
    finally:
        bp.free()


# ---- several ranks ----------------------------------------------------------------------------------------------------------
def _rank_fits():
    out = []
    for g in MIXED:
        for Pn in (2, 4):
            for half in (False, True):
                for stages in (1, 2):
                    out.append(pytest.param(g, Pn, half, stages, id=f"{g}-{Pn}-{'half' if half else 'full'}-{stages}"))
    return out


@pytest.mark.parametrize("graph,Pn,half,stages", _rank_fits())
def test_virtual_ranks_are_the_oracle(graph, Pn, half, stages):
    """LocalWorld(2 | 4) through fit: the full and the half form of leg 2 (both groups' node counts are multiples of 32 x ranks
    and of 128: the half form deals each group's order), one and two stages; SimRank++ for 2 ranks, plain for 4."""
    cls = "BipartiteSimRankPP" if Pn == 2 else "BipartiteSimRank"
    c = loop_of(graph, cls, False)
    assert c.n1 % (32 * Pn) == 0 and c.n2 % (32 * Pn) == 0
    U = c.updates
    s1, s2, k = c.oracle(U, TINY)
    est, got = fit(c, cls, U, TINY, mode="sparse", world=LocalWorld(Pn, symmetric_shards=half, leg2_stages=stages, loop="c"))
    check_frames(got, c, (s1, s2), f"{Pn} ranks")
    assert est.converged_at == k


def _shard_columns(ops, side):
    out = []
    for i, h in enumerate(side.handles):
        inf = side.info(i)
        ids = np.empty(inf["col_hi"] - inf["col_lo"], dtype=np.int32)
        assert ops.lib.simrank_shardplan_columns(h, ids.ctypes.data) == 0
        out.append(ids)
    return np.concatenate(out)


def _shard_cases():
    out = []
    for g in MIXED:
        for Pn in (2, 4):
            for what, form, stages in (("plain", 0, 1), ("plain", 1, 2), ("pp", 1, 1), ("asym prior", 0, 2)):
                out.append(pytest.param(g, Pn, what, form, stages, id=f"{g}-{Pn}-{what.replace(' ', '_')}-{'half' if form else 'full'}-{stages}"))
    return out


@pytest.mark.parametrize("graph,Pn,what,leg2_form,stages", _shard_cases())
def test_shard_biplans_are_the_oracle(ops, graph, Pn, what, leg2_form, stages):
    """engine.ShardBiPlans on 2 and 4 virtual ranks, stepped with both counts, then run().  Every rank's column ids, read from
    the ranks' plans and put together, are the group's solver order: the stable length order, in the half form dealt to the
    ranks in runs of 128 (planprep.hip deal_order, restated in tests/exact.py) — per group."""
    from simrank_amd.engine import ShardBiPlans
    c = X.bi_loop(graph, pp=what != "plain", kinds=(False, True) if what == "asym prior" else None)
    U = c.updates
    assert U >= 1
    g12, g21 = csrs(c)
    prior = dict(apriori1=c.A1, apriori2=c.A2, lbd1=c.lbd, lbd2=c.lbd) if c.kinds is not None else {}
    bp = ShardBiPlans(ops, g12, g12.rowscale, g21.rowscale, world=Pn, c1=0.5, c2=0.5, evidence=c.pp, strict_reference=False,
                      leg2_form=leg2_form, stages=stages, **prior)
    try:
        got_orders = []
        for g in (1, 2):
            side = bp.side(g - 1)
            assert side.info(0)["half_form"] == bool(leg2_form)
            order = _shard_columns(ops, side)
            want = X.dealt_order(X.stable_length_order(c.lengths(g)), Pn if leg2_form else 1)
            assert np.array_equal(order, want), f"group {g}: column ids of the ranks"
            assert not P.is_identity(order)
            got_orders.append(order)
        assert len(got_orders[0]) != len(got_orders[1]) or not np.array_equal(*got_orders)
        if leg2_form:                       # (the deal is a real one in one group at least: one run of 128 per rank deals nothing)
            assert any(not np.array_equal(o, X.stable_length_order(c.lengths(g))) for g, o in zip((1, 2), got_orders))
        for g, kind in ((0, 0), (0, 1), (1, 2)):
            bp.reset()
            old = (np.eye(c.n1), np.eye(c.n2))
            for u, new in enumerate(c.pairs, 1):
                eps = X.count_eps(new[g], old[g])[kind][0]
                wants = tuple(int((np.abs(new[j] - old[j]) > eps).sum()) for j in (0, 1))
                assert bp.step(eps, exact_count=True) == wants, (g, kind, u, eps)
                old = new
            same2((bp.result(1), bp.result(2)), c, U, f"{Pn} ranks stepped")
        s1, s2, k = c.oracle(U, TINY)
        bp.reset()
        assert bp.run(U, TINY) == (U if k is None else k, k)
        P.same(bp.result(1), s1, "run: S1")
        P.same(bp.result(2), s2, "run: S2")
    finally:
        bp.free()


def test_thread_ranks_on_a_mixed_graph():
    """Two CONCURRENT ranks (one thread group: the code path of an RCCL rank), SimRank++ in the half form on "mixed512"."""
    from simrank_amd.engine import ShardBiPlans
    c = X.bi_loop("mixed512", pp=True)
    U = c.updates
    g12, g21 = csrs(c)
    s1, s2, k = c.oracle(U, TINY)

    def rank(r, rops, comm):
        bp = ShardBiPlans(rops, g12, g12.rowscale, g21.rowscale, world=2, comm=comm, c1=0.5, c2=0.5, evidence=True,
                          strict_reference=False, leg2_form=1, stages=1)
        try:
            return bp.run(U, TINY), bp.result(1, root=0, i_am_root=(r == 0)), bp.result(2, root=0, i_am_root=(r == 0))
        finally:
            bp.free()
    outs = P._thread_ranks(2, rank)
    assert all(o[0] == (U if k is None else k, k) for o in outs)
    P.same(outs[0][1], s1, "S1")
    P.same(outs[0][2], s2, "S2")


# ---- float64 storage --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", MIXED)
@pytest.mark.parametrize("cls", ["BipartiteSimRank", "BipartiteSimRankPP"])
def test_f64_storage_is_the_oracle(graph, cls):
    """storage_precision="f64": 53 bits, its own count of exact updates (more than float32's), the oracle's float64 bits."""
    c = loop_of(graph, cls, False, mantissa=53)
    U = c.updates
    assert U > loop_of(graph, cls, False).updates
    s1, s2, k = c.oracle(U, TINY)
    est, got = fit(c, cls, U, TINY, storage_precision="f64")
    check_frames(got, c, (s1, s2), "f64")
    assert est.converged_at == k
    Ut, eps, step = c.tie_eps()
    s1, s2, k = c.oracle(Ut, eps)
    est, got = fit(c, cls, Ut, eps, storage_precision="f64")
    assert est.converged_at == k == Ut - 1
    check_frames(got, c, (s1, s2), "f64, eps on the tie")


# ---- hand-backs per group -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [None, 2])
def test_handbacks_per_group(world):
    """The exact S1 (512 x 512) and S2 (256 x 256) of "mixed512" through every hand-back, per group, each through its own
    group's order and its inverse: fit(top_k=) against a host selection in the project's total order, fit(min_similarity=t)
    with t a value that occurs, and the kept model's rows, similarity both ways and most_similar with group = 1 | 2 — before
    and after compact()."""
    cls = "BipartiteSimRank"
    c = loop_of("mixed512", cls, False)
    U = c.updates
    S = c.oracle(U, TINY)[:2]
    labs = (c.lab1, c.lab2)
    kw = dict(mode="sparse", world=LocalWorld(world)) if world else {}
    est, got = fit(c, cls, U, TINY, top_k=10, **kw)
    for j in (0, 1):
        P._same_long(got[j], P._host_topk(S[j], labs[j], 10))
    ts = []
    for j in (0, 1):
        off = np.unique(S[j][~np.eye(len(labs[j]), dtype=bool)])
        ts.append(float(off[-3]))
    t = min(ts)                                                         # a value that occurs in one group at least
    assert any(np.any(S[j] == t) for j in (0, 1))
    est, got = fit(c, cls, U, TINY, min_similarity=t, **kw)
    for j in (0, 1):
        P._same_long(got[j], P._dense_pairs(S[j], labs[j], t))
    est, model = fit(c, cls, U, TINY, keep=True, **kw)
    assert model is est
    rng = np.random.default_rng(11)
    try:
        for packed in (False, True):
            if packed:
                est.compact()
            for j, group in ((0, 1), (1, 2)):
                n = len(labs[j])
                nodes = [0, 31, 32, n - 1, n // 2 + 5] + rng.choice(n, size=20, replace=False).tolist()
                rows = est.rows(nodes, group=group)
                assert list(rows.index) == nodes and list(rows.columns) == labs[j]
                P.same(rows.values, S[j][nodes], f"rows, group {group}")
                a = rng.integers(0, n, size=400).tolist() + [0, n - 1]
                b = rng.integers(0, n, size=400).tolist() + [n - 1, 0]
                P.same(est.similarity(a, b, group=group), S[j][a, b], f"similarity(a, b), group {group}")
                P.same(est.similarity(b, a, group=group), S[j][b, a], f"similarity(b, a), group {group}")
                want = P._host_topk(S[j], labs[j], 10)
                pick = np.concatenate([np.arange(10 * v, 10 * v + 10) for v in nodes])
                P._same_long(est.most_similar(nodes, 10, group=group), want.iloc[pick].reset_index(drop=True))
    finally:
        est.release()
