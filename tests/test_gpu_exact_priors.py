"""Whole loops WITH A PRIOR on graphs whose iterates stay exact (tests/exact.py: prior_case, bi_prior_case), bit for bit
against the oracle: AprioriSimRank and BipartitleAprioriSimRank, symmetric and asymmetric priors.

The graphs are those of tests/test_gpu_exact_fits.py (row scales powers of two, C = 0.5); the prior lives on a dyadic grid
(integers below 4 times 1/4, a diagonal of values that differ from 1 and from each other) and lbd is 0.5 or 0.25, so every
term of (1 - lbd) * E * C * W S W^T + lbd * A — the blend included — is representable for U updates, which exact_updates
computes (and pins on the CPU: tests/test_exact_cpu.py).  Within U the float64 oracle's frame is the only right answer in
any summation order: np.array_equal, no tolerance.  An asymmetric prior makes the iterates asymmetric (at hundreds of
thousands of places: a transposed answer cannot pass); the plans then run leg 2 as leg 1's launch on Tt with a transposed
store and the epilogue as a pass of its own, in place, whose count is a count over all n^2 elements.
SimRank.py:438-455, :470-492."""
import contextlib
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import ingest
from simrank_amd.driver import LocalWorld
from tests import exact as X
from tests.leg2_rule import short_groups

pytestmark = pytest.mark.gpu

TINY = 1e-30                    # an eps no difference of these runs is below, but zero
LEG2_WIDTHS = (0, 8, 16)
# the two-launch upper-triangle leg 2 on the plain pattern (as tests/test_gpu_exact_fits.py)
TWO_LAUNCH = dict(fuse_sym=0, dense_sym=0, ids16=1, restrict_support=0, balance=2)
KIND = {True: "symmetric", False: "asymmetric"}


@pytest.fixture(scope="module")
def ops():
    from simrank_amd.engine import HipOps
    return HipOps(0)


@contextlib.contextmanager
def knobs(ops, **kw):
    """Process-wide tuning values for the plans created inside; restored."""
    saved = {k: ops.get_tuning(k) for k in kw}
    ops.set_tuning(**kw)
    try:
        yield
    finally:
        ops.set_tuning(**saved)


def same(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, c = bad[0]
        swapped = int((got == want.T).sum()) if want.shape[0] == want.shape[1] else -1
        raise AssertionError(f"{what}: {len(bad)} elements differ from the oracle, first at ({r}, {c}): {got[r, c]!r} != "
                             f"{want[r, c]!r} ({swapped} equal the oracle's TRANSPOSE)")


def same_frame(got, want_S, labels, what=""):
    assert list(got.index) == labels and list(got.columns) == labels
    same(got.values, want_S, what)


def fit(c, iterations, eps, **kw):
    est = SRA.AprioriSimRank()
    got = est.fit(c.df, c.A, C=0.5, lbd=c.lbd, iterations=iterations, eps=eps, verbose=False, **kw)
    return est, got


def directed_csr(c):
    nodes, csr = ingest.directed(c.df, False, "from", "to", "weight")
    assert nodes == c.labels
    assert np.array_equal(ingest.spread(csr), np.ones(c.n))               # (so the row scale of W is the graph's)
    return csr


def solver_order(ops, get):
    """The caller's node id at each solver position, read back from the plan ("ids" of simrank_plan_get & co)."""
    n = get("iterate_rows")
    order = np.empty(n, dtype=np.int32)
    ops.d2h(order, get("ids"))
    ops.synchronize()
    assert np.array_equal(np.sort(order), np.arange(n))
    return order


def is_identity(order):
    return bool(np.array_equal(order, np.arange(len(order))))


def cases(graphs, symmetric=(True, False), lbds=X.PRIOR_LBD):
    return [pytest.param(g, s, l, id=f"{g[0]}{g[1]}-{g[2]}-{KIND[s]}-{l}") for g in graphs for s in symmetric for l in lbds]


# ---- 1, 2: fit() ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,symmetric,lbd", cases(X.PRIOR_GRAPHS))
@pytest.mark.parametrize("mode", ["auto", "sparse"])
def test_fit_is_the_oracle(graph, symmetric, lbd, mode):
    c = X.prior_case(graph, symmetric, lbd)
    U = c.updates
    assert U >= 2
    S, k = c.oracle(U, TINY)
    est, got = fit(c, U, TINY, mode=mode)
    same_frame(got, S, c.labels, "fit")
    assert est.converged_at == k
    assert np.array_equal(np.asarray(est.Evidence), c.E)
    if not symmetric or mode == "sparse":
        assert est.engine_mode == "sparse"


@pytest.mark.parametrize("graph,symmetric,lbd", cases(X.PRIOR_GRAPHS))
def test_fit_stops_on_a_tie_where_the_oracle_stops(graph, symmetric, lbd):
    """eps = max |S_{U-1} - S_{U-2}|: the test at loop index U - 1 passes only under strict > — in the fused epilogue for a
    symmetric prior, in the in-place pass for an asymmetric one; one grid step less and all U updates are applied."""
    c = X.prior_case(graph, symmetric, lbd)
    U, eps, step = X.tie_eps(c.iterates())
    S, k = c.oracle(U, eps)
    assert k == U - 1
    est, got = fit(c, U, eps)
    assert est.converged_at == k
    same_frame(got, S, c.labels, "eps on the tie")
    S, k = c.oracle(U, eps - step)
    assert k is None
    est, got = fit(c, U, eps - step)
    assert est.converged_at is None
    same_frame(got, S, c.labels, "eps one step below the tie")


# ---- 3, 4, 8: the plan, update by update ------------------------------------------------------------------------------
def _stepped(plan, c, check=None, runs=(0, 1, 2, 0)):
    """simrank_plan_step with exact_count = 1, the whole loop once per entry of `runs` (reset() before each): after every
    update the oracle's iterate, and n_changed == int((abs(S_u - S_{u-1}) > eps).sum()) for eps = TINY (0), a difference
    that occurs in the update (1), that minus one grid step (2) — X.count_eps.  `check(plan, u)`: what else must hold."""
    its = c.iterates()
    for kind in runs:
        plan.reset()
        for u in range(1, c.updates + 1):
            eps, want = X.count_eps(its[u], its[u - 1])[kind]
            got = plan.step(eps, exact_count=True)
            assert got == want, (kind, u, eps, got, want)
            if check is not None:
                check(plan, u)
            same(plan.result(), its[u], f"run with eps kind {kind}, update {u}")


def _asym_paths(plan, u):
    assert plan.get("leg2_short_groups") == 0 and plan.get("leg1_skipped") == 0, u


@pytest.mark.parametrize("graph,symmetric,lbd", cases(X.PRIOR_GRAPHS))
@pytest.mark.parametrize("identity_leg1", ["1", "0"])
def test_plan_stepped_update_by_update(ops, monkeypatch, graph, symmetric, lbd, identity_leg1):
    """engine.Plan: the iterate and the count of every update, with and without the identity's leg 1, four runs on one
    plan.  The symmetric form's count carries the weight 2 of mirrored elements, the asymmetric pass counts all n^2
    elements: both must be NumPy's count on the oracle's iterates.  (Every row of a regular graph has d entries, so the
    solver's order — a stable sort by row length — is the caller's here, asserted: the reorder is the next test's.)"""
    from simrank_amd.engine import Plan
    monkeypatch.setenv("SIMRANK_IDENTITY_LEG1", identity_leg1)
    c = X.prior_case(graph, symmetric, lbd)
    assert c.updates >= 2
    plan = Plan(ops, directed_csr(c), coef=0.5, evidence=True, apriori=c.A, lbd=lbd)
    try:
        assert is_identity(solver_order(ops, plan.get))
        _stepped(plan, c, check=None if symmetric else _asym_paths)
    finally:
        plan.free()


@pytest.mark.parametrize("graph,symmetric,lbd", cases([X.MIXED_GRAPH], lbds=(0.5,)))
@pytest.mark.parametrize("reorder", [1, 0])
def test_plan_stepped_after_a_reorder_that_permutes_the_prior(ops, graph, symmetric, lbd, reorder):
    """pow2_degree_graph(1031, (2, 4), ...) WITH the evidence factor: rows of 2 and of 4 entries in a shuffled order, so the
    solver's ascending-length order is a real permutation (asserted from the plan's "ids"; with reorder = 0 it is the
    identity, asserted too) and the plan's upload permutes the prior — A[ord[i]][ord[j]] — and the hand-back undoes it:
    an ord / inv mix-up, harmless on a symmetric prior's transposed pairs only, shows in the bits of either kind."""
    from simrank_amd.engine import Plan
    c = X.prior_case(graph, symmetric, lbd)
    assert c.updates >= 2
    plan = Plan(ops, directed_csr(c), coef=0.5, evidence=True, apriori=c.A, lbd=lbd, reorder=bool(reorder))
    try:
        order = solver_order(ops, plan.get)
        assert is_identity(order) == (reorder == 0)
        if reorder:
            assert not np.array_equal(c.A[np.ix_(order, order)], c.A[np.ix_(np.argsort(order), np.argsort(order))])
        _stepped(plan, c, check=None if symmetric else _asym_paths)
    finally:
        plan.free()


@pytest.mark.parametrize("graph,symmetric,lbd", cases(X.PRIOR_GRAPHS, symmetric=(True,)))
@pytest.mark.parametrize("width", LEG2_WIDTHS)
def test_plan_stepped_on_each_path_of_leg2_with_a_symmetric_prior(ops, monkeypatch, graph, symmetric, lbd, width):
    """The two-launch upper-triangle leg 2 forced, leg2_short = 0, 8, 16: gather3 kSym's fused blend on the general path and
    on the short path, which one said by the plan after every update and held against the rule in NumPy."""
    from simrank_amd.engine import Plan
    monkeypatch.setenv("SIMRANK_IDENTITY_LEG1", "1")
    c = X.prior_case(graph, symmetric, lbd)
    n, d = graph[1], graph[2]
    rule = short_groups([d] * n, width)
    assert rule == (0 if width < d else ((n + 31) // 32 + 3) // 4)

    def check(plan, u):
        assert plan.get("leg2_short_groups") == rule, (u, plan.get("leg2_short_groups"), rule)
    with knobs(ops, leg2_short=width, **TWO_LAUNCH):
        plan = Plan(ops, directed_csr(c), coef=0.5, evidence=True, apriori=c.A, lbd=lbd)
        try:
            _stepped(plan, c, check=check, runs=(1, 2))
        finally:
            plan.free()


def _covered(ops, plan):
    steps, cov, rem = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert ops.lib.simrank_graph_fused_stats(plan.graph_handle(), C.byref(steps), C.byref(cov), C.byref(rem)) == 0
    return cov.value


@pytest.mark.parametrize("graph,symmetric,lbd", cases(X.HUB_GRAPHS, lbds=(0.5,)))
@pytest.mark.parametrize("form", ["fuse_min 2", "split blocks"])
def test_matrix_core_part_inside_a_loop_with_a_prior(ops, graph, symmetric, lbd, form):
    """pow2_degree_graph: half of all references on 48 hub columns, so the one-launch kernel has dense sets (asserted:
    entries covered by matrix-core steps > 0) — with the asymmetric prior BOTH legs run it, leg 2 on Tt.  The plan-level
    loop with a prior and without the evidence factor; degrees (2, 4) for a third exact update.  (At the default fuse_min
    a plan chooses no dense set on these graphs — DESIGN.md §7 —, so both forms set the knobs, as the kernel-level exact
    module does.)  The solver's order is a real permutation here as well."""
    from simrank_amd.engine import Plan
    c = X.prior_case(graph, symmetric, lbd, evidence=False)
    assert c.updates >= 2
    csr = directed_csr(c)
    kw = dict(fuse_min=2, fuse_steps=1) if form == "fuse_min 2" else dict(fuse_min=3, fuse_steps=2, fuse_unit=4, fuse_rows=400)
    with knobs(ops, **kw):
        plan = Plan(ops, csr, coef=0.5, evidence=False, apriori=c.A, lbd=lbd)
        try:
            covered = _covered(ops, plan)
            print(f"{graph} {form}: {covered} of {csr.nnz} entries on the matrix cores")
            assert covered > 0, "no dense set on the hub graph"
            assert not is_identity(solver_order(ops, plan.get))
            _stepped(plan, c, check=None if symmetric else _asym_paths, runs=(0, 1, 2))
        finally:
            plan.free()


# ---- 5: the two-matrix loop -----------------------------------------------------------------------------------------
def _bi_id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else None


@pytest.mark.parametrize("shape", X.BI_PRIOR, ids=_bi_id)
@pytest.mark.parametrize("kinds", X.BI_PRIOR_KINDS, ids=["sym-sym", "asym-sym", "sym-asym"])
def test_bipartite_pair_is_the_oracle(ops, shape, kinds):
    """BipartitleAprioriSimRank.fit and engine.BiPlan stepped, with the counts of both half-updates; one asymmetric prior puts
    both sides on the un-fused path."""
    from simrank_amd.engine import BiPlan
    c = X.bi_prior_case(*shape, *kinds)
    U = c.updates
    assert U >= 2
    want = c.oracle(U, TINY)
    est = SRA.BipartitleAprioriSimRank()
    s1, s2 = est.fit(c.df, c.A1, c.A2, C1=0.5, C2=0.5, lbd1=c.lbd, lbd2=c.lbd, iterations=U, eps=TINY, verbose=False,
                     strict_reference=False)
    assert list(s1.index) == list(want["sorted1"]) and list(s2.index) == list(want["sorted2"])
    same(s1.values, want["S1"], "S1")
    same(s2.values, want["S2"], "S2")
    assert est.converged_at == want["k"]
    _, _, lab1, lab2, g12, g21 = ingest.bipartite(c.df, False, "user", "item", "weight")
    assert list(lab1) == list(want["sorted1"]) and list(lab2) == list(want["sorted2"])
    bp = BiPlan(ops, g12, g12.rowscale, g21.rowscale, c1=0.5, c2=0.5, evidence=True, apriori1=c.A1, apriori2=c.A2,
                lbd1=c.lbd, lbd2=c.lbd, strict_reference=False)
    try:
        for kind in (0, 1, 2):
            bp.reset()
            old = (np.eye(c.n1), np.eye(c.n2))
            for u, new in enumerate(c.pairs, 1):
                # one eps for both half-updates of a step: group 1's, and each side counted in NumPy at that eps
                eps = X.count_eps(new[0], old[0])[kind][0]
                wants = tuple(int((np.abs(new[j] - old[j]) > eps).sum()) for j in (0, 1))
                assert bp.step(eps, exact_count=True) == wants, (kind, u, eps)
                same(bp.result_group(1), new[0], f"S1 after step {u}")
                same(bp.result_group(2), new[1], f"S2 after step {u}")
                old = new
    finally:
        bp.free()


# ---- 6: ranks -------------------------------------------------------------------------------------------------------
def _worlds():
    out = []
    for P in (2, 4, 8):
        out += [(P, True, True, 1), (P, True, True, 2), (P, True, False, 1), (P, True, False, 2),
                (P, False, False, 1), (P, False, False, 3)]
    return out


def _rank_cases():
    """(graph, P, symmetric, half, stages): the half form only where the node count allows it (a multiple of 32 P: the first
    graph) — elsewhere symmetric_shards=True would quietly be the full form again."""
    return [pytest.param(g, *w, id=f"{g[1]}-{g[2]}-{w[0]}-{KIND[w[1]]}-{'half' if w[2] else 'full'}-{w[3]}")
            for g in X.PRIOR_RANK_GRAPHS for w in _worlds() if not w[2] or g[1] % (32 * w[0]) == 0]


@pytest.mark.parametrize("graph,P,symmetric,half,stages", _rank_cases())
def test_virtual_ranks_are_the_oracle(monkeypatch, graph, P, symmetric, half, stages):
    """LocalWorld(P): the sharded loop with a symmetric prior in the full and the half form, with an asymmetric prior in the
    full form with its second exchange; which form the ranks took is read from the plans the fit creates."""
    from simrank_amd import engine
    forms = []
    create = engine.ShardPlans.__init__

    def spy(self, *a, **kw):
        create(self, *a, **kw)
        forms.append(self.info(0)["half_form"])
    monkeypatch.setattr(engine.ShardPlans, "__init__", spy)
    lbd = X.PRIOR_LBD[(P // 2 + stages) % 2]                                # both over the grid
    c = X.prior_case(graph, symmetric, lbd)
    U = c.updates
    assert U >= 2
    S, k = c.oracle(U, TINY)
    est, got = fit(c, U, TINY, mode="sparse", world=LocalWorld(P, symmetric_shards=half, leg2_stages=stages, loop="c"))
    same_frame(got, S, c.labels, f"{P} ranks")
    assert est.converged_at == k
    assert forms == [half], forms


def _shard_cases():
    """(graph, P, symmetric, leg2_form, stages, lbd): 2, 4 and 8 ranks; the half form where every rank gets whole tiles; lbd
    0.5 and 0.25 over the grid; the graph with rows of 2 and 4 entries, whose order is a real permutation, in the full form."""
    out = []
    for g in X.PRIOR_RANK_GRAPHS + [X.MIXED_GRAPH]:
        for P in (2, 4, 8):
            forms = [(True, 0, 1), (True, 0, 2), (False, 0, 1), (False, 0, 3)]
            if g[1] % (32 * P) == 0:
                forms += [(True, 1, 1), (True, 1, 2)]
            for i, (sym, form, stages) in enumerate(forms):
                lbd = 0.5 if g == X.MIXED_GRAPH else X.PRIOR_LBD[(i + P // 2) % 2]
                out.append(pytest.param(g, P, sym, form, stages, lbd,
                                        id=f"{g[0]}{g[1]}-{P}-{KIND[sym]}-{'half' if form else 'full'}-{stages}-{lbd}"))
    return out


@pytest.mark.parametrize("graph,P,symmetric,leg2_form,stages,lbd", _shard_cases())
def test_shard_plans_are_the_oracle(ops, graph, P, symmetric, leg2_form, stages, lbd):
    """engine.ShardPlans on 2, 4 and 8 virtual ranks, stepped, with the count of every update (the half form counts a
    mirrored element twice, the asymmetric form every element once: NumPy's count either way), then run().  The ranks'
    column ids put together are the solver's order: a real permutation on the mixed graph (asserted), where every rank
    uploads its columns of the prior as A[ord[i]][ord[m_lo + j]]; the identity for an asymmetric prior on a regular graph."""
    from simrank_amd.engine import ShardPlans
    c = X.prior_case(graph, symmetric, lbd)
    U = c.updates
    assert U >= 2
    its = c.iterates()
    sp = ShardPlans(ops, directed_csr(c), world=P, coef=0.5, evidence=True, apriori=c.A, lbd=c.lbd, leg2_form=leg2_form,
                    stages=stages)
    try:
        assert sp.info(0)["half_form"] == bool(leg2_form)
        order = np.concatenate([sp.block(i)[1] for i in range(P)])
        assert np.array_equal(np.sort(order), np.arange(c.n))
        if graph == X.MIXED_GRAPH:
            assert not is_identity(order)
        elif not symmetric:
            assert is_identity(order)                  # (equal row lengths, and asymmetric plans are not dealt)
        for kind in (0, 1, 2):
            sp.reset()
            for u in range(1, U + 1):
                eps, want = X.count_eps(its[u], its[u - 1])[kind]
                assert sp.step(eps, exact_count=True) == want, (kind, u, eps)
            same(sp.result(), its[U], f"after {U} steps")
        S, k = c.oracle(U, TINY)
        sp.reset()
        assert sp.run(U, TINY) == (U if k is None else k, k)
        same(sp.result(), S, "run")
    finally:
        sp.free()


@pytest.mark.parametrize("kinds", X.BI_PRIOR_KINDS[1:], ids=["asym-sym", "sym-asym"])
@pytest.mark.parametrize("stages", [1, 2])
def test_sharded_two_matrix_loop_with_one_asymmetric_prior(ops, kinds, stages):
    """engine.ShardBiPlans on four virtual ranks and BipartitleAprioriSimRank on LocalWorld(2), on the graph where the
    asymmetry reaches the other side: both iterates asymmetric, a second exchange per half-update."""
    from simrank_amd.engine import ShardBiPlans
    c = X.bi_prior_case(*X.BI_PRIOR[3], *kinds)
    U = c.updates
    _, _, _, _, g12, g21 = ingest.bipartite(c.df, False, "user", "item", "weight")
    bp = ShardBiPlans(ops, g12, g12.rowscale, g21.rowscale, world=4, c1=0.5, c2=0.5, evidence=True, apriori1=c.A1,
                      apriori2=c.A2, lbd1=c.lbd, lbd2=c.lbd, strict_reference=False, leg2_form=0, stages=stages)
    try:
        bp.reset()
        old = (np.eye(c.n1), np.eye(c.n2))
        for u, new in enumerate(c.pairs, 1):
            eps = X.count_eps(new[0], old[0])[1][0]
            wants = tuple(int((np.abs(new[j] - old[j]) > eps).sum()) for j in (0, 1))
            assert bp.step(eps, exact_count=True) == wants, (u, eps)
            old = new
        same(bp.result(1), c.pairs[-1][0], "S1")
        same(bp.result(2), c.pairs[-1][1], "S2")
    finally:
        bp.free()
    want = c.oracle(U, TINY)
    est = SRA.BipartitleAprioriSimRank()
    s1, s2 = est.fit(c.df, c.A1, c.A2, C1=0.5, C2=0.5, lbd1=c.lbd, lbd2=c.lbd, iterations=U, eps=TINY, verbose=False,
                     strict_reference=False, mode="sparse", world=LocalWorld(2, leg2_stages=stages))
    same(s1.values, want["S1"], "S1 on two ranks")
    same(s2.values, want["S2"], "S2 on two ranks")
    assert est.converged_at == want["k"]


def _thread_ranks(world, fn):
    from simrank_amd.engine import ThreadRanks
    tr = ThreadRanks(world)
    try:
        return tr.run(fn, timeout=120.0)
    finally:
        tr.close()


def test_thread_ranks_with_an_asymmetric_prior():
    """Four CONCURRENT ranks (simrank_comm_thread_group: the code path of an RCCL rank) on the asymmetric directed loop."""
    from simrank_amd.engine import ShardPlans
    c = X.prior_case(("regular", 1031, 4), False, 0.5)
    csr, U = directed_csr(c), c.updates
    S, k = c.oracle(U, TINY)

    def rank(r, rops, comm):
        sp = ShardPlans(rops, csr, world=4, comm=comm, coef=0.5, evidence=True, apriori=c.A, lbd=c.lbd, leg2_form=0, stages=2)
        try:
            return sp.run(U, TINY), sp.result(root=0, i_am_root=(r == 0))
        finally:
            sp.free()
    outs = _thread_ranks(4, rank)
    assert all(o[0] == (U if k is None else k, k) for o in outs)
    same(outs[0][1], S, "thread ranks")


def test_thread_ranks_on_the_two_matrix_loop_with_an_asymmetric_prior():
    from simrank_amd.engine import ShardBiPlans
    c = X.bi_prior_case(*X.BI_PRIOR[3], False, True)
    U = c.updates
    _, _, _, _, g12, g21 = ingest.bipartite(c.df, False, "user", "item", "weight")
    want = c.oracle(U, TINY)

    def rank(r, rops, comm):
        bp = ShardBiPlans(rops, g12, g12.rowscale, g21.rowscale, world=3, comm=comm, c1=0.5, c2=0.5, evidence=True,
                          apriori1=c.A1, apriori2=c.A2, lbd1=c.lbd, lbd2=c.lbd, strict_reference=False, leg2_form=0, stages=1)
        try:
            return bp.run(U, TINY), bp.result(1, root=0, i_am_root=(r == 0)), bp.result(2, root=0, i_am_root=(r == 0))
        finally:
            bp.free()
    outs = _thread_ranks(3, rank)
    assert all(o[0] == (U, want["k"]) for o in outs)
    same(outs[0][1], want["S1"], "S1")
    same(outs[0][2], want["S2"], "S2")


# ---- 7: the other precisions ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,symmetric,lbd", cases(X.PRIOR_F64, lbds=(0.5,)))
def test_f64_storage_is_the_oracle(graph, symmetric, lbd):
    """storage_precision="f64" with a float64 prior: 53 bits.  The asymmetric prior takes f64.hip's full form
    (leg_b_kernel<false> and transpose_epilogue_kernel): its only exact test.  Then its count, on a tie."""
    c = X.prior_case(graph, symmetric, lbd, mantissa=53)
    U = c.updates
    assert U > X.prior_case(graph, symmetric, lbd).updates or U == 10
    S, k = c.oracle(U, TINY)
    est, got = fit(c, U, TINY, storage_precision="f64")
    same_frame(got, S, c.labels, "f64")
    assert est.converged_at == k
    U, eps, step = X.tie_eps(c.iterates(), fmt=np.float64)
    S, k = c.oracle(U, eps)
    est, got = fit(c, U, eps, storage_precision="f64")
    assert est.converged_at == k == U - 1
    same_frame(got, S, c.labels, "f64, eps on the tie")
    S, k = c.oracle(U, eps - step)
    est, got = fit(c, U, eps - step, storage_precision="f64")
    assert est.converged_at is None and k is None
    same_frame(got, S, c.labels, "f64, eps one step below the tie")


@pytest.mark.parametrize("graph", X.PRIOR_FP16, ids=lambda g: f"{g[1]}-{g[2]}")
def test_fp16_held_matrices_with_a_symmetric_prior(graph):
    """half.hip holds the prior x 2^14 in fp16: a 1-bit prior, 11 bits, two exact updates (pinned on the CPU; one only on
    (1031, 4) and on the bipartite pairs, which are left out for that)."""
    c = X.prior_case(graph, True, 0.5, bits=1, mantissa=11)
    U = c.updates
    assert U >= 2
    S, k = c.oracle(U, TINY)
    est, got = fit(c, U, TINY, storage_precision="fp16")
    same_frame(got, S, c.labels, "fp16-held")
    assert est.converged_at == k


# ---- 9: hand-backs of an exact asymmetric S ---------------------------------------------------------------------------
def _host_topk(S, labels, k):
    """The fit(top_k=k) frame from a dense matrix in the project's total order: similarity descending, then the caller's
    column order; the node itself left out."""
    v = S.copy()
    np.fill_diagonal(v, -np.inf)
    order = np.argsort(-v, axis=1, kind="stable")[:, :k]
    rows = np.repeat(np.arange(len(labels)), k)
    lab = pd.Index(labels)
    return pd.DataFrame({"node": lab.take(rows), "rank": np.tile(np.arange(1, k + 1), len(labels)),
                         "neighbor": lab.take(order.ravel()), "similarity": S[rows, order.ravel()]})


def _dense_pairs(S, labels, t):
    mask = S >= t
    np.fill_diagonal(mask, False)
    r, c = np.nonzero(mask)
    lab = pd.Index(labels)
    return pd.DataFrame({"node": lab.take(r), "neighbor": lab.take(c), "similarity": S[r, c]})


def _same_long(got, want):
    assert len(got) == len(want) > 0
    for col in want.columns:
        assert np.array_equal(got[col].to_numpy(), want[col].to_numpy()), col
    assert got["similarity"].dtype == np.float64


@pytest.mark.parametrize("graph", [("regular", 1031, 4), X.MIXED_GRAPH], ids=["regular", "mixed"])
@pytest.mark.parametrize("world", [None, 2])
def test_handbacks_of_an_asymmetric_matrix(graph, world):
    """An exact asymmetric S shows an S[a, b] / S[b, a] swap anywhere between the device and the caller, without a
    tolerance: fit(top_k=), fit(min_similarity=) with t a value that occurs, and the kept model's rows, similarity(a, b) AND
    similarity(b, a), most_similar — before and after compact().  On the mixed graph every one of them goes through a
    solver order that is a real permutation (asserted on the kept model's plan) and its inverse."""
    c = X.prior_case(graph, False, 0.5)
    U = c.updates
    S, k = c.oracle(U, TINY)
    assert int((S != S.T).sum()) > c.n
    kw = dict(mode="sparse", world=LocalWorld(world)) if world else {}
    est, got = fit(c, U, TINY, top_k=10, **kw)
    _same_long(got, _host_topk(S, c.labels, 10))
    off = S[~np.eye(c.n, dtype=bool)]
    t = float(np.unique(off)[-40])                                       # a value that occurs, near the top
    est, got = fit(c, U, TINY, min_similarity=t, **kw)
    _same_long(got, _dense_pairs(S, c.labels, t))
    est, model = fit(c, U, TINY, keep=True, **kw)
    assert model is est
    if world is None:
        solver = est._model[0]
        assert is_identity(solver_order(solver.ops[0], solver.plan.get)) == (graph != X.MIXED_GRAPH)
    rng = np.random.default_rng(9)
    try:
        for packed in (False, True):
            if packed:
                est.compact()
            nodes = [0, 31, 32, 1030, 517] + rng.choice(c.n, size=20, replace=False).tolist()
            rows = est.rows(nodes)
            assert list(rows.index) == nodes and list(rows.columns) == c.labels
            same(rows.values, S[nodes], "rows")
            a = rng.integers(0, c.n, size=400).tolist() + [0, 1030]
            b = rng.integers(0, c.n, size=400).tolist() + [1030, 0]
            assert int((S[a, b] != S[b, a]).sum()) > 100
            same(est.similarity(a, b), S[a, b], "similarity(a, b)")
            same(est.similarity(b, a), S[b, a], "similarity(b, a)")
            want = _host_topk(S, c.labels, 10)
            pick = np.concatenate([np.arange(10 * v, 10 * v + 10) for v in nodes])
            _same_long(est.most_similar(nodes, 10), want.iloc[pick].reset_index(drop=True))
    finally:
        est.release()
