"""The exactly summable operands of tests/exact.py, without a GPU: the builder's own assertions on every shape the GPU
tests use, the emulated bf16 split (a non-zero lo term in every column; one dropped lo term changes the bits of the
product), the epilogue reference, the planted ties, and the table of exact updates on regular graphs."""
import numpy as np
import pytest

from oracle import simrank_oracle as O
from tests import exact as X


_CORNER = X.LEG1_FUSED + [s for s, _, _ in X.LEG1_SHARD]


# (the unit-cut shape has rows of thousands of entries: no fp16 budget, and no fp16 test uses it)
@pytest.mark.parametrize("shape,mantissa,headroom", [(s, m, h) for s in _CORNER for m, h in ((24, 0), (24, 5), (11, 0))]
                         + [(X.LEG1_UNITS, 24, 0)])
def test_builder_holds_its_condition_on_every_corner_shape(shape, mantissa, headroom):
    M, K, L = shape
    if shape == X.LEG1_UNITS:
        csr = X.corner_case(M, K, 3, hubs=5500, p_hub=0.6)
    else:
        csr = X.corner_case(M, K, M + L, hubs=min(K, 150))
    op = X.summable_operand(csr, L, mantissa=mantissa, headroom=headroom, seed=L)
    bits = mantissa - headroom
    assert 0 < op.used < 1
    assert (op.K > 0).any() and (op.K < 0).any()                       # both signs
    tot = X.pattern(csr) @ np.abs(op.K)
    assert int(tot.max()) < 2 ** bits                                   # the condition, once more, in integers
    wide = np.abs(op.K).max(axis=0)
    assert np.all(wide >= 2 ** (bits - 3)) and np.all(wide < 2 ** (bits - 2)) and np.all(wide & 1)
    fmt = np.float32 if mantissa == 24 else np.float64
    assert np.array_equal(op.X.astype(fmt).astype(np.float64), op.X)
    assert op.exp.min() >= -20 and op.exp.max() <= 20
    # the wide rows walk through every 16-row step's residues (every fragment slot carries some)
    if L >= 32 and K >= 32:
        assert len(set((np.abs(op.K).argmax(axis=0) % 16).tolist())) == 16


def test_guide_value_of_the_issue():
    """corner_csr(520, 400): the longest row has 69 entries; 16-bit entries and one 22-bit entry per column."""
    csr = X.corner_case(520, 400, 520 + 333, hubs=150)
    assert X.longest_row(csr) == 69
    op = X.summable_operand(csr, 333, seed=333)
    rest = np.sort(np.abs(op.K), axis=0)[:-1]
    assert rest.max() < 2 ** 16 and np.abs(op.K).max() >= 2 ** 21
    assert 0.2 < op.used < 0.6


@pytest.mark.parametrize("case", ["gather", "star", "wide_ids"])
def test_builder_on_the_other_patterns(case):
    if case == "gather":
        for M, K, L in X.LEG1_GATHER:
            X.summable_operand(X.gather_case(M, K, M + L), L, seed=L)
    elif case == "star":
        csr = X.star_case()
        assert X.longest_row(csr) == 1500
        X.summable_operand(csr, 257, seed=1)
    else:
        X.summable_operand(X.wide_ids_case(), 64, seed=1)


def test_builder_refuses_an_operand_that_is_not_summable():
    csr = X.corner_case(129, 77, 1, hubs=77)
    op = X.summable_operand(csr, 33, seed=0)
    K = op.K.copy()
    K[:, 0] = 2 ** 22                                                    # a row of two such entries passes 2^23, three 2^24
    with pytest.raises(AssertionError, match="not exactly summable"):
        X.check_summable(csr, K, 24)
    with pytest.raises(AssertionError, match="powers of two"):
        X.summable_operand(X.CSR(csr.n_rows, csr.n_cols, csr.rowptr, csr.col, csr.rowscale * 0.3), 4)


@pytest.mark.parametrize("shape", X.LEG1_FUSED[:4])
def test_split_has_a_lo_term_in_every_column_and_dropping_one_shows(shape):
    M, K, L = shape
    csr = X.corner_case(M, K, M + L, hubs=min(K, 150))
    op = X.summable_operand(csr, L, seed=L)
    x = op.X.astype(np.float32)
    hi, mid, lo = X.split3f(x)
    assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), op.X)
    assert (lo != 0).any(axis=0).all() and (mid != 0).any(axis=0).all()
    want = X.product64(csr, op.X).astype(np.float32)
    # drop lo for ONE operand row that a pattern row references: the bits of the product change
    j = int(np.flatnonzero((lo != 0).any(axis=1) & (np.bincount(csr.col, minlength=K) > 0)
                           & (np.asarray(X.pattern(csr).T @ (csr.rowscale > 0)) > 0))[0])
    broken = op.X.copy()
    broken[j] -= lo[j]
    got = X.product64(csr, broken).astype(np.float32)
    assert not np.array_equal(got, want)
    # ... and so does dropping only the low half of one lo term (what a tolerance of 2e-6 cannot see)
    c = int(np.flatnonzero(lo[j] != 0)[0])
    half = op.X.copy()
    half[j, c] -= np.ldexp(1.0, int(op.exp[c]))                          # the lowest bit of the wide entry
    assert not np.array_equal(X.product64(csr, half).astype(np.float32), want)


@pytest.mark.parametrize("n", X.LEG2_N)
@pytest.mark.parametrize("variant", ["plain", "evidence", "all"])
def test_symmetric_case_is_summable_symmetric_and_exact_through_the_epilogue(n, variant):
    csr, sym, counts, prior, lbd, want = X.leg2_case(n, variant)
    assert np.array_equal(sym.S, sym.S.T) and 0 < sym.used1 < 1 and 0 < sym.used2 < 1
    assert (sym.KS > 0).any() and (sym.KS < 0).any()
    assert np.array_equal(sym.Tt, X.product64(csr, sym.S).T)             # leg 2's operand IS leg 1's exact result
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert np.array_equal(np.diag(want), np.ones(n))
    if variant == "plain":
        hi, mid, lo = X.split3f(sym.Tt.astype(np.float32))
        assert (lo != 0).any() and (mid != 0).any()


def test_fp16_symmetric_case():
    for n in (64, 129, 520):
        csr, sym, counts, prior, lbd, want = X.leg2_case(n, "evidence", mantissa=11)
        assert np.array_equal(sym.Tt.astype(np.float16).astype(np.float64), sym.Tt)
        assert np.array_equal(sym.S.astype(np.float16).astype(np.float64), sym.S)


def test_epilogue_reference_refuses_what_would_round():
    prod = np.array([[2.0 ** 24 - 1, 3.0], [5.0, 7.0]])
    X.exact_epilogue(prod, 0.5)
    with pytest.raises(AssertionError, match="rounds in float32"):
        X.exact_epilogue(prod, 0.5, counts=np.array([[3, 0], [1, 255]], dtype=np.uint8))
    got = X.exact_epilogue(np.array([[8.0, 16.0], [24.0, 32.0]]), 0.5, np.array([[3, 0], [1, 255]], dtype=np.uint8),
                           np.array([[4.0, 4.0], [-8.0, 4.0]]), 0.25)
    assert np.array_equal(got, [[1.0, 1.0], [0.75 * 6.0 - 2.0, 1.0]])
    got = X.exact_epilogue(np.array([[8.0, 16.0], [24.0, 32.0]]), 0.5, np.array([[3, 0], [1, 255]], dtype=np.uint8),
                           diag_col0=1)
    assert np.array_equal(got, [[3.5, 0.0], [1.0, 16.0]])
    # the oracle's own expression
    W = np.array([[0.5, 0.5], [0.0, 1.0]])
    S = np.array([[1.0, 0.25], [0.25, 1.0]])
    E = np.array([[0.5, 0.75], [0.75, 0.5]])
    A = np.array([[4.0, 8.0], [8.0, 4.0]])
    ours = X.exact_epilogue(W @ S @ W.T, 0.5, np.array([[1, 2], [2, 1]], dtype=np.uint8), A, 0.25)
    assert np.array_equal(ours, O.update(W, S, 0.5, E, A, 0.25))


def test_planted_ties():
    rng = np.random.default_rng(0)
    want = (rng.integers(-2 ** 12, 2 ** 12, size=(70, 45)) * 2.0 ** -6).astype(np.float64)
    places = X.tie_places(70, 45)
    assert (69, 44) in places and (0, 0) in places and any(r < c for r, c in places) and any(r > c for r, c in places)
    p = X.plant_previous(want, 2.0 ** -3, places)
    assert set(p.kinds) == {"on", "above", "below"}
    d = np.abs(want - p.previous.astype(np.float64))
    assert p.count == p.kinds.count("above") == int((d > 2.0 ** -3).sum())
    assert int((d >= 2.0 ** -3).sum()) == p.kinds.count("above") + p.kinds.count("on")     # a >= would count the ties
    assert int((d > 0).sum()) == len(p.kinds)
    sq = want[:45, :45]
    sq = np.triu(sq) + np.triu(sq, 1).T
    ps = X.plant_previous(sq, 2.0 ** -3, X.tie_places(45, 45), symmetric=True)
    assert np.array_equal(ps.previous, ps.previous.T) and ps.count > ps.kinds.count("above") // 2


_GRAPHS = [(300, 2), (300, 4), (1031, 4), (2100, 8)]
_PLAIN = {(300, 2): (7, 21), (300, 4): (4, 20), (1031, 4): (4, 20), (2100, 8): (3, 21)}      # updates, bits of the grid
_PP = {(300, 2): 8, (300, 4): 3, (1031, 4): 3, (2100, 8): 2}                                  # updates ((300, 2): at least)


@pytest.mark.parametrize("n,d", _GRAPHS)
def test_exact_updates_on_regular_graphs(n, d):
    """The table of the issue: how many updates stay exact in float32 on regular_graph(n, d) with C = 0.5; the iterates the
    count allows are unchanged by a cast to float32, and the eps of the tie tests is a difference that occurs in the run."""
    df = X.regular_graph(n, d, seed=n + d)
    nodes, G = O.directed_graph(df)
    assert np.array_equal(G.sum(axis=1), np.ones(n)) and np.array_equal(np.unique(G), [0.0, 1.0 / d])
    assert np.array_equal(O.weight(G), G)                                # spread exactly 1
    E = O.evidence(G)
    plain = X.exact_updates(G, 0.5)
    assert (plain.updates, plain.grid_bits) == _PLAIN[(n, d)] and plain.bits < 24
    pp = X.exact_updates(G, 0.5, E, limit=8)
    assert pp.updates == _PP[(n, d)] and pp.bits < 24
    print(f"regular_graph({n}, {d}): plain {plain}, ++ {pp}")
    for Ev, r in ((None, plain), (E, pp)):
        its = X.oracle_iterates(G, 0.5, Ev, r.updates)
        for S in its:
            assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
        U, eps, step = X.tie_eps(its)
        assert 2 <= U <= r.updates
        assert np.any(np.abs(its[U - 1] - its[U - 2]) == eps)
        S, k = O.iterate_directed(G, 0.5, U, eps, E=Ev)
        assert k == U - 1 and np.array_equal(S, its[U - 1])
        S, k = O.iterate_directed(G, 0.5, U, eps - step, E=Ev)
        assert k is None and np.array_equal(S, its[U])


def test_exact_updates_in_the_other_formats():
    df = X.regular_graph(300, 2, seed=302)
    _, G = O.directed_graph(df)
    assert X.exact_updates(G, 0.5, mantissa=11).updates == 3            # fp16-held matrices and the fp16 wire
    assert X.exact_updates(G, 0.5, mantissa=53).updates == 17           # float64: 3 bits an update
    assert X.exact_updates(G, 0.5, O.evidence(G), mantissa=11).updates >= 2


def test_biregular_graph():
    df = X.biregular_graph(256, 128, 2, seed=1)
    assert set(df.groupby("user").size()) == {2} and set(df.groupby("item").size()) == {4}
    *_, G12, G21 = O.bipartite_graph(df)
    assert np.array_equal(np.unique(G12), [0, 0.5]) and np.array_equal(np.unique(G21), [0, 0.25])


# ---- the graphs built for leg 2's short path (tests/test_gpu_exact_short.py) ----------------------------------------
def test_short_rule_over_the_graph_list():
    """The rule of tests/leg2_rule.py on every graph: some groups short at 8, strictly more at 16; every graph with more than
    one group keeps a group that is NOT short at 16 (the general path runs in the same launch), except the equal-length
    ones; n = 64 is one short group, n = 63 has no image; the lengths are the ones the docstring of short_lengths names."""
    from tests import leg2_rule as R
    L = X.short_lengths()
    assert set(L) == set(X.SHORT_GRAPHS)
    rule = {name: {w: R.short_groups(L[name][0], w) for w in X.SHORT_WIDTHS} for name in L}
    print(rule)
    assert all(r[0] == 0 for r in rule.values())
    assert 0 < sum(r[8] for r in rule.values()) < sum(r[16] for r in rule.values())
    for name, (lengths, _) in L.items():
        groups = R.tile_groups(lengths)
        assert len(lengths) <= 700 and rule[name][8] <= rule[name][16] <= groups
        if name not in X.SHORT_EQUAL and groups > 1:
            assert rule[name][16] < groups, name
    assert [len(L[k][0]) for k in ("boundary", "ragged21", "ragged1")] == [660, 661, 641]
    for name in ("boundary", "ragged21", "ragged1"):
        assert rule[name] == {0: 0, 8: 3, 16: 5} and R.tile_groups(L[name][0]) == 6
        assert R.group_flags(L[name][0], 8) == [True, False, False, False, True, True]
        assert R.group_flags(L[name][0], 16) == [True, True, True, False, True, True]
        assert {0, 8, 9, 16, 17} <= set(L[name][0]) and not any(L[name][0][64:96])      # ... and a wholly empty tile
    assert rule["n64"] == {0: 0, 8: 1, 16: 1} and R.tile_groups(L["n64"][0]) == 1
    assert rule["n63"] == {0: 0, 8: 0, 16: 0}
    assert R.group_flags(L["n129"][0], 8) == R.group_flags(L["n129"][0], 16) == [False, True]
    heavy = L["heavy_row"][0]
    tiles = R.tiles_of(np.concatenate([[0], np.cumsum(heavy)]), len(heavy))
    assert max(heavy) == X.HEAVY_ROW == 400 and len(tiles) - 1 > (len(heavy) + 31) // 32       # the block is cut
    assert any(t % 32 for t in tiles[:-1]) and 0 < rule["heavy_row"][8] == rule["heavy_row"][16] < R.tile_groups(heavy)
    assert rule["equal8"] == {0: 0, 8: 2, 16: 2} and rule["equal16"] == {0: 0, 8: 0, 16: 2}
    assert set(L["equal8"][0]) == {8} and set(L["equal16"][0]) == {16}


@pytest.mark.parametrize("name", X.SHORT_GRAPHS)
@pytest.mark.parametrize("variant", ["plain", "evidence", "all"])
def test_short_cases_are_summable_and_every_row_holds_a_planted_tie(name, variant):
    csr, sym, counts, prior, lbd, want, lengths = X.short_case(name, variant)
    n = csr.n_rows
    assert np.array_equal(np.diff(csr.rowptr), lengths) and X.is_pow2_or_zero(csr.rowscale)
    bits = 24 - X.HEADROOM[variant]
    assert 0 < sym.used1 < 1 and 0 < sym.used2 < 1
    P = X.pattern(csr)
    assert int(np.asarray(np.abs(sym.KT) @ P.T).max()) < 2 ** bits          # leg 2's condition, once more, in integers
    assert np.array_equal(sym.Tt, X.product64(csr, sym.S).T) and np.array_equal(want, want.T)
    assert np.array_equal(np.diag(want), np.ones(n))
    places = X.tie_places_every_row(n)
    assert len(places) == len(set(places)) and 4 * n <= len(places) + 4 * 32 and len(places) <= 5 * n
    for a in (0, n // 2, n - 1):
        b0 = a // 32 * 32
        assert {(a, a), (a, b0), (a, min(n - 1, b0 + 31)), (a, n - 1), (a, (7 * a + 3) % n)} <= set(places)
    want32, p, q = X.short_planted(name, variant)
    assert set(p.kinds) == {"on", "above", "below"} and set(q.kinds) == {"on", "below"}
    d = np.abs(want32.astype(np.float64) - p.previous.astype(np.float64))
    assert np.array_equal(p.previous, p.previous.T) and (d > 0).any(axis=1).all()       # every row holds a planted tie
    assert p.count == int((d > X.SHORT_EPS).sum()) > 0
    assert int((d >= X.SHORT_EPS).sum()) > p.count                                     # a >= would count the ties
    # some planted differences count and some do not
    moved = (d > X.SHORT_EPS).any(axis=1)
    quiet = ((d > 0) & (d <= X.SHORT_EPS)).any(axis=1)
    assert moved.any() and quiet.any()
    dq = np.abs(want32.astype(np.float64) - q.previous.astype(np.float64))
    assert q.count == 0 and not (dq > X.SHORT_EPS).any() and (dq > 0).any(axis=1).all()


def test_exact_updates_on_the_graph_with_rows_of_16():
    """regular_graph(520, 16), the whole loop that is general at leg2_short = 8 and short at 16 (tests/test_gpu_exact_fits.py):
    2 exact updates plain (enough for a tie), 1 for SimRank++ (too few: that class is left out there)."""
    df = X.regular_graph(520, 16, seed=520 + 16)
    _, G = O.directed_graph(df)
    assert np.array_equal(np.unique(G), [0.0, 1.0 / 16]) and np.array_equal((G != 0).sum(axis=1), np.full(520, 16))
    plain = X.exact_updates(G, 0.5)
    assert (plain.updates, plain.grid_bits) == (2, 18) and plain.bits < 24
    assert X.exact_updates(G, 0.5, O.evidence(G), limit=8).updates == 1
    its = X.oracle_iterates(G, 0.5, None, 2)
    U, eps, step = X.tie_eps(its)
    assert U == 2 and np.any(np.abs(its[1] - its[0]) == eps)
    S, k = O.iterate_directed(G, 0.5, U, eps)
    assert k == 1 and np.array_equal(S, its[1])
    S, k = O.iterate_directed(G, 0.5, U, eps - step)
    assert k is None and np.array_equal(S, its[2])


# ---- whole loops with a prior (tests/test_gpu_exact_priors.py) ------------------------------------------------------
# exact updates of (1 - lbd) * E * 0.5 * W S W^T + lbd * A with a 2-bit prior: graph -> {lbd: updates}; the same for a
# symmetric and an asymmetric prior.  (Loop limit 8; 4 from 2000 nodes on.)
_PRIOR_U = {("regular", 300, 2): {0.5: 8, 0.25: 4}, ("regular", 1031, 4): {0.5: 3, 0.25: 2}, ("regular", 2100, 2): {0.5: 4, 0.25: 4},
            ("regular", 2100, 4): {0.5: 3, 0.25: 2}, ("regular", 512, 4): {0.5: 3, 0.25: 2}}


def _prior_pins(c, fmt=np.float32):
    """What the GPU tests lean on, for one PriorCase: iterates unchanged by a cast to the format, asymmetric at more than n
    places where the prior is (a transposed answer cannot pass), a tie eps with a representable step, and the loop index
    of the oracle's loop at that eps and one step below."""
    U = c.updates
    assert U >= 2
    its = c.iterates()
    for u, S in enumerate(its):
        assert np.array_equal(S.astype(fmt).astype(np.float64), S)
        assert np.array_equal(np.diag(S), np.ones(c.n))
        if u >= 1 and not c.symmetric:
            assert int((S != S.T).sum()) > c.n, u
        elif u >= 1:
            assert np.array_equal(S, S.T)
    Ut, eps, step = X.tie_eps(its, fmt=fmt)
    assert 2 <= Ut <= U and np.any(np.abs(its[Ut - 1] - its[Ut - 2]) == eps)
    S, k = c.oracle(Ut, eps)
    assert k == Ut - 1 and S is its[Ut - 1]
    S, k = c.oracle(Ut, eps - step)
    assert k is None and S is its[Ut]
    return Ut, eps, step


@pytest.mark.parametrize("graph", X.PRIOR_GRAPHS + X.PRIOR_RANK_GRAPHS[:1])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("lbd", X.PRIOR_LBD)
def test_exact_updates_with_a_prior(graph, symmetric, lbd):
    """The table of DESIGN.md §7: exact_updates with the blend booked (and, for an asymmetric prior, both legs on the iterate
    and its transpose) asserts oracle.update's bits at every counted update itself; here the counts, and the pins."""
    c = X.prior_case(graph, symmetric, lbd)
    assert c.updates == _PRIOR_U[graph][lbd] and c.exact().bits <= 24
    assert np.array_equal(c.A, c.A.T) == symmetric and len(set(np.diag(c.A))) == c.n and not np.any(np.diag(c.A) == 1)
    Ut, eps, step = _prior_pins(c)
    if c.n < 2000:                                      # (the oracle's own loop, once more, where it costs little)
        S, k = O.iterate_directed(c.G, 0.5, Ut, eps, E=c.E, apriori=c.A, lbd=lbd)
        assert k == Ut - 1 and np.array_equal(S, c.iterates()[Ut - 1])
        S, k = O.iterate_directed(c.G, 0.5, c.updates, 1e-30, E=c.E, apriori=c.A, lbd=lbd)
        want = c.oracle(c.updates, 1e-30)               # (k is not None where the loop reaches its fixed point exactly)
        assert k == want[1] and np.array_equal(S, want[0])


def test_exact_updates_refuse_what_the_blend_rounds():
    """The bookkeeping sees the blend: a prior one bit below the grid the budget allows costs updates, one 20 bits below
    leaves none; and it refuses an update that is not the oracle's (a transposed prior)."""
    c = X.prior_case(("regular", 300, 2), False, 0.5)
    fine = X.exact_updates(c.G, 0.5, c.E, limit=8, prior=c.A + 2.0 ** -22 * (1 - np.eye(c.n)), lbd=0.5).updates
    assert 1 <= fine < c.updates
    assert X.exact_updates(c.G, 0.5, c.E, limit=8, prior=c.A + 2.0 ** -30 * (1 - np.eye(c.n)), lbd=0.5).updates == 0
    r = X._one_update(c.G, c.iterates()[1], 0.5, c.E, 24, c.A, 0.5)
    assert np.array_equal(r[0], c.iterates()[2])
    with pytest.raises(AssertionError, match="not the oracle's"):
        X._is_oracle_update(c.G, c.iterates()[1], 0.5, c.E, c.A.T, 0.5, r[0])


@pytest.mark.parametrize("degrees,updates", [((1, 2, 4, 8), 2), ((2, 4), 3)])
def test_hub_graph_with_a_prior_and_no_evidence(degrees, updates):
    """pow2_degree_graph(1031, degrees, 48, 0.5): in-degrees from the set, no self loop, no repeated edge, row scales powers of
    two, half of all references on 48 hub columns that 40 rows and more (32 and more for degrees 2 and 4) reference; exact
    updates of the plan-level loop with a prior and WITHOUT the evidence factor."""
    graph = ("hubs", 1031, degrees)
    df = X.loop_graph(graph)
    assert set(df.groupby("to").size()) == set(degrees) and not (df["from"] == df["to"]).any()
    refs = np.bincount(df["from"], minlength=1031)
    assert refs[:48].sum() == len(df) // 2 and refs[:48].min() >= (40 if 8 in degrees else 32) and refs[48:].max() < 20
    for symmetric in (True, False):
        c = X.prior_case(graph, symmetric, 0.5, evidence=False)
        assert X.is_pow2_or_zero(c.G.max(axis=1)) and c.E is None
        assert c.updates == updates
        _prior_pins(c)


@pytest.mark.parametrize("n1,n2,d1,lbd,matched", X.BI_PRIOR)
@pytest.mark.parametrize("sym1,sym2", X.BI_PRIOR_KINDS)
def test_exact_updates_of_the_two_matrix_loop_with_priors(n1, n2, d1, lbd, matched, sym1, sym2):
    c = X.bi_prior_case(n1, n2, d1, lbd, matched, sym1, sym2)
    assert c.updates >= 2
    want = c.oracle(c.updates, 1e-30)
    last = c.pairs[-1] if want["k"] is None else c.pairs[want["k"] - 1]      # (d1 = 1 reaches its fixed point exactly)
    assert np.array_equal(want["S1"], last[0]) and np.array_equal(want["S2"], last[1])
    for s1, s2 in c.pairs:
        for S in (s1, s2):
            assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
        a1, a2 = int((s1 != s1.T).sum()), int((s2 != s2.T).sum())
        if sym1 and sym2:
            assert a1 == a2 == 0
        else:
            assert (a2 if sym1 else a1) > (n2 if sym1 else n1)           # the side of the asymmetric prior
    if matched and not (sym1 and sym2):
        s1, s2 = c.pairs[-1]                                              # ... and there it reaches the other side too
        assert int((s1 != s1.T).sum()) > n1 and int((s2 != s2.T).sum()) > n2


def test_exact_updates_with_a_prior_in_the_other_formats():
    """float64: the theoretical grid; fp16-held matrices: 11 bits and a 1-bit prior, two updates on the graphs with d = 2,
    one only with d = 4 and on the bipartite pairs, which are left out on the GPU for that."""
    for graph in X.PRIOR_F64:
        for symmetric in (True, False):
            c = X.prior_case(graph, symmetric, 0.5, mantissa=53)
            assert c.updates > X.prior_case(graph, symmetric, 0.5).updates or c.updates == 10
            assert X.tie_eps(c.iterates(), fmt=np.float64)[0] >= 2
    for graph in X.PRIOR_FP16:
        c = X.prior_case(graph, True, 0.5, bits=1, mantissa=11)
        assert c.updates == 2 and float(np.abs(c.A).max()) < 3.99
        for S in c.iterates():
            assert np.array_equal((S * 16384.0).astype(np.float16).astype(np.float64), S * 16384.0)
        assert np.array_equal((c.A * 16384.0).astype(np.float16).astype(np.float64), c.A * 16384.0)
    assert X.prior_case(("regular", 512, 4), True, 0.5, bits=1, mantissa=11).updates == 1
    assert X.BiPriorCase(256, 256, 2, True, True, 0.5, bits=1, mantissa=11).updates == 1


def test_lowbit_exp_reads_the_bits_as_frexp_and_log2_did():
    """lowbit_exp takes mantissa and exponent from the float64 word; the earlier form went through frexp and log2.  The same
    answer on integers times a power of two, on 1 - 2^-k, on a scalar, on zeros and on values 2^-40 apart."""
    def earlier(a):
        a = np.asarray(a, dtype=np.float64)
        a = a[a != 0]
        if a.size == 0:
            return None
        m, e = np.frexp(np.abs(a))
        mant = (m * 2.0 ** 53).astype(np.int64)
        low = mant & -mant
        return int((e.astype(np.int64) - 53 + np.log2(low.astype(np.float64)).astype(np.int64)).min())
    rng = np.random.default_rng(0)
    for a in (rng.integers(-2 ** 20, 2 ** 20, (200, 200)) * 2.0 ** -17, np.array([0.75, -3.0, 0.0, 2.0 ** -40]), np.array([[1.0]]),
              rng.random((100, 100)), np.float64(0.5), 1 - 0.5 ** rng.integers(0, 60, (50, 50)).astype(float), np.zeros(4),
              rng.integers(1, 2 ** 52, 1000).astype(np.float64) * 2.0 ** -300):
        assert X.lowbit_exp(a) == earlier(a)


# ---- leg 2 on rectangular patterns, and the two-matrix loops with a real reorder --------------------------------------
# sha256 (first 16 hex digits) over S, Tt, the integer S, the integer (pattern . S) and both budget shares of
# summable_symmetric(corner_case(n, n, n, hubs=min(n, 150)), headroom=h, seed=n) as it was while it took square patterns only
_SQUARE_BITS = {(64, 0): "badda9f113f297e1", (64, 3): "4ad71d4c30b69f9f", (64, 5): "e16d09bf996bddfa",
                (129, 0): "e3db8f91f29c0b61", (129, 3): "ecd458c199a82b23", (129, 5): "ab1a17c5fe6f1952",
                (1031, 0): "b7de7dd4a2f23c6d", (1031, 3): "a6460a4adb3e118f", (1031, 5): "3385361dfc898c8d",
                (2100, 0): "c9876c1cfefc5107", (2100, 3): "90012c1ffe7b531b", (2100, 5): "f50369243373af08"}


@pytest.mark.parametrize("n", X.LEG2_N)
def test_square_patterns_summable_symmetric_unchanged_bit_for_bit(n):
    """The n x K generalisation returns, on a square pattern, every bit it returned before (what the 13 forms of the square
    leg-2 test, the short-path module and the fp16 tests are built on)."""
    import hashlib
    csr = X.corner_case(n, n, n, hubs=min(n, 150))
    for variant, h in X.HEADROOM.items():
        sym = X.summable_symmetric(csr, headroom=h, seed=n)
        d = hashlib.sha256()
        for a in (sym.S, sym.Tt, sym.KS, sym.KT):
            d.update(np.ascontiguousarray(a).tobytes())
        d.update(repr((sym.used1, sym.used2)).encode())
        assert d.hexdigest()[:16] == _SQUARE_BITS[(n, h)], (n, variant)
        assert X.leg2_case(n, variant)[1].S.shape == (n, n)


# short groups of corner_case(M, K, M + K, hubs=min(K, 150)) by tests/leg2_rule.py at width 16 (0 everywhere at width 8)
_RECT_SHORT16 = {(129, 77): 0, (520, 333): 2, (64, 1000): 0, (1031, 2100): 4, (2100, 700): 8, (660, 20): 5, (63, 200): 0}


@pytest.mark.parametrize("shape", X.LEG2_RECT + [X.LEG2_RECT_BELOW], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("variant", ["plain", "evidence", "all"])
def test_rectangular_case_is_summable_symmetric_and_exact_through_the_epilogue(shape, variant):
    """An n x K pattern: S is K x K, Tt = (W S)^T is K x n, W . Tt is n x n and EXACTLY symmetric; the integer condition of both
    legs holds at the headroom of every variant; the rule's short groups are the ones the GPU tests expect."""
    from tests.leg2_rule import short_groups
    M, K = shape
    csr, sym, counts, prior, lbd, want = X.rect_case(M, K, variant)
    assert (csr.n_rows, csr.n_cols) == (M, K) and sym.S.shape == (K, K) and sym.Tt.shape == (K, M) and want.shape == (M, M)
    assert np.array_equal(sym.S, sym.S.T) and 0 < sym.used1 < 1 and 0 < sym.used2 < 1
    assert np.array_equal(sym.Tt, X.product64(csr, sym.S).T)
    prod = X.product64(csr, sym.Tt)
    assert np.array_equal(prod, prod.T) and np.array_equal(want, want.T)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want) and np.array_equal(np.diag(want), np.ones(M))
    worst = int(np.asarray(np.abs(sym.KT) @ X.pattern(csr).T).max())         # leg 2's condition, once more, in integers
    assert worst < 2 ** (24 - X.HEADROOM[variant])
    lengths = np.diff(csr.rowptr).tolist()
    assert short_groups(lengths, 16) == _RECT_SHORT16[shape] and short_groups(lengths, 8) == 0
    if variant == "plain":
        hi, mid, lo = X.split3f(sym.Tt.astype(np.float32))
        assert (lo != 0).any() and (mid != 0).any()


def test_rectangular_fp16_and_short_cases():
    """The fp16 budget on the two rectangular shapes of the half.hip test; the short path's graphs with K = n + 37 and K = 20
    columns keep their row lengths (so the rule's answer) and their exact symmetry."""
    for M, K in ((520, 333), (129, 77)):
        for variant in ("plain", "evidence", "all"):
            csr, sym, counts, prior, lbd, want = X.rect_case(M, K, variant, mantissa=11, exponent=-6)
            assert np.array_equal(sym.Tt.astype(np.float16).astype(np.float64), sym.Tt) and np.array_equal(want, want.T)
    for name in ("boundary", "ragged21", "ragged1", "n64"):
        lengths = X.short_lengths()[name][0]
        for K in (len(lengths) + 37, 20):
            assert max(lengths) <= K
            csr, sym, counts, prior, lbd, want, got_lengths = X.short_case(name, "all", K)
            assert csr.n_cols == K and got_lengths == list(lengths) and int(csr.col.max()) < K
            assert sym.Tt.shape == (K, len(lengths)) and np.array_equal(want, want.T)
    sq = X.short_case("n64", "all")
    assert sq[0].n_cols == 64 and sq[1].S.shape == (64, 64)


def test_pow2_bidegree_graphs_have_two_real_reorders():
    """Both sides of every graph of BI_MIXED: the prescribed power-of-two degrees, every node present, no repeated pair, a
    stable length order that is a real permutation — and for n1 = n2 two orders that differ (the builder asserts all of it;
    here once more from the edge list).  The hub graph: 48 items referenced by 8 users each."""
    for name, (deg1, deg2, seed) in X.BI_MIXED.items():
        df = X.bi_graph(name)
        assert not df.duplicated(["user", "item"]).any() and len(df) == sum(deg1) == sum(deg2)
        d1, d2 = np.bincount(df["user"], minlength=len(deg1)), np.bincount(df["item"], minlength=len(deg2))
        assert sorted(d1.tolist()) == sorted(deg1) and sorted(d2.tolist()) == sorted(deg2) and d1.min() >= 1 and d2.min() >= 1
        o1, o2 = X.stable_length_order(d1), X.stable_length_order(d2)
        for o, d in ((o1, d1), (o2, d2)):
            assert np.array_equal(np.sort(o), np.arange(o.size)) and not np.array_equal(o, np.arange(o.size))
            assert np.all(np.diff(d[o]) >= 0) and np.argsort(o).tolist() != o.tolist()        # (so ord != inv as well)
        if len(deg1) == len(deg2):
            assert not np.array_equal(o1, o2)
    assert int((np.bincount(X.bi_graph("hub512")["item"]) == 8).sum()) == 48
    with pytest.raises(AssertionError):
        X.pow2_bidegree_graph([2] * 8, [2] * 8, 0)                           # equal degrees: the order is the identity


# exact updates of the two-matrix loops of tests/test_gpu_exact_bipartite.py (float32 unless said; priors: 2-bit loop_priors,
# lbd 0.5).  Left out on the GPU for having none or too few: priors WITH evidence on "hub512" have 1 like the plain prior, the
# issue's graph with hub items of degree 16 has 0 with evidence; "mixed512" with priors and evidence has 1 (run: one update).
_BI_U = {("mixed384", "plain"): 3, ("mixed384", "pp"): 2, ("mixed384", "strict"): 4, ("mixed384", "priors"): 2,
         ("mixed384", "priors no ev"): 2, ("mixed384", "plain f64"): 6, ("mixed384", "pp f64"): 6,
         ("mixed512", "plain"): 2, ("mixed512", "pp"): 2, ("mixed512", "priors"): 1, ("mixed512", "priors no ev"): 2,
         ("mixed512", "plain f64"): 6, ("mixed512", "pp f64"): 4,
         ("hub512", "plain"): 2, ("hub512", "pp"): 1, ("hub512", "priors"): 1, ("hub512", "priors no ev"): 1}
_BI_KW = {"plain": dict(), "pp": dict(pp=True), "strict": dict(pp=True, strict=True), "plain f64": dict(mantissa=53),
          "pp f64": dict(pp=True, mantissa=53)}


@pytest.mark.parametrize("name,kind", list(_BI_U), ids=lambda v: v.replace(" ", "_"))
def test_exact_updates_of_the_two_matrix_loop_with_a_real_reorder(name, kind):
    """exact_updates_bipartite on the oracle's G12, G21, E1, E2 (as tests/test_gpu_exact_fits.py's bipartite test): the counts
    the GPU module runs, and the minima it needs — 2 on the mixed graphs plain and SimRank++ (the second iteration is the
    first in which group 1 reads a non-trivial S2), 1 on the hub graph plain and with a prior without evidence."""
    if kind.startswith("priors"):
        loops = [X.bi_loop(name, pp=kind == "priors", kinds=k) for k in ((True, True), (False, True), (False, False))]
    else:
        loops = [X.bi_loop(name, **_BI_KW[kind])]
    for c in loops:
        assert c.updates == _BI_U[(name, kind)], (c.kinds, c.exact)
        fmt = np.float64 if c.mantissa == 53 else np.float32
        for s1, s2 in c.pairs:
            for S in (s1, s2):
                assert np.array_equal(S.astype(fmt).astype(np.float64), S) and np.array_equal(np.diag(S), np.ones(len(S)))
            if c.kinds is not None and not all(c.kinds):
                assert int((s1 != s1.T).sum()) + int((s2 != s2.T).sum()) > 0
        if c.kinds is None and c.mantissa == 24:
            ref = O.fit_bipartite_pp if c.pp else O.fit_bipartite
            kw = dict(strict_reference=c.strict) if c.pp else {}
            want = ref(c.df, C1=0.5, C2=0.5, iterations=c.updates, eps=1e-30, verbose=False, **kw)
            s1, s2, k = c.oracle(c.updates, 1e-30)
            assert k == want["k"] and np.array_equal(s1, want["S1"]) and np.array_equal(s2, want["S2"])
            if c.updates >= 2:
                Ut, eps, step = c.tie_eps()                  # (asserts where the oracle's loop stops, on the tie and below it)
                assert 2 <= Ut <= c.updates
    if name.startswith("mixed") and kind in ("plain", "pp"):
        assert _BI_U[(name, kind)] >= 2
    if name == "hub512" and kind in ("plain", "priors no ev"):
        assert _BI_U[(name, kind)] >= 1
