"""libsimrank_explain.so and ``explain`` on a real MI355X.

Kernel level, on synthetic blocks (tests/blocks.py; padding holds a finite sentinel above every value, which a kernel that
reads padding would let win a selection and change every sum): ``gather`` bit for bit against ``explain_ref.block_gather``
in all four layouts with the strides and bases of ``blocks.variants``, many pairs in one call with list lengths at both
sides of a lane group, a wave and a workgroup, some empty, rows and columns listed twice, positions outside the block on
either side, a launch hint that is too small, guard words after every output and a second run with the same bits;
``reduce`` bit for bit on dyadic blocks (whose sums are exact in any order, which is asserted) and within the derived bound
on wide ones, the count exact, a planted NaN poisoning exactly its row, its column and ``raw``; ``select`` bit for bit
against ``explain_ref.best`` for k on both sides of a wave, with plateaus of equal values, both zeros, NaN and negatives.

Model level: ``explain`` equals ``explain_ref`` over the model's own ``rows`` for every storage, a ``LocalWorld(3)``,
compact, loaded and pruned models, both bipartite groups, a ++ and a weighted fit; and ``propagated`` of a float64 fit of t
updates is the shipped loop's value after t + 1."""
import contextlib
import io
import math

import numpy as np
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _explain, synth
from simrank_amd._driver import join
from tests import blocks as B
from tests import exact as X
from tests import explain_ref as ER
from tests.graphs import bipartite_random
from tests.test_gpu_cluster import VARIANTS, as_groups, dev, device, make_model  # noqa: F401 (fixtures)
from tests.test_gpu_companion_blocks import same_bits
from tests.test_gpu_groups import planted

pytestmark = pytest.mark.gpu

GUARD_F64 = 1e300
GUARD_I32 = 0x5A5A5A5A
GUARD_I64 = 0x5A5A5A5A5A5A5A5A
LENS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025)
KS = (1, 2, 63, 64, 65, 1024)


# ---- the calls -------------------------------------------------------------------------------------------------------------
class Case:
    """The lists of the pairs of one call and what follows from them."""

    def __init__(self, lists_a, lists_b):
        self.lists_a = [np.asarray(l, dtype=np.int32) for l in lists_a]
        self.lists_b = [np.asarray(l, dtype=np.int32) for l in lists_b]
        self.ptr_a, self.pos_a = join(self.lists_a)
        self.ptr_b, self.pos_b = join(self.lists_b)
        self.na, self.nb = np.diff(self.ptr_a), np.diff(self.ptr_b)
        self.terms = self.na * self.nb
        self.band_ptr = np.zeros(len(lists_a) + 1, dtype=np.int64)
        np.cumsum(self.terms, out=self.band_ptr[1:])
        self.n = len(lists_a)

    def pieces(self, band):
        return [band[self.band_ptr[p]:self.band_ptr[p + 1]].reshape(self.na[p], self.nb[p]) for p in range(self.n)]


def some(ids):
    return ids if ids.size else np.zeros(1, dtype=np.int32)


class Run:
    """The device arrays of one case; ``gather`` fills the band from a block, ``load`` from a host array."""

    def __init__(self, dev, case):
        self.dev, self.case, self.lib, self.st = dev, case, _explain.load(), dev.ops.stream
        self.band_h = np.full(int(case.band_ptr[-1]) + 1, GUARD_F64)
        self.band = dev.put(self.band_h)
        self.a_pos, self.b_pos = dev.put(some(case.pos_a)), dev.put(some(case.pos_b))
        self.a_ptr, self.b_ptr, self.bp = dev.put(case.ptr_a), dev.put(case.ptr_b), dev.put(case.band_ptr)

    def gather(self, S, layout, stride, n_rows, n_cols, hint=None):
        c = self.case
        _explain.check(self.lib.simrank_explain_gather(
            S, layout, stride, n_rows, n_cols, self.a_pos, self.a_ptr, self.b_pos, self.b_ptr, self.bp, c.n,
            int(c.terms.max()) if hint is None else hint, self.band, self.st), "gather")
        got = self.dev.get(self.band, self.band_h)
        assert got[-1] == GUARD_F64
        return got[:-1]

    def load(self, band):
        self.dev.ops.h2d(self.band, np.ascontiguousarray(band, dtype=np.float64))

    def reduce(self, hints=None):
        c = self.case
        rs_h, cs_h = np.full(c.pos_a.size + 1, GUARD_F64), np.full(c.pos_b.size + 1, GUARD_F64)
        raw_h, cnt_h = np.full(c.n + 1, GUARD_F64), np.full(c.n + 1, GUARD_I64, dtype=np.int64)
        rs, cs, raw, cnt = (self.dev.put(h) for h in (rs_h, cs_h, raw_h, cnt_h))
        max_rows, max_cols = hints or (int(c.na.max()), int(c.nb.max()))
        _explain.check(self.lib.simrank_explain_reduce(self.band, self.a_ptr, self.b_ptr, self.bp, c.n, max_rows, max_cols, rs,
                                                       cs, raw, cnt, self.st), "reduce")
        out = [self.dev.get(d, h) for d, h in ((rs, rs_h), (cs, cs_h), (raw, raw_h), (cnt, cnt_h))]
        assert out[0][-1] == GUARD_F64 and out[1][-1] == GUARD_F64 and out[2][-1] == GUARD_F64 and out[3][-1] == GUARD_I64
        return [o[:-1] for o in out]

    def select(self, k):
        c = self.case
        i_h, v_h = np.full(c.n * k + 1, GUARD_I32, dtype=np.int32), np.full(c.n * k + 1, GUARD_F64)
        bi, bj, bv = self.dev.put(i_h), self.dev.put(i_h), self.dev.put(v_h)
        _explain.check(self.lib.simrank_explain_select(self.band, self.a_ptr, self.b_ptr, self.bp, c.n, k, bi, bj, bv, self.st),
                       "select")
        gi, gj, gv = self.dev.get(bi, i_h), self.dev.get(bj, i_h), self.dev.get(bv, v_h)
        assert gi[-1] == GUARD_I32 and gj[-1] == GUARD_I32 and gv[-1] == GUARD_F64
        return gi[:-1].reshape(c.n, k), gj[:-1].reshape(c.n, k), gv[:-1].reshape(c.n, k)


def make_case(rng, n_rows, n_cols, lens=LENS):
    """One pair per length: |I(a)| = lens[i] against |I(b)| = lens[(5 i + 3) mod len]: every length on either side, empty
    lists on either side, positions drawn with repeats (the blocks have fewer rows than the lists entries), and in the
    longer lists a position outside the block, below and above."""
    m = len(lens)
    lists_a = [rng.integers(0, n_rows, size=lens[i]).astype(np.int64) for i in range(m)]
    lists_b = [rng.integers(0, n_cols, size=lens[(5 * i + 3) % m]).astype(np.int64) for i in range(m)]
    outside_r, outside_c = [-1, n_rows, 2 ** 31 - 1, -2 ** 31], [n_cols, -1, -2 ** 31, 2 ** 31 - 1]
    for i in range(m):
        if lists_a[i].size >= 31 and i % 2 == 0:
            lists_a[i][[3, lists_a[i].size - 1]] = [outside_r[i % 4], outside_r[(i + 1) % 4]]
        if lists_b[i].size >= 31 and i % 2 == 1:
            lists_b[i][[5, 0]] = [outside_c[i % 4], outside_c[(i + 1) % 4]]
    return Case(lists_a, lists_b)


def want_pieces(A, case):
    return [ER.block_gather(A, a, b) for a, b in zip(case.lists_a, case.lists_b)]


def flat(pieces):
    return np.concatenate([p.ravel() for p in pieces]) if pieces else np.empty(0)


def check_reduce(got, pieces, case, exact, what):
    """``got`` of ``Run.reduce`` against ``explain_ref.reduce`` of every piece: bit for bit where the sums are exact,
    within ``m * 2^-52 * sum |x|`` otherwise; the count exactly."""
    rs, cs, raw, cnt = got
    for p, piece in enumerate(pieces):
        w_rs, w_cs, w_raw, w_cnt = ER.reduce(piece)
        g = (rs[case.ptr_a[p]:case.ptr_a[p + 1]], cs[case.ptr_b[p]:case.ptr_b[p + 1]], raw[p:p + 1])
        assert cnt[p] == w_cnt, (what, p, "contributors")
        if exact:
            finite = piece[~np.isnan(piece)]
            assert math.fsum(finite.tolist()) == float(np.sum(finite))      # the sums of this block are exact in any order
            for a, b, name in zip(g, (w_rs, w_cs, np.array([w_raw])), ("rows", "columns", "raw")):
                same_bits(a, b, (what, p, name))
        else:
            for a, b, tol, name in zip(g, (w_rs, w_cs, np.array([w_raw])), ER.bounds(piece), ("rows", "columns", "raw")):
                tol = np.atleast_1d(tol)
                assert np.array_equal(np.isnan(a), np.isnan(b)), (what, p, name)
                ok = ~np.isnan(b)
                assert (np.abs(a[ok] - b[ok]) <= tol[ok]).all(), (what, p, name, np.abs(a[ok] - b[ok]).max())


def check_select(got, pieces, k, what):
    gi, gj, gv = got
    for p, piece in enumerate(pieces):
        wi, wj, wv = ER.best(piece, k)
        same_bits(gi[p], wi, (what, k, p, "i"))
        same_bits(gj[p], wj, (what, k, p, "j"))
        same_bits(gv[p], wv, (what, k, p, "value"))


# ---- 1. gather, and the chain on what it gathered -----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_gather_reduce_and_select_on_blocks(dev, layout):
    more = fewer = none = 0
    for s, (n_rows, n_cols) in enumerate(B.SHAPES):
        kind = ("dyadic", "wide")[s % 2]
        blk = B.make_block(layout, n_rows, n_cols, B.variants(layout, n_rows, n_cols)[0][1], 500 + s, kind=kind)
        A = blk.A
        # the 1025-entry lists once per kind; elsewhere up to 257
        case = make_case(np.random.default_rng([s, layout, 3]), n_rows, n_cols, LENS if s in (5, 6) else LENS[:-1])
        pieces = want_pieces(A, case)
        want = flat(pieces)
        assert np.isnan(want).any() and case.n >= 12 and (case.terms == 0).sum() >= 2
        for v, (tag, stride, base) in enumerate(B.variants(layout, n_rows, n_cols)):
            what = (layout, n_rows, n_cols, tag, kind)
            S = dev.put(B.encode(layout, A, stride, blk.sentinel).tobytes(), base)
            run = Run(dev, case)
            got = run.gather(S, layout, stride, n_rows, n_cols)
            same_bits(got, want, (what, "gather"))
            same_bits(run.gather(S, layout, stride, n_rows, n_cols), got, (what, "a second run"))
            same_bits(Run(dev, case).gather(S, layout, stride, n_rows, n_cols, hint=1), want, (what, "a hint too small"))
            if v == 0:
                check_reduce(run.reduce(), pieces, case, kind == "dyadic", what)
                if s % 3 == 0:
                    check_reduce(run.reduce(hints=(1, 1)), pieces, case, kind == "dyadic", (what, "hints too small"))
                for k in KS if s in (5, 6) else (KS[s % len(KS)],):
                    first = run.select(k)
                    check_select(first, pieces, k, what)
                    if k == 64:
                        for a, b in zip(first, run.select(k)):
                            same_bits(a, b, (what, "select again"))
                    n_contrib = np.array([int(ER.contributors(p).sum()) for p in pieces])
                    more, fewer, none = more + int((n_contrib > k).sum()), fewer + int(((n_contrib < k) & (n_contrib > 0)).sum()), \
                        none + int((n_contrib == 0).sum())
            dev.release()
    assert more >= 5 and fewer >= 5 and none >= 5


def test_many_small_pairs_in_one_call(dev):
    """3000 pairs of 0 .. 40 x 0 .. 40 in one call (one workgroup along y each), some empty on either side."""
    layout, n_rows, n_cols = B.ROWMAJOR_F32, 70, 129
    _, stride, base = B.variants(layout, n_rows, n_cols)[0]
    blk = B.make_block(layout, n_rows, n_cols, stride, 77, kind="dyadic")
    rng = np.random.default_rng(8)
    la = [rng.integers(0, n_rows, size=rng.integers(0, 41)) for _ in range(3000)]
    lb = [rng.integers(0, n_cols, size=rng.integers(0, 41)) for _ in range(3000)]
    case = Case(la, lb)
    pieces = want_pieces(blk.A, case)
    run = Run(dev, case)
    same_bits(run.gather(dev.put(blk.raw, base), layout, stride, n_rows, n_cols), flat(pieces), "gather")
    rs, cs, raw, cnt = run.reduce()
    same_bits(rs, np.concatenate([p.sum(axis=1) + 0.0 for p in pieces]), "rows")               # (dyadic: exact in any order)
    same_bits(cs, np.concatenate([p.sum(axis=0) + 0.0 for p in pieces]), "columns")
    same_bits(raw, np.array([p.sum() + 0.0 for p in pieces]), "raw")
    assert cnt.tolist() == [int(ER.contributors(p).sum()) for p in pieces]
    check_select(run.select(10), pieces, 10, "small pairs")


def test_a_pair_longer_than_its_share_of_the_grid(dev):
    """6000 pairs of 0 .. 40 x 0 .. 40, one of 70 x 60 and one of 3 x 300 in one call.  explain.hip caps the workgroups along y
    at 16384 / n_pairs = 2: the 70 x 60 pair has five chunks of 1024 terms and the 3 x 300 pair five strips of 64 columns, so
    the gather's chunk loop and the column sums' strip loop take a second and a third turn (with 3000 pairs the cap is 5 and
    every loop runs once)."""
    layout, n_rows, n_cols = B.ROWMAJOR_F32, 70, 129
    _, stride, base = B.variants(layout, n_rows, n_cols)[0]
    blk = B.make_block(layout, n_rows, n_cols, stride, 78, kind="dyadic")
    rng = np.random.default_rng(9)
    la = [rng.integers(0, n_rows, size=rng.integers(0, 41)) for _ in range(6000)]
    lb = [rng.integers(0, n_cols, size=rng.integers(0, 41)) for _ in range(6000)]
    la[1234:1234], lb[1234:1234] = [rng.integers(0, n_rows, size=70)], [rng.integers(0, n_cols, size=60)]
    la.append(rng.integers(0, n_rows, size=3)), lb.append(rng.integers(0, n_cols, size=300))
    n_pairs = len(la)
    max_terms = max(len(a) * len(b) for a, b in zip(la, lb))
    cap = 16384 // n_pairs                                                    # kBlocksWanted / n_pairs
    assert n_pairs == 6002 and max_terms == 4200 and -(-max_terms // 1024) > cap >= 1
    assert -(-max(len(b) for b in lb) // 64) > cap
    case = Case(la, lb)
    pieces = want_pieces(blk.A, case)
    assert pieces[1234].shape == (70, 60) and pieces[-1].shape == (3, 300)
    run = Run(dev, case)
    same_bits(run.gather(dev.put(blk.raw, base), layout, stride, n_rows, n_cols), flat(pieces), "gather")
    rs, cs, raw, cnt = run.reduce()
    same_bits(rs, np.concatenate([p.sum(axis=1) + 0.0 for p in pieces]), "rows")               # (dyadic: exact in any order)
    same_bits(cs, np.concatenate([p.sum(axis=0) + 0.0 for p in pieces]), "columns")
    same_bits(raw, np.array([p.sum() + 0.0 for p in pieces]), "raw")
    assert cnt.tolist() == [int(ER.contributors(p).sum()) for p in pieces]
    check_select(run.select(10), pieces, 10, "a long pair among many")


# ---- 2. planted values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_a_planted_nan_poisons_its_row_its_column_and_raw(dev, layout):
    n_rows, n_cols = 9, 150
    A, stride, base, raw_bytes = planted(layout, n_rows, n_cols, {(4, 77): np.nan})
    S = dev.put(raw_bytes, base)
    la, lb = [[1, 4, 7, 2], [0, 1, 2, 3], [4]], [[5, 77, 149, 6, 70], [77, 78], [76, 78]]
    case = Case(la, lb)
    run = Run(dev, case)
    pieces = want_pieces(A, case)
    same_bits(run.gather(S, layout, stride, n_rows, n_cols), flat(pieces), layout)
    rs, cs, raw, cnt = run.reduce()
    check_reduce((rs, cs, raw, cnt), pieces, case, True, layout)
    assert np.isnan(rs).tolist() == [False, True, False, False] + [False] * 5
    assert np.isnan(cs).tolist() == [False, True, False, False, False] + [False] * 4
    assert np.isnan(raw).tolist() == [True, False, False] and cnt[0] == int(ER.contributors(pieces[0]).sum()) < 20
    check_select(run.select(3), pieces, 3, layout)


def test_select_ties_zeros_nan_and_negatives(dev):
    """Bands written by hand: a plateau of equal values that spans several i and j (both tie keys decide), +0.0, -0.0 and
    NaN (never listed), negative values (listed after the positive ones), a piece of zeros and NaN alone, an empty one, and
    a piece of 300 x 70 with the plateau past the first turn of the kernel."""
    nan = float("nan")
    rng = np.random.default_rng(4)
    small = np.array([[0.5, 0.75, 0.5, -0.0], [0.5, nan, 0.5, 0.0], [-1.0, 0.5, -0.25, 0.5], [0.0, -2.0, nan, 0.75]])
    nothing = np.array([[0.0, -0.0, nan], [nan, 0.0, -0.0]])
    big = rng.integers(-200, 200, size=(300, 70)) / 64.0
    big[rng.random(big.shape) < 0.2] = 0.0
    big[rng.random(big.shape) < 0.05] = nan
    big[100:140, 20:50] = 2.5                                              # 1200 equal values, above most of the others
    big[260:, :10] = 2.5
    wide_row = np.full((1, 5000), 0.125)                                   # one row: every tie is decided by j
    wide_row[0, ::7] = 0.25
    tall = wide_row.T.copy()                                               # one column: every tie is decided by i
    pieces = [small, nothing, big, np.zeros((0, 4)), wide_row, np.zeros((3, 0)), tall, -np.abs(small)]
    case = Case([np.zeros(p.shape[0], dtype=np.int32) for p in pieces], [np.zeros(p.shape[1], dtype=np.int32) for p in pieces])
    run = Run(dev, case)
    run.load(flat(pieces))
    seen = set()
    for k in KS + (7, 256, 257, 1000):
        got = run.select(k)
        check_select(got, pieces, k, "by hand")
        n_contrib = [int(ER.contributors(p).sum()) for p in pieces]
        seen |= {"more" if c > k else "none" if c == 0 else "fewer" for c in n_contrib}
    assert seen == {"more", "fewer", "none"}
    gi, gj, gv = run.select(65)
    assert gv[0][:8].tolist() == [0.75, 0.75] + [0.5] * 6 and gv[0][8:11].tolist() == [-0.25, -1.0, -2.0] and gi[0][11] == -1
    assert list(zip(gi[0][:8], gj[0][:8])) == [(0, 1), (3, 3), (0, 0), (0, 2), (1, 0), (1, 2), (2, 1), (2, 3)]
    assert (gi[1] == -1).all() and (gv[1] == 0).all() and (gi[3] == -1).all() and (gi[5] == -1).all()
    rs, cs, raw, cnt = run.reduce()
    check_reduce((rs, cs, raw, cnt), pieces, case, True, "by hand")
    assert cnt.tolist()[:2] == [11, 0] and not np.signbit(raw[3]) and raw[3] == 0.0 and raw[5] == 0.0


# ---- 3. through the estimators ----------------------------------------------------------------------------------------------------
def spec_of(model, side):
    return model._model[0].specs[side]


def pairs_for(spec, n, rng, count=24):
    """Pairs of one side: random ones, a node without neighbours on either side, the pair with the most common neighbours
    among the sampled nodes, and a repeated pair."""
    rowptr, col = np.asarray(spec.csr.rowptr, dtype=np.int64), np.asarray(spec.csr.col)
    deg = np.diff(rowptr)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, n, size=(count, 2)) if a != b]
    bare = np.flatnonzero(deg == 0)
    some_node = int(np.argmax(deg))
    if bare.size:
        pairs += [(int(bare[0]), some_node), (some_node, int(bare[0]))]
    # two nodes that share a neighbour: the first two rows that list the most listed column
    hub = int(np.bincount(col, minlength=1).argmax())
    sharing = [u for u in range(n) if hub in col[rowptr[u]:rowptr[u + 1]]][:2]
    if len(sharing) == 2:
        pairs.append((sharing[0], sharing[1]))
    return pairs + [pairs[0]], bool(bare.size), len(sharing) == 2


def check_side(model, side, n_sides, k, dyadic=False):
    kw = {} if n_sides == 1 else {"group": side + 1}
    src_kw = {} if n_sides == 1 else {"group": n_sides - side}
    frames = as_groups(model.frame())
    index, src_index = frames[side].index, frames[n_sides - 1 - side].index
    spec = spec_of(model, side)
    pairs_in, has_bare, has_common = pairs_for(spec, len(index), np.random.default_rng([side, k]))
    a, b = [index[p[0]] for p in pairs_in], [index[p[1]] for p in pairs_in]
    rows_of = lambda ids: model.rows(src_index[np.asarray(ids, dtype=np.int64)], **src_kw).to_numpy()
    evidence = spec.evidence_from is not None
    want, want_terms, want_nb = ER.explain_ref(rows_of, spec.csr, spec.rowscale, spec.coef, spec.lbd, evidence, pairs_in, k)
    pairs, terms, neighbors = model.explain(a, b, k=k, **kw)
    again = model.explain(a, b, k=k, **kw)
    for f, g in zip((pairs, terms, neighbors), again):
        assert f.equals(g)                                                 # the same call gives the same bits twice
    assert pairs.columns.tolist() == ["a", "b", "similarity", "terms", "contributors", "common", "evidence", "raw", "propagated"]
    assert pairs["a"].tolist() == a and pairs["b"].tolist() == b
    same_bits(pairs["similarity"].to_numpy(), model.similarity(a, b, **kw), "similarity")
    for name in ("terms", "contributors", "common"):
        assert pairs[name].dtype == np.int64 and pairs[name].tolist() == want[name].tolist(), name
    same_bits(pairs["evidence"].to_numpy(), want["evidence"], "evidence")
    raw = pairs["raw"].to_numpy()
    if dyadic:
        same_bits(raw, want["raw"], "raw")
        same_bits(pairs["propagated"].to_numpy(), want["propagated"], "propagated")
    else:
        assert (np.abs(raw - want["raw"]) <= want["raw_bound"]).all()
        scale = np.asarray(spec.rowscale, dtype=np.float64)
        mine = np.array([ER.propagated(r, scale[p[0]], scale[p[1]], spec.coef, spec.lbd, e if evidence else None)
                         for r, p, e in zip(raw, pairs_in, want["evidence"])])
        same_bits(pairs["propagated"].to_numpy(), mine, "propagated")      # host arithmetic on the model's own raw
    # the k best: labels, values and order exactly
    assert terms.columns.tolist() == ["pair", "rank", "via_a", "via_b", "similarity", "share"]
    assert list(zip(terms["pair"], terms["rank"], terms["via_a"], terms["via_b"])) == \
        [(p, r, src_index[i], src_index[j]) for p, r, i, j, _ in want_terms]
    same_bits(terms["similarity"].to_numpy(), np.array([v for *_, v in want_terms], dtype=np.float64), "top-k values")
    with np.errstate(invalid="ignore", divide="ignore"):
        same_bits(terms["share"].to_numpy(), terms["similarity"].to_numpy() / raw[terms["pair"].to_numpy()], "share of a term")
    # the marginals, in the order of the CSR rows
    assert neighbors.columns.tolist() == ["pair", "of", "neighbor", "sum", "share"]
    assert list(zip(neighbors["pair"], neighbors["of"], neighbors["neighbor"])) == [(p, of, src_index[i]) for p, of, i, _, _ in want_nb]
    sums = neighbors["sum"].to_numpy()
    w_sum, w_tol = np.array([s for *_, s, _ in want_nb]), np.array([t for *_, t in want_nb])
    if dyadic:
        same_bits(sums, w_sum, "marginals")
    else:
        assert (np.abs(sums - w_sum) <= w_tol).all()
    # shares sum to 1 where raw > 0: with u = 2^-53 a marginal is within (its terms) * u * sum |x| of exact, so one side's
    # marginals add up to the exact total within max(na, nb) * u * sum |x|; raw, the float sum of a's marginals, is within
    # (na + nb) * u * sum |x| of it; every division rounds once: (2 (na + nb) + 2) * u * sum |x| / raw covers both sides
    for p in np.flatnonzero(raw > 0):
        both = int((neighbors["pair"] == p).sum())
        tol = (2 * both + 2) * 2.0 ** -53 * want["abs"][p] / raw[p]
        for of in "ab":
            part = neighbors[(neighbors["pair"] == p) & (neighbors["of"] == of)]
            assert abs(math.fsum(part["share"]) - 1.0) <= tol, (p, of)
    assert (pairs.iloc[0] == pairs.iloc[-1]).all() or pairs.iloc[0].isna().any()          # the repeated pair
    return has_bare, has_common and bool((pairs["common"] > 0).any()), bool((pairs["contributors"] > k).any())


def check_model(model, k=5, dyadic=False):
    n_sides = len(as_groups(model.frame()))
    before = [f.to_numpy().copy() for f in as_groups(model.frame())]
    seen = [check_side(model, side, n_sides, k, dyadic) for side in range(n_sides)]
    for f, b in zip(as_groups(model.frame()), before):
        assert np.array_equal(B.bits(f.to_numpy()), B.bits(b))              # the model is unchanged
    return [any(s[i] for s in seen) for i in range(3)]


@pytest.fixture(scope="module")
def powerlaw():
    return synth.powerlaw_directed(300, 4.0, seed=11)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_simrankpp_on_a_power_law_graph(variant, powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, variant, tmp_path)
    try:
        bare, common, more = check_model(model)
        assert bare and common and more                                     # the cases the pairs are there for
    finally:
        model.release()


def test_simrank_weighted(tmp_path):
    df = synth.powerlaw_directed(300, 4.0, seed=11)
    df["weight"] = np.random.default_rng(3).integers(1, 6, size=len(df)).astype(np.float64)
    model = make_model("SimRank", df, "f32-kept", tmp_path, weighted=True)
    try:
        check_model(model, k=12)
    finally:
        model.release()


@pytest.mark.parametrize("variant", ["f32-kept", "f64-kept", "world3-kept", "f32-compact-fp16"])
def test_bipartite_simrankpp_both_groups(variant, tmp_path):
    df = bipartite_random(90, 50, 0.06, 12)
    model = make_model("BipartiteSimRankPP", df, variant, tmp_path, strict_reference=False)
    try:
        check_model(model, k=7)
    finally:
        model.release()


def test_a_pruned_model_explains_its_matrix_p(powerlaw, tmp_path):
    model = make_model("SimRankPP", powerlaw, "f32-kept", tmp_path)
    try:
        model.prune(10)
        assert model.kept_neighbors == 10
        check_model(model)
    finally:
        model.release()


def test_bands_cut_by_the_slab_give_the_same_frames(powerlaw, tmp_path, monkeypatch):
    from simrank_amd import _query
    model = make_model("SimRankPP", powerlaw, "f32-compact", tmp_path)
    try:
        index = model.frame().index
        rng = np.random.default_rng(2)
        a, b = index[rng.integers(0, 150, size=60)], index[rng.integers(150, 300, size=60)]
        want = model.explain(a, b, k=4)
        monkeypatch.setattr(_query, "SLAB_BYTES", 8 * 64)                    # a few small pieces per band, most pairs alone
        monkeypatch.setattr(_explain, "BIG_TERMS", 40)
        for f, g in zip(model.explain(a, b, k=4), want):
            assert f.equals(g)
    finally:
        model.release()


@pytest.mark.parametrize("variant", ["f32-kept", "f64-kept", "world3-kept", "f32-compact"])
def test_a_fit_with_dyadic_iterates(variant, tmp_path):
    """regular_graph(256, 4) with C = 0.5, as tests/test_gpu_groups.py fits it: the iterate lies on a dyadic grid, every
    float64 sum of its elements is exact in any order, and the sums equal ``explain_ref``'s bit for bit."""
    from oracle import simrank_oracle as O
    from simrank_amd.driver import LocalWorld
    df = X.regular_graph(256, 4, seed=260)
    _, G = O.directed_graph(df)
    updates = X.exact_updates(G, 0.5, None, mantissa=24, limit=8).updates
    assert updates >= 2
    kw, then = VARIANTS[variant]
    kw = dict(kw)
    if "world" in kw:
        kw.update(world=LocalWorld(kw["world"]), mode="sparse")
    est = SRA.SimRank()
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(df, C=0.5, iterations=updates, eps=1e-30, verbose=False, keep=True, **kw)
    if then == "compact":
        est.compact()
    try:
        check_model(est, dyadic=True)
    finally:
        est.release()


@pytest.mark.parametrize("cls", ["SimRank", "SimRankPP"])
def test_propagated_is_the_next_update_of_the_shipped_loop(cls):
    """A kept float64 fit of t = 3 updates explains what the dense float64 fit of 4 updates holds: relative within
    ``(|I(a)| + |I(b)| + 8) * 2^-53``, the bound tests/test_explain_cpu.py derives against the reference."""
    df = synth.powerlaw_directed(300, 4.0, seed=11)
    fits = {}
    for t in (3, 4):
        est = getattr(SRA, cls)()
        with contextlib.redirect_stdout(io.StringIO()):
            frame = est.fit(df, iterations=t, eps=1e-30, verbose=False, keep=(t == 3), storage_precision="f64")
        assert est.converged_at is None                                      # neither stopped early
        fits[t] = (est, frame)
    est, _ = fits[3]
    try:
        nxt = fits[4][1]
        index = nxt.index
        deg = np.diff(np.asarray(spec_of(est, 0).csr.rowptr, dtype=np.int64))
        nodes = np.random.default_rng(6).choice(len(index), 40, replace=False)
        pairs_in = [(int(a), int(b)) for a in nodes for b in nodes if a != b]
        pairs, _, _ = est.explain([index[a] for a, _ in pairs_in], [index[b] for _, b in pairs_in], k=1)
        want = nxt.to_numpy()[[a for a, _ in pairs_in], [b for _, b in pairs_in]]
        tol = np.array([(deg[a] + deg[b] + 8) * 2.0 ** -53 for a, b in pairs_in])
        got = pairs["propagated"].to_numpy()
        print("largest error in units of the bound:", float(np.max(np.abs(got - want) / np.maximum(tol * np.abs(want), 1e-300))))
        assert (np.abs(got - want) <= tol * np.abs(want)).all()
        assert (want > 0).sum() > 100
    finally:
        est.release()
