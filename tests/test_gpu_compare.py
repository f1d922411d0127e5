"""libsimrank_compare.so and ``model.compare`` on a real MI355X, bit for bit against tests/compare_ref.py.

Block level, through the C entry on tests/blocks.py blocks (kind="wide": many binades; padding holds a finite sentinel far
above every value, which a kernel that counted padding would report as a difference): B is A cast to B's stored type
(what ``compact(precision="fp16")`` does to an f32 model) with a seeded fraction of elements perturbed: one-ulp changes,
sign-of-zero flips, NaN and +-inf planted on one side or on both, and one row whose maximum occurs twice.  All 16 layout
pairs; every shape of ``blocks.SHAPES`` and every stride / base of ``blocks.variants`` on four pairs; n_tol = 0, 1 and 8;
the histogram ADDED to a non-zero pattern; guard elements after every output; one 3000 x 1025 all-equal block; and
8 197 x 40 and 24 577 x 40 blocks of ``blocks.make_long`` on six pairs: more rows than the capped grid has waves, so a
wave takes a second, third and fourth row.

Model level, on a 600-node directed graph (the generator of tests/test_gpu_neighbors.py at a size whose N - 1 neighbours
``most_similar`` still lists) and that module's bipartite graph: ``compare`` equals
``compare_ref.model`` on the two ``frame()``s and the two ``most_similar`` frames; both models are left unchanged."""
import contextlib
import io

import numpy as np
import pytest

import simrank_amd
import simrank_amd.SimRank as SRA
from simrank_amd import _compare, synth
from simrank_amd.driver import LocalWorld
from simrank_amd.engine import HipOps
from tests import blocks as B
from tests import compare_ref as R
from tests.graphs import bipartite_random
from tests.test_gpu_neighbors import dev, device, same_bits  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

GUARD_F64 = 1e300
GUARD_I32 = 0x5A5A5A5A
GUARD_U32 = 0xA5A5A5A5
TOLS = {0: (), 1: (0.0,), 8: (0.0, 2.0 ** -30, 2.0 ** -20, 1e-5, 2.0 ** -11, 0.5, 3.0, 1e300)}
HIST0 = (np.arange(R.BINS, dtype=np.uint64) * np.uint64(3) + np.uint64(1)) << np.uint64(33)     # what the bins hold before
TWICE = 3.0                                             # the planted double maximum: fits every stored type


# ---- a pair of blocks ---------------------------------------------------------------------------------------------------
def cast(layout, values):
    """float64 values -> the layout's stored type, rounded (to nearest even; out of range: inf)."""
    with np.errstate(over="ignore", invalid="ignore"):
        if layout == B.PANEL_F16:
            return (np.asarray(values, dtype=np.float64) * B.HALF_SCALE).astype(np.float16)
        return np.asarray(values, dtype=np.float64).astype(B.STORED[layout])


def place(layout, M, stride, sentinel):
    """A matrix of STORED elements as the block's flat stored array, padding = the sentinel (a value)."""
    n_rows, n_cols = M.shape
    raw = np.full(B.n_elems(layout, n_rows, n_cols, stride), cast(layout, sentinel), dtype=B.STORED[layout])
    raw[B.offsets(layout, n_rows, n_cols, stride).ravel()] = M.ravel()
    return raw


def pair(la, lb, n_rows, n_cols, seed, fraction=0.1):
    """(MA, MB): the stored elements [n_rows, n_cols] of the two sides.  MA is ``make_block``'s wide block of layout la; MB
    is MA cast to lb's stored type, with perturbations planted in either or both."""
    stride = n_rows + 3 if la in B.PANEL else n_cols + 4
    blk = B.make_block(la, n_rows, n_cols, stride, seed, kind="wide")
    MA = cast(la, blk.A)
    assert np.array_equal(B.bits(B.widen(la, MA)), B.bits(blk.A))
    MB = cast(lb, blk.A)
    rng = np.random.default_rng([seed, la, lb, n_rows, n_cols])
    size = n_rows * n_cols
    picks = rng.permutation(size)[:max(1, int(fraction * size))]
    kinds = ["ulp_up", "ulp_down", "zero_flip", "zero_flip", "nan_b", "nan_a", "nan_both", "inf_b", "inf_both", "inf_opposite",
             "ninf_a", "ulp_up", "ulp_down", "ulp_up"]
    twice_row = n_rows // 2 if n_cols >= 3 else -1
    big = {B.PANEL_F16: np.float16(np.inf), B.ROWMAJOR_F64: np.float64(np.inf)}
    inf = lambda layout: big.get(layout, np.float32(np.inf))
    for i, at in enumerate(picks.tolist()):
        r, c = divmod(at, n_cols)
        what = kinds[i % len(kinds)]
        if r == twice_row and not what.startswith("ulp"):
            continue                                        # (nothing in that row may pass the planted maximum)
        tb, ta = MB.dtype.type, MA.dtype.type
        if what.startswith("ulp"):
            with np.errstate(over="ignore"):                # (the largest finite value steps to infinity)
                MB[r, c] = np.nextafter(MB[r, c], inf(lb) if what == "ulp_up" else -inf(lb))
        elif what == "zero_flip":
            MA[r, c], MB[r, c] = ta(0.0), tb(-0.0)
        elif what == "nan_b":
            MB[r, c] = tb(np.nan)
        elif what == "nan_a":
            MA[r, c] = ta(np.nan)
        elif what == "nan_both":
            MA[r, c], MB[r, c] = ta(np.nan), tb(np.nan)
        elif what == "inf_b":
            MB[r, c] = inf(lb)
        elif what == "inf_both":
            MA[r, c], MB[r, c] = inf(la), inf(lb)
        elif what == "inf_opposite":
            MA[r, c], MB[r, c] = inf(la), -inf(lb)
        elif what == "ninf_a":
            MA[r, c] = -inf(la)
    if twice_row >= 0:
        c1, c2 = sorted(rng.choice(n_cols, size=2, replace=False).tolist())
        for c in (c1, c2):
            MA[twice_row, c], MB[twice_row, c] = MA.dtype.type(0.0), cast(lb, TWICE)
    return MA, MB, twice_row


def run_sweep(dev, SA, la, sa, SB, lb, sb, n_rows, n_cols, tol, floor=0.0):
    """One call of the C entry into pre-filled outputs, each one element (``over``: one row) longer than it has to be ->
    (max_abs, arg_abs, max_rel, arg_rel, over, hist) as the device left them, guards included."""
    lib, st, n_tol = _compare.load(), dev.ops.stream, len(tol)
    f64_h, i32_h = np.full(n_rows + 1, GUARD_F64), np.full(n_rows + 1, GUARD_I32, dtype=np.int32)
    over_h = np.full((n_rows + 1, max(n_tol, 1)), GUARD_U32, dtype=np.uint32)
    hist_h = np.concatenate([HIST0, [np.uint64(7)]])
    d_abs, d_rel, d_aabs, d_arel = dev.put(f64_h), dev.put(f64_h), dev.put(i32_h), dev.put(i32_h)
    d_over, d_hist = dev.put(over_h), dev.put(hist_h)
    tol_h = np.ascontiguousarray(tol, dtype=np.float64)
    _compare.check(lib.simrank_compare_sweep(SA, la, sa, SB, lb, sb, n_rows, n_cols, tol_h.ctypes.data if n_tol else None,
                                             n_tol, floor, d_abs, d_aabs, d_rel, d_arel, d_over if n_tol else None, d_hist,
                                             st), "sweep")
    return (dev.get(d_abs, f64_h), dev.get(d_aabs, i32_h), dev.get(d_rel, f64_h), dev.get(d_arel, i32_h),
            dev.get(d_over, over_h), dev.get(d_hist, hist_h))


def expected(ref, n_rows, n_tol):
    max_abs, arg_abs, max_rel, arg_rel, over, hist = ref
    f = lambda x: np.concatenate([x, [GUARD_F64]])
    i = lambda x: np.concatenate([x, np.array([GUARD_I32], dtype=np.int32)])
    over_w = np.full((n_rows + 1, max(n_tol, 1)), GUARD_U32, dtype=np.uint32)
    over_w[:n_rows, :n_tol] = over
    return f(max_abs), i(arg_abs), f(max_rel), i(arg_rel), over_w, np.concatenate([HIST0 + hist, [np.uint64(7)]])


NAMES = ("max_abs", "arg_abs", "max_rel", "arg_rel", "over", "hist")


def check_pair(dev, la, lb, n_rows, n_cols, seed, variants_a=None, variants_b=None, floor=2.0 ** -20):
    """Every variant of either side, n_tol = 0, 1 and 8, against one reference; a second run gives the same bits."""
    MA, MB, twice_row = pair(la, lb, n_rows, n_cols, seed)
    A, Bm = B.widen(la, MA), B.widen(lb, MB)
    refs = {n_tol: R.sweep(A, Bm, tol, floor) for n_tol, tol in TOLS.items()}
    d = R.distance(A, Bm)
    assert refs[8][5].sum() == n_rows * n_cols and (refs[1][4][:, 0] + (d == 0).sum(axis=1) == n_cols).all()
    if twice_row >= 0:
        assert refs[8][0][twice_row] == TWICE and (d[twice_row] == TWICE).sum() == 2
        assert refs[8][1][twice_row] == np.flatnonzero(d[twice_row] == TWICE)[0]
    sa_, sb_ = B.SENTINEL[(la, "wide")], B.SENTINEL[(lb, "wide")]
    for tag_a, stride_a, base_a in variants_a or B.variants(la, n_rows, n_cols)[:1]:
        SA = dev.put(place(la, MA, stride_a, sa_).tobytes(), base_a)
        for tag_b, stride_b, base_b in variants_b or B.variants(lb, n_rows, n_cols)[:1]:
            SB = dev.put(place(lb, MB, stride_b, sb_).tobytes(), base_b)
            for n_tol, tol in TOLS.items():
                what = (la, lb, n_rows, n_cols, tag_a, tag_b, n_tol)
                got = run_sweep(dev, SA, la, stride_a, SB, lb, stride_b, n_rows, n_cols, tol, floor)
                for g, w, name in zip(got, expected(refs[n_tol], n_rows, n_tol), NAMES):
                    same_bits(g, w, (what, name))
            again = run_sweep(dev, SA, la, stride_a, SB, lb, stride_b, n_rows, n_cols, TOLS[8], floor)
            for g, a in zip(got, again):
                assert np.array_equal(B.bits(g), B.bits(a)), what
        dev.release()
    return refs[8]


# ---- 1. the C entry on synthetic blocks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("la", B.LAYOUTS)
@pytest.mark.parametrize("lb", B.LAYOUTS)
def test_all_sixteen_layout_pairs(dev, la, lb):
    seen = np.zeros(R.BINS, dtype=np.uint64)
    for i, (n_rows, n_cols) in enumerate([(7, 31), (9, 63), (70, 129)]):
        ref = check_pair(dev, la, lb, n_rows, n_cols, 40 + i)
        seen += ref[5]
    assert seen[0] and seen[2047] and (seen[1:2047] != 0).sum() >= 3      # zeros, infinities and finite differences


@pytest.mark.parametrize("la,lb", [(B.ROWMAJOR_F32, B.PANEL_F16), (B.PANEL_F32, B.ROWMAJOR_F64),
                                   (B.ROWMAJOR_F32, B.ROWMAJOR_F32), (B.PANEL_F16, B.PANEL_F16)])
def test_every_shape_stride_and_base(dev, la, lb):
    for i, (n_rows, n_cols) in enumerate(B.SHAPES):
        check_pair(dev, la, lb, n_rows, n_cols, 60 + i, B.variants(la, n_rows, n_cols), B.variants(lb, n_rows, n_cols))


@pytest.mark.parametrize("floor", [0.0, 0.5, 1.7e308])
def test_the_rules_of_rel_in_their_order(dev, floor):
    """Hand-made float64 rows: below the floor comes first (also where the difference of two finite values overflows), a
    NaN or infinite operand is below no finite floor, then d == inf, then the division."""
    inf, nan = np.inf, np.nan
    A = np.array([[1.5e308, nan, inf, 1.0, 0.25, -0.5, 0.0, -0.0, inf, -inf, nan, 3.0],
                  [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    Bm = np.array([[-1.5e308, 1.0, 1.0, 1.0, 0.125, 0.25, 2.0 ** -1074, 0.0, inf, inf, nan, -1.0],
                   [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0 + 2.0 ** -52]])
    la = lb = B.ROWMAJOR_F64
    SA, SB = dev.put(place(la, A, 12, 0.0).tobytes()), dev.put(place(lb, Bm, 12, 0.0).tobytes())
    ref = R.sweep(A, Bm, TOLS[8], floor)
    if floor == 1.7e308:
        assert ref[2].tolist() == [inf, 0.0] and ref[3].tolist() == [1, 0]        # the overflowed pair of column 0 is +0.0
    got = run_sweep(dev, SA, la, 12, SB, lb, 12, 2, 12, TOLS[8], floor)
    for g, w, name in zip(got, expected(ref, 2, 8), NAMES):
        same_bits(g, w, (floor, name))


def test_an_empty_row_and_no_rows(dev):
    S = dev.put(np.zeros(64, dtype=np.float32))
    got = run_sweep(dev, S, B.ROWMAJOR_F32, 4, S, B.PANEL_F16, 5, 5, 0, TOLS[1])
    want = expected(R.sweep(np.zeros((5, 0)), np.zeros((5, 0)), TOLS[1]), 5, 1)
    for g, w, name in zip(got, want, NAMES):
        same_bits(g, w, ("no columns", name))
    assert got[1][:5].tolist() == [-1] * 5 and got[0][:5].tolist() == [0.0] * 5
    got = run_sweep(dev, S, B.ROWMAJOR_F32, 4, S, B.PANEL_F16, 0, 0, 4, TOLS[1])
    for g, w, name in zip(got, expected(R.sweep(np.zeros((0, 4)), np.zeros((0, 4)), TOLS[1]), 0, 1), NAMES):
        same_bits(g, w, ("no rows", name))


def test_an_all_equal_block_of_many_rows(dev):
    """3000 x 1025: more rows than one turn of a small grid, every element in ONE non-zero bin (the wave aggregates 64
    lanes into one add), and a workgroup's bins hold several rows before they are flushed."""
    n_rows, n_cols, la, lb = 3000, 1025, B.ROWMAJOR_F32, B.PANEL_F16
    A, Bm = np.full((n_rows, n_cols), 0.5), np.full((n_rows, n_cols), 0.25)
    Bm[:, 1024] = 0.5                                       # the last column agrees: the ragged quad counts zeros
    Bm[1234, 77] = -0.5                                     # one larger difference: d = 1.0
    (_, stride_a, base_a), (_, stride_b, base_b) = B.variants(la, n_rows, n_cols)[0], B.variants(lb, n_rows, n_cols)[0]
    SA = dev.put(place(la, cast(la, A), stride_a, 2.0 ** 100).tobytes(), base_a)
    SB = dev.put(place(lb, cast(lb, Bm), stride_b, 3.5).tobytes(), base_b)
    ref = R.sweep(A, Bm, TOLS[8], 0.0)
    assert ref[5][1021] == n_rows * 1024 - 1 and ref[5][0] == n_rows and ref[5][1023] == 1
    got = run_sweep(dev, SA, la, stride_a, SB, lb, stride_b, n_rows, n_cols, TOLS[8], 0.0)
    for g, w, name in zip(got, expected(ref, n_rows, 8), NAMES):
        same_bits(g, w, ("all equal", name))
    assert got[1][1234] == 77 and got[1][0] == 0


# ---- 1b. past the grid cap: a wave takes a second, third and fourth row ------------------------------------------------------
TURN = 2048 * 4                                         # SIMRANK_COMPARE_MAX_GRID workgroups of four waves, one row per wave
TALL = (8197, 24577)                                    # a second turn of five rows; four turns, the last of ONE row
TALL_PAIRS = [(l, l) for l in B.LAYOUTS] + [(B.ROWMAJOR_F32, B.PANEL_F16), (B.ROWMAJOR_F64, B.PANEL_F32)]


def tall_pair(la, lb, n_rows, n_cols, seed):
    """(MA, MB, equal rows): stored elements of two tall blocks.  Both are ``blocks.make_long``'s values (the binary16
    pool where either side is binary16, so that both casts are exact); about one element in twenty of B is then changed:
    one ulp up or down, a flipped sign of zero, NaN on one side or on both, an infinity.  One row of every turn of more
    than three rows is equal throughout (its answer is (0.0, column 0) and all its elements are zeros of the histogram);
    the first and the last row of every turn differ."""
    base = B.PANEL_F16 if B.PANEL_F16 in (la, lb) else la
    V = B.make_long(base, n_rows, n_cols, n_rows + 3 if base in B.PANEL else n_cols + 4, seed).A
    MA, MB = cast(la, V), cast(lb, V)
    assert np.array_equal(B.widen(la, MA), V) and np.array_equal(B.widen(lb, MB), V)
    rng = np.random.default_rng([seed, la, lb, n_rows])
    turns = [(lo, min(lo + TURN, n_rows)) for lo in range(0, n_rows, TURN)]
    equal = np.array([lo + min(5 + 3 * t, hi - lo - 2) for t, (lo, hi) in enumerate(turns) if hi - lo > 3])   # (no two one turn apart)
    ends = np.array([r for lo, hi in turns for r in (lo, hi - 1) if r not in equal])
    change = rng.random((n_rows, n_cols)) < 0.05
    change[ends, rng.integers(0, n_cols, size=ends.size)] = True
    change[equal] = False
    kind = np.where(change, rng.integers(0, 8, size=change.shape), -1)
    ta, tb = MA.dtype.type, MB.dtype.type
    up, down, flip = kind == 0, (kind == 1) | (kind == 2), kind == 3
    MB[up], MB[down] = np.nextafter(MB[up], tb(np.inf)), np.nextafter(MB[down], tb(-np.inf))
    MA[flip], MB[flip] = ta(0.0), tb(-0.0)
    MB[(kind == 4) | (kind == 6)] = tb(np.nan)
    MA[(kind == 5) | (kind == 6)] = ta(np.nan)
    MB[kind == 7] = tb(np.inf)
    # What a carried-over best would get wrong: the first row of turn t differs in ONE place, column 7 + t, by about
    # 2^-(t + 1): less than the first row of the turn before it.  The row one turn before an equal row differs too.
    # And NaN on one side and on both in the second row of every turn of more than two rows.
    for t, (lo, hi) in enumerate(turns):
        MA[lo], MB[lo] = cast(la, V[lo]), cast(lb, V[lo])
        MB[lo, 7 + t] = cast(lb, V[lo, 7 + t] + 2.0 ** -(t + 1))
        if hi - lo > 2:
            MB[lo + 1, 3], MA[lo + 1, 4], MB[lo + 1, 4] = tb(np.nan), ta(np.nan), tb(np.nan)
        if hi - 1 > lo:                                     # (the last row's change may have been a flipped zero: no difference)
            MA[hi - 1, 9], MB[hi - 1, 9] = cast(la, V[hi - 1, 9]), np.nextafter(cast(lb, V[hi - 1, 9]), tb(np.inf))
    for r in equal[equal >= TURN]:
        MB[r - TURN, 2] = np.nextafter(cast(lb, V[r - TURN, 2]), tb(np.inf))
    return MA, MB, equal, turns


@pytest.mark.parametrize("n_rows", TALL)
@pytest.mark.parametrize("la,lb", TALL_PAIRS)
def test_more_rows_than_the_grid_has_waves(dev, la, lb, n_rows):
    """8 197 x 40 and 24 577 x 40: the grid is capped at 2 048 workgroups, so a wave takes rows r, r + 8 192, ...: a row's
    best, its place and its counts start afresh at every row, while a lane's zeros run on over all its rows."""
    n_cols, floor = 40, 2.0 ** -20
    MA, MB, equal, turns = tall_pair(la, lb, n_rows, n_cols, 90)
    A, Bm = B.widen(la, MA), B.widen(lb, MB)
    d = R.distance(A, Bm)
    assert n_rows > TURN and len(turns) == -(-n_rows // TURN)
    for lo, hi in turns:                                    # every turn holds rows that differ, NaN on one side and on both
        assert (d[lo] > 0).any() and (d[hi - 1] > 0).any()
        na, nb = np.isnan(A[lo:hi]), np.isnan(Bm[lo:hi])
        assert hi - lo == 1 or ((na ^ nb).any() and (na & nb).any())
    # a later row of a wave whose maximum is BELOW that of the wave's row one turn before: a best that is carried over shows
    late = [lo for lo, _ in turns if lo] + equal[equal >= TURN].tolist()
    assert len(late) >= len(turns) - 1 and all(d[r].max() < d[r - TURN].max() for r in late)
    assert (d[TURN:].max(axis=1) < d[:n_rows - TURN].max(axis=1)).sum() >= len(late)
    refs = {n_tol: R.sweep(A, Bm, TOLS[n_tol], floor) for n_tol in (8, 1)}
    assert (refs[8][0][equal] == 0.0).all() and (refs[8][1][equal] == 0).all() and (refs[8][4][equal] == 0).all()
    assert len(equal) >= len(turns) - 1 and refs[8][5][0] >= n_cols * len(equal) and refs[8][5].sum() == n_rows * n_cols
    sa_, sb_ = B.SENTINEL[(la, "wide")], B.SENTINEL[(lb, "wide")]
    va, vb = B.variants(la, n_rows, n_cols), B.variants(lb, n_rows, n_cols)
    for i in range(max(len(va), len(vb))):
        (tag_a, stride_a, base_a), (tag_b, stride_b, base_b) = va[i % len(va)], vb[i % len(vb)]
        SA = dev.put(place(la, MA, stride_a, sa_).tobytes(), base_a)
        SB = dev.put(place(lb, MB, stride_b, sb_).tobytes(), base_b)
        for n_tol in (1, 8) if i == 0 else (8,):
            what = (la, lb, n_rows, tag_a, tag_b, n_tol)
            got = run_sweep(dev, SA, la, stride_a, SB, lb, stride_b, n_rows, n_cols, TOLS[n_tol], floor)
            for g, w, name in zip(got, expected(refs[n_tol], n_rows, n_tol), NAMES):
                same_bits(g, w, (what, name))
        again = run_sweep(dev, SA, la, stride_a, SB, lb, stride_b, n_rows, n_cols, TOLS[8], floor)
        for g, a in zip(got, again):
            assert np.array_equal(B.bits(g), B.bits(a)), what
        dev.release()


# ---- 2. through the estimators -------------------------------------------------------------------------------------------
def fit(cls, df, iterations=3, then=None, tmp_path=None, **kw):
    if "world" in kw:
        kw.update(world=LocalWorld(kw["world"]), mode="sparse")
    est = getattr(SRA, cls)()
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(df, iterations=iterations, eps=1e-30, verbose=False, keep=True, **kw)
    if then == "compact":
        est.compact()
    elif then == "compact-fp16":
        est.compact(precision="fp16")
    elif then == "load":
        est.save(tmp_path / "dense.bin")
        est.release()
        est = simrank_amd.load_model(tmp_path / "dense.bin")
    return est


@pytest.fixture(scope="module")
def graph():
    return synth.er_directed(600, 0.005, seed=7)


def groups_of(x):
    return list(x) if isinstance(x, tuple) else [x]


def check_frames(got, want, index, what):
    (summary, nodes, histogram), (want_s, want_n, want_h) = got, want
    assert nodes.index.equals(index) and nodes.columns.tolist() == list(want_n), what
    for name, col in want_n.items():
        if col.dtype.kind == "f":
            same_bits(nodes[name].to_numpy(), col, (what, name))
        else:
            assert nodes[name].dtype == col.dtype and nodes[name].tolist() == col.tolist(), (what, name)
    assert len(summary) == 1 and summary.columns.tolist() == list(want_s), what
    for name, value in want_s.items():
        if isinstance(value, float):
            same_bits(summary[name].to_numpy(), np.array([value]), (what, name))
        else:
            assert summary[name][0] == value, (what, name)
    assert histogram.dtype == np.int64 and histogram.index.tolist() == list(range(R.BINS)), what
    assert np.array_equal(histogram.to_numpy(), want_h) and histogram.sum() == len(index) ** 2, what


def check_compare(a, b, tolerances=(1e-5, 0.0, 2.0 ** -12), floor=2.0 ** -30, ks=(1, 10, None)):
    """``a.compare(b)`` against the reference on the frames, for every top_k; both models unchanged."""
    frames_a, frames_b = groups_of(a.frame()), groups_of(b.frame())
    kws = [{"group": 1}, {"group": 2}] if len(frames_a) == 2 else [{}]
    probe = [list(f.index[[0, len(f) // 2, len(f) - 1]]) for f in frames_a]
    before = [[m.rows(p, **kw).to_numpy().copy() for p, kw in zip(probe, kws)] for m in (a, b)]
    bytes_before = (a.device_bytes, b.device_bytes)
    out = None
    for k in ks:
        n_min = min(len(f) for f in frames_a)
        k = n_min - 1 if k is None else k
        got = groups_of(a.compare(b, tolerances=tolerances, top_k=k, floor=floor)) if len(frames_a) == 2 else \
            [a.compare(b, tolerances=tolerances, top_k=k, floor=floor)]
        assert len(got) == len(frames_a)
        for g, fa, fb, kw in zip(got, frames_a, frames_b, kws):
            index, kk = fa.index, min(k, len(fa) - 1)
            ids = [R.id_table(m.most_similar(list(index), kk, **kw), index, kk) for m in (a, b)]
            want = R.model(fa.to_numpy(), fb.to_numpy(), index, tolerances, floor, (ids[0], ids[1], kk))
            check_frames(g, want, index, (k, kw))
        out = got
    none = a.compare(b, tolerances=(), top_k=None)
    for g, fa, fb in zip(groups_of(none) if len(frames_a) == 2 else [none], frames_a, frames_b):
        check_frames(g, R.model(fa.to_numpy(), fb.to_numpy(), fa.index, (), 0.0), fa.index, "no lists")
    after = [[m.rows(p, **kw).to_numpy() for p, kw in zip(probe, kws)] for m in (a, b)]
    for x, y in zip(before, after):
        for u, v in zip(x, y):
            assert np.array_equal(B.bits(u), B.bits(v))                      # both models answer as before
    at_rest = HipOps.pool_stats()                           # (the calls above also warmed the pool's size classes)
    a.compare(b, tolerances=tolerances, top_k=k, floor=floor)
    a.compare(b, tolerances=(), top_k=None)
    assert (a.device_bytes, b.device_bytes) == bytes_before and HipOps.pool_stats() == at_rest   # the temporaries are gone
    return out


def test_f32_kept_against_fp16_kept(graph):
    a, b = fit("SimRank", graph), fit("SimRank", graph, storage_precision="fp16")
    try:
        summary, nodes, _ = check_compare(a, b)[0]
        assert summary["differing"][0] > 0 and summary["max_rel"][0] > 0 and summary["max_abs"][0] < 0.01
    finally:
        a.release(), b.release()


def test_f32_compact_against_f64_kept(graph):
    a, b = fit("SimRank", graph, then="compact"), fit("SimRank", graph, storage_precision="f64")
    try:
        summary, _, _ = check_compare(a, b)[0]
        assert summary["differing"][0] > 0 and summary["max_abs"][0] < 1e-5
    finally:
        a.release(), b.release()


def test_a_local_world_against_a_loaded_model(graph, tmp_path):
    a, b = fit("SimRank", graph, world=3), fit("SimRank", graph, then="load", tmp_path=tmp_path)
    try:
        check_compare(a, b)
    finally:
        a.release(), b.release()


def test_two_and_three_updates(graph):
    a, b = fit("SimRank", graph, iterations=2), fit("SimRank", graph, iterations=3)
    try:
        summary, nodes, _ = check_compare(a, b)[0]
        assert summary["over@1e-05"][0] > 0 and summary["identical_lists"][0] < len(nodes) and nodes["overlap"].max() <= len(nodes) - 1
    finally:
        a.release(), b.release()


def test_a_model_against_itself(graph):
    a = fit("SimRank", graph)
    try:
        summary, nodes, histogram = check_compare(a, a)[0]
        assert summary["differing"][0] == 0 and summary["max_abs"][0] == 0.0 and summary["max_rel"][0] == 0.0
        n = len(nodes)
        assert 500 < n <= 600 and summary["identical_lists"][0] == n and histogram[0] == n * n
        assert (nodes["max_abs"] == 0.0).all() and (nodes["differing"] == 0).all()
        assert nodes["at"].tolist() == [nodes.index[0]] * n
    finally:
        a.release()


def test_a_bipartite_pair_returns_two_triples():
    df = bipartite_random(33, 65, 0.15, 12)
    a = fit("BipartiteSimRankPP", df, strict_reference=False)
    b = fit("BipartiteSimRankPP", df, then="compact-fp16", strict_reference=False)
    try:
        got = a.compare(b)
        assert isinstance(got, tuple) and len(got) == 2 and all(len(t) == 3 for t in got)
        assert [len(t[1]) for t in got] == [33, 65]
        check_compare(a, b)
    finally:
        a.release(), b.release()
