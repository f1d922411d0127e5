"""libsimrank_exemplars.so and ``exemplars`` on a real MI355X.

Kernel level, on synthetic blocks (tests/blocks.py; padding holds a finite sentinel above every value, which a kernel that
reads padding would add to a gain or write into the cover): ``gains`` in all four layouts with the strides and bases of
``blocks.variants``, on the column counts at both sides of a quad, a panel, a wave's 256 columns and a workgroup's pass
of 1024 (and four passes: the unrolled loop), with every row (NULL) and with scattered lists that repeat rows and name
rows outside on both sides, against covers of zeros, above every element, equal to elements (the strict ``>``) and mixed.
On ``dyadic`` blocks every sum is exact, so a gain equals ``math.fsum`` of its terms bit for bit; on ``wide`` blocks it
equals ``exemplars_ref.ordered_sum`` (the header's order restated) bit for bit and lies inside the stated bound.  Guard
words after every output, a second run with the same bits, more listed rows than the grid cap.  Past one unrolled trip:
ten widths from 3 075 to 12 289 columns at which a thread makes two and three unrolled trips, an unrolled trip and then
single quads, and the threads of one wave part ways at the unrolled bound.  ``cover`` with lists of 1, 2 and 65 rows
against ``exemplars_ref.block_cover``, the vector bit for bit and the counters exact from a start that is not zero, and
on more columns than the grid's first turn holds.

Model level: for every storage, a ``LocalWorld(3)``, compact, loaded and pruned models and both bipartite groups,
``lazy=True`` (with ``BATCH`` cut to 3) equals ``lazy=False`` in everything but ``evaluated``; ``coverage`` and
``raised`` equal the NumPy statement on ``model.rows`` of the device's own picks; every gain lies within the bound of the
exact gain on ``model.frame()`` and every pick is greedy up to twice that bound; ``given`` is honoured and the picks seed
``kmedoids``.  On a fit whose iterates are dyadic the picks and gains equal ``exemplars_ref.greedy`` on the frame bit for
bit, exact ties included."""
import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _exemplars, synth
from tests import blocks as B
from tests import exact as X
from tests import exemplars_ref as ER
from tests.graphs import bipartite_random
from tests.test_exemplars_cpu import DYADIC_K
from tests.test_gpu_cluster import VARIANTS, as_groups, dev, device, make_model  # noqa: F401 (fixtures)
from tests.test_gpu_companion_blocks import same_bits

pytestmark = pytest.mark.gpu

GUARD_F64 = 1e300
GUARD_U32 = 0xA5A5A5A5
N_COLS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
N_ROWS = (1, 9, 70)
OUTSIDE = (-1, -2 ** 31, 2 ** 31 - 1)


# ---- the calls -------------------------------------------------------------------------------------------------------------
def run_gains(dev, S, layout, stride, n_rows, n_cols, rows, cover_dev):
    """One call of the C entry into a pre-filled output one element longer than it has to be, as the device left it."""
    n_list = n_rows if rows is None else len(rows)
    out_h = np.full(n_list + 1, GUARD_F64)
    out = dev.put(out_h)
    rows_dev = None if rows is None else dev.put(np.ascontiguousarray(rows, dtype=np.int32))
    _exemplars.check(_exemplars.load().simrank_exemplars_gains(S, layout, stride, n_rows, n_cols, rows_dev, n_list, cover_dev,
                                                               out, dev.ops.stream), "gains")
    return dev.get(out, out_h)


def run_cover(dev, S, layout, stride, n_rows, n_cols, rows, cover, raised):
    """One call of the C entry: (cover and the word after it, the counters and the word after them)."""
    cover_h = np.append(np.asarray(cover, dtype=np.float64), GUARD_F64)
    raised_h = np.append(np.asarray(raised, dtype=np.uint32), np.uint32(GUARD_U32))
    cover_dev, raised_dev = dev.put(cover_h), dev.put(raised_h)
    _exemplars.check(_exemplars.load().simrank_exemplars_cover(
        S, layout, stride, n_rows, n_cols, dev.put(np.ascontiguousarray(rows, dtype=np.int32)), len(rows), cover_dev,
        raised_dev, dev.ops.stream), "cover")
    return dev.get(cover_dev, cover_h), dev.get(raised_dev, raised_h)


def block_of(layout, n_rows, n_cols, stride, seed, kind):
    """``blocks.make_block``; a dyadic block of more columns than the binary16 pool has values (4 094) is drawn with
    repeats by ``blocks.make_long``: nothing here needs a row's values distinct."""
    if kind == "dyadic" and n_cols > 4000:
        return B.make_long(layout, n_rows, n_cols, stride, seed)
    return B.make_block(layout, n_rows, n_cols, stride, seed, kind=kind)


def covers_of(A, rng):
    """name -> cover [n_cols], each >= +0.0 and free of NaN, every value one the block's grid holds: zeros; above every
    element; a row's own positive elements (that row gains exactly nothing: the strict ``>``); elements of random rows
    in half the columns."""
    n_rows, n_cols = A.shape
    r0 = int(rng.integers(n_rows))
    pick = np.abs(A[rng.integers(0, n_rows, size=n_cols), np.arange(n_cols)])
    return {"zeros": np.zeros(n_cols), "above": np.full(n_cols, float(np.abs(A).max()) * 2 + 1.0),
            "a row": np.where(A[r0] > 0, A[r0], 0.0), "mixed": np.where(rng.random(n_cols) < 0.5, 0.0, pick)}, r0


def listed(rng, n_rows, m):
    """m listed rows: scattered, with repeats, three of them outside the block."""
    rows = rng.integers(0, n_rows, size=m).astype(np.int64)
    rows[[1, m // 2, m - 1]] = [n_rows, OUTSIDE[0], OUTSIDE[int(rng.integers(1, 3))]]
    return rows


def want_gains(A, rows, cover, kind):
    """The reference per kind: the exact sum on dyadic blocks (which the restated order must reach as well), the restated
    order on wide ones, checked against the bound."""
    want = ER.block_gains(A, rows, cover)
    for r, w in zip(range(A.shape[0]) if rows is None else rows, want):
        if not 0 <= r < A.shape[0]:
            assert np.isnan(w)
            continue
        t = ER.terms(A[r], cover)
        if kind == "dyadic":
            assert w == ER.exact_sum(t)
        else:
            assert abs(w - ER.exact_sum(t)) <= ER.bound(t)
    return want


# ---- 1. gains on synthetic blocks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_gains_equal_the_reference(dev, layout):
    gained = nothing = 0
    for ri, n_rows in enumerate(N_ROWS):
        for ci, n_cols in enumerate(N_COLS):
            kind = ("dyadic", "wide")[(ri + ci) % 2]
            variants = B.variants(layout, n_rows, n_cols)
            blk = block_of(layout, n_rows, n_cols, variants[0][1], 500 + ri * 100 + ci, kind)
            A = blk.A
            rng = np.random.default_rng([ri, ci, layout, 4])
            covers, r0 = covers_of(A, rng)
            rows = listed(rng, n_rows, 21)
            want = {name: (want_gains(A, None, c, kind), want_gains(A, rows, c, kind)) for name, c in covers.items()}
            assert not want["above"][0].any() and want["a row"][0][r0] == 0.0 and not np.signbit(want["above"][0]).any()
            gained += int((want["mixed"][0] > 0).sum())
            nothing += int((want["mixed"][0] == 0).sum())
            for tag, stride, base in variants:
                S = dev.put(B.encode(layout, A, stride, blk.sentinel).tobytes(), base)
                for name, c in covers.items():
                    what = (layout, kind, n_rows, n_cols, tag, name)
                    # (the "offset" variants also move the cover off 16 bytes: the element-by-element path reads it)
                    cover_dev = dev.put(np.append(c, GUARD_F64), 8 if tag == "offset" else 0)
                    got = run_gains(dev, S, layout, stride, n_rows, n_cols, None, cover_dev)
                    same_bits(got, np.append(want[name][0], GUARD_F64), what + ("every row",))
                    got_l = run_gains(dev, S, layout, stride, n_rows, n_cols, rows, cover_dev)
                    same_bits(got_l, np.append(want[name][1], GUARD_F64), what + ("listed",))
                    again = run_gains(dev, S, layout, stride, n_rows, n_cols, rows, cover_dev)
                    assert np.array_equal(B.bits(got_l), B.bits(again)), what      # a second run: the same bits
                    same_bits(dev.get(cover_dev, np.append(c, GUARD_F64)), np.append(c, GUARD_F64), what + ("cover",))
                dev.release()
    assert gained >= 200 and nothing >= 3


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_nan_inf_and_negative_zero_entries(dev, layout):
    from tests.test_gpu_groups import planted
    n_rows, n_cols = 9, 150
    nan, inf = float("nan"), float("inf")
    plant = {(2, c): nan for c in range(n_cols)}                           # row 2 is NaN everywhere: it gains +0.0
    plant.update({(4, 7): nan, (4, 8): -0.0, (4, 9): 0.0, (5, 8): -0.0, (6, 140): nan})
    if layout != B.PANEL_F16:
        plant.update({(3, 11): inf, (7, 11): inf, (3, 149): -inf})
    A, stride, base, raw = planted(layout, n_rows, n_cols, plant)
    S = dev.put(raw, base)
    zeros = np.zeros(n_cols)
    for cover in (zeros, np.where(np.nan_to_num(A[3], nan=0.0, posinf=1.0, neginf=0.0) > 0, 0.5, 0.0)):
        cover_dev = dev.put(cover)
        want = ER.block_gains(A, None, cover, total=ER.exact_sum)
        assert want[2] == 0.0 and not np.isnan(want).any() and (layout == B.PANEL_F16 or want[3] == want[7] == inf)
        same_bits(run_gains(dev, S, layout, stride, n_rows, n_cols, None, cover_dev), np.append(want, GUARD_F64), (layout, "gains"))
    # applied: a NaN never covers, -0.0 never raises +0.0, +inf covers and is then never passed (inf > inf is false)
    rows = [2, 4, 5, 3, 7, 6]
    want_c, want_r = ER.block_cover(A, rows, zeros, np.zeros(len(rows)))
    got_c, got_r = run_cover(dev, S, layout, stride, n_rows, n_cols, rows, zeros, np.zeros(len(rows)))
    same_bits(got_c, np.append(want_c, GUARD_F64), (layout, "cover"))
    assert got_r.tolist() == want_r.tolist() + [GUARD_U32] and got_r[0] == 0 and not np.signbit(got_c[:n_cols]).any()
    assert layout == B.PANEL_F16 or (got_c[11] == inf and not np.isnan(got_c).any())
    cover_dev = dev.put(want_c)
    want = ER.block_gains(A, None, want_c, total=ER.exact_sum)
    assert not want[rows].any()
    same_bits(run_gains(dev, S, layout, stride, n_rows, n_cols, None, cover_dev), np.append(want, GUARD_F64), (layout, "after"))


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_more_listed_rows_than_the_grid_cap(dev, layout):
    """One workgroup takes several turns: the list is longer than twice SIMRANK_EXEMPLARS_GRID_CAP."""
    n_rows, n_cols = 9, 257
    _, stride, base = B.variants(layout, n_rows, n_cols)[0]
    blk = B.make_block(layout, n_rows, n_cols, stride, 77, kind="wide")
    rng = np.random.default_rng([layout, 77])
    rows = listed(rng, n_rows, 2 * _exemplars.GRID_CAP + 37)
    cover = covers_of(blk.A, rng)[0]["mixed"]
    per_row = np.append(ER.block_gains(blk.A, None, cover), np.nan)
    want = per_row[np.where((rows >= 0) & (rows < n_rows), rows, n_rows)]
    S = dev.put(blk.raw, base)
    got = run_gains(dev, S, layout, stride, n_rows, n_cols, rows, dev.put(cover))
    same_bits(got, np.append(want, GUARD_F64), layout)
    assert np.isnan(want).sum() >= 3 and (want > 0).sum() > 2 * _exemplars.GRID_CAP


CHUNK = 4 * _exemplars.THREADS                     # columns the workgroup covers in one pass
UNROLL = 4                                         # passes of one unrolled trip
LONG_COLS = (3075, 3076, 3077, 4100, 5001, 7171, 7172, 7173, 8193, 12289)
LONG_DYADIC = (3076, 5001, 7173)


def trips_of(n_cols):
    """gains_kernel<L, true>'s three column loops restated: per thread its (unrolled trips, single-quad trips, element
    trips) -> int [THREADS, 3]."""
    out = np.zeros((_exemplars.THREADS, 3), dtype=np.int64)
    for t in range(_exemplars.THREADS):
        c0 = 4 * t
        while c0 + (UNROLL - 1) * CHUNK + 4 <= n_cols:
            c0, out[t, 0] = c0 + UNROLL * CHUNK, out[t, 0] + 1
        while c0 + 4 <= n_cols:
            c0, out[t, 1] = c0 + CHUNK, out[t, 1] + 1
        while c0 < n_cols:
            c0, out[t, 2] = c0 + CHUNK, out[t, 2] + 1
    return out


def check_the_long_widths_reach_every_regime():
    trips ={n: trips_of(n) for n in LONG_COLS}
    unrolled = {n: t[:, 0] for n, t in trips.items()}
    assert not unrolled[3075].any() and unrolled[3076].tolist() == [1] + [0] * 255 == unrolled[3077].tolist()
    assert (unrolled[7171] == 1).all() and unrolled[7172].tolist() == [2] + [1] * 255 == unrolled[7173].tolist()
    split = [n for n in LONG_COLS if unrolled[n][:64].min() != unrolled[n][:64].max()]   # threads of one wave part ways
    assert split == [3076, 3077, 7172, 7173]
    assert [n for n in LONG_COLS if unrolled[n].max() >= 2] == [7172, 7173, 8193, 12289]
    assert (unrolled[8193] == 2).all() and (unrolled[12289] == 3).all()
    for n in (8193, 12289):                                                 # whole trips and one column: thread 0's
        assert trips[n][:, 1].sum() == 0 and trips[n][:, 2].tolist() == [1] + [0] * 255
    then_single = [n for n in LONG_COLS if ((trips[n][:, 0] >= 1) & (trips[n][:, 1] >= 1)).any()]
    assert then_single == [4100, 5001, 7171, 7172, 7173]                    # (at 3076 thread 0 ends at 4096: nothing is left)
    assert trips[4100][:, 1].tolist() == [1] + [0] * 255 and not trips[4100][:, 2].any()     # no partial quad
    assert trips[5001][:, 1].sum() == 226 and trips[5001][226].tolist() == [1, 0, 1]         # and one
    assert trips[3077][:, 2].sum() == 1 and trips[7173][:, 2].sum() == 1


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_gains_past_one_unrolled_trip(dev, layout):
    """Widths at which a thread makes a second unrolled trip, an unrolled trip and then single quads, and at which the
    threads of a wave part ways at the unrolled bound (``check_the_long_widths_reach_every_regime``); on the wide blocks
    a running sum holds up to thirteen terms, so their order shows.  The crooked and offset variants take the element
    path over 4 to 13 passes."""
    check_the_long_widths_reach_every_regime()
    n_rows = 3
    rows = np.array([2, 0, 2, n_rows, 1, -1], dtype=np.int64)
    for ci, (n_cols, kind) in enumerate([(n, "wide") for n in LONG_COLS] + [(n, "dyadic") for n in LONG_DYADIC]):
        variants = B.variants(layout, n_rows, n_cols)
        blk = block_of(layout, n_rows, n_cols, variants[0][1], 1300 + ci, kind) if kind == "wide" else \
            B.make_long(layout, n_rows, n_cols, variants[0][1], 1300 + ci)
        A = blk.A
        rng = np.random.default_rng([ci, layout, 6])
        covers = {name: c for name, c in covers_of(A, rng)[0].items() if name in ("zeros", "mixed")}
        want = {name: (want_gains(A, None, c, kind), want_gains(A, rows, c, kind)) for name, c in covers.items()}
        assert (want["mixed"][0] > 0).all()
        for tag, stride, base in variants:
            S = dev.put(B.encode(layout, A, stride, blk.sentinel).tobytes(), base)
            for name, c in covers.items():
                what = (layout, kind, n_cols, tag, name)
                cover_dev = dev.put(np.append(c, GUARD_F64), 8 if tag == "offset" else 0)
                got = run_gains(dev, S, layout, stride, n_rows, n_cols, None, cover_dev)
                same_bits(got, np.append(want[name][0], GUARD_F64), what + ("every row",))
                got_l = run_gains(dev, S, layout, stride, n_rows, n_cols, rows, cover_dev)
                same_bits(got_l, np.append(want[name][1], GUARD_F64), what + ("listed",))
                again = run_gains(dev, S, layout, stride, n_rows, n_cols, rows, cover_dev)
                assert np.array_equal(B.bits(got_l), B.bits(again)), what
            dev.release()


# ---- 2. cover on synthetic blocks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_cover_equals_the_reference(dev, layout):
    raised_some = 0
    for ri, n_rows in enumerate(N_ROWS):
        for ci, n_cols in enumerate(N_COLS):
            variants = B.variants(layout, n_rows, n_cols)
            blk = block_of(layout, n_rows, n_cols, variants[0][1], 900 + ri * 100 + ci, ("wide", "dyadic")[(ri + ci) % 2])
            A = blk.A
            rng = np.random.default_rng([ri, ci, layout, 5])
            start = covers_of(A, rng)[0]["mixed"]
            cases = []
            for m in (1, 2, 65):
                rows = rng.integers(0, n_rows, size=m).astype(np.int64)    # (repeats: a row applied again raises nothing)
                if m == 65:
                    rows[[3, 40, 64]] = [n_rows, OUTSIDE[0], OUTSIDE[2]]
                first = rng.integers(0, 1000, size=m) * (m != 2)           # counters that do not start at zero
                cases.append((rows, first, ER.block_cover(A, rows, start, first)))
                raised_some += int((cases[-1][2][1] - first > 0).sum())
            for tag, stride, base in variants:
                S = dev.put(B.encode(layout, A, stride, blk.sentinel).tobytes(), base)
                for rows, first, (want_c, want_r) in cases:
                    what = (layout, n_rows, n_cols, tag, len(rows))
                    got_c, got_r = run_cover(dev, S, layout, stride, n_rows, n_cols, rows, start, first)
                    same_bits(got_c, np.append(want_c, GUARD_F64), what + ("cover",))
                    assert got_r.tolist() == want_r.tolist() + [GUARD_U32], what
                dev.release()
    assert raised_some >= 100


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_cover_second_turn_of_the_column_loop(dev, layout):
    """More columns than GRID_CAP workgroups of THREADS hold: the first 257 threads of the grid take a second turn."""
    first_turn = _exemplars.GRID_CAP * _exemplars.THREADS
    n_rows, n_cols = 2, first_turn + 257
    tag, stride, base = B.variants(layout, n_rows, n_cols)[0]
    blk = B.make_long(layout, n_rows, n_cols, stride, 41)
    A = blk.A
    rng = np.random.default_rng([layout, 41])
    start = covers_of(A, rng)[0]["mixed"]
    S = dev.put(blk.raw, base)
    for rows in ([1], [1, 0, 2, 1]):                                        # (row 2 is outside)
        first = rng.integers(1, 1000, size=len(rows))
        want_c, want_r = ER.block_cover(A, rows, start, first)
        got_c, got_r = run_cover(dev, S, layout, stride, n_rows, n_cols, rows, start, first)
        same_bits(got_c, np.append(want_c, GUARD_F64), (layout, rows, "cover"))
        assert got_r.tolist() == want_r.tolist() + [GUARD_U32], (layout, rows)
        # the expected counters rise in columns of the first turn and of the second
        cover = start.copy()
        for i, r in enumerate(rows):
            if r < n_rows:
                up = A[r] > cover
                assert up.sum() == want_r[i] - first[i]
                assert i > 1 or (up[:first_turn].any() and up[first_turn:].any()), (layout, rows, i)
                cover[up] = A[r][up]
        assert len(rows) == 1 or (want_r[2] == first[2] and want_r[3] == first[3])      # a row outside, a row again


# ---- 3. through the estimators ----------------------------------------------------------------------------------------------------
def exact_gains(S, cover):
    """(exact gain, bound) of every row of the dense S against ``cover``."""
    with np.errstate(invalid="ignore"):
        T = np.where(S > cover, S - cover, 0.0)
    exact = np.array([ER.exact_sum(t) for t in T])
    return exact, (S.shape[1] + 1) * 2.0 ** -52 * exact


def check_side(model, kw, f, k, monkeypatch, dyadic=False):
    index, n = f.index, len(f)
    S = f.to_numpy()
    rows_of = lambda labels: model.rows(list(labels), **kw).to_numpy()
    given = [index[i] for i in np.random.default_rng(n).choice(n, 3, replace=False)]
    out = None
    for giv in (None, given):
        at = [] if giv is None else index.get_indexer(giv).tolist()
        monkeypatch.setattr(_exemplars, "BATCH", 3)                         # picks take several rounds
        picks, coverage = model.exemplars(k, given=giv, lazy=True, **kw)
        monkeypatch.undo()
        plain, coverage_p = model.exemplars(k, given=giv, lazy=False, **kw)
        what = (kw, giv is not None)
        # the frames, and lazy against plain
        assert picks.index.tolist() == list(range(k)) and picks.index.name == "rank", what
        assert picks.columns.tolist() == ["exemplar", "gain", "raised", "evaluated"], what
        assert picks.dtypes.tolist()[1:] == [np.float64, np.int64, np.int64], what
        assert picks["exemplar"].tolist() == plain["exemplar"].tolist(), what
        same_bits(picks["gain"].to_numpy(), plain["gain"].to_numpy(), (what, "lazy gain"))
        assert picks["raised"].tolist() == plain["raised"].tolist(), what
        assert plain["evaluated"].tolist() == [n - len(at) - p for p in range(k)], what
        assert picks["evaluated"][0] == n - len(at) and (picks["evaluated"][1:] >= 1).all(), what
        assert picks["evaluated"].sum() < plain["evaluated"].sum(), what
        assert coverage.name == "coverage" and coverage.dtype == np.float64 and coverage.index.equals(index), what
        same_bits(coverage.to_numpy(), coverage_p.to_numpy(), (what, "lazy coverage"))
        picked = index.get_indexer(picks["exemplar"]).tolist()
        assert len(set(picked)) == k and not set(picked) & set(at), what       # given rows are never picked
        # coverage and raised: the NumPy statement on model.rows of the device's own picks
        R = rows_of([index[i] for i in at + picked])
        same_bits(coverage.to_numpy(), ER.coverage(R), (what, "coverage"))
        cover = np.zeros(n)
        for row in R[:len(at)]:
            ER.apply(row, cover)
        for p, row in enumerate(R[len(at):]):
            # the reported gain against the exact gain on the frame, and greedy up to rounding
            exact, bound = exact_gains(S, cover)
            c = picked[p]
            assert abs(picks["gain"][p] - exact[c]) <= bound[c], (what, p, picks["gain"][p], exact[c], bound[c])
            candidates = np.ones(n, dtype=bool)
            candidates[at + picked[:p]] = False
            best = int(np.argmax(np.where(candidates, exact, -1.0)))
            assert exact[c] >= exact[best] - 2 * bound[best], (what, p, exact[c], exact[best], bound[best])
            assert picks["raised"][p] == ER.apply(row, cover), (what, p)
        same_bits(cover, coverage.to_numpy(), (what, "cover"))
        assert picks["gain"][0] > 0 and picks["raised"][0] > 0 and (np.diff(picks["gain"].to_numpy()) <= 0).all(), what
        out = picks if giv is None else out
    labels, clusters, _ = model.kmedoids(out["exemplar"], max_iter=2, **kw)  # a Series of labels seeds kmedoids
    assert len(clusters) == k and labels.index.equals(index)
    if dyadic:
        want = ER.greedy(S, DYADIC_K)
        got, _ = model.exemplars(DYADIC_K, **kw)
        assert got["exemplar"].tolist() == index[want[0]].tolist()
        same_bits(got["gain"].to_numpy(), want[1], "frame: gain")
        assert got["raised"].tolist() == want[2].tolist()
    return out


def check_model(model, monkeypatch, k=12, dyadic=False):
    frames = as_groups(model.frame())
    groups = [{"group": 1}, {"group": 2}] if len(frames) == 2 else [{}]
    before = [f.to_numpy().copy() for f in frames]
    for f, kw in zip(frames, groups):
        check_side(model, kw, f, k, monkeypatch, dyadic)
    for f, b in zip(as_groups(model.frame()), before):
        assert np.array_equal(B.bits(f.to_numpy()), B.bits(b))                # the model is unchanged
    model.release()
    with pytest.raises(RuntimeError, match="released"):
        model.exemplars(1, **groups[0])


@pytest.fixture(scope="module")
def powerlaw():
    return synth.powerlaw_directed(300, 4.0, seed=11)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_simrankpp_on_a_power_law_graph(variant, powerlaw, tmp_path, monkeypatch):
    model = make_model("SimRankPP", powerlaw, variant, tmp_path)
    try:
        check_model(model, monkeypatch)
    finally:
        model.release()


@pytest.mark.parametrize("variant", ["f32-kept", "f64-kept", "world3-kept", "f32-compact-fp16"])
def test_bipartite_simrankpp(variant, tmp_path, monkeypatch):
    df = bipartite_random(90, 50, 0.06, 12)
    model = make_model("BipartiteSimRankPP", df, variant, tmp_path, strict_reference=False)
    try:
        check_model(model, monkeypatch, k=7)
    finally:
        model.release()


def test_a_pruned_model_is_answered_for_its_matrix_p(powerlaw, tmp_path, monkeypatch):
    model = make_model("SimRankPP", powerlaw, "f32-kept", tmp_path)
    try:
        model.prune(10)
        assert model.kept_neighbors == 10
        check_model(model, monkeypatch)
    finally:
        model.release()


@pytest.mark.parametrize("variant", ["f32-kept", "f64-kept", "world3-kept", "f32-compact"])
def test_a_fit_with_dyadic_iterates(variant, tmp_path, monkeypatch):
    """regular_graph(256, 4) with C = 0.5, as tests/test_gpu_groups.py fits it: the iterate lies on a dyadic grid, every
    float64 sum of its elements and of their differences is exact in any order, and greedy on the frame is the model's,
    the exact ties that tests/test_exemplars_cpu.py finds there included."""
    import contextlib
    import io
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
        check_model(est, monkeypatch, dyadic=True)
    finally:
        est.release()
