"""libsimrank_diverse.so at its C interface, on the blocks of tests/blocks.py: asymmetric, both signs, dyadic and wide, the
padding a sentinel above every value: a sentinel that is read wins its pen and shows up in the penalties and the picks.
All four layouts with the strides and bases of ``blocks.variants``, shapes with a ragged last quad and on both sides of
the 1024-candidate chunk, ``row_pos`` random into the block's rows (and NULL), ``col_pos`` NULL and a permutation with one
entry outside the block, bands that hold -inf, NaN, +inf, both zeros and plateaus of equal scores longer than a wave, on
16 bytes and off them.  All four outputs, the empty slots and the guard row are compared bit for bit with
tests/diverse_ref.py.  Greedy picks are prefix-consistent: the reference runs once at the largest k and is cut for the
smaller ones.  The lists entry point runs on synthetic tables against their dense P."""
import numpy as np
import pytest

from simrank_amd import _diverse
from tests import blocks as B
from tests import diverse_ref as D
from tests.test_gpu_companion_blocks import INVALID, Dev, dev, device, out_of, same_bits  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SHAPES = [(7, 1), (8, 33), (70, 129), (9, 1023), (8, 1025), (7, 2050)]
DS = (0.0, 0.25, 1.0)
SPECIAL = np.array([-np.inf, np.nan, np.inf, 0.0, -0.0])
FILL = 1e300                                       # what every float64 output holds before the call
MANY = 1100                                        # more candidates than this: the rows that are picked to the end are sparse


def make_band(rng, n_out, sparse):
    """float64 [5, n_out]: random dyadic scores of both signs with the special values sprinkled in; a plateau (one value
    over a stretch longer than a wave, or the whole row) with a few better and worse; only special values; both zeros
    only; a row without any candidate.  ``sparse``: at most ~260 live candidates per row, across the whole row (the
    others -inf), so that picking to the end stays short."""
    band = np.empty((5, n_out))
    band[0] = rng.integers(-32, 33, size=n_out) / 8.0
    at = rng.random(n_out) < 0.15
    band[0, at] = rng.choice(SPECIAL, size=int(at.sum()))
    band[1] = 1.5
    lo = int(rng.integers(0, max(1, n_out - 150)))
    band[1, :lo] = rng.integers(-8, 24, size=lo) / 8.0
    band[1, lo + 150:] = rng.integers(-8, 24, size=max(0, n_out - lo - 150)) / 8.0
    band[2] = rng.choice(SPECIAL, size=n_out)
    band[3] = rng.choice([0.0, -0.0], size=n_out)
    band[4] = rng.choice([-np.inf, np.nan], size=n_out)
    if sparse:
        for q in range(4):
            keep = np.zeros(n_out, dtype=bool)
            keep[rng.choice(n_out, size=110, replace=False)] = True
            if q == 1:
                keep[lo:lo + 150] = True                                   # (the plateau stays whole)
            band[q, ~keep] = -np.inf
    return band


def call_pick(dev, lib, S, blk, row_pos, col_pos, band_dev, ld, n_sets, n_out, k, d, what):
    """One call with pre-filled, over-long outputs and a guard row -> (idx, score, pen, val) [n_sets + 1, k]."""
    outs = [out_of(dev, (n_sets + 1, k), np.int32, -7)] + [out_of(dev, (n_sets + 1, k), np.float64, FILL) for _ in range(3)]
    work = dev.put(np.full(max(1, _diverse.load().simrank_diverse_workspace_bytes(n_sets, n_out) // 8), np.nan))
    _diverse.check(lib.simrank_diverse_pick(
        S, blk.layout, blk.stride, blk.n_rows, blk.n_cols, None if row_pos is None else dev.put(row_pos),
        None if col_pos is None else dev.put(col_pos), n_out, band_dev, ld, n_sets, k, 1.0 - d, d,
        *[o[0] for o in outs], work, dev.ops.stream), str(what))
    return [dev.get(ptr, host) for ptr, host in outs]


def check_outputs(got, want, n_sets, k, what):
    """The first k picks of the reference (run at a k at least as large), the guard row untouched."""
    for g, w, fill in zip(got, want, (-7, FILL, FILL, FILL)):
        same_bits(g[:n_sets], np.ascontiguousarray(w[:n_sets, :k]), what)
        assert (g[n_sets] == fill).all(), (what, "guard row")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_pick_is_the_statement(dev, layout, shape):
    lib = _diverse.load()
    n_rows, n_cols = shape
    n_out = n_cols
    i = SHAPES.index(shape)
    rng = np.random.default_rng([layout, i])
    sparse = n_out > MANY
    band = make_band(rng, n_out, sparse)
    n_sets = len(band)
    rows = rng.integers(0, n_rows, size=n_out).astype(np.int32)
    perm = rng.permutation(n_cols).astype(np.int32)
    if n_cols > 1:
        perm[n_cols // 2] = n_cols                                         # one mapped column outside the block: never read
    k_all = max(n_out + 3, 5)                                              # (the reference runs once, at the largest k)
    wants, penalised = {}, False                   # (a block's values do not depend on its stride: one reference per map and d)
    for tag, stride, base in B.variants(layout, n_rows, n_cols):
        blk = B.make_block(layout, n_rows, n_cols, stride, i, kind=("dyadic", "wide")[i % 2])
        A = blk.A
        S = dev.put(blk.raw, base)
        for col_pos in (None, perm):
            cols = np.arange(n_out) if col_pos is None else col_pos.astype(np.int64)
            ok = cols < n_cols
            M = np.full((n_rows, n_out), np.nan)
            M[:, ok] = A[:, cols[ok]]
            for d in DS:
                if (col_pos is None, d) not in wants:
                    want = wants[(col_pos is None, d)] = D.band_picks(band, lambda b: M[rows[b]], k_all, d)
                    assert (want[0][[1, 3], 0] >= 0).all() and (want[0][4] == -1).all()
                    assert not (np.abs(want[2]) >= blk.sentinel).any()     # (a sentinel that is read passes every pen)
                    penalised |= bool((want[2] > 0).any())
            # the band on 16 bytes with an even leading dimension (16-byte moves), and 8 bytes in with an odd one
            for ld, shift in ((n_out + (n_out & 1) + 2, 0), (n_out + (1 - (n_out & 1)) + 2, 8)):
                host = np.full((n_sets + 1, ld), np.inf)                   # padding and guard row: +inf would win every pick
                host[:n_sets, :n_out] = band
                band_dev = dev.put(host, shift)
                for d in DS:
                    what = (layout, shape, tag, col_pos is None, ld, d)
                    for k in (1, 5, n_out, n_out + 3):
                        if sparse or k <= 5 or shift == 0:                 # (the dense full-length picks once per block)
                            got = call_pick(dev, lib, S, blk, rows, col_pos, band_dev, ld, n_sets, n_out, k, d, what)
                            check_outputs(got, wants[(col_pos is None, d)], n_sets, k, (what, k))
        # row_pos NULL: candidate b reads row b; past the block's rows nothing is read and no pen moves
        if n_out <= MANY:
            R = np.full((n_out, n_out), np.nan)
            R[:min(n_rows, n_out)] = A[:min(n_rows, n_out), :n_out]
            want = D.band_picks(band, lambda b: R[b], 5, 0.25)
            check_outputs(call_pick(dev, lib, S, blk, None, None, dev.put(band), n_out, n_sets, n_out, 5, 0.25, "no row_pos"),
                          want, n_sets, 5, (layout, shape, tag, "no row_pos"))
        dev.release()
    assert penalised or n_out == 1                                         # (the penalties were at work)


@pytest.mark.parametrize("kk", [1, 7, 50])
def test_pick_lists_is_the_statement_on_the_dense_p(dev, kk):
    lib, st = _diverse.load(), dev.ops.stream
    n = 70
    rng = np.random.default_rng(kk)
    ids = np.full((n, kk), -1, dtype=np.int32)
    vals = np.zeros((n, kk))
    for a in range(n):
        others = np.delete(np.arange(n), a)
        m = int(rng.integers(0, kk + 1)) if a % 3 else kk                  # lists that are full, short and empty
        slots = np.sort(rng.choice(kk, size=min(m, n - 1), replace=False))  # (-1 slots in the middle of a list too)
        ids[a, slots] = rng.choice(others, size=slots.size, replace=False)
        vals[a, slots] = rng.integers(-16, 64, size=slots.size) / 64.0
    if kk > 1:
        ids[3, 0], vals[3, 0] = n + 5, 9.0                                  # an id outside 0 .. n - 1: an empty slot
    diag = rng.integers(1, 64, size=n) / 64.0
    P = D.dense_p(ids, vals, diag)
    assert not np.array_equal(P, P.T)
    band = make_band(rng, n, False)
    n_sets = len(band)
    ids_dev, vals_dev, diag_dev = dev.put(ids), dev.put(vals), dev.put(diag)
    for ld, shift in ((n + 2, 0), (n + 1, 8)):
        host = np.full((n_sets + 1, ld), np.inf)
        host[:n_sets, :n] = band
        band_dev = dev.put(host, shift)
        for d in DS:
            want = D.band_picks(band, lambda b: P[b], n + 3, d)
            for k in (1, 5, n, n + 3):
                outs = [out_of(dev, (n_sets + 1, k), np.int32, -7)] + [out_of(dev, (n_sets + 1, k), np.float64, FILL) for _ in range(3)]
                work = dev.put(np.full(lib.simrank_diverse_workspace_bytes(n_sets, n) // 8, np.nan))
                _diverse.check(lib.simrank_diverse_pick_lists(ids_dev, vals_dev, diag_dev if d else None, n, kk, band_dev, ld,
                                                              n_sets, k, 1.0 - d, d, *[o[0] for o in outs], work, st), "lists")
                check_outputs([dev.get(p, h) for p, h in outs], want, n_sets, k, ("lists", kk, ld, d, k))
            if d:
                assert (want[2] > 0).any()


def test_bad_arguments_are_refused_without_a_device_call(dev):
    lib = _diverse.load()
    S, band, work, idx, score, pen, val = (dev.put(np.zeros(16)) for _ in range(7))
    args = lambda **kw: [kw.get("S", S), kw.get("layout", 3), 4, 4, 4, None, None, 4, kw.get("band", band), kw.get("ld", 4), 1,
                         kw.get("k", 1), 0.5, kw.get("lam", 0.5), idx, score, pen, val, kw.get("work", work), dev.ops.stream]
    for bad in (dict(layout=7), dict(S=None), dict(band=None), dict(ld=3), dict(k=0), dict(lam=1.25), dict(lam=float("nan")),
                dict(work=None), dict(band=band + 4)):
        assert lib.simrank_diverse_pick(*args(**bad)) == INVALID, bad
        assert lib.simrank_diverse_last_error()
    assert lib.simrank_diverse_pick_lists(S, S, None, 4, -1, band, 4, 1, 1, 0.5, 0.5, idx, score, pen, val, work,
                                          dev.ops.stream) == INVALID
    assert lib.simrank_diverse_pick(*args()) == 0                          # (the same arguments in order are accepted)
    dev.ops.synchronize()
    assert dev.get(idx, np.zeros(4, dtype=np.int32))[0] == 0               # all scores 0: the first candidate
