"""libsimrank_operator.so at its C interface, on the blocks of tests/blocks.py: asymmetric, both signs, the padding a
sentinel above every value, so that an element read from the wrong place changes a sum.

Bit for bit: on the dyadic blocks, with an X of small integers times powers of two, every product and every partial sum
in any order is exact in a double (tests/operator_ref.assert_exact shows it in integer arithmetic before the device
runs), so the device must give the bits of the NumPy product whatever its order of summation: all four layouts with the
strides and bases of ``blocks.variants`` (a panel stride above the rows, a row-major stride that breaks 16-byte
alignment, a base 4 / 8 bytes in), shapes on both sides of a strip, a tile and a panel, every column tile width and
both sides of d = 8, where the matrix-vector forms end, both directions, NULL and permuted maps, three (alpha, beta) with
powers of two, NaN in ``out`` where beta = 0, leading dimensions above d and a guard row; and, on the long blocks of
``operator_ref.LONG_CASES`` (``blocks.make_long``), with two and three tiles of the contraction per workgroup in each of
the three kernels, which no shape above reaches: there a part is one tile.  To a bound: on the wide blocks with a normal X, within K 2^-52 sum |S| |X| of the
NumPy product, and the same bits twice."""
import numpy as np
import pytest

from simrank_amd import _operator
from tests import blocks as B
from tests import operator_ref as R
from tests.test_gpu_companion_blocks import INVALID, Dev, dev, device, same_bits  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (70, 1100), (33, 65), (257, 31)]
DS = (1, 3, 8, 9, 32, 33, 64)                   # both sides of 8 (the matrix-vector forms end), 32 and 64 (column tiles)
SCALES = ((1.0, 0.0), (0.5, 1.0), (2.0, -1.0))
GUARD = 1e300


def effective(A, row_pos, col_pos, transpose):
    """The matrix the product multiplies by: A under the two maps (a position outside the block reads NaN), transposed."""
    n_rows, n_cols = A.shape
    rows = np.arange(n_rows) if row_pos is None else np.asarray(row_pos, dtype=np.int64)
    cols = np.arange(n_cols) if col_pos is None else np.asarray(col_pos, dtype=np.int64)
    ok_r, ok_c = (rows >= 0) & (rows < n_rows), (cols >= 0) & (cols < n_cols)
    E = np.full((n_rows, n_cols), np.nan)
    E[np.ix_(ok_r, ok_c)] = A[np.ix_(rows[ok_r], cols[ok_c])]
    return E.T if transpose else E


def call_apply(dev, lib, S, blk, row_pos, col_pos, transpose, X, d, alpha, beta, out0, what, ld_extra=3):
    """One call on X[:, :d] with leading dimensions above d, ``out0`` [n_out, d] what out holds before -> out [n_out, d];
    the padding of out and a guard row must still hold GUARD afterwards."""
    n_out = blk.n_cols if transpose else blk.n_rows
    n_in = blk.n_rows if transpose else blk.n_cols
    ld_x, ld_out = d + ld_extra, d + ld_extra + 1
    hx = np.full((max(n_in, 1), ld_x), GUARD)
    hx[:n_in, :d] = X[:, :d]
    ho = np.full((n_out + 1, ld_out), GUARD)
    ho[:n_out, :d] = out0
    out = dev.put(ho)
    work = dev.put(np.full(lib.simrank_operator_workspace_bytes(blk.n_rows, blk.n_cols, transpose, d) // 8, np.nan))
    _operator.check(lib.simrank_operator_apply(
        S, blk.layout, blk.stride, blk.n_rows, blk.n_cols, None if row_pos is None else dev.put(row_pos),
        None if col_pos is None else dev.put(col_pos), transpose, dev.put(hx), ld_x, d, alpha, beta, out, ld_out, work,
        dev.ops.stream), str(what))
    got = dev.get(out, ho)
    assert (got[n_out] == GUARD).all() and (got[:, d:] == GUARD).all(), (what, "guard")
    return np.ascontiguousarray(got[:n_out, :d])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_apply_is_the_numpy_product_bit_for_bit(dev, layout, shape):
    lib = _operator.load()
    n_rows, n_cols = shape
    i = SHAPES.index(shape)
    rng = np.random.default_rng([layout, i, 11])
    perms = (rng.permutation(n_rows).astype(np.int32), rng.permutation(n_cols).astype(np.int32))
    Xs = [R.exact_operand(rng, n_cols, max(DS), layout), R.exact_operand(rng, n_rows, max(DS), layout)]
    for tag, stride, base in B.variants(layout, n_rows, n_cols):
        blk = B.make_block(layout, n_rows, n_cols, stride, i, kind="dyadic")
        S = dev.put(blk.raw, base)
        for transpose in (0, 1):
            X = Xs[transpose]
            n_out = n_cols if transpose else n_rows
            for maps in ((None, None), perms, (perms[0], None), (None, perms[1])):
                E = effective(blk.A, maps[0], maps[1], transpose)
                R.assert_exact(E, X)
                P = E @ X
                for d in DS:
                    for alpha, beta in SCALES:
                        if maps[0] is None or maps[1] is None or (alpha, beta) == SCALES[1] or d in (3, 64):
                            out0 = (np.full((n_out, d), np.nan) if beta == 0.0
                                    else rng.integers(-64, 65, size=(n_out, d)) / 4.0)
                            R.assert_exact(E, X[:, :d], alpha, beta, out0)
                            want = alpha * P[:, :d] + (0.0 if beta == 0.0 else beta * out0)
                            what = (layout, shape, tag, transpose, maps[0] is None, maps[1] is None, d, alpha, beta)
                            got = call_apply(dev, lib, S, blk, maps[0], maps[1], transpose, X, d, alpha, beta, out0, what)
                            same_bits(got, want, what)
            dev.release()
            S = dev.put(blk.raw, base)
        dev.release()


@pytest.mark.parametrize("case", R.LONG_CASES, ids=R.LONG_IDS)
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_apply_over_several_tiles_per_part_bit_for_bit(dev, layout, case):
    """The shapes of ``operator_ref.LONG_CASES``: a workgroup walks two or three tiles of the contraction, so the prefetch
    of the next tile, the barriers between two tiles and a last part that is shorter than the others all run.  Same
    protocol as above; the split is asked of the library, not trusted."""
    lib = _operator.load()
    R.assert_long_cases_walk_several_tiles(lib)
    kernel, n_rows, n_cols, transpose, ds, _, _ = case
    i = R.LONG_CASES.index(case)
    rng = np.random.default_rng([layout, i, 14])
    perms = (rng.permutation(n_rows).astype(np.int32), rng.permutation(n_cols).astype(np.int32))
    n_out, n_in = (n_cols, n_rows) if transpose else (n_rows, n_cols)
    X = R.exact_operand(rng, n_in, max(ds), layout)
    for tag, stride, base in B.variants(layout, n_rows, n_cols):
        blk = B.make_long(layout, n_rows, n_cols, stride, i)
        S = dev.put(blk.raw, base)
        for maps in ((None, None), perms):
            E = effective(blk.A, maps[0], maps[1], transpose)
            R.assert_exact(E, X)
            P = E @ X
            for d in ds:
                tiles, parts, per, last = R.split_of(lib, case, d)
                assert per >= 2, (case, d, tiles, parts)
                for alpha, beta in SCALES[:2]:
                    out0 = (np.full((n_out, d), np.nan) if beta == 0.0 else rng.integers(-64, 65, size=(n_out, d)) / 4.0)
                    R.assert_exact(E, X[:, :d], alpha, beta, out0)
                    want = alpha * P[:, :d] + (0.0 if beta == 0.0 else beta * out0)
                    what = (layout, kernel, n_rows, n_cols, tag, transpose, maps[0] is None, d, alpha, beta, per, last)
                    got = call_apply(dev, lib, S, blk, maps[0], maps[1], transpose, X, d, alpha, beta, out0, what)
                    same_bits(got, want, what)
        dev.release()


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_apply_to_the_bound_on_wide_blocks_and_the_same_bits_twice(dev, layout):
    lib = _operator.load()
    for i, (n_rows, n_cols) in enumerate(SHAPES):
        rng = np.random.default_rng([layout, i, 12])
        perms = (rng.permutation(n_rows).astype(np.int32), rng.permutation(n_cols).astype(np.int32))
        for tag, stride, base in B.variants(layout, n_rows, n_cols):
            blk = B.make_block(layout, n_rows, n_cols, stride, i, kind="wide")
            S = dev.put(blk.raw, base)
            for transpose in (0, 1):
                n_out, n_in = (n_cols, n_rows) if transpose else (n_rows, n_cols)
                X = rng.standard_normal((n_in, 64))
                for maps in ((None, None), perms):
                    E = effective(blk.A, maps[0], maps[1], transpose)
                    for d in (3, 8, 64):
                        what = (layout, n_rows, n_cols, tag, transpose, maps[0] is None, d)
                        nan = np.full((n_out, d), np.nan)
                        got = call_apply(dev, lib, S, blk, maps[0], maps[1], transpose, X, d, 1.0, 0.0, nan, what)
                        want, bound = E @ X[:, :d], R.product_bound(E, X[:, :d])
                        err = np.abs(got - want)
                        print(what, "largest error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
                        assert (err <= bound).all(), what
                        again = call_apply(dev, lib, S, blk, maps[0], maps[1], transpose, X, d, 1.0, 0.0, nan, what)
                        same_bits(again, got, (what, "twice"))
            dev.release()


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_a_bad_position_poisons_exactly_its_sums(dev, layout):
    lib = _operator.load()
    n_rows, n_cols = 70, 129
    rng = np.random.default_rng([layout, 13])
    for tag, stride, base in B.variants(layout, n_rows, n_cols)[:1]:
        blk = B.make_block(layout, n_rows, n_cols, stride, 5, kind="dyadic")
        S = dev.put(blk.raw, base)
        rows, cols = np.arange(n_rows, dtype=np.int32), np.arange(n_cols, dtype=np.int32)
        bad_rows, bad_cols = rows.copy(), cols.copy()
        bad_rows[7], bad_cols[100] = n_rows, -1
        for transpose in (0, 1):
            n_out, n_in = (n_cols, n_rows) if transpose else (n_rows, n_cols)
            X = R.exact_operand(rng, n_in, 5, layout)
            X[3] = 0.0                                                       # (NaN x 0 is still NaN)
            for row_pos, col_pos in ((bad_rows, None), (None, bad_cols), (bad_rows, bad_cols)):
                E = effective(blk.A, row_pos, col_pos, transpose)
                with np.errstate(invalid="ignore"):
                    want = E @ X
                # the bad row poisons out[7] (or, transposed, every sum); the bad column every sum (or out[100])
                poisoned = np.isnan(want).all(axis=1)
                expect = np.zeros(n_out, dtype=bool)
                for pos, at, along_out in ((row_pos, 7, not transpose), (col_pos, 100, bool(transpose))):
                    if pos is not None:
                        expect |= (np.arange(n_out) == at) if along_out else True
                assert np.array_equal(poisoned, expect) and not np.isnan(want[~expect]).any()
                got = call_apply(dev, lib, S, blk, row_pos, col_pos, transpose, X, 5, 1.0, 0.0, np.zeros((n_out, 5)), layout)
                same_bits(got, want, (layout, transpose, row_pos is None, col_pos is None))
        dev.release()


def test_bad_arguments_are_refused_without_a_device_call(dev):
    lib = _operator.load()
    S, X, out, work = (dev.put(np.zeros(64)) for _ in range(4))
    args = lambda **kw: [kw.get("S", S), kw.get("layout", 3), kw.get("stride", 4), kw.get("n_rows", 4), 4, None, None,
                         kw.get("transpose", 0), kw.get("X", X), kw.get("ld_x", 2), kw.get("d", 2), 1.0, 0.0,
                         kw.get("out", out), kw.get("ld_out", 2), kw.get("work", work), dev.ops.stream]
    for bad in (dict(layout=7), dict(S=None), dict(X=None), dict(out=None), dict(work=None), dict(d=0), dict(d=65), dict(ld_x=1),
                dict(ld_out=1), dict(stride=3), dict(n_rows=-1), dict(transpose=3), dict(X=X + 4)):
        assert lib.simrank_operator_apply(*args(**bad)) == INVALID, bad
        assert lib.simrank_operator_last_error()
    assert lib.simrank_operator_apply(*args()) == 0                          # (the same arguments in order are accepted)
    dev.ops.synchronize()
    assert (dev.get(out, np.zeros(8)) == 0.0).all()
