"""The rule of leg 2's short path restated in NumPy (api.hip build_tiles / build_short_image), and graphs with prescribed row
lengths that sit at its edges (no GPU).  Shared by tests/leg2_short_worker.py, tests/exact.py and the exact tests: what a
test expects of "leg2_short_groups" / "leg2_short_taken" comes from here, never from the library."""
import numpy as np

from simrank_amd.ingest import CSR


def from_lengths(lengths, seed, K=None):
    """Rows of exactly these lengths, columns drawn without repetition; the caller's order (a plan keeps it with
    reorder = False, a graph made by HipOps.graph always).  `K`: the number of columns (None: as many as rows)."""
    n = len(lengths)
    K = n if K is None else K
    assert max(lengths, default=0) <= K
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(K, size=k, replace=False)).astype(np.int32) for k in lengths]
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(lengths)
    col = np.concatenate(rows + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    deg = np.asarray(lengths, dtype=np.float64)
    return CSR(n, K, rowptr, col, np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0))


def boundary_lengths(ragged=20):
    """Groups of four 32-row tiles (one workgroup each) at the edges of both widths, then a ragged last tile:
    0: rows of 0..8 entries, one tile wholly empty            short at 8 and at 16
    1: three tiles of <= 8, one tile with rows of exactly 9   general path at 8, short at 16
    2: rows of exactly 16 and fewer                           short at 16 only
    3: three tiles of <= 8, one tile with a row of 17         never short
    4: rows of exactly 8                                      short at both
    5: `ragged` rows of <= 8 (the ragged last tile)           short at both"""
    rng = np.random.default_rng(21)
    g0 = np.concatenate([rng.integers(0, 9, 32), np.full(32, 8), np.zeros(32, int), rng.integers(0, 9, 32)])
    # (no 32-row block above 256 entries: build_tiles would cut it, and a cut tile is never short)
    g1 = np.concatenate([rng.integers(0, 9, 64), np.full(16, 9), rng.integers(1, 9, 48)])
    g2 = np.concatenate([np.full(8, 16), rng.integers(0, 9, 24), rng.integers(0, 9, 96)])
    g2[40] = 16
    t17 = rng.integers(0, 9, 32)
    t17[5] = 17
    g3 = np.concatenate([rng.integers(0, 9, 32), t17, rng.integers(0, 9, 64)])
    g4 = np.full(128, 8)
    g5 = rng.integers(0, 9, ragged)                  # (drawn last: the 576 rows before it do not depend on `ragged`)
    return np.concatenate([g0, g1, g2, g3, g4, g5]).astype(int).tolist()


def heavy_row_lengths(heavy=400):
    """One row of `heavy` entries among rows of <= 8: its 32-row block is cut into pieces (tuning balance), which shifts the
    groups of four tiles behind it off the 128-row grid; the groups of cut tiles take the general path, their neighbours
    the short one."""
    rng = np.random.default_rng(23)
    lengths = rng.integers(0, 9, 700)
    lengths[200] = heavy
    return lengths.astype(int).tolist()


def tiles_of(rowptr, n, balance=2):
    """api.hip build_tiles: 32-row blocks, those heavier than balance x the mean cut into halves."""
    nnz = int(rowptr[-1])
    if nnz <= 0:
        return []
    nblk = (n + 31) // 32
    limit = max(balance * ((nnz + nblk - 1) // nblk), 256)
    out = []
    for b in range(nblk):
        stack = [(b * 32, min(n, b * 32 + 32))]
        while stack:
            lo, hi = stack.pop()
            if rowptr[hi] - rowptr[lo] <= limit or hi - lo <= 1:
                out.append(lo)
            else:
                mid = lo + (hi - lo + 1) // 2
                stack.append((mid, hi))
                stack.append((lo, mid))
    out.append(n)
    return out


def group_flags(lengths, width):
    """Per group of four consecutive tiles: is it short at `width`?  A group is short when each of its tiles is a whole
    32-row block (or the ragged last one) and no row of it has more than `width` entries.  [] when there is no image at all
    (width 0, fewer than 64 rows, no entries)."""
    n = len(lengths)
    if width == 0 or n < 64:
        return []
    rowptr = np.concatenate([[0], np.cumsum(lengths)])
    t = tiles_of(rowptr, n)
    n_tiles = len(t) - 1
    flags = []
    for k in range((n_tiles + 3) // 4):
        ok = True
        for i in range(4 * k, min(4 * k + 4, n_tiles)):
            lo, hi = t[i], t[i + 1]
            ok = ok and lo % 32 == 0 and hi == min(n, lo + 32) and (hi == lo or max(lengths[lo:hi]) <= width)
        flags.append(bool(ok))
    return flags


def short_groups(lengths, width):
    """The rule: how many groups of four consecutive tiles are short at `width`."""
    return sum(group_flags(lengths, width))


def tile_groups(lengths):
    """Groups of four tiles a launch of the upper-triangle leg has (0 without entries)."""
    n = len(lengths)
    t = tiles_of(np.concatenate([[0], np.cumsum(lengths)]), n)
    return (max(0, len(t) - 1) + 3) // 4
