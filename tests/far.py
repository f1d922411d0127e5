"""Far placement of a tests/blocks.py block: the offsets of row 65535 of a kept model without its 17 GB.

The C interfaces of the companion libraries take (S, layout, stride, n_rows, n_cols).  A 70 x 1100 block whose stride is
2^26 elements has rows that start past element 2^31 (row 32) and past 2^32 (row 64), as the rows of a compact f32 model
of N = 65536 do; only its 77 000 live values have to exist.  The four geometries, each with the strides and bases of
``blocks.variants`` (vector path, scalar path, a base 4 / 8 bytes in; panels stay on 16 bytes):

    ROWMAJOR_F32   stride 2^26 (+ 4 | + 1)   row 32 is the first at >= 2^31 elements, row 64 the first at >= 2^32
    ROWMAJOR_F64   stride 2^25 (+ 2 | + 1)   row 64 is the first at >= 2^31 elements (2^34 bytes)
    PANEL_F32      stride 2^22 rows          panel 16 starts at 2^31 elements, panel 32 at 2^32; panels 0 .. 34
    PANEL_F16      stride 2^22 rows          panel 8 starts at 2^31 elements, panel 16 at 2^32 (2^33 bytes); panels 0 .. 17

``pieces`` turns a logical matrix into a scatter plan [(byte offset, bytes)]: per row-major row its columns between two
margins of the block's sentinel, per panel its rows followed by sentinel rows.  ``Arena`` is ONE device allocation of
2 x E bytes (E: the largest extent) with the block's base in its middle, so that an element offset narrowed to 32 bits,
sign-wrapped (>= base - 2^31 elements) or zero-extended (>= base), still lands inside it and reads the FILLER: a bit
pattern that is finite and above every value of the block in the layout's stored type, so a wrong address wins every
top-k, passes every threshold and changes every sum.  References, sentinels and the bit-for-bit rule are those of
tests/blocks.py; tests/test_far_cpu.py pins the geometry and the plan."""
import collections
import functools

import numpy as np

from tests import blocks as B

N_ROWS, N_COLS = 70, 1100
MARGIN = 32                                         # bytes of sentinel on either side of a row-major row (two 16-byte pieces)
GUARD_ROWS = 8                                      # sentinel rows after a panel's rows (a wave of a sweep takes eight rows)
FAR_STRIDE = {B.ROWMAJOR_F32: 1 << 26, B.ROWMAJOR_F64: 1 << 25, B.PANEL_F32: 1 << 22, B.PANEL_F16: 1 << 22}
# rows and columns on each side of every boundary of every geometry, and the last ones
EDGE_ROWS = (0, 31, 32, 63, 64, N_ROWS - 1)
EDGE_COLS = (0, 511, 512, 1023, 1024, N_COLS - 1)

# the filler as the stored bits of one element; f32 and float64 are one repeated byte (a memset), binary16 is the
# largest finite value: the only one above every value of a wide binary16 block, which holds all the others
FILLER_BITS = {B.PANEL_F32: np.uint32(0x7b7b7b7b), B.ROWMAJOR_F32: np.uint32(0x7b7b7b7b), B.PANEL_F16: np.uint16(0x7bff),
               B.ROWMAJOR_F64: np.uint64(0x7b7b7b7b7b7b7b7b)}

Geometry = collections.namedtuple("Geometry", "layout tag stride base")


def itemsize(layout):
    return np.dtype(B.STORED[layout]).itemsize


def geometries(layout, stride=None):
    """The layout's geometries at its far stride (or at ``stride``, for the check on a host array): blocks.variants' tags."""
    s = FAR_STRIDE[layout] if stride is None else stride
    if layout in B.PANEL:
        return [Geometry(layout, "panel", s, 0)]
    v = 16 // itemsize(layout)
    return [Geometry(layout, "aligned", s + v, 0), Geometry(layout, "crooked", s + 1, 0), Geometry(layout, "offset", s + v, 16 // v)]


ALL = [g for layout in B.LAYOUTS for g in geometries(layout)]


def extent(g, n_rows=N_ROWS, n_cols=N_COLS):
    """Bytes from the block's base to the end of its last stored element."""
    return B.n_elems(g.layout, n_rows, n_cols, g.stride) * itemsize(g.layout)


def filler(layout, n=1):
    """n elements of filler in the layout's stored type."""
    return np.full(n, FILLER_BITS[layout]).view(B.STORED[layout])


def stored_pieces(g, M, pad):
    """The scatter plan of a matrix ``M`` of STORED elements in geometry ``g``, padding = the stored element ``pad``:
    [(byte offset from the block's base, bytes)], ascending and disjoint, inside [0, extent).  Row-major: one piece per
    row, its columns with MARGIN bytes of padding before and after where the neighbouring rows and the extent leave
    room.  Panels: one piece per panel, the 128-byte segments of rows 0 .. n_rows - 1 (columns past n_cols hold the
    padding) and up to GUARD_ROWS rows of padding."""
    n_rows, n_cols = M.shape
    size, dtype = itemsize(g.layout), B.STORED[g.layout]
    assert M.dtype == dtype
    out = []
    if g.layout in B.PANEL:
        w = B.PANEL[g.layout]
        guard = min(GUARD_ROWS, g.stride - n_rows)
        for p in range(-(-n_cols // w)):
            seg = np.full((n_rows + guard, w), pad, dtype=dtype)
            cols = M[:, p * w:(p + 1) * w]
            seg[:n_rows, :cols.shape[1]] = cols
            out.append((p * g.stride * w * size, seg.tobytes()))
        return out
    m = MARGIN // size
    gap = g.stride - n_cols
    after = min(m, gap)
    for r in range(n_rows):
        before = min(m, gap - after) if r else 0
        row = np.full(before + n_cols + after, pad, dtype=dtype)
        row[before:before + n_cols] = M[r]
        out.append(((r * g.stride - before) * size, row.tobytes()))
    return out


def pieces(g, A, sentinel):
    """``stored_pieces`` of the logical float64 matrix ``A``, padding = the sentinel (a value)."""
    return stored_pieces(g, B.store(g.layout, A), B.store(g.layout, sentinel))


def live_offsets(g, n_rows=N_ROWS, n_cols=N_COLS):
    """int64 [n_rows, n_cols]: element offsets of the live values (blocks.offsets at the geometry's stride)."""
    return B.offsets(g.layout, n_rows, n_cols, g.stride)


# half the arena: the largest extent, its base included, on a multiple of 4 KiB
HALF = -(-max(g.base + extent(g) for g in ALL) // 4096) * 4096
ARENA = 2 * HALF
HEADROOM = 4 << 30                                 # free device memory wanted beyond the arena


@functools.lru_cache(maxsize=None)
def block(layout, kind, seed=0, overflow=0):
    """The 70 x 1100 block of (layout, kind) at a small stride: its ``A``, sentinel and lists are those of every far
    geometry of the layout (make_block draws the values from the shape, not from the stride)."""
    stride = N_ROWS + 3 if layout in B.PANEL else N_COLS + 4
    return B.make_block(layout, N_ROWS, N_COLS, stride, seed, kind=kind, overflow=overflow)


class Arena:
    """The device allocation and what is placed in it.  ``ops``: a HipOps."""

    def __init__(self, ops):
        self.ops, self.ptr, self.filled, self.placed = ops, ops._malloc(ARENA), None, []
        self.pattern, self.dirty = None, True      # the 16 bytes every piece of the arena held after the last fill
        self.base = self.ptr + HALF                # where a block with base 0 starts

    def fill(self, layout):
        """Every byte of the arena = the layout's filler (a memset, or doubling device copies of 1 MiB of the pattern)."""
        pattern = filler(layout, 16 // itemsize(layout)).tobytes()
        self.filled = layout
        if pattern == self.pattern and not self.dirty:
            return
        self.placed = []
        raw = filler(layout, (1 << 20) // itemsize(layout)).view(np.uint8)
        if (raw == raw[0]).all():
            from simrank_amd._lib import check
            check(self.ops.lib.simrank_memset(self.ptr, int(raw[0]), ARENA, self.ops.stream), "simrank_memset")
        else:
            self.ops.h2d(self.ptr, raw)
            done = raw.nbytes
            while done < ARENA:
                step = min(done, ARENA - done)
                self.ops.copy_bytes(self.ptr + done, self.ptr, step)
                done += step
        self.ops.synchronize()
        self.pattern, self.dirty = pattern, False

    def write(self, at, raw):
        """Bytes at the device address ``at`` (inside the arena), remembered so that ``clear`` puts the filler back."""
        self.touch(at, len(raw))
        self.ops.h2d(at, np.frombuffer(raw, dtype=np.uint8))

    def place(self, g, A, sentinel):
        """The block in the arena -> its device pointer S."""
        assert self.filled is not None and B.STORED[self.filled] == B.STORED[g.layout]
        S = self.base + g.base
        for off, raw in pieces(g, A, sentinel):
            self.write(S + off, raw)
        return S

    def touch(self, at, nbytes):
        """A range a kernel is about to write (an output or a band in the arena): ``clear`` puts the filler back."""
        assert self.ptr <= at and at + nbytes <= self.ptr + ARENA
        assert all(at + nbytes <= a or a + n <= at for a, n in self.placed), "two placements overlap"
        self.placed.append((at, nbytes))
        self.dirty = True

    def clear(self):
        """The filler over everything placed or touched since the fill."""
        self.ops.synchronize()
        size = itemsize(self.filled)
        for at, n in self.placed:
            lo, hi = (at - self.ptr) // size * size, -(-(at + n - self.ptr) // size) * size      # whole elements of the pattern
            self.ops.h2d(self.ptr + lo, filler(self.filled, (hi - lo) // size).view(np.uint8))
        self.ops.synchronize()
        self.placed, self.dirty = [], False

    def free(self):
        self.ops.synchronize()
        self.ops._free(self.ptr)
        self.ptr = None
