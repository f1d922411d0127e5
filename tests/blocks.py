"""Synthetic blocks for the companion libraries, and a plain NumPy statement of every entry point they export.

A fitted S is symmetric, mostly zero and lies in [0, 1]: a kernel that reads (c, r) for (r, c), the wrong panel or the
wrong 16-byte piece usually lands on the same bits.  ``make_block`` builds the opposite: no two elements of a row or of a
column equal (but for a sprinkled minority of zeros and repeats whose positions it returns), ``A[r][c] != A[c][r]``,
both signs, every value exactly representable in the layout's stored type, and every element of padding a sentinel that
is finite and larger than every real value: it would pass any threshold and win any top-k.

The addressing is the one written down in include/simrank_query.h:

    0 PANEL_F32      f32, 32-column panels   (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31)
    1 ROWMAJOR_F32   f32                     (r, c) at r * stride + c
    2 PANEL_F16      binary16 of value x 2^14, 64-column panels   (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63)
    3 ROWMAJOR_F64   float64                 (r, c) at r * stride + c

``kind="dyadic"``: multiples of 2^-8 with magnitude below 16 (binary16 holds 11 bits, so layout 2 takes multiples of 2^-10
below 2: the same 2^13 steps).  A sum of up to 512 of them is below 2^22 steps, exact in f32 in any order; times a power
of two it stays exact.  ``kind="wide"``: many binades, with (f32 layouts) values whose fp16-held form is subnormal, exact
round-to-nearest-even ties, +0 and -0 and the largest values that still fit; values the form cannot hold only when
``overflow=n`` asks for n of them.

``make_long`` builds the blocks with one LONG dimension (tens of thousands of rows or columns) that ``make_block`` cannot:
the same dyadic values drawn with repeats, for the tests in which one workgroup takes several turns.

The references below are written for reading, not for speed; tests/test_blocks_cpu.py pins them and the generator.
"""
from fractions import Fraction

import numpy as np

PANEL_F32, ROWMAJOR_F32, PANEL_F16, ROWMAJOR_F64 = 0, 1, 2, 3
LAYOUTS = (PANEL_F32, ROWMAJOR_F32, PANEL_F16, ROWMAJOR_F64)
STORED = {PANEL_F32: np.float32, ROWMAJOR_F32: np.float32, PANEL_F16: np.float16, ROWMAJOR_F64: np.float64}
PANEL = {PANEL_F32: 32, PANEL_F16: 64}          # columns of a panel
HALF_SCALE = 16384.0                            # fp16-held values are value x 2^14
TILE = 32                                       # SIMRANK_FOLDIN_TILE
PACK_FILL = 0xA5                                # every byte of a pack destination before the call

# (layout, kind) -> the padding sentinel as a VALUE (what the block would mean there): finite, above every real value
SENTINEL = {(PANEL_F32, "dyadic"): 1024.0, (ROWMAJOR_F32, "dyadic"): 1024.0, (PANEL_F16, "dyadic"): 3.0,
            (ROWMAJOR_F64, "dyadic"): 1024.0, (PANEL_F32, "wide"): 2.0 ** 100, (ROWMAJOR_F32, "wide"): 2.0 ** 100,
            (PANEL_F16, "wide"): 65504.0 / HALF_SCALE, (ROWMAJOR_F64, "wide"): 2.0 ** 600}


# ---- addressing -----------------------------------------------------------------------------------------------------
def n_elems(layout, n_rows, n_cols, stride):
    """Stored elements of a block: whole panels (the last one too), or n_rows rows of ``stride``."""
    if layout in PANEL:
        assert stride >= n_rows
        return -(-n_cols // PANEL[layout]) * stride * PANEL[layout]
    assert stride >= n_cols
    return n_rows * stride


def offsets(layout, n_rows, n_cols, stride):
    """int64 [n_rows, n_cols]: the element offset of (r, c)."""
    r = np.arange(n_rows, dtype=np.int64)[:, None]
    c = np.arange(n_cols, dtype=np.int64)[None, :]
    if layout == PANEL_F32:
        return ((c >> 5) * stride + r) * 32 + (c & 31)
    if layout == PANEL_F16:
        return ((c >> 6) * stride + r) * 64 + (c & 63)
    return r * stride + c


def store(layout, values):
    """float64 values -> the layout's stored type, asserting that nothing is lost (inf stays inf)."""
    values = np.asarray(values, dtype=np.float64)
    if layout == PANEL_F16:
        with np.errstate(over="ignore"):
            out = (values * HALF_SCALE).astype(np.float16)
        back = out.astype(np.float64) / HALF_SCALE
    else:
        with np.errstate(over="ignore"):
            out = values.astype(STORED[layout])
        back = out.astype(np.float64)
    assert np.array_equal(back, values), "a value is not representable in the layout's stored type"
    return out


def widen(layout, stored):
    """Stored elements -> float64 as the device widens them: f32 -> double; binary16 h -> (float)h * 2^-14 -> double."""
    if layout == PANEL_F16:
        return (np.asarray(stored, dtype=np.float16).astype(np.float32) * np.float32(1.0 / HALF_SCALE)).astype(np.float64)
    return np.asarray(stored).astype(np.float64)


def encode(layout, A, stride, sentinel):
    """The logical matrix as the flat stored array of the block, every element of padding = ``sentinel`` (a value)."""
    n_rows, n_cols = A.shape
    raw = np.full(n_elems(layout, n_rows, n_cols, stride), store(layout, sentinel), dtype=STORED[layout])
    raw[offsets(layout, n_rows, n_cols, stride).ravel()] = store(layout, A).ravel()
    return raw


def decode(layout, raw, n_rows, n_cols, stride):
    """float64 [n_rows, n_cols] of a block's bytes (or its flat stored array)."""
    flat = np.frombuffer(raw, dtype=STORED[layout]) if isinstance(raw, (bytes, bytearray)) else np.asarray(raw)
    return widen(layout, flat[offsets(layout, n_rows, n_cols, stride)])


def bits(a):
    """The array's bits as unsigned integers of the element size: what "equal" means in the GPU tests."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- the generator --------------------------------------------------------------------------------------------------
class Block:
    """What ``make_block`` returns; unpacks as ``A, raw = make_block(...)``."""

    def __init__(self, layout, A, stride, sentinel, zeros, repeats, special):
        self.layout, self.A, self.stride, self.sentinel = layout, A, stride, sentinel
        self.n_rows, self.n_cols = A.shape
        self.zeros = zeros            # int [m, 2]: (r, c) of the exact zeros
        self.repeats = repeats        # int [m, 3]: (r, c, c_first): A[r][c] repeats A[r][c_first] on purpose
        self.special = special        # kind="wide": name -> list of (r, c) of the planted values
        self.stored = encode(layout, A, stride, sentinel)
        self.raw = self.stored.tobytes()

    def __iter__(self):
        return iter((self.A, self.raw))


def _pool(layout, kind, rng, want):
    """Distinct non-zero candidate values (float64, exactly storable), shuffled."""
    if kind == "dyadic":
        mag = np.arange(1, 2048) * 2.0 ** -10 if layout == PANEL_F16 else np.arange(1, 4096) * 2.0 ** -8
    elif layout == PANEL_F16:
        # every positive finite binary16 below the sentinel 65504, subnormals included
        mag = np.arange(1, 0x7bff, dtype=np.uint16).view(np.float16).astype(np.float64) / HALF_SCALE
    else:
        # a full significand times 2^e: |x| from 2^-41 to 2 in f32 (fp16-held forms that are zero, subnormal and normal),
        # 2^-120 to 2 in float64
        p = 24 if layout != ROWMAJOR_F64 else 53
        lo = -41 if layout != ROWMAJOR_F64 else -120
        m = rng.integers(1 << (p - 1), 1 << p, size=2 * want + 64, dtype=np.int64)
        e = rng.integers(lo - (p - 1), 1 - p + 1, size=m.size)
        mag = np.unique(np.ldexp(m.astype(np.float64), e.astype(np.int32)))
    vals = np.concatenate([mag, -mag])
    rng.shuffle(vals)
    return vals


def _wide_specials(layout, overflow):
    """name -> values planted in a wide f32 block: what narrowing to the fp16-held form has to get right."""
    if layout not in (PANEL_F32, ROWMAJOR_F32):
        return {}
    f32 = np.float32
    below = float(np.nextafter(f32(65520.0 / HALF_SCALE), f32(0)))        # x * 2^14 just below 65520: still 65504
    sp = {
        "tie_down": [2049.0 / HALF_SCALE, -2049.0 / HALF_SCALE],           # halfway 2048 | 2050: even is 2048
        "tie_up": [2051.0 / HALF_SCALE, -2051.0 / HALF_SCALE],             # halfway 2050 | 2052: even is 2052
        "sub_tie_zero": [2.0 ** -39],                                      # x * 2^14 = 2^-25: halfway 0 | 2^-24 -> 0
        "sub_tie_up": [3 * 2.0 ** -39],                                    # 3 * 2^-25: halfway 2^-24 | 2^-23 -> 2^-23
        "sub_exact": [2.0 ** -38, 1023 * 2.0 ** -38],                      # smallest and largest subnormal
        "sub_round": [5.25 * 2.0 ** -38, -777.75 * 2.0 ** -38],            # subnormal results that need a rounding
        "neg_zero": [-0.0],
        "pos_zero": [0.0],
        "largest": [65504.0 / HALF_SCALE, below, -65504.0 / HALF_SCALE],   # the largest that still fit
    }
    if overflow:
        over = [65520.0 / HALF_SCALE, 4.0, -5.0, 2.0 ** 33, float("inf"), -65536.0 / HALF_SCALE]   # 65520 ties to infinity
        sp["overflow"] = [over[i % len(over)] for i in range(overflow)]
    return sp


def make_block(layout, n_rows, n_cols, stride, seed, *, kind="dyadic", overflow=0, zero_fraction=0.04):
    """-> ``Block`` (unpacks as ``A, raw``): the logical float64 matrix [n_rows, n_cols] and the raw bytes of the block in
    ``layout`` with ``stride``, padding = the sentinel.  See the module's docstring for what it guarantees; it asserts it."""
    assert layout in LAYOUTS and kind in ("dyadic", "wide") and n_rows >= 1 and n_cols >= 1
    assert overflow == 0 or (kind == "wide" and layout in (PANEL_F32, ROWMAJOR_F32))
    rng = np.random.default_rng([seed, layout, n_rows, n_cols, 0 if kind == "dyadic" else 1])
    pool = _pool(layout, kind, rng, n_rows * n_cols)
    if pool.size >= n_rows * n_cols:
        A = pool[:n_rows * n_cols].reshape(n_rows, n_cols).copy()          # all distinct
    else:
        # A[r][c] = pool[(pr[r] + pc[c]) mod M] with pr, pc injective: a row's and a column's values are distinct;
        # A[r][c] != A[c][r] needs pr[i] - pc[i] distinct over the i that are both a row and a column
        M = pool.size
        assert M >= max(n_rows, n_cols)
        pc = rng.permutation(M)[:n_cols]
        pr = np.empty(n_rows, dtype=np.int64)
        free_pr, used_d = list(rng.permutation(M)), set()
        for i in range(n_rows):
            for j, cand in enumerate(free_pr):
                d = (cand - pc[i]) % M if i < n_cols else None
                if d is None or d not in used_d:
                    pr[i] = cand
                    used_d.add(d)
                    del free_pr[j]
                    break
        A = pool[(pr[:, None] + pc[None, :]) % M]

    def mirror_differs(r, c, v):
        return not (r != c and r < n_cols and c < n_rows and A[c, r] == v)

    taken = np.zeros(A.shape, dtype=bool)
    # planted values of the wide kind (each once; an overflow block is asked for by the caller)
    special = {}
    for name, vals in _wide_specials(layout, overflow).items() if kind == "wide" else ():
        special[name] = []
        for v in vals:
            for _ in range(64):
                r, c = int(rng.integers(n_rows)), int(rng.integers(n_cols))
                if not taken[r, c] and mirror_differs(r, c, v) and (v == 0 or (not (A[r] == v).any() and not (A[:, c] == v).any())):
                    A[r, c], taken[r, c] = v, True
                    special[name].append((r, c))
                    break
    # exact zeros, a minority
    for _ in range(int(round(zero_fraction * A.size))):
        r, c = int(rng.integers(n_rows)), int(rng.integers(n_cols))
        if not taken[r, c] and mirror_differs(r, c, 0.0):
            A[r, c], taken[r, c] = 0.0, True
    # deliberate repeats within a row: a value met twice, so that a tie rule has something to decide
    repeats = []
    for _ in range(max(1, n_rows // 2) if n_cols >= 3 else 0):
        r = int(rng.integers(n_rows))
        c1, c2 = (int(x) for x in rng.choice(n_cols, size=2, replace=False))
        v = A[r, c1]
        if taken[r, c1] or taken[r, c2] or not mirror_differs(r, c2, v) or (A[:, c2] == v).any():
            continue
        A[r, c2], taken[r, c2], taken[r, c1] = v, True, True
        repeats.append((r, c2, c1))
    zeros = np.argwhere(A == 0)
    repeats = np.asarray(repeats, dtype=np.int64).reshape(-1, 3)
    sentinel = SENTINEL[(layout, kind)]
    blk = Block(layout, A, stride, sentinel, zeros, repeats, special)
    check_block(blk, overflow=overflow)
    return blk


def check_block(blk, overflow=0):
    """What ``make_block`` promises, asserted."""
    A, (n_rows, n_cols) = blk.A, blk.A.shape
    assert np.array_equal(bits(decode(blk.layout, blk.raw, n_rows, n_cols, blk.stride)), bits(A))   # exactly what the device holds
    finite = A[np.isfinite(A)]
    assert np.isfinite(blk.sentinel) and (np.abs(finite) < blk.sentinel).all() and not (A == blk.sentinel).any()
    assert overflow or np.isfinite(A).all()
    if A.size >= 8:
        assert (A > 0).any() and (A < 0).any()
    # padding: everything the addressing does not reach holds the sentinel
    pad = np.ones(blk.stored.size, dtype=bool)
    pad[offsets(blk.layout, n_rows, n_cols, blk.stride).ravel()] = False
    assert np.array_equal(bits(blk.stored[pad]), bits(np.full(int(pad.sum()), store(blk.layout, blk.sentinel))))
    # distinct along rows and columns but for the zeros and the listed repeats
    free = A != 0
    free[blk.repeats[:, 0], blk.repeats[:, 1]] = False
    for line, ok in list(zip(A, free)) + list(zip(A.T, free.T)):
        v = line[ok]
        assert np.unique(v).size == v.size
    assert (~free).sum() <= max(2, A.size // 4)                           # a minority
    m = min(n_rows, n_cols)
    sq = A[:m, :m]
    off = ~np.eye(m, dtype=bool)
    assert (sq[off] != sq.T[off]).all()
    for r, c2, c1 in blk.repeats:
        assert A[r, c2] == A[r, c1]


def make_long(layout, n_rows, n_cols, stride, seed, *, zero_fraction=0.04):
    """-> ``Block``: a block with one LONG dimension (tens of thousands of rows or of columns), which ``make_block`` cannot
    build: its pool has 8 190 values, it wants one per row and per column and deals the rows in a Python loop.  The
    logical matrix is drawn, with repeats, from the same dyadic pool (both signs, every value exactly storable), about
    ``zero_fraction`` of it exact zeros; padding holds the layout's dyadic sentinel.  Rows and columns are NOT distinct:
    use it where the reference has an exact tie rule.  ``repeats`` is empty; ``check_long`` asserts the rest."""
    assert layout in LAYOUTS and n_rows >= 1 and n_cols >= 1
    rng = np.random.default_rng([seed, layout, n_rows, n_cols, 2])
    pool = _pool(layout, "dyadic", rng, 0)
    A = pool[rng.integers(0, pool.size, size=(n_rows, n_cols))]
    A[rng.random((n_rows, n_cols)) < zero_fraction] = 0.0
    blk = Block(layout, A, stride, SENTINEL[(layout, "dyadic")], np.argwhere(A == 0),
                np.zeros((0, 3), dtype=np.int64), {})
    check_long(blk)
    return blk


def check_long(blk):
    """What ``make_long`` promises, asserted: the stored block decodes to A bit for bit (so every value is exactly storable),
    everything the addressing does not reach holds the sentinel, the sentinel is above every value, both signs and zeros."""
    A, (n_rows, n_cols) = blk.A, blk.A.shape
    at = offsets(blk.layout, n_rows, n_cols, blk.stride).ravel()
    assert np.array_equal(bits(widen(blk.layout, blk.stored[at])), bits(A.ravel()))
    assert np.isfinite(A).all() and (np.abs(A) < blk.sentinel).all()
    pad = np.ones(blk.stored.size, dtype=bool)
    pad[at] = False
    assert pad.sum() == blk.stored.size - A.size                          # an injective addressing
    assert (bits(blk.stored[pad]) == bits(store(blk.layout, blk.sentinel).reshape(1))[0]).all()
    if A.size >= 200:
        assert (A > 0).any() and (A < 0).any() and len(blk.zeros)


# ---- query ----------------------------------------------------------------------------------------------------------
def ref_rows(A, row_pos, col_pos, n_out):
    """simrank_query_rows: float64 [n_q, n_out]; a position outside the block reads NaN."""
    n_rows, n_cols = A.shape
    cols = np.arange(n_out) if col_pos is None else np.asarray(col_pos, dtype=np.int64)
    out = np.full((len(row_pos), n_out), np.nan)
    ok_c = (cols >= 0) & (cols < n_cols)
    for q, r in enumerate(row_pos):
        if 0 <= r < n_rows:
            out[q, ok_c] = A[r, cols[ok_c]]
    return out


def ref_pairs(A, a_pos, b_pos):
    n_rows, n_cols = A.shape
    return np.array([A[a, b] if 0 <= a < n_rows and 0 <= b < n_cols else np.nan for a, b in zip(a_pos, b_pos)], dtype=np.float64)


def _best(values, ids, candidate, k):
    """(ids int32 [k], values float64 [k]): the k best candidates in the total order (value descending, id ascending);
    slots past them hold -1 / 0.0."""
    at = np.flatnonzero(candidate)
    order = at[np.lexsort((ids[at], -values[at]))][:k]
    idx, val = np.full(k, -1, dtype=np.int32), np.zeros(k, dtype=np.float64)
    idx[:order.size], val[:order.size] = ids[order], values[order]
    return idx, val


def ref_topk(A, row_pos, row_ids, col_ids, k):
    """simrank_query_topk: the row's own node excluded BY ID; a row outside the block has no candidates."""
    n_rows, n_cols = A.shape
    ids = np.arange(n_cols, dtype=np.int64) if col_ids is None else np.asarray(col_ids, dtype=np.int64)
    idx, val = np.full((len(row_pos), k), -1, dtype=np.int32), np.zeros((len(row_pos), k))
    for q, (r, rid) in enumerate(zip(row_pos, row_ids)):
        if 0 <= r < n_rows:
            idx[q], val[q] = _best(A[r], ids, (ids != rid) & ~np.isnan(A[r]), k)
    return idx, val


def ref_band_topk(band, col_ids, k):
    """simrank_sets_topk on a float64 band [n_sets, n_out]: -inf and NaN are no candidates."""
    band = np.asarray(band, dtype=np.float64)
    ids = np.arange(band.shape[1], dtype=np.int64) if col_ids is None else np.asarray(col_ids, dtype=np.int64)
    idx, val = np.full((len(band), k), -1, dtype=np.int32), np.zeros((len(band), k))
    for q, row in enumerate(band):
        with np.errstate(invalid="ignore"):
            idx[q], val[q] = _best(row, ids, row > -np.inf, k)
    return idx, val


# ---- select ---------------------------------------------------------------------------------------------------------
def ref_select(A, row_ids, col_ids, t32):
    """simrank_select_count / _emit: (counts int32 [n_rows], per row (ids int32, values f32) of the hits in column
    order): S[r][c] >= t32 in f32 and col_ids[c] != row_ids[r]."""
    n_rows, n_cols = A.shape
    rid = np.arange(n_rows) if row_ids is None else np.asarray(row_ids)
    cid = np.arange(n_cols) if col_ids is None else np.asarray(col_ids)
    V = A.astype(np.float32)
    assert np.array_equal(V.astype(np.float64), A)
    rows = []
    for r in range(n_rows):
        hit = np.flatnonzero((V[r] >= np.float32(t32)) & (cid != rid[r]))
        rows.append((cid[hit].astype(np.int32), V[r, hit]))
    return np.array([len(i) for i, _ in rows], dtype=np.int32), rows


def ref_offsets(counts):
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    return off, int(off[-1])


def ref_emit(rows, offs, capacity, ids_out, vals_out):
    """What simrank_select_emit leaves in the two arrays it was given (any length): hit j of row r at offs[r] + j, nothing
    at or past offs[r + 1] nor at or past ``capacity``."""
    ids_out, vals_out = ids_out.copy(), vals_out.copy()
    for r, (ids, vals) in enumerate(rows):
        end = min(int(offs[r + 1]), capacity)
        for j in range(len(ids)):
            s = int(offs[r]) + j
            if 0 <= s < end:
                ids_out[s], vals_out[s] = ids[j], vals[j]
    return ids_out, vals_out


# ---- fold-in --------------------------------------------------------------------------------------------------------
def acc_type(layout):
    return np.float64 if layout == ROWMAJOR_F64 else np.float32


def ref_gather(A, layout, col_ids, col_base, list_ptr, list_pos, w, n_tile, T, *, reverse=False, acc=None):
    """simrank_foldin_gather on the array T [n_src, 32] it was given (a copy comes back): for every column c of the block
    with 0 <= id(c) < n_src the WHOLE line T[id(c)] = w[q] * sum_e A[list_pos[e]][c] (q < n_tile; 0 beyond), the sums in
    the layout's type (``acc`` overrides it) in list order (``reverse``: backwards), times w in float64, rounded to T's."""
    acc = acc_type(layout) if acc is None else acc
    n_rows, n_cols = A.shape
    T = T.copy()
    ids = col_base + np.arange(n_cols) if col_ids is None else np.asarray(col_ids, dtype=np.int64)
    line = np.zeros((n_cols, TILE), dtype=T.dtype)
    for q in range(n_tile):
        s = np.zeros(n_cols, dtype=acc)
        members = list(list_pos[list_ptr[q]:list_ptr[q + 1]])
        for r in (reversed(members) if reverse else members):
            s = s + (A[r].astype(acc) if 0 <= r < n_rows else acc(np.nan))
        line[:, q] = (np.float64(w[q]) * s.astype(np.float64)).astype(T.dtype)
    ok = (ids >= 0) & (ids < T.shape[0])
    T[ids[ok]] = line[ok]
    return T


def ref_member(list_ptr, list_ids, w, n_tile, n_src):
    member = np.zeros(n_src, dtype=np.uint32)
    for q in range(n_tile):
        if w[q] > 0:
            for j in list_ids[list_ptr[q]:list_ptr[q + 1]]:
                if 0 <= j < n_src:
                    member[j] |= np.uint32(1 << q)
    return member


def finish(acc, cnt, sc, coef, lbd, evidence, prior, *, fused=None):
    """The epilogue of simrank_foldin_apply in its written evaluation order, every step one IEEE double operation.
    ``fused``: how a compiler may contract the last line into ONE multiply-add: "head" = fma(head, prod, lbd * prior),
    "prior" = fma(lbd, prior, head * prod); evaluated exactly and rounded once."""
    acc, sc = float(acc), float(sc)
    prod = sc * acc
    if evidence:
        if not sc > 0.0:
            cnt = 0
        E = 1.0 - 2.0 ** -min(int(cnt), 255)
        keep = 1.0 - lbd
        head = (keep * E) * coef
    else:
        head = coef
    if prior is None:
        return head * prod
    prior = float(prior)
    plain = head * prod + lbd * prior
    if fused is None or not np.isfinite(plain):
        return plain
    if fused == "head":
        exact = Fraction(head) * Fraction(prod) + Fraction(lbd * prior)
    else:
        exact = Fraction(head * prod) + Fraction(lbd) * Fraction(prior)
    return plain if exact == 0 else float(exact)                           # (an exact zero keeps IEEE's sign rule)


def ref_apply(rowptr, col, scale, T, member, coef, lbd, prior, n_tile, out, *, reverse=False, acc=None, fused=None):
    """simrank_foldin_apply on the array ``out`` [>= n_tile, ld] it was given (a copy comes back): out[q][b] for q <
    n_tile and b < n_out.  The sums run in T's type (``acc`` overrides it) over the row in its order (``reverse``:
    backwards); with dyadic operands every order gives the same bits, which tests/test_blocks_cpu.py checks."""
    acc = T.dtype.type if acc is None else acc
    out = out.copy()
    n_out, n_src = len(rowptr) - 1, T.shape[0]
    for b in range(n_out):
        row = list(col[rowptr[b]:rowptr[b + 1]])
        s, cnt = np.zeros(TILE, dtype=acc), np.zeros(TILE, dtype=np.int64)
        for j in (reversed(row) if reverse else row):
            if 0 <= j < n_src:
                s = s + T[j].astype(acc)
                if member is not None:
                    cnt += (int(member[j]) >> np.arange(TILE)) & 1
            else:
                s = s + acc(np.nan)
        for q in range(n_tile):
            out[q, b] = finish(s[q], cnt[q], scale[b], coef, lbd, member is not None,
                               None if prior is None else prior[q, b], fused=fused)
    return out


# ---- model ----------------------------------------------------------------------------------------------------------
def narrow(x):
    """f32 values -> the bits of the fp16-held form: binary16 of x * 2^14, round to nearest even."""
    with np.errstate(over="ignore"):
        return (np.asarray(x, dtype=np.float32) * np.float32(HALF_SCALE)).astype(np.float16)


def ref_pack(src, dst_layout, dst_stride, dst_rows, dst_cols, row_map, col_dst, col_src, n_list, dst_stored):
    """simrank_model_pack: ``src`` a ``Block``, ``dst_stored`` the destination's flat stored array before the call (a copy
    comes back) -> (the array after it, the number ADDED to *overflow).  An entry of a map that points outside its block
    is skipped."""
    out = dst_stored.copy()
    converts = STORED[src.layout] != STORED[dst_layout]
    stored_src = src.stored[offsets(src.layout, src.n_rows, src.n_cols, src.stride)]
    at = offsets(dst_layout, dst_rows, dst_cols, dst_stride)
    sr = np.arange(dst_rows) if row_map is None else np.asarray(row_map, dtype=np.int64)
    sc = np.arange(n_list) if col_src is None else np.asarray(col_src, dtype=np.int64)[:n_list]
    dc = np.arange(n_list) if col_dst is None else np.asarray(col_dst, dtype=np.int64)[:n_list]
    rows = np.flatnonzero((sr >= 0) & (sr < src.n_rows))
    read = (sc >= 0) & (sc < src.n_cols)
    v = stored_src[np.ix_(sr[rows], sc[read])]
    over = 0
    if converts:
        v = narrow(v)
        over = int(((bits(v) & 0x7c00) == 0x7c00).sum())                   # (counted where read, written or not)
    written = (dc[read] >= 0) & (dc[read] < dst_cols)
    assert np.unique(dc[read][written]).size == written.sum()              # (a destination column named twice has no one answer)
    out[at[np.ix_(rows, dc[read][written])]] = v[:, written]
    return out, over


# ---- sets -----------------------------------------------------------------------------------------------------------
def ref_score(A, col_pos, n_out, set_ptr, set_pos, set_w, excl_ptr, excl_cols):
    """simrank_sets_score: ``sets_ref.scores`` (one product and one sum per member, in list order) on the mapped columns;
    a member outside the rows or a mapped column outside the block poisons with NaN; the listed OUTPUT columns of a
    basket hold -inf."""
    from tests import sets_ref
    n_rows, n_cols = A.shape
    cols = np.arange(n_out) if col_pos is None else np.asarray(col_pos, dtype=np.int64)
    ok_c = (cols >= 0) & (cols < n_cols)
    M = np.full((n_rows + 1, n_out), np.nan)                               # row n_rows: what a bad position reads
    M[:n_rows, ok_c] = A[:, cols[ok_c]]
    lists, weights = [], []
    for q in range(len(set_ptr) - 1):
        pos = np.asarray(set_pos[set_ptr[q]:set_ptr[q + 1]], dtype=np.int64)
        lists.append(np.where((pos >= 0) & (pos < n_rows), pos, n_rows))
        weights.append(set_w[set_ptr[q]:set_ptr[q + 1]])
    with np.errstate(invalid="ignore", over="ignore"):
        out = sets_ref.scores(M, lists, weights)
    if excl_ptr is not None:
        for q in range(len(set_ptr) - 1):
            for j in excl_cols[excl_ptr[q]:excl_ptr[q + 1]]:
                if 0 <= j < n_out:
                    out[q, j] = -np.inf
    return out


# ---- the cases both test modules use ----------------------------------------------------------------------------------
# (rows, columns), never square.  Columns at both sides of: a 32- and a 64-column panel, 128 and 256 columns of a fold-in
# workgroup, 256 x 4 columns in flight per select wave, 1024 of a rows / sets chunk, 512 / 1024 / 2048 of a pack chunk.
# Rows: select takes 8 per wave, rows / pack deal rows to 8 labels.
SHAPES = [(7, 1), (1, 3), (7, 31), (8, 33), (9, 63), (70, 65), (9, 127), (70, 129), (7, 255), (8, 257), (9, 1023), (8, 1025),
          (7, 2050)]


def variants(layout, n_rows, n_cols):
    """[(tag, stride, bytes the block starts into its allocation)]: panels with stride > n_rows; row-major with slack that
    keeps the rows on 16 bytes, with a stride that breaks it, and with a base 4 (f32) or 8 (float64) bytes in: the three
    ways onto the non-vector paths."""
    if layout in PANEL:
        return [("panel", n_rows + 3, 0)]
    v = 4 if layout == ROWMAJOR_F32 else 2                                 # elements of 16 bytes
    aligned = -(-n_cols // v) * v + v
    crooked = aligned + 1
    assert aligned % v == 0 and crooked % v != 0 and (layout != ROWMAJOR_F64 or crooked % 2 == 1)
    return [("aligned", aligned, 0), ("crooked", crooked, 0), ("offset", aligned, 16 // v)]


def gather_case(n_rows, n_tile, seed):
    """(list_ptr int32 [n_tile + 1], list_pos int32, w float64 [n_tile]) for simrank_foldin_gather: lists that are empty,
    of 1 and of 37 entries and longer than the kernel's unrolled body of 4 (none above 512: the exactness bound), row
    positions repeated; weights powers of two, one of them 0 on a list that is not empty (a dead row)."""
    rng = np.random.default_rng([seed, n_rows, n_tile])
    lens = [37, 0, 1, 9, 4, 5, 64, 2, 3, 8, 100, 6]
    ws = [0.5, 1.0, 2.0, 0.0, 4.0, 0.25, 1.0, 0.125]
    lists = [rng.integers(0, n_rows, size=lens[q % len(lens)]).astype(np.int32) for q in range(n_tile)]
    ptr = np.zeros(n_tile + 1, dtype=np.int32)
    np.cumsum([l.size for l in lists], out=ptr[1:])
    pos = np.concatenate(lists).astype(np.int32)
    w = np.array([ws[q % len(ws)] for q in range(n_tile)], dtype=np.float64)
    assert ptr[-1] <= 512 * n_tile and max(l.size for l in lists) <= 512
    return ptr, pos, w


APPLY_ROWS = [0, 1, 3, 4, 5, 31, 32, 33, 255, 256, 257, 600]             # both sides of SIMRANK_FOLDIN_LONG_ROW = 256
LONG_ROW = 256


def apply_case(t_dtype, seed=0):
    """A small random CSR for simrank_foldin_apply with the row lengths above (and 25 short rows: 37 rows, two
    workgroups), a dyadic T [97, 32] of ``t_dtype``, member words whose bit 3 is set everywhere (the count of new node 3
    is the row's length: it reaches 255 and passes it), a scale with one 0, a dyadic prior, dyadic coef and lbd."""
    rng = np.random.default_rng([seed, 7])
    n_src = 97
    lens = APPLY_ROWS + list(rng.integers(0, 21, size=25))
    lens = [int(lens[i]) for i in rng.permutation(len(lens))]
    n_out = len(lens)
    rowptr = np.zeros(n_out + 1, dtype=np.int32)
    np.cumsum(lens, out=rowptr[1:])
    col = rng.integers(0, n_src, size=int(rowptr[-1])).astype(np.int32)
    scale = rng.choice([0.25, 0.5, 1.0, 2.0], size=n_out)
    scale[lens.index(33)] = 0.0
    T = (rng.integers(-1023, 1024, size=(n_src, TILE)) * 2.0 ** -8).astype(t_dtype)
    member = (rng.random((n_src, TILE)) < 0.5)      # (a long row counts far above 53: E = 1 exactly)
    member[:, 3] = True
    member = (member * (1 << np.arange(TILE, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
    prior = rng.integers(-4095, 4096, size=(TILE, n_out)) * 2.0 ** -8
    long_rows = np.array([b for b in range(n_out) if lens[b] > LONG_ROW], dtype=np.int32)
    return dict(rowptr=rowptr, col=col, scale=scale, T=T, member=member, prior=prior, coef=0.75, lbd=0.25,
                long_rows=long_rows, n_out=n_out, n_src=n_src, lens=lens)
