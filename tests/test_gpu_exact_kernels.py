"""Every form of both legs, through HipOps, BIT FOR BIT against float64 NumPy on exactly summable operands (tests/exact.py).

On these operands the float32 result of any correct summation order is the exact result, so no tolerance is chosen
anywhere: every path, knob and layout must return one array of bits, the float64 reference cast to float32.  Operands have
both signs and one entry per column whose bf16 hi + mid + lo split needs all three terms.  Every result and operand lies in
a matrix whose padding (columns between `cols` and `ld`, a guard row behind the last row; for panel-blocked matrices the
rows and columns that pad a panel and a guard behind the last panel) holds a sentinel before the launch and must hold it
afterwards.  The convergence count is checked on planted ties: `previous` is built from the REFERENCE and differs from it
by exactly eps, eps + one step or eps - one step at the places where a count goes wrong (diagonal, both triangles, last
row / column, the tail panel, a mirrored tile, the ends of a panel); the count must be the reference's strict > count.
Both `.dot`s of SimRank.py:139 / :298 / :361, the element-wise lines :140, :316, :362, :453, the count of :74."""
import contextlib

import numpy as np
import pytest

from simrank_amd.ingest import CSR
from tests import exact as X
from tests.leg2_rule import short_groups
from tests.test_gpu_kernels import dense64

pytestmark = pytest.mark.gpu

KNOBS = ("panel", "fuse", "fuse_min", "fuse_steps", "fuse_unit", "fuse_group", "fuse_shards", "fuse_rows", "fuse_order",
         "fuse_sym", "ids16", "dense_min", "dense_cols", "dense_sym", "lean", "triangle", "balance", "addr32", "leg2_short")


@pytest.fixture(scope="module")
def ops():
    from simrank_amd.engine import HipOps
    o = HipOps(0)
    saved = {k: o.get_tuning(k) for k in KNOBS}
    o.set_tuning(fuse_steps=1, fuse_min=2)       # small test graphs: a dense set however few steps it makes
    yield o
    o.set_tuning(**saved)


@contextlib.contextmanager
def knobs(ops, **kw):
    """Tuning values for the graphs created inside (a graph keeps the knobs it was created with)."""
    saved = {k: ops.get_tuning(k) for k in kw}
    ops.set_tuning(**kw)
    try:
        yield
    finally:
        ops.set_tuning(**saved)


# ---- matrices with a sentinel in everything that is not an element -------------------------------------------------
class _Block:
    """Device memory of our own size behind a Matrix (`external=`)."""

    def __init__(self, ops, nbytes):
        self.ops, self.ptr = ops, ops._malloc(nbytes)

    def data_ptr(self):
        return self.ptr

    def __del__(self):
        try:
            self.ops._free(self.ptr)
        except Exception:
            pass


def _sentinel(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.uint8(X.SENTINEL_U8)
    if dtype == np.float16:
        return np.float16(-65504.0)
    return X.SENTINEL


def guarded(ops, rows, cols, host=None, dtype=np.float32, pad=4, ld=None):
    """Row-major matrix with ld > cols and one guard row; elements = `host` (or the sentinel, for a result)."""
    dtype = np.dtype(dtype)
    ld = ld if ld is not None else ops.pitch(cols, dtype) + pad * (4 if dtype == np.uint8 and pad % 4 == 0 else 1)
    blk = _Block(ops, (rows + 1) * ld * dtype.itemsize)
    m = ops.matrix(rows, cols, dtype, ld=ld, external=blk)
    image = np.full((rows + 1, ld), _sentinel(dtype), dtype=dtype)
    if host is not None:
        image[:rows, :cols] = host
    ops.h2d(m.ptr, image)
    m.image, m.is_input = image, host is not None
    return m


def guarded_blocked(ops, rows, cols, host=None, dtype=np.float32, scale=1.0):
    """Panel-blocked matrix (fp16: 64-column panels, holding value x scale) with a guard of 8 rows behind its last panel."""
    dtype = np.dtype(dtype)
    m = ops.matrix(rows, cols, dtype, blocked=True)
    ops._free(m.ptr)
    m.ptr = 0
    blk = _Block(ops, m.nbytes + 8 * m.ld * dtype.itemsize)
    m.ptr, m.external, m.scale = blk.ptr, blk, scale
    image = np.full((m.panels * m.rows_pad + 8, m.ld), _sentinel(dtype), dtype=dtype)
    if host is not None:
        v = image[:m.panels * m.rows_pad].reshape(m.panels, m.rows_pad, m.ld)
        for p in range(m.panels):
            w = min(m.ld, cols - m.ld * p)
            piece = np.asarray(host)[:, m.ld * p:m.ld * p + w]
            v[p, :rows, :w] = (piece.astype(np.float64) * scale).astype(dtype) if dtype == np.float16 else piece
    ops.h2d(m.ptr, image)
    m.image, m.is_input = image, host is not None
    return m


def raw(ops, m):
    out = np.empty_like(m.image)
    ops.synchronize()
    ops.d2h(out, m.ptr)
    return out


def same_bits(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_untouched(ops, *matrices):
    """Inputs: every byte as uploaded.  Results: every byte that is not an element still the sentinel."""
    for m in matrices:
        now = raw(ops, m)
        if m.is_input:
            assert same_bits(now, m.image), "an operand was written to"
            continue
        mask = np.ones(now.shape, dtype=bool)                 # True = not an element
        if m.blocked:
            v = mask[:m.panels * m.rows_pad].reshape(m.panels, m.rows_pad, m.ld)
            for p in range(m.panels):
                v[p, :m.rows, :min(m.ld, m.cols - m.ld * p)] = False
        else:
            mask[:m.rows, :m.cols] = False
        s = np.full(1, _sentinel(m.dtype), dtype=m.dtype).view(np.uint8)
        bad = (now.view(np.uint8).reshape(now.shape + (-1,)) != s).any(axis=-1) & mask
        assert not bad.any(), f"{int(bad.sum())} padding elements overwritten, first at {tuple(np.argwhere(bad)[0])} of {now.shape}"


def f32(a):
    out = np.asarray(a, dtype=np.float64).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), a)
    return out


def equal_bits(got, want, what=""):
    """Values bit for bit (NaN never occurs; -0.0 is compared as a value)."""
    assert got.shape == want.shape and not np.isnan(got).any(), what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, first at ({r}, {c}): got {got[r, c]!r} "
                             f"({got[r, c].view(np.uint32):#010x}), want {want[r, c]!r} ({want[r, c].view(np.uint32):#010x})")


# ---- leg 1 and the plain product ----------------------------------------------------------------------------------
def leg1_blocked(ops, g, x32, M):
    x = guarded_blocked(ops, x32.shape[0], x32.shape[1], x32)
    yt = guarded_blocked(ops, x32.shape[1], M)
    ops.spmm(g, x, yt, transpose_out=True)
    out = ops.download(yt)
    check_untouched(ops, x, yt)
    return out


def leg_rowmajor(ops, g, x32, M, transpose, pad=4):
    K, L = x32.shape
    x = guarded(ops, K, L, x32, pad=pad)
    y = guarded(ops, L, M, pad=pad) if transpose else guarded(ops, M, L, pad=pad)
    ops.spmm(g, x, y, transpose_out=transpose)
    out = ops.download(y)
    check_untouched(ops, x, y)
    return out


def leg_chunked(ops, g, xw, x_col0, L, M, tb, pad):
    """The transposed leg into the chunks of an all-to-all (t_block rows of the result per chunk, t_pad floats of padding per
    row): -> L x M; the padding and a guard behind the last chunk keep the sentinel."""
    nblk = -(-M // tb)
    size = nblk * L * (tb + pad)
    y = guarded(ops, 1, size, ld=size)
    ops.spmm(g, xw, y, n_cols=L, transpose_out=True, t_block=tb, t_pad=pad, x_col0=x_col0)
    now = raw(ops, y)
    flat = now[0]
    out = np.empty((L, M), dtype=np.float32)
    used = np.zeros(size, dtype=bool)
    for h in range(nblk):
        lo, hi = h * tb, min(M, (h + 1) * tb)
        w = hi - lo + pad
        at = h * L * (tb + pad)
        out[:, lo:hi] = flat[at:at + L * w].reshape(L, w)[:, :hi - lo]
        u = used[at:at + L * w].reshape(L, w)
        u[:, :hi - lo] = True
    s = X.SENTINEL.view(np.uint32)
    assert (flat.view(np.uint32)[~used] == s).all() and (now[1].view(np.uint32) == s).all(), "chunk padding overwritten"
    check_untouched(ops, xw)
    return out


@pytest.mark.parametrize("shape", X.LEG1_FUSED)
def test_leg1_every_path_gives_the_reference_bits(ops, shape):
    """One graph, one operand: the one-launch kernel under every knob that changes its plan (dense-set threshold, units,
    groups, launch order, id width), the two-launch leg, the gather kernels on both layouts at every panel width, the
    block-dense part — ONE array of bits, the reference."""
    M, K, L = shape
    csr = X.corner_case(M, K, M + L, hubs=min(K, 150))
    op = X.summable_operand(csr, L, seed=L)
    x32 = f32(op.X)
    want = f32(X.product64(csr, op.X))
    split = dict(fuse_rows=400)
    fused = [dict(fuse_min=2), dict(fuse_min=4), dict(fuse_unit=4, **split), dict(fuse_unit=6, **split),
             dict(fuse_unit=32, **split), dict(fuse_group=1), dict(fuse_group=4, fuse_min=4), dict(ids16=0),
             dict(fuse_min=100)]
    fused += [dict(fuse_min=3, fuse_steps=2, fuse_unit=4, fuse_rows=400, fuse_order=o) for o in (1, 2, 3)]
    ran_cores = 0
    for kw in fused:
        with knobs(ops, **kw):
            g = ops.graph(csr)
            steps, cov, rem = ops.fused_stats(g)
            assert cov + rem == csr.nnz
            ran_cores += cov > 0
            assert kw.get("ids16", 1) or ops.graph_get(g, "fused_ids16") == 0
            equal_bits(leg1_blocked(ops, g, x32, M), want.T, f"one-launch leg 1 {kw}")
    assert ran_cores >= 8                                          # (the matrix-core phase ran: these graphs have dense sets)
    with knobs(ops, fuse=0):
        g0 = ops.graph(csr)
        assert ops.fused_stats(g0) == (0, 0, csr.nnz)
        equal_bits(leg1_blocked(ops, g0, x32, M), want.T, "two-launch leg 1 (fuse=0, blocked)")
    for panel in (0, 16, 32, 64, 128, 256):
        with knobs(ops, panel=panel, fuse=0):
            g = ops.graph(csr)
            equal_bits(leg_rowmajor(ops, g, x32, M, False), want, f"gather, panel {panel}")
            equal_bits(leg_rowmajor(ops, g, x32, M, True), want.T, f"gather transposed, panel {panel}")
    with knobs(ops, fuse=0):
        g = ops.graph(csr)
        for pad in (1, 2, 3):                                      # an ld off the 16-byte grid: the scalar variant
            equal_bits(leg_rowmajor(ops, g, x32, M, False, pad=pad), want, f"scalar variant, ld + {pad}")
        equal_bits(leg_rowmajor(ops, g, x32, M, True, pad=1), want.T, "scalar variant, transposed")
    with knobs(ops, dense_min=3, dense_cols=32, dense_sym=1, fuse=0):
        g = ops.graph(csr)
        nt, dk, cov = ops.dense_stats(g)
        assert M < 500 or (nt >= 1 and 0 < cov < csr.nnz)
        equal_bits(leg_rowmajor(ops, g, x32, M, False), want, "block-dense part + gather")
        equal_bits(leg_rowmajor(ops, g, x32, M, True), want.T, "block-dense part + gather, transposed")
    g = ops.graph(csr)                                             # the one-launch leg on a row-major operand
    equal_bits(leg_rowmajor(ops, g, x32, M, True), want.T, "one-launch leg 1, row-major")


@pytest.mark.parametrize("shape", X.LEG1_GATHER)
@pytest.mark.parametrize("panel", [0, 16, 32, 64, 128, 256])
def test_gather_path_with_empty_and_long_rows(ops, shape, panel):
    """random_csr: rows without entries, rows without weight, two long rows; every panel width, plain and transposed (one
    block with pitched rows, and per-destination chunks with padding)."""
    M, K, L = shape
    csr = X.gather_case(M, K, M + L)
    op = X.summable_operand(csr, L, seed=panel)
    x32, want = f32(op.X), f32(X.product64(csr, op.X))
    with knobs(ops, panel=panel, fuse=0):
        g = ops.graph(csr)
        equal_bits(leg_rowmajor(ops, g, x32, M, False), want, "plain")
        equal_bits(leg_rowmajor(ops, g, x32, M, True), want.T, "transposed")
        equal_bits(leg_rowmajor(ops, g, x32, M, False, pad=3), want, "scalar variant")
        for tb, pad in ((max(1, M // 3), 5), (16 if M >= 16 else 2, 0)):
            equal_bits(leg_chunked(ops, g, guarded(ops, K, L, x32), 0, L, M, tb, pad), want.T, f"t_block {tb} t_pad {pad}")


def test_dense_set_cut_into_units_adds_its_slabs_exactly(ops):
    """A dense set of more than 2048 columns is cut into units with one slab of partial sums each, added in memory."""
    M, K, L = X.LEG1_UNITS
    csr = X.corner_case(M, K, 3, hubs=5500, p_hub=0.6)
    op = X.summable_operand(csr, L, seed=8)
    x32, want = f32(op.X), f32(X.product64(csr, op.X))
    with knobs(ops, fuse=0):
        g = ops.graph(csr)                                         # the dense part's default knobs
        nt, dk, cov = ops.dense_stats(g)
        assert nt >= 1 and dk > 2048 + 2048
        equal_bits(leg_rowmajor(ops, g, x32, M, False), want, "slabs, plain")
        equal_bits(leg_rowmajor(ops, g, x32, M, True), want.T, "slabs, transposed")
    for unit in (4, 32, 1 << 20):                                  # the one-launch kernel's units meet in memory too
        with knobs(ops, fuse_unit=unit):
            g = ops.graph(csr)
            assert ops.fused_stats(g)[0] > 16 * 4
            equal_bits(leg1_blocked(ops, g, x32, M), want.T, f"one-launch, fuse_unit {unit}")


def test_star_rows_go_to_the_matrix_cores_whole(ops):
    csr = X.star_case()
    op = X.summable_operand(csr, 257, seed=4)
    x32, want = f32(op.X), f32(X.product64(csr, op.X))
    g = ops.graph(csr)
    steps, cov, rem = ops.fused_stats(g)
    assert cov >= 1500 + 500 and steps >= 1500 // 16
    equal_bits(leg1_blocked(ops, g, x32, 1500), want.T, "star")


def test_ids_beyond_16_bits(ops):
    csr = X.wide_ids_case(65537)
    op = X.summable_operand(csr, 64, seed=9)
    x32, want = f32(op.X), f32(X.product64(csr, op.X))
    for fuse_min in (2, 100):
        with knobs(ops, fuse_min=fuse_min):
            g = ops.graph(csr)
            assert ops.graph_get(g, "fused_ids16") == 0
            equal_bits(leg1_blocked(ops, g, x32, csr.n_rows), want.T, f"K = 65537, fuse_min {fuse_min}")


@pytest.mark.parametrize("shape,tb,pad", X.LEG1_SHARD)
def test_leg1_on_a_sharded_ranks_operand(ops, shape, tb, pad):
    """What one rank of a column-sharded update holds: a row-major column block of a wider matrix, the transposed result in the
    chunks of the all-to-all — the one-launch kernel and the gather kernels (fuse_shards = 0)."""
    M, K, L = shape
    csr = X.corner_case(M, K, M + L, hubs=min(K, 200), p_hub=0.4)
    op = X.summable_operand(csr, L + 64, seed=6)
    c0 = 32
    want = f32(X.product64(csr, op.X[:, c0:c0 + L]))
    for kw in (dict(), dict(fuse_shards=0)):
        with knobs(ops, **kw):
            g = ops.graph(csr)
            xw = guarded(ops, K, L + 64, f32(op.X))
            if tb == 0:
                y = guarded(ops, L, M)
                ops.spmm(g, xw, y, n_cols=L, transpose_out=True, x_col0=c0)
                got = ops.download(y)
                check_untouched(ops, xw, y)
            else:
                got = leg_chunked(ops, g, xw, c0, L, M, tb, pad)
            equal_bits(got, want.T, f"sharded operand {kw}")


# ---- leg 2 with the epilogue, and the count -----------------------------------------------------------------------
EPS = 1.0          # a power of two on every element's grid (the results are integers times 2^-18 and coarser)


def _ep(put, counts, prior, lbd, prev, symmetric, **kw):
    ep = dict(coef=0.5, previous=put(prev), eps=EPS, diag_col0=0, symmetric=symmetric, **kw)
    if counts is not None:
        ep["evidence"] = put(counts, np.uint8)
    if prior is not None:
        ep.update(apriori=put(f32(prior)), lbd=lbd)
    return ep


def _leg2(ops, g, tt32, n, blocked, symmetric, counts, prior, lbd, prev, **kw):
    """-> (result, exact count, count_any's count); every operand and the result guarded."""
    mk = guarded_blocked if blocked else guarded
    ins = []

    def put(a, dtype=np.float32):
        ins.append(mk(ops, a.shape[0], a.shape[1], a, dtype))
        return ins[-1]
    x = put(tt32)
    ep = _ep(put, counts, prior, lbd, prev, symmetric, **kw)
    y = mk(ops, n, tt32.shape[1])
    ops.spmm(g, x, y, epilogue=ep)
    got, exact = ops.download(y), ops.read_changed()
    y2 = mk(ops, n, tt32.shape[1])
    ops.spmm(g, x, y2, epilogue=dict(ep, count_any=True))
    some = ops.read_changed()
    assert np.array_equal(ops.download(y2), got)
    check_untouched(ops, y, y2, *ins)
    return got, exact, some


def _check_counts(run, want32, what, planted=None):
    """`run(previous)` -> (result, exact count, count_any count) against planted ties: the reference's strict > count; then
    with nothing above eps: zero, both forms.  `planted`: (all three kinds, "on" and "below" only) of X.plant_previous made
    elsewhere from the same reference at places of the caller's (default: here, at X.tie_places)."""
    n, L = want32.shape
    if planted is None:
        sym = n == L and np.array_equal(want32, want32.T)
        places = X.tie_places(n, L)
        planted = (X.plant_previous(want32, EPS, places, symmetric=sym),
                   X.plant_previous(want32, EPS, places, symmetric=sym, only=("on", "below")))
    p, q = planted
    assert p.count > 0
    got, exact, some = run(p.previous)
    equal_bits(got, want32, what)
    assert exact == p.count, (what, exact, p.count, p.kinds[:24])
    assert 0 < some <= exact, (what, some, exact)
    assert q.count == 0
    got, exact, some = run(q.previous)
    equal_bits(got, want32, what)
    assert exact == 0 and some == 0, (what, exact, some)           # ties and near misses: a >= would count them


# every form of leg 2 with the epilogue: (what, knobs of the graph, panel-blocked operands, upper triangle + mirror) — shared
# with tests/test_gpu_exact_rect.py, which runs the same list on rectangular patterns
LEG2_FORMS = [("row-major full (gather3)", dict(fuse=0), False, False),
              ("row-major triangle (gather3)", dict(fuse=0), False, True),
              ("row-major full, panel 64 (emit_row)", dict(fuse=0, panel=64), False, False),
              ("row-major triangle, lean=0 (emit_row)", dict(fuse=0, lean=0), False, True),
              ("row-major, block-dense part", dict(fuse=0, dense_min=3, dense_cols=32, dense_sym=1), False, True),
              ("blocked one-launch (fused)", dict(fuse_sym=1), True, True),
              ("blocked one-launch, 32-bit ids", dict(fuse_sym=1, ids16=0), True, True),
              ("blocked one-launch, split blocks", dict(fuse_sym=1, fuse_min=3, fuse_steps=2, fuse_unit=4, fuse_rows=400), True, True),
              ("blocked one-launch, fuse_group 1", dict(fuse_sym=1, fuse_group=1), True, True),
              ("blocked two-launch (gather3 kSym)", dict(fuse_sym=0), True, True),
              # ... and the same leg saying which of its two paths it runs (dense_sym=0: no dense part whatever the
              # pattern, so that the launch is the one the rule of tests/leg2_rule.py speaks about)
              ("blocked two-launch, general path (gather3 kSym)", dict(fuse_sym=0, dense_sym=0, balance=2, leg2_short=0), True, True),
              ("blocked two-launch, short path (gather3 kSym SHORT)", dict(fuse_sym=0, dense_sym=0, balance=2, leg2_short=16), True, True),
              ("blocked full form", dict(fuse_sym=0), True, False)]


def _leg2_scalar(ops, g, tt32, n, counts, prior, lbd, prev):
    """An ld off the 16-byte grid: the scalar kernel (no triangle form there).  -> as _leg2."""
    put = lambda a, dtype=np.float32: guarded(ops, a.shape[0], a.shape[1], a, dtype, pad=1)
    x, y = put(tt32), guarded(ops, n, n, pad=1)
    ep = _ep(put, counts, prior, lbd, prev, False)
    ops.spmm(g, x, y, epilogue=ep)
    got, exact = ops.download(y), ops.read_changed()
    ops.spmm(g, x, y, epilogue=dict(ep, count_any=True))
    some = ops.read_changed()
    check_untouched(ops, x, y)
    return got, exact, some


@pytest.mark.parametrize("n", X.LEG2_N)
@pytest.mark.parametrize("variant", ["plain", "evidence", "all"])
def test_leg2_every_form_gives_the_reference_bits_and_the_strict_count(ops, n, variant):
    """A symmetric leg 2 (Tt = (W S)^T of a symmetric S, exactly): the full form and the upper triangle + mirror of spmm.hip on
    both layouts (gather3's emit_row3, spmm.hip:864; the wider-panel kernel's emit_row, :252, vector and scalar), the
    one-launch leg 2 of fused.hip (:615) whole, with split blocks, grouped units and 32-bit ids, the two-launch symmetric
    leg with the block-dense part, and the standalone epilogue (:1468)."""
    csr, sym, counts, prior, lbd, want = X.leg2_case(n, variant)
    want32, tt32 = f32(want), f32(sym.Tt)
    lengths = np.diff(csr.rowptr).tolist()
    for what, kw, blocked, symmetric in LEG2_FORMS:
        with knobs(ops, **kw):
            g = ops.graph(csr)
            if "one-launch" in what:
                assert ops.fused_stats(g)[1] > 0 and ops.graph_get(g, "fused_ids16") == kw.get("ids16", 1)
            _check_counts(lambda prev: _leg2(ops, g, tt32, n, blocked, symmetric, counts, prior, lbd, prev), want32, what)
            if "leg2_short" in kw:
                rule = short_groups(lengths, kw["leg2_short"])
                assert ops.graph_get(g, "leg2_short_groups") == rule == ops.graph_get(g, "leg2_short_taken"), (what, rule)
                assert kw["leg2_short"] or rule == 0
    # an ld off the 16-byte grid: the scalar kernel (no triangle form there)
    with knobs(ops, fuse=0):
        g = ops.graph(csr)
        _check_counts(lambda prev: _leg2_scalar(ops, g, tt32, n, counts, prior, lbd, prev), want32, "scalar variant")
    # the un-fused epilogue on the exact product

    def standalone(prev):
        put = lambda a, dtype=np.float32: guarded(ops, a.shape[0], a.shape[1], a, dtype)
        q, y = put(f32(X.product64(csr, sym.Tt) / 1.0)), guarded(ops, n, n)
        ep = _ep(put, counts, prior, lbd, prev, False)
        ops.epilogue_apply(q, y, n, n, ep)
        got, exact = ops.download(y), ops.read_changed()
        check_untouched(ops, q, y)
        return got, exact, exact
    _check_counts(standalone, want32, "epilogue_apply")


@pytest.mark.parametrize("n", [129, 1031])
def test_leg2_restricted_to_the_support_of_the_evidence(ops, n):
    """epilogue restrict_support (forced, as tests/test_gpu_restricted.py forces it: fuse_sym = 0): lane groups whose 32 counts
    are all zero skip their gathers — whole 32-column segments of zero counts are planted so that some are skipped."""
    csr, sym, counts, prior, lbd, want = X.leg2_case(n, "all")
    rng = np.random.default_rng(n)
    counts = counts.copy()
    nt = -(-n // 32)
    for t in rng.choice(nt * nt, size=nt * nt // 2, replace=False):
        i, j = divmod(int(t), nt)
        counts[32 * i:32 * i + 32, 32 * j:32 * j + 32] = 0
        counts[32 * j:32 * j + 32, 32 * i:32 * i + 32] = 0
    want32 = f32(X.exact_epilogue(X.product64(csr, sym.Tt), 0.5, counts, prior, lbd))
    tt32 = f32(sym.Tt)
    for blocked, symmetric in ((True, True), (False, True), (False, False)):
        with knobs(ops, fuse_sym=0, fuse=0 if not blocked else 1, restrict_support=1):
            g = ops.graph(csr)
            _check_counts(lambda prev: _leg2(ops, g, tt32, n, blocked, symmetric, counts, prior, lbd, prev,
                                             restrict_support=True), want32, f"restricted, blocked={blocked}, triangle={symmetric}")


@pytest.mark.parametrize("n", [129, 520])
def test_gemm_nt_with_the_epilogue(ops, n):
    """dense.hip (v_mfma_f32_32x32x2_f32): C = W . Tt as A . B^T with the epilogue and the count of dense.hip:165."""
    csr, sym, counts, prior, lbd, want = X.leg2_case(n, "all")
    want32 = f32(want)
    A, B = f32(dense64(csr).toarray()), f32(sym.Tt.T)

    def run(prev):
        put = lambda a, dtype=np.float32: guarded(ops, a.shape[0], a.shape[1], a, dtype)
        a, b, c = put(A), put(B), guarded(ops, n, n)
        ep = _ep(put, counts, prior, lbd, prev, False)
        ops.gemm_nt(a, b, c, n, n, n, epilogue=ep)
        got, exact = ops.download(c), ops.read_changed()
        check_untouched(ops, a, b, c)
        return got, exact, exact
    _check_counts(run, want32, "gemm_nt")


def _shard_graph(world, mb, balance, ops):
    n = world * mb
    rng = np.random.default_rng(world * 1000 + mb)
    lens = np.minimum(n, (rng.pareto(1.1, size=n) * 5).astype(int) + (rng.random(n) < 0.9))
    lens[rng.choice(n, 3, replace=False)] = [n, n // 2, 300 % n]
    lens = np.concatenate([np.sort(lens[h * mb:(h + 1) * mb]) for h in range(world)])
    rows = [np.sort(rng.choice(n, size=d, replace=False)) for d in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    csr = X.pow2_rowscale(CSR(n, n, rowptr, np.concatenate(rows).astype(np.int32), np.ones(n)), n)
    with knobs(ops, balance=balance, dense_min=0):
        return csr, ops.graph(csr)


@pytest.mark.parametrize("world,mb,balance", [(2, 64, 2), (4, 128, 2), (3, 96, 0), (8, 32, 2)])
def test_half_form_shard_leg2(ops, world, mb, balance):
    """simrank_spmm_shard and its staged form: tiles i <= j with the reference's bits, i < j also transposed (in place for
    the rank's own shard, else packed in the send chunk), everything else untouched; a mirrored element counts twice — on
    planted ties, from the reference."""
    n, T = world * mb, mb // 32
    csr, g = _shard_graph(world, mb, balance, ops)
    chunk = max(1, T * (T - 1) // 2 * 1024)
    for rank in (0, world - 1):
        op = X.summable_operand(csr, mb, headroom=3, seed=rank, exponents=(0, 0))
        counts = X.epilogue_counts((n, mb), rank)
        want32 = f32(X.exact_epilogue(X.product64(csr, op.X), 0.5, counts, diag_col0=rank * mb))
        p = X.plant_previous(want32, EPS, [(rank * mb + r, c) for r, c in X.tie_places(mb, mb)] + [(0, 0), (n - 1, mb - 1)])
        moved = np.abs(want32.astype(np.float64) - p.previous.astype(np.float64)) > EPS
        assert moved.sum() == p.count > 0
        stagings = [[(0, T)]] + ([[(0, 1), (1, T)]] if T > 1 else []) + ([[(0, 2), (2, 3), (3, T)]] if T > 3 else [])
        for stages in stagings:
            put = lambda a, dtype=np.float32: guarded(ops, a.shape[0], a.shape[1], a, dtype)
            x, y, send = put(f32(op.X)), guarded(ops, n, mb), guarded(ops, 1, world * chunk, ld=world * chunk)
            ep = dict(coef=0.5, evidence=put(counts, np.uint8), previous=put(p.previous), eps=EPS, diag_col0=rank * mb)
            want = np.full((n, mb), X.SENTINEL, np.float32)
            want_send = np.full(world * chunk, X.SENTINEL, np.float32)
            want_changed = 0
            for k, (lo, hi) in enumerate(stages):
                # a stage's range of every chunk sits together (the solver's layout): world * (slots before it) floats in
                slot0 = lo * (lo - 1) // 2
                stage_chunk = (hi * (hi - 1) // 2 - slot0) * 1024
                off = world * slot0 * 1024
                if len(stages) == 1:
                    ops.spmm_shard(g, x, y, dict(ep), rank, world, send, chunk)
                    stage_chunk = chunk
                else:
                    ops.spmm_shard_stage(g, x, y, dict(ep), rank, world, send, off, stage_chunk, lo, hi, k == 0)
                for h in range(world):
                    for i in range(T):
                        r = slice(h * mb + 32 * i, h * mb + 32 * i + 32)
                        for j in range(max(i, lo), hi):
                            c = slice(32 * j, 32 * j + 32)
                            want[r, c] = want32[r, c]
                            want_changed += int(moved[r, c].sum()) * (2 if i < j else 1)
                            if i < j and h == rank:
                                want[rank * mb + 32 * j:rank * mb + 32 * j + 32, 32 * i:32 * i + 32] = want32[r, c].T
                            elif i < j:
                                at = off + h * stage_chunk + (j * (j - 1) // 2 + i - slot0) * 1024
                                want_send[at:at + 1024] = want32[r, c].T.reshape(-1)
            got, changed, sent = raw(ops, y)[:n, :mb], ops.read_changed(), raw(ops, send)[0]
            assert same_bits(got, want), f"rank {rank}, stages {stages}"
            assert same_bits(sent, want_send), f"rank {rank}, stages {stages}: send chunks"
            assert changed == want_changed, (rank, stages, changed, want_changed)
            check_untouched(ops, x, y, send)


# ---- fp16-held matrices (half.hip) ----------------------------------------------------------------------------------
@pytest.fixture
def hops(ops):
    # half.hip takes whole blocks (no units whose sums meet in memory), as fits on fp16-held matrices create their graphs
    with knobs(ops, fuse_unit=1 << 20):
        yield ops


def stored16(v64, scale):
    """What an fp16-held matrix stores for exact values v: v x scale rounded ONCE to nearest-even; as float64."""
    return (np.asarray(v64, dtype=np.float64) * scale).astype(np.float16).astype(np.float64)


def half_values(ops, m):
    """The stored fp16 numbers of a panel-blocked fp16 matrix (float64 [rows, cols]) and whether its padding is untouched."""
    now = raw(ops, m)
    v = now[:m.panels * m.rows_pad].reshape(m.panels, m.rows_pad, 64)
    out = np.concatenate([v[p, :m.rows] for p in range(m.panels)], axis=1)[:, :m.cols]
    return out.astype(np.float64)


@pytest.mark.parametrize("shape", [(520, 400, 333), (129, 77, 65), (64, 1000, 96), (2100, 2100, 160)])
@pytest.mark.parametrize("scale", [1.0, 16384.0])
def test_half_leg1_is_the_exact_sum(hops, shape, scale):
    """Operands held as half x 2^14 and half x 1 (11-bit budget): the f32 sums are exact, and so is the fp16 result."""
    ops = hops
    M, K, L = shape
    csr = X.corner_case(M, K, M + L, hubs=min(K, 150))
    lo = -14 - int(np.log2(scale))
    op = X.summable_operand(csr, L, mantissa=11, seed=L, exponents=(lo, lo + 18))
    want = stored16(X.product64(csr, op.X).T, scale)
    assert np.array_equal(want, X.product64(csr, op.X).T * scale)            # (no rounding at all: sums below 2^11 steps)
    for fuse_min in (2, 4, 128):
        with knobs(ops, fuse_min=fuse_min):
            g = ops.graph(csr)
            x = guarded_blocked(ops, K, L, op.X, np.float16, scale)
            yt = guarded_blocked(ops, L, M, None, np.float16, scale)
            ops.spmm(g, x, yt, transpose_out=True)
            got = half_values(ops, yt)
            check_untouched(ops, x, yt)
            assert np.array_equal(got, want), (fuse_min, int((got != want).sum()))


def _half_leg2(ops, csr, g, Tt, counts, prior, lbd, prev_stored, eps_stored, scale, symmetric, col0=0):
    n, L = csr.n_rows, Tt.shape[1]
    x = guarded_blocked(ops, Tt.shape[0], L, Tt, np.float16, scale)
    pv = guarded_blocked(ops, n, L, prev_stored / scale, np.float16, scale)
    y = guarded_blocked(ops, n, L, None, np.float16, scale)
    ins = [x, pv]
    ep = dict(coef=0.5, previous=pv, eps=eps_stored / scale, set_diag=True, symmetric=symmetric, diag_col0=col0)
    if counts is not None:
        ins.append(guarded_blocked(ops, n, L, counts, np.uint8))
        ep["evidence"] = ins[-1]
    if prior is not None:
        ins.append(guarded_blocked(ops, n, L, f32(prior)))
        ep.update(apriori=ins[-1], lbd=lbd)
    ops.spmm(g, x, y, epilogue=ep)
    got, changed = half_values(ops, y), ops.read_changed()
    ops.spmm(g, x, y, epilogue=dict(ep, count_any=True))
    some = ops.read_changed()
    assert np.array_equal(half_values(ops, y), got)
    check_untouched(ops, y, *ins)
    return got, changed, some


HALF_EPS = 2.0 ** -6 + 2.0 ** -12          # stored units: eps + half the spacing below 1 (2^-12) is a whole spacing there


@pytest.mark.parametrize("n", [64, 129, 520, 2100])
@pytest.mark.parametrize("variant,scale", [("plain", 1.0), ("evidence", 1.0), ("all", 1.0), ("evidence", 16384.0), ("all", 16384.0)])
def test_half_leg2_rounds_the_exact_result_once_and_counts_by_its_rule(hops, n, variant, scale):
    """Upper triangle + mirror on fp16-held matrices: the stored result is the exact value rounded ONCE to nearest-even; the
    count follows half.hip's header — |new before rounding - old stored| > eps + half the spacing at old — computed from the
    reference, with planted differences a spacing and more off that bound on either side and one exactly on it (the
    diagonal: new = 1, old = 1 - eps - 2^-12 in stored units)."""
    e = -6 - int(np.log2(scale))
    half_leg2_protocol(hops, X.leg2_case(n, variant, mantissa=11, exponent=e), scale)


def half_leg2_protocol(ops, case, scale):
    """The protocol of the test above on one case of X.leg2_on (a square pattern, or — tests/test_gpu_exact_rect.py — an
    n x K one: the operand has K rows, everything else n)."""
    csr, sym, counts, prior, lbd, want = case
    n = csr.n_rows
    assert scale == 1.0 or np.abs(want).max() < 4
    want_st = want * scale                                                     # exact, before rounding
    places = [rc for rc in X.tie_places(n, n) if rc[0] < rc[1]]
    prev, kinds = X.plant_previous_half(want_st, HALF_EPS, places, symmetric=True)
    d = n // 2
    prev[d, d] = scale - HALF_EPS * 1.0 - 2.0 ** -12 if scale == 1.0 else prev[d, d]
    if scale == 1.0:
        assert float(np.float16(prev[d, d])) == prev[d, d] and abs(1.0 - prev[d, d]) == HALF_EPS + X.half_spacing(prev[d, d])
    moved = X.half_moved(want_st, prev, HALF_EPS)
    assert moved.sum() == 2 * kinds.count("above") and not moved[d, d]
    g = ops.graph(csr)
    got, changed, some = _half_leg2(ops, csr, g, sym.Tt, counts, prior, lbd, prev, HALF_EPS, scale, True)
    assert np.array_equal(got, stored16(want, scale)), int((got != stored16(want, scale)).sum())
    assert changed == int(moved.sum()) and 0 < some <= changed
    # nothing beyond the widened eps (the tie stays): zero
    quiet = stored16(want, scale)
    quiet[d, d] = prev[d, d]
    assert not X.half_moved(want_st, quiet, HALF_EPS).any()
    got, changed, some = _half_leg2(ops, csr, g, sym.Tt, counts, prior, lbd, quiet, HALF_EPS, scale, True)
    assert np.array_equal(got, stored16(want, scale)) and changed == 0 and some == 0


@pytest.mark.parametrize("n,col0,L", [(520, 128, 192), (1000, 936, 64), (200, 64, 136)])
@pytest.mark.parametrize("variant,scale", [("plain", 1.0), ("evidence", 16384.0)])
def test_half_leg2_full_form_on_a_column_block(hops, n, col0, L, variant, scale):
    """The column block [col0, col0 + L) of a sharded update on fp16-held matrices: every element once, each moved element
    counted once, the diagonal where row == col0 + column."""
    ops = hops
    csr = X.corner_case(n, n, n + L, hubs=min(n, 120))
    lo = -8 - int(np.log2(scale))
    op = X.summable_operand(csr, L, mantissa=11, seed=col0, exponents=(lo, lo))
    counts = X.epilogue_counts((n, L), n) if variant == "evidence" else None
    want = X.exact_epilogue(X.product64(csr, op.X), 0.5, counts, diag_col0=col0)
    want[np.arange(col0, col0 + L), np.arange(L)] = 1.0
    want_st = want * scale
    prev, kinds = X.plant_previous_half(want_st, HALF_EPS, X.tie_places(n, L))
    moved = X.half_moved(want_st, prev, HALF_EPS)
    assert moved.sum() == kinds.count("above") > 0
    g = ops.graph(csr)
    got, changed, some = _half_leg2(ops, csr, g, op.X, counts, None, None, prev, HALF_EPS, scale, False, col0)
    assert np.array_equal(got, stored16(want, scale)), int((got != stored16(want, scale)).sum())
    assert changed == int(moved.sum()) and 0 < some <= changed
