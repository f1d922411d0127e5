"""The evidence counts where the existing tests stop: more than 65 536 columns (a second pass of the LDS-counter kernel,
the upper triangle in two passes, the rule that decides between triangle and full form), the largest single pass
(65 536 columns, 128 KiB of LDS), pairs with up to 65 536 common neighbours (the counter cap at 0x4000), the caps of the
hub list (more than 4096 candidates, fewer than 8, a hub count saturated before the walk adds tens of thousands), and
every store path next to memory it must not touch.

Every case runs under three tunings (hub columns + triangle, hub columns + full form, LDS counters alone + triangle),
asserts the graph's "ev_hubs" against the rule restated in tests/evidence_ref.py before it looks at a count, and
compares ALL bytes of the output — the block, its guard columns, guard row and padding, pre-filled with 0xA5 — with
min(P P^T, 255) from tests/evidence_ref.py.  Integer arithmetic: no tolerance anywhere.  The expected image of an output
is built once on the host and shared by the three tunings; the output comes down in chunks, so a 4.3 GB case costs its
download and one pass of comparison per tuning.  tests/test_evidence_cpu.py pins what the patterns hold."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import evidence_ref as E

pytestmark = pytest.mark.gpu
RTOL = 1e-5
TUNINGS = [("hubs+tri", True, 1), ("hubs+full", True, 0), ("walk+tri", False, 1)]
CHUNK = 1 << 28                     # bytes of an output brought down at a time
HEADROOM = 4 << 30


@pytest.fixture(scope="module")
def ops():
    from simrank_amd.engine import HipOps
    return HipOps(0)


def geometry(M, L, blocked, ld):
    """(rows_pad, ld, bytes of a unit, units) of an output image: a unit is a panel of the blocked layout (rows padded as
    engine.Matrix pads them) or a row of the row-major one, whose last row is a guard row."""
    if blocked:
        from simrank_amd.engine import BLOCK_PAD_ROWS
        rows_pad = -(-M // 8) * 8 + BLOCK_PAD_ROWS
        return rows_pad, 32, rows_pad * 32, -(-L // 32)
    assert ld >= L
    return 0, ld, ld, M + 1


class Out:
    """Device memory for an M x L block of counts: panel-blocked (padding rows behind every panel, padding columns behind
    the last one) or row-major with pitch ld (guard columns where ld > L) and one guard row; `skew` bytes off the
    allocation's alignment.  Quacks like engine.Matrix for HipOps.evidence_counts.  `image(R, col0)` is what it must hold
    after the counts of columns [col0, col0 + L) went into memory that was 0xA5 throughout."""

    def __init__(self, ops, M, L, blocked, ld=None, skew=0):
        self.ops, self.M, self.L, self.cols, self.blocked = ops, M, L, L, blocked
        self.rows_pad, self.ld, self.unit, self.units = geometry(M, L, blocked, ld)
        self.nbytes = self.unit * self.units
        self.base = ops._malloc(self.nbytes + 16)
        self.ptr = self.base + skew
        assert self.base % 16 == 0 and skew < 16
        self.what = f"{M} x {L} {'blocked' if blocked else f'row-major ld {ld}'} skew {skew}"

    def free(self):
        if self.base:
            self.ops._free(self.base)
        self.base = self.ptr = 0

    def __del__(self):
        self.free()

    def prefill(self):
        from simrank_amd.engine import check
        check(self.ops.lib.simrank_memset(C.c_void_p(self.base), E.GUARD, self.nbytes + 16, self.ops.stream), "simrank_memset")

    def offsets(self, r, c):
        r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
        return ((c >> 5) * self.rows_pad + r) * 32 + (c & 31) if self.blocked else r * self.ld + c

    def where(self, off):
        """(row, column) of a byte of the image; rows >= M and columns >= L are guards."""
        if self.blocked:
            panel, rest = divmod(off, self.unit)
            return rest // 32, panel * 32 + rest % 32
        return divmod(off, self.ld)

    def image(self, R, col0):
        img = np.zeros(self.nbytes, dtype=np.uint8)
        if self.blocked:
            v = img.reshape(self.units, self.rows_pad, 32)
            v[:, self.M:, :] = E.GUARD
            if self.L % 32:
                v[-1, :, self.L % 32:] = E.GUARD
        else:
            v = img.reshape(self.M + 1, self.ld)
            v[:, self.L:] = E.GUARD
            v[self.M] = E.GUARD
        blk = (R if (col0 == 0 and self.L == R.shape[1]) else R[:, col0:col0 + self.L]).tocoo()
        assert blk.nnz == 0 or blk.data.min() > 0
        img[self.offsets(blk.row, blk.col)] = blk.data.astype(np.uint8)
        return img

    def assert_holds(self, img, what):
        buf = np.empty(min(CHUNK, self.nbytes), dtype=np.uint8)
        for s in range(0, self.nbytes, CHUNK):
            e = min(self.nbytes, s + CHUNK)
            got, want = buf[:e - s], img[s:e]
            self.ops.d2h(got, self.ptr + s)
            self.ops.synchronize()
            if np.array_equal(got, want):
                continue
            bad = np.flatnonzero(got != want)
            first = [(self.where(s + int(i)), int(got[i]), int(want[i])) for i in bad[:8]]
            pytest.fail(f"{what}, {self.what}: {bad.size} wrong bytes in [{s}, {e}); ((row, column), got, want): {first}")


def need_memory(nbytes):
    from simrank_amd import _f64
    free, total = C.c_int64(0), C.c_int64(0)
    _f64.check(_f64.load().simrank_f64_mem_info(C.byref(free), C.byref(total)), "simrank_f64_mem_info")
    print(f"device memory: {free.value / 2 ** 30:.1f} GiB free of {total.value / 2 ** 30:.1f} GiB; needed {nbytes / 2 ** 30:.1f} GiB")
    if free.value < nbytes + HEADROOM:
        pytest.skip(f"the device reports {free.value / 2 ** 30:.1f} GiB free, the case needs {nbytes / 2 ** 30:.1f} GiB plus "
                    f"{HEADROOM / 2 ** 30:.0f} GiB of headroom")


def run_case(ops, case, outputs, R=None):
    """outputs: [(col0, Out)].  Three graphs, one per tuning; every output under each of them."""
    p = case.pattern
    R = E.counts(p) if R is None else R
    images = [out.image(R, col0) for col0, out in outputs]
    for name, hubs_on, tri in TUNINGS:
        ev_hub = case.ev_hub if hubs_on else 0
        g = ops.graph(p, knobs=dict(ev_hub=ev_hub, ev_tri=tri))
        assert ops.graph_get(g, "ev_hubs") == len(E.hubs(p, ev_hub)), (name, ops.graph_get(g, "ev_hubs"))
        for (col0, out), img in zip(outputs, images):
            out.prefill()
            ops.evidence_counts(g, col0, out)
            out.assert_holds(img, f"{name} (ev_hub {ev_hub}, ev_tri {tri}), columns [{col0}, {col0 + out.L})")
        g.free()
    for _, out in outputs:
        out.free()


def small_outputs(ops, M, blocks):
    """Each block panel-blocked (16-byte aligned, and 4 bytes off: no 16-byte stores), row-major on a pitch of whole
    16-byte lines (4- and 16-byte stores, their tails where L is not a multiple) and row-major on an odd pitch one byte
    off alignment (byte stores)."""
    outs = []
    for col0, L in blocks:
        outs += [(col0, Out(ops, M, L, True)), (col0, Out(ops, M, L, False, ld=-(-L // 16) * 16 + 16)),
                 (col0, Out(ops, M, L, False, ld=L + 1 + L % 2, skew=1)), (col0, Out(ops, M, L, True, skew=4))]
    return outs


def test_counter_cap(ops):
    """(a) Pairs with exactly 65 536, 65 535, 16 384, 16 383, 255 and 254 common neighbours side by side in one row of
    counters; the column blocks (1, M - 1) and (2, 5) flip the half of the LDS word each of them lands in and end off the
    4-byte grid.  No hub part whatever ev_hub says."""
    case = E.cap_case()
    M = case.pattern.n_rows
    assert len(E.hubs(case.pattern, case.ev_hub)) == 0
    run_case(ops, case, small_outputs(ops, M, [(0, M), (1, M - 1), (2, 5)]))


def test_hub_list_cut_at_4096_and_a_saturated_hub_count(ops):
    """(b) 5000 candidate columns: 4096 on the matrix cores, 904 left to the walk; rows 0 and 1 come out of the hub
    product at 255 and the walk adds 61 440."""
    case = E.cap_case(hub_rows=64)
    M = case.pattern.n_rows
    assert len(E.hubs(case.pattern, case.ev_hub)) == 4096
    run_case(ops, case, small_outputs(ops, M, [(0, M), (1, M - 1), (2, 5)]))


@pytest.mark.parametrize("n_planted", [7, 8])
def test_hub_list_of_seven_is_none_and_of_eight_is_eight(ops, n_planted):
    """(b) Seven candidates: no hub part; eight: an image of 32 columns, 24 of them zero."""
    case = E.few_hubs_case(n_planted)
    M = case.pattern.n_rows
    assert len(E.hubs(case.pattern, case.ev_hub)) == (8 if n_planted == 8 else 0)
    run_case(ops, case, small_outputs(ops, M, [(0, M), (100, 333)]))


def test_wide_operand_small_output(ops):
    """(c) 300 x 70 000: ids above 65 535 in the transposed pattern's lists, all 16 hub columns above 65 536."""
    case = E.wide_case()
    M = case.pattern.n_rows
    assert len(E.hubs(case.pattern, case.ev_hub)) == 16
    run_case(ops, case, small_outputs(ops, M, [(0, M), (7, 290)]))


# n, blocked, pitch (row-major), column block; what it is
BIG = [
    (65536, True, None, None),            # (d) the largest single pass; column 65 535 is the high half of the last LDS word
    (65535, False, 65535, None),          # (d) row-major on the natural pitch: an odd word count, byte stores
    (65537, False, 65552, None),          # (e) the second pass has ONE column
    (65632, True, None, None),            # (e) the second pass has 96 columns
    (65632, False, 65568, (40, 65560)),   # (e) a column block: never the triangle; its second pass has 24 columns
]
_big = {}


def big_case(n):
    """(pattern, counts): built once per size and shared, never changed."""
    if n not in _big:
        case = E.big_case(n)
        _big[n] = (case, E.counts(case.pattern))
    return _big[n]


@pytest.mark.parametrize("n,blocked,ld,block", BIG, ids=["65536-blocked", "65535-rowmajor", "65537-rowmajor", "65632-blocked",
                                                          "65632-rowmajor-block"])
def test_single_pass_limit_and_two_passes(ops, n, blocked, ld, block):
    """(d), (e) Whole squares at and around 65 536 columns and a column block across the line.  With hub columns and
    ev_tri = 1 a whole square beyond 65 536 is the upper triangle in two passes plus the mirror; with ev_hub = 0 it is the
    full form — the rule itself; the bytes are the same.  (n = 65 535 on its natural pitch has no guard columns: its
    guard row follows the last row directly.)"""
    case, R = big_case(n)
    col0, L = block or (0, n)
    _, _, unit, units = geometry(n, L, blocked, ld)
    need_memory(unit * units)
    assert len(E.hubs(case.pattern, case.ev_hub)) >= 38
    run_case(ops, case, [(col0, Out(ops, n, L, blocked, ld=ld))], R)


def test_through_the_plan_beyond_65536(ops):
    """(f) SimRank++ at n = 65 632 through engine.Plan: the counts the plan keeps (hub columns, the triangle in two
    passes, the mirror, panel-blocked, in the plan's own node order) handed back in the caller's order equal the
    reference, whole; and after two updates eight rows of one more — the ends, both sides of the 65 536 line, three
    planted rows — equal a float64 recomputation with the evidence factor 1 - 2^-count, within the suite's 1e-5
    (the method of test_gpu_parity.py::test_config5_pl65536_simrank_pp_properties)."""
    from simrank_amd.engine import Plan
    n = 65632
    case, R = big_case(n)
    p = case.pattern
    need_memory(3 * 4 * n * n + n * n)
    deg = np.diff(p.rowptr)
    rs32 = np.where(p.rowscale.astype(np.float32) > 0, 1.0 / np.maximum(deg, 1), 0.0).astype(np.float32)
    saved = ops.get_tuning("ev_hub")
    ops.set_tuning(ev_hub=case.ev_hub)
    try:
        plan = Plan(ops, p, rowscale=rs32, coef=0.8, evidence=True)
    finally:
        ops.set_tuning(ev_hub=saved)
    assert ops.graph_get(plan.graph_handle(), "ev_hubs") == len(E.hubs(p, case.ev_hub))
    # fewer than half of the 32-column segments can be live in ANY node order: the plan restricts leg 2 to supp(E)
    assert 2 * R.nnz < n * -(-n // 32)
    assert plan.get("restrict_support") == 1
    got = plan.evidence_counts()
    assert got.shape == (n, n) and got.dtype == np.uint8
    for r0 in range(0, n, 4096):
        r1 = min(n, r0 + 4096)
        want = E.band(R, r0, r1, 0, n)
        if not np.array_equal(got[r0:r1], want):
            bad = np.argwhere(got[r0:r1] != want)
            pytest.fail(f"plan counts, rows [{r0}, {r1}): {len(bad)} wrong bytes; (row, column, got, want): "
                        f"{[(r0 + a, b, got[r0 + a, b], want[a, b]) for a, b in bad[:8]]}")
    del got
    for _ in range(2):
        plan.step(0.0)
    planted = sorted({a for pair in case.planted for a in pair})
    rows = [0, 1, 65535, 65536, n - 1] + [a for a in planted if a not in (65535, 65536)][:3]
    assert len(set(rows)) == 8
    need = sorted(set(np.concatenate([p.col[p.rowptr[a]:p.rowptr[a + 1]] for a in rows]).tolist()))
    pos = {i: k for k, i in enumerate(need)}
    part = plan.rows(need).astype(np.float64)
    rs = rs32.astype(np.float64)
    Pat = sp.csr_matrix((np.ones(p.col.size), p.col, p.rowptr), shape=(n, n))
    W = sp.diags(rs) @ Pat
    t_rows = {a: rs[a] * part[[pos[int(i)] for i in p.col[p.rowptr[a]:p.rowptr[a + 1]]]].sum(axis=0) for a in rows}
    plan.step(0.0)
    after = plan.rows(rows).astype(np.float64)
    for k, a in enumerate(rows):
        cnt = R[a].toarray().ravel().astype(np.float64)
        want = 0.8 * (W @ t_rows[a]) * (1.0 - 0.5 ** cnt)
        want[a] = 1.0
        np.testing.assert_allclose(after[k], want, rtol=RTOL, atol=1e-30, err_msg=f"row {a}")
        outside = cnt == 0
        outside[a] = False
        assert np.all(after[k][outside] == 0.0) and after[k][a] == 1.0
    assert any(after[k].sum() > 1.0 for k in range(len(rows)))
    plan.free()
