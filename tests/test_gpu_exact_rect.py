"""Leg 2 on RECTANGULAR patterns, every form, BIT FOR BIT against float64 NumPy on exactly summable operands.

In a two-matrix update leg 2 of group 1 is W12 . Tt with W12 n1 x n2 and Tt = (W12 . S2)^T n2 x n1: the operand has K = n2 rows
on panels of x_rows_pad rows, the result n = n1 rows on panels of y_rows_pad rows.  The square cases of
tests/test_gpu_exact_kernels.py and tests/test_gpu_exact_short.py have K = n, so a mix-up of the two row counts — in a
descriptor's size, a sentinel id, a range check, a tail panel, the mirror's address — changes nothing there.  Here the pattern
is n x K (tests/exact.py summable_symmetric: S symmetric K x K, Tt K x n, W . Tt n x n and exactly symmetric) with K < n and
K > n, the operand's rows_pad above the result's at (1031, 2100) and below it at (2100, 700), K = 20 below a panel's width.
Same protocol as the square tests, whose helpers are imported: one float64 reference cast once, the strict > count on
planted ties with the weight 2 of mirrored elements, zero on a quiet `previous` with both count forms, count_any in
(0, exact], every operand and result guarded and the guards checked, and the path every launch took asserted against the
rule of tests/leg2_rule.py.  No tolerance anywhere."""
import numpy as np
import pytest

from tests import exact as X
from tests import test_gpu_exact_kernels as K
from tests import test_gpu_exact_short as S
from tests.leg2_rule import short_groups
from tests.test_gpu_exact_kernels import hops, ops  # noqa: F401  (the fixtures: fuse_steps=1, fuse_min=2 as the square tests)

pytestmark = pytest.mark.gpu

VARIANTS = ("plain", "evidence", "all")
_planted = {}


def _id(shape):
    return f"{shape[0]}x{shape[1]}"


def planted(M, Kc, variant):
    """-> (want float32, Tt float32, (Planted all kinds, Planted "on" / "below")) at X.tie_places(M, M); once per case."""
    key = (M, Kc, variant)
    if key not in _planted:
        csr, sym, counts, prior, lbd, want = X.rect_case(M, Kc, variant)
        want32 = K.f32(want)
        places = X.tie_places(M, M)
        _planted[key] = (want32, K.f32(sym.Tt), (X.plant_previous(want32, K.EPS, places, symmetric=True),
                                                X.plant_previous(want32, K.EPS, places, symmetric=True, only=("on", "below"))))
    return _planted[key]


@pytest.mark.parametrize("shape", X.LEG2_RECT, ids=_id)
@pytest.mark.parametrize("variant", VARIANTS)
def test_rect_leg2_every_form_gives_the_reference_bits_and_the_strict_count(ops, shape, variant):
    """K.LEG2_FORMS — full and triangle, row-major and blocked, emit_row on a wide panel and with lean=0, the block-dense part,
    the one-launch leg whole, with 32-bit ids, split blocks and fuse_group=1, the two-launch leg on its general and its short
    path, the blocked full form — and the scalar variant on an odd ld.  None of them is refused on a rectangular pattern
    (spmm.hip asks n_cols_x == n_rows of the triangle forms, nothing of K)."""
    M, Kc = shape
    csr, sym, counts, prior, lbd, want = X.rect_case(M, Kc, variant)
    want32, tt32, pq = planted(M, Kc, variant)
    assert tt32.shape == (Kc, M)
    lengths = np.diff(csr.rowptr).tolist()
    for what, kw, blocked, symmetric in K.LEG2_FORMS:
        with K.knobs(ops, **kw):
            g = ops.graph(csr)
            if "one-launch" in what:
                assert ops.fused_stats(g)[1] > 0 and ops.graph_get(g, "fused_ids16") == kw.get("ids16", 1), what
            K._check_counts(lambda prev: K._leg2(ops, g, tt32, M, blocked, symmetric, counts, prior, lbd, prev), want32,
                            f"{M} x {Kc} {what}", planted=pq)
            if "leg2_short" in kw:
                rule = short_groups(lengths, kw["leg2_short"])
                assert ops.graph_get(g, "leg2_short_groups") == rule == ops.graph_get(g, "leg2_short_taken"), (what, rule)
                assert kw["leg2_short"] or rule == 0
    with K.knobs(ops, fuse=0):
        g = ops.graph(csr)
        K._check_counts(lambda prev: K._leg2_scalar(ops, g, tt32, M, counts, prior, lbd, prev), want32,
                        f"{M} x {Kc} scalar variant", planted=pq)


SHORT_RECT = ("boundary", "ragged21", "ragged1", "n64")


def _short_K(name, kind):
    n = len(X.short_lengths()[name][0])
    return n + 37 if kind == "wider" else 20


@pytest.mark.parametrize("width", X.SHORT_WIDTHS)
@pytest.mark.parametrize("kind", ["wider", "K20"])
@pytest.mark.parametrize("variant", ["plain", "all"])
@pytest.mark.parametrize("name", SHORT_RECT)
def test_short_graphs_on_rectangular_patterns(ops, name, variant, kind, width):
    """The short path's own graphs (row lengths at the edges of both widths, ragged last tiles) with K = n + 37 and K = 20
    operand rows: the image's ids address an operand of another height than `previous`, whose rows the early loads of
    short_group3 address.  A tie in every row; the rule's groups for the image and for every launch."""
    Kc = _short_K(name, kind)
    case = X.short_case(name, variant, Kc)
    want32, p, q = X.short_planted(name, variant, Kc)
    assert case[0].n_cols == Kc and case[1].Tt.shape == (Kc, len(case[6]))
    rule = short_groups(case[6], width)
    g = S._graph(ops, case[0], width)
    assert S._path(ops, g) == (rule, 0), (name, Kc, width)
    run, taken = S._run(ops, g, case)
    K._check_counts(run, want32, f"{name} K={Kc} {variant} leg2_short={width}", planted=(p, q))
    assert taken == [rule, rule] and S._path(ops, g) == (rule, rule), (name, Kc, width, taken, rule)
    assert (rule > 0) == (width > 0)                            # (these graphs were built to have short groups at both widths)


@pytest.mark.parametrize("variant", VARIANTS)
def test_below_the_triangle_form(ops, variant):
    """63 rows, K = 200: no upper-triangle form and no image below 64 rows.  A launch that asks for the triangle gets the full
    form — the same reference, every element counted once, no short group built or taken."""
    M, Kc = X.LEG2_RECT_BELOW
    csr, sym, counts, prior, lbd, want = X.rect_case(M, Kc, variant)
    want32, tt32, pq = planted(M, Kc, variant)
    assert short_groups(np.diff(csr.rowptr).tolist(), 16) == 0
    for what, kw, blocked, symmetric in K.LEG2_FORMS:
        with K.knobs(ops, **kw):
            g = ops.graph(csr)
            K._check_counts(lambda prev: K._leg2(ops, g, tt32, M, blocked, symmetric, counts, prior, lbd, prev), want32,
                            f"{M} x {Kc} {what}", planted=pq)
            assert ops.graph_get(g, "leg2_short_groups") == 0 == ops.graph_get(g, "leg2_short_taken"), what


@pytest.mark.parametrize("shape", [(520, 333), (129, 77)], ids=_id)
@pytest.mark.parametrize("variant,scale", [("plain", 1.0), ("evidence", 1.0), ("all", 1.0), ("evidence", 16384.0), ("all", 16384.0)])
def test_half_leg2_on_rectangular_patterns(hops, shape, variant, scale):
    """half.hip's leg 2 (what the bipartite fp16 fit runs on its rectangular legs): the exact result rounded once and the count
    by its rule, the protocol of the square test on an 11-bit budget."""
    M, Kc = shape
    e = -6 - int(np.log2(scale))
    K.half_leg2_protocol(hops, X.rect_case(M, Kc, variant, mantissa=11, exponent=e), scale)
