"""Leg 2's short path (spmm.hip short_group3, api.hip build_short_image; tuning "leg2_short" = 0, 8, 16) BIT FOR BIT against
float64 NumPy on exactly summable operands, on graphs built for it, with the path that every launch took asserted.

The graphs (tests/exact.py short_lengths) are in the caller's order with prescribed row lengths, so the rule of
tests/leg2_rule.py says for every width how many groups of four tiles are short; `simrank_graph_get` must report that
number for the image ("leg2_short_groups") and for the launch ("leg2_short_taken") — 0 at width 0, where the general
two-launch upper-triangle leg (gather3 kSym without SHORT) runs on the very same operands.  Every result is the reference's
bits at EVERY width (not a comparison between widths).  What is new in short_group3 changes no result bit when it goes
wrong, only a count: the previous iterate of all four passes is loaded early through a descriptor, its rows addressed by
the image's byte-packed row indices.  So `previous` carries a planted tie in every row (X.tie_places_every_row: the
diagonal, both ends of the row's own 32-column block, the last column, a column of another panel; differences of exactly
eps, eps + one step, eps - one step), and the exact count must be the reference's strict > count — every slot of every pass
of every lane group of every tile is compared with a row of its own.  Operands, results and padding are guarded as in
tests/test_gpu_exact_kernels.py."""
import numpy as np
import pytest

from tests import exact as X
from tests import test_gpu_exact_kernels as K
from tests.leg2_rule import group_flags, short_groups

pytestmark = pytest.mark.gpu

# the two-launch leg 2 on the plain pattern: no one-launch leg 2, no dense part, 16-bit ids, the tiling the rule restates
BASE = dict(fuse=1, fuse_sym=0, dense_sym=0, ids16=1, restrict_support=0, balance=2, stream_nt=1, sym_desc=1, addr32=1)
VARIANTS = ("plain", "evidence", "all")


@pytest.fixture(scope="module")
def ops():
    from simrank_amd.engine import HipOps
    return HipOps(0)


def _graph(ops, csr, width, **kw):
    """A graph created under BASE, `kw` and leg2_short = width (the tuning is read when a graph is created; restored)."""
    with K.knobs(ops, **{**BASE, **kw, "leg2_short": width}):
        return ops.graph(csr)


def _path(ops, g):
    return ops.graph_get(g, "leg2_short_groups"), ops.graph_get(g, "leg2_short_taken")


def _run(ops, g, case, blocked=True, symmetric=True, **ep_kw):
    """-> run(previous) for K._check_counts, and the list of "leg2_short_taken" read after each of its launches."""
    csr, sym, counts, prior, lbd, want, _ = case
    tt32, taken = K.f32(sym.Tt), []

    def run(prev):
        out = K._leg2(ops, g, tt32, csr.n_rows, blocked, symmetric, counts, prior, lbd, prev, **ep_kw)
        taken.append(ops.graph_get(g, "leg2_short_taken"))
        return out
    return run, taken


@pytest.mark.parametrize("width", X.SHORT_WIDTHS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", X.SHORT_GRAPHS)
def test_short_graphs_give_the_reference_bits_the_rule_and_the_strict_count(ops, name, variant, width):
    case = X.short_case(name, variant)
    want32, p, q = X.short_planted(name, variant)
    rule = short_groups(case[6], width)
    g = _graph(ops, case[0], width)
    assert _path(ops, g) == (rule, 0), (name, width)               # the image is there, nothing has been launched
    run, taken = _run(ops, g, case)
    K._check_counts(run, want32, f"{name} {variant} leg2_short={width}", planted=(p, q))
    assert taken == [rule, rule] and _path(ops, g) == (rule, rule), (name, width, taken, rule)
    assert width or rule == 0


@pytest.mark.parametrize("width", X.SHORT_WIDTHS)
@pytest.mark.parametrize("name", X.SHORT_GRAPHS)
def test_without_a_previous_iterate(ops, name, width):
    """No `previous`: short_group3 makes a descriptor of zero bytes for its early loads.  The same bits, the same path."""
    csr, sym, counts, prior, lbd, want, lengths = X.short_case(name, "all")
    n = csr.n_rows
    g = _graph(ops, csr, width)
    put = lambda a, dtype=np.float32: K.guarded_blocked(ops, a.shape[0], a.shape[1], a, dtype)
    x, ev, ap, y = put(K.f32(sym.Tt)), put(counts, np.uint8), put(K.f32(prior)), K.guarded_blocked(ops, n, n)
    ops.spmm(g, x, y, epilogue=dict(coef=0.5, evidence=ev, apriori=ap, lbd=lbd, diag_col0=0, symmetric=True))
    got = ops.download(y)
    K.check_untouched(ops, x, ev, ap, y)
    K.equal_bits(got, K.f32(want), f"{name} without previous, leg2_short={width}")
    rule = short_groups(lengths, width)
    assert _path(ops, g) == (rule, rule)


@pytest.mark.parametrize("knob", ["stream_nt", "sym_desc"])
@pytest.mark.parametrize("width", [8, 16])
def test_knobs_that_the_short_path_reads(ops, knob, width):
    """stream_nt = 0: the mirror's plain vector store; sym_desc = 0: the launch list (and its flagged copy) in ascending panel
    order.  Same bits, same counts, same path."""
    case = X.short_case("boundary", "all")
    want32, p, q = X.short_planted("boundary", "all")
    rule = short_groups(case[6], width)
    assert rule > 0
    g = _graph(ops, case[0], width, **{knob: 0})
    run, taken = _run(ops, g, case)
    K._check_counts(run, want32, f"boundary all {knob}=0 leg2_short={width}", planted=(p, q))
    assert taken == [rule, rule] and _path(ops, g) == (rule, rule)


NOT_SHORT = {"ids16=0": (dict(ids16=0), True, True, {}),
             "row-major": (dict(), False, True, {}),
             "restrict_support": (dict(restrict_support=1), True, True, dict(restrict_support=True)),
             "full form": (dict(), True, False, {})}


@pytest.mark.parametrize("width", [8, 16])
@pytest.mark.parametrize("form", list(NOT_SHORT))
def test_launches_that_must_not_take_the_short_path_say_so(ops, form, width):
    """32-bit ids (the image holds 16-bit ids), row-major operands (the mirror is stored panel-blocked), leg 2 restricted to
    the evidence's support (another instantiation) and the full form (no triangle): the graph has its image, the launch
    takes no group of it, and the bits and the count are the reference's."""
    kw, blocked, symmetric, ep_kw = NOT_SHORT[form]
    case = X.short_case("boundary", "all")
    want32, p, q = X.short_planted("boundary", "all")
    rule = short_groups(case[6], width)
    assert rule > 0
    g = _graph(ops, case[0], width, **kw)
    assert _path(ops, g) == (rule, 0)
    run, taken = _run(ops, g, case, blocked, symmetric, **ep_kw)
    K._check_counts(run, want32, f"boundary all {form} leg2_short={width}", planted=(p, q))
    assert taken == [0, 0] and _path(ops, g) == (rule, 0), (form, taken)


def test_taken_is_of_the_latest_launch(ops):
    """"leg2_short_taken" follows the launches on ONE graph: the short path, then the full form (0), then the short path."""
    case = X.short_case("n129", "plain")
    want32, p, q = X.short_planted("n129", "plain")
    rule = short_groups(case[6], 16)
    assert rule == 1 and group_flags(case[6], 16) == [False, True]     # the one-row tile's group beside a general group
    g = _graph(ops, case[0], 16)
    for symmetric, want_taken in ((True, rule), (False, 0), (True, rule)):
        run, taken = _run(ops, g, case, True, symmetric)
        K.equal_bits(run(p.previous)[0], want32, f"n129, triangle={symmetric}")
        assert taken == [want_taken]
