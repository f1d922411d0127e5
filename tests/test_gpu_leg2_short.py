"""The short path of the upper-triangle leg 2 (csrc/api.hip build_short_image, csrc/spmm.hip short_group3; tuning
"leg2_short" = 0, 8 or 16).

Every case is five updates of engine.Plan in ONE child process started with SIMRANK_POOL_POISON=1 (what a kernel leaves
unwritten is NaN there), with leg2_short = 0, 8 and 16, with the exact count and with count_any
(tests/leg2_short_worker.py; its JSON record is shared by the tests below).  Graphs: power-law graphs of 520, 1031 and 2100
nodes (off the 32 and 128 grids, many short tiles, a ragged last tile), an Erdos-Renyi graph of 500, a graph in the caller's
order whose groups of four tiles sit at the edges of both widths (rows of exactly 8, 9, 16 and 17 entries in neighbouring
tiles, empty rows, a wholly empty tile, three short tiles beside a long one, a ragged last tile), and a graph with one
heavy row whose cut tiles sit next to short ones.  One case runs 18 updates with eps = 1e-4, down to counts of (almost) zero.

Under count_any a count stops at the first difference a wave sees: its value depends on the order the waves ran in (two
runs of ONE setting differ), so what is compared there is whether each update's count is zero."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "leg2_short_worker.py")
GRAPHS = ["pl520", "pl1031", "pl2100", "er500", "boundary", "heavy_row"]


@pytest.fixture(scope="module")
def seen():
    env = dict(os.environ, SIMRANK_POOL_POISON="1")
    run = subprocess.run([sys.executable, WORKER, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    return json.loads(run.stdout.strip().splitlines()[-1])


def _same_bits(r):
    assert r["finite"] and r["bit_equal"], r
    assert r["counts_exact"]["0"] == r["counts_exact"]["8"] == r["counts_exact"]["16"], r
    assert r["counts_any_nonzero"]["0"] == r["counts_any_nonzero"]["8"] == r["counts_any_nonzero"]["16"], r
    # an exact count of zero <=> a count_any of zero
    assert [c != 0 for c in r["counts_exact"]["0"]] == r["counts_any_nonzero"]["0"], r


def _takes_the_rule(r):
    for w in ("0", "8", "16"):
        assert r["groups"][w] == [r["rule"][w], r["rule"][w]], (w, r["groups"], r["rule"])


@pytest.mark.parametrize("graph", GRAPHS)
def test_short_path_changes_no_bit(seen, graph):
    """result() and the count of every one of the five updates are bit-equal for leg2_short = 0, 8 and 16, within the parity
    bar (1e-5 relative) of the float64 oracle, and the plan's "leg2_short_groups" is the rule recomputed in NumPy: above 0
    at both widths on every graph, more at 16 than at 8 where rows of 9 .. 16 entries exist."""
    r = seen[f"{graph}/plain"]
    print(graph, r)
    _same_bits(r)
    assert r["within_parity"], r["max_rel_err"]
    _takes_the_rule(r)
    assert r["rule"]["0"] == 0 and 0 < r["rule"]["8"] <= r["rule"]["16"]


def test_counts_near_convergence_are_the_same(seen):
    """18 updates with the fit's eps = 1e-4: the exact counts fall from nearly every element to (almost) none, where one
    row compared with the wrong row of the previous iterate would show; bit-equal across the three settings in every
    update, as is result(), and a count_any of zero exactly where the exact count is zero."""
    r = seen["pl520/to_convergence"]
    print(r)
    _same_bits(r)
    assert r["within_parity"], r["max_rel_err"]
    _takes_the_rule(r)
    counts = r["counts_exact"]["16"]
    assert len(counts) == 18 and counts[-1] * 100 < counts[0], counts


def test_boundaries_fall_back_where_the_rule_says(seen):
    """The caller-order graph: groups 0, 4 and the ragged group 5 are short at 8; group 1 (rows of 9) and group 2 (rows of
    16) join at 16; group 3 (one row of 17 beside three short tiles) never."""
    r = seen["boundary/plain"]
    assert r["rule"]["8"] == 3 and r["rule"]["16"] == 5, r["rule"]
    _takes_the_rule(r)


def test_heavy_row_cuts_tiles_next_to_short_ones(seen):
    """The block of the 400-entry row is cut: more tiles than 32-row blocks, so at least one group is not short for its
    shape alone, and the groups around it are."""
    r = seen["heavy_row/plain"]
    assert r["tiles"] > r["blocks"], r
    assert 0 < r["rule"]["8"] == r["rule"]["16"] < r["tile_groups"], r
    _takes_the_rule(r)


@pytest.mark.parametrize("name", ["pp/unrestricted", "prior/symmetric"])
def test_evidence_and_symmetric_prior_take_the_short_path(seen, name):
    r = seen[name]
    print(name, r)
    _same_bits(r)
    assert r["within_parity"], r["max_rel_err"]
    _takes_the_rule(r)
    assert r["rule"]["8"] > 0


@pytest.mark.parametrize("name", ["pp/restricted", "prior/asymmetric", "ids32"])
def test_other_launches_take_no_short_group(seen, name):
    """Leg 2 restricted to the evidence's support (another instantiation), an asymmetric prior (no triangle form) and 32-bit
    ids (the image holds 16-bit ids): the rule finds short groups, the launch takes none, the bits are the same."""
    r = seen[name]
    print(name, r)
    _same_bits(r)
    assert r["within_parity"], r["max_rel_err"]
    assert r["rule"]["8"] > 0
    assert all(g == [0, 0] for g in r["groups"].values()), r["groups"]


def test_fp16_held_matrices_are_untouched(seen):
    r = seen["fp16"]
    print(r)
    _same_bits(r)
    assert all(g == [0, 0] for g in r["groups"].values()), r["groups"]
