"""Leg 1 without the units of the transposed product that a triangle-form leg 2 never reads (csrc/planprep.hip
first_block_table, csrc/fused.hip FusedArgs::first_block, csrc/side.h side_leg_pair; tuning "leg1_skip").

Every case is five updates of engine.Plan in ONE child process started with SIMRANK_POOL_POISON=1 — what leg 1 leaves
unwritten is NaN there, so a tile that leg 2 does read would poison the result — once with leg1_skip = 1 and once with 0
(tests/leg1_skip_worker.py; its JSON record is shared by the tests below).  Graphs: the three power-law graphs whose refined
order leaves 20 %, 40 % and 52 % of the 128-row blocks dead (sizes off the 32 and 128 grids, empty rows, unreferenced nodes),
an Erdos-Renyi graph, a graph whose row 0 references everything (nothing may be skipped), a graph where only rows of the
last block reference anything (nearly everything is).  The refined node order is forced at these sizes (tuning leg1_order = 1:
by default a plan takes it from 16384 nodes on); the 16 500-node case runs with the default.  Tunings: the defaults, split blocks, fuse_group = 4, no dense set,
32-bit ids, the one-launch leg 2 forced."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "leg1_skip_worker.py")
GRAPHS = ["pl520", "pl1031", "pl2100", "er500", "row0_all", "last_block"]
VARIANTS = ["default", "split", "grouped", "no_set", "ids32", "one_launch_leg2"]


def _worker(*extra):
    env = dict(os.environ, SIMRANK_POOL_POISON="1")
    run = subprocess.run([sys.executable, WORKER, ROOT, *extra], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    return json.loads(run.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def seen():
    return _worker()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("graph", GRAPHS)
def test_skipping_leg1_changes_no_bit(seen, graph, variant):
    """result() and the count of every one of the five updates are bit-equal with and without the skip, both within the
    parity bar (1e-5 relative) of the float64 oracle; the skipped-unit count is what the node order, recomputed in NumPy,
    says: at these sizes a unit is one block (or a share of a split one), so the count EQUALS the number of dead
    (block, panel) pairs where no block is split and is at least that where some are — above 0 on every graph but the one
    whose row 0 references everything, where it is 0."""
    r = seen[f"{graph}/{variant}"]
    print(graph, variant, r)
    assert r["finite"] and r["bit_equal"] and r["counts_equal"]
    assert r["within_parity"], r["max_rel_err"]
    assert r["units"] == r["units_off"] > 0 and r["skipped_off"] == 0
    if graph == "row0_all":
        assert r["dead_blocks"] == 0 and r["skipped"] == 0
    else:
        assert r["dead_blocks"] > 0
        if variant == "split":
            assert r["skipped"] >= r["dead_blocks"]
        else:
            assert r["skipped"] == r["dead_blocks"]
    if graph == "last_block":
        assert r["dead_blocks"] * 6 >= r["blocks"] * 5          # five of the six blocks of every panel


@pytest.mark.parametrize("name", ["pp/restricted", "pp/unrestricted", "prior/symmetric"])
def test_evidence_and_symmetric_prior_skip_too(seen, name):
    """SimRank++ (leg 2 restricted to the evidence's support and not) and a symmetric prior: triangle forms, so leg 1 skips —
    the same bits as without, within the parity bar of the oracle."""
    r = seen[name]
    print(name, r)
    assert r["finite"] and r["bit_equal"] and r["counts_equal"] and r["within_parity"], r
    assert r["skipped"] == r["dead_blocks"] > 0 and r["skipped_off"] == 0


def test_asymmetric_prior_never_skips(seen):
    """An asymmetric prior's leg 2 is leg 1's kernel over ALL of the transposed product: the key changes nothing and the plan
    reports no skipped unit."""
    r = seen["prior/asymmetric"]
    print(r)
    assert r["finite"] and r["bit_equal"] and r["counts_equal"] and r["within_parity"], r
    assert r["skipped"] == 0 and r["skipped_off"] == 0 and r["units"] > 0


def test_grouped_units_skip_whole_or_not_at_all():
    """16 500 nodes: the smallest size at which units of several blocks survive (a panel keeps 64 units), fuse_group = 4.
    A grouped unit is skipped only when its LAST block is dead: fewer units than dead blocks go, more than none, and the
    sampled rows of the result and every count keep their bits."""
    r = _worker("big")["big/grouped"]
    print(r)
    assert r["finite"] and r["bit_equal"] and r["counts_equal"]
    assert 0 < r["skipped"] < r["dead_blocks"] and r["skipped_off"] == 0 and r["units"] < r["blocks"]
