"""The launch caps the GPU tests mirror, read from the source text the way tests/companion_abi.py reads headers: the shapes
of tests/test_gpu_sweep_turns.py, of the tall blocks of tests/test_gpu_compare.py, of the many pairs of
tests/test_gpu_explain.py and of ``operator_ref.LONG_CASES`` must still lie past them, so that a changed cap makes a test
fail here instead of turning those tests back into one-turn tests."""
import os
import re

from simrank_amd import _compare, _operator
from tests import blocks as B
from tests import operator_ref as R

CSRC = os.path.join(os.path.dirname(os.path.abspath(_operator.__file__)), "csrc")


def constant(text, name):
    """The value of ``constexpr <type> name = <integer expression>;`` or ``#define name <integer>`` in ``text``."""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([0-9*+ ()]+);" % name, text) or re.search(r"#define\s+%s\s+(\d+)\b" % name, text)
    assert m, name
    return int(eval(m.group(1), {"__builtins__": {}}))


def source(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_shared_sweep_and_compare_caps():
    companion = source("companion.h")
    grid, threads = constant(companion, "kSweepMaxGrid"), constant(companion, "kSweepThreads")
    assert (grid, threads) == (2048, 256)
    # the row -> wave map the turns follow: a panel wave takes eight rows, a row-major wave one; a wave strides by the grid
    assert re.search(r"static constexpr int L = ROWMAJOR \? 64 : 8;", companion) and "constexpr int R = 64 / L;" in companion
    assert "r0 += nwaves * R" in companion
    waves = threads // 64
    row_major, panel = grid * waves, grid * waves * 8
    assert (row_major, panel) == (8192, 65536)
    # tests/test_gpu_sweep_turns.py mirrors them; it imports GPU test modules, so its numbers are restated here
    sweep_rows = {B.ROWMAJOR_F32: (8197, 24577), B.ROWMAJOR_F64: (8197, 24577), B.PANEL_F32: (65536, 65545), B.PANEL_F16: (65536, 65545)}
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_sweep_turns.py")).read()
    assert "MAX_GRID, WAVES = %d, %d " % (grid, waves) in text and "BAND = %d " % row_major in text
    assert "(65536, 65545) if layout in B.PANEL else (8197, 24577)" in text
    for layout, (at_least_two, more) in sweep_rows.items():
        turn = panel if layout in B.PANEL else row_major
        turns = [-(-n // turn) for n in (at_least_two, more)]
        assert turns == ([1, 2] if layout in B.PANEL else [2, 4]), (layout, turns)
        assert more % turn in (1, 9)                                       # the last turn: one row, or a wave of eight and one row
    # compare.hip: its own cap, a wave a row at a time in every layout
    assert constant(open(_compare.HEADER_PATH).read(), "SIMRANK_COMPARE_MAX_GRID") == 2048
    compare = source("compare.hip")
    assert "constexpr int kMaxGrid = SIMRANK_COMPARE_MAX_GRID;" in compare and constant(compare, "kThreads") == 256
    assert "for (int64_t r = wave; r < n_rows; r += nwaves)" in compare
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_compare.py")).read()
    assert "TURN = 2048 * 4 " in text and "TALL = (8197, 24577)" in text
    assert [-(-n // (2048 * 4)) for n in (8197, 24577)] == [2, 4]


def test_the_explain_cap():
    explain = source("explain.hip")
    wanted, chunk = constant(explain, "kBlocksWanted"), constant(explain, "kThreads") * constant(explain, "kUnroll")
    assert (wanted, chunk) == (16384, 1024) and "constexpr int kChunk = kThreads * kUnroll;" in explain
    n_pairs, max_terms, max_cols = 6002, 70 * 60, 300                      # tests/test_gpu_explain.py's long pairs among many
    cap = wanted // n_pairs
    assert 1 <= cap < -(-max_terms // chunk) and cap < -(-max_cols // 64)
    assert wanted // 3000 >= -(-1600 // chunk)                             # (what the 3000 small pairs alone never passed)


def test_the_operator_split():
    op = source("operator.hip")
    assert constant(op, "kWantGroups") == 1536 and constant(op, "kDepth") == 32
    assert constant(op, "kRowsStrip") == 16 and constant(op, "kRowsDepth") == 256 and constant(op, "kColsDepth") == 64
    assert "constexpr int kColsStrip = 4 * kThreads;" in op and constant(op, "kThreads") == 256
    header = open(_operator.HEADER_PATH).read()
    assert constant(header, "SIMRANK_OPERATOR_MAX_PARTS") == 64 and constant(header, "SIMRANK_OPERATOR_STRIP") == 128
    assert constant(header, "SIMRANK_OPERATOR_NARROW") == 8
    for kernel, n_rows, n_cols, transpose, ds, strip, depth in R.LONG_CASES:
        narrow = max(ds) <= 8
        assert all((d <= 8) == narrow for d in ds)
        assert (strip, depth) == ((1024, 64) if narrow and transpose else (16, 256) if narrow else (128, 32)), kernel
        n_in = n_rows if transpose else n_cols
        assert -(-n_in // depth) > 64                                      # more tiles than parts: some part walks two
    R.assert_long_cases_walk_several_tiles(_operator.load())
