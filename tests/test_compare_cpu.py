"""libsimrank_compare.so (include/simrank_compare.h) and ``model.compare`` on a machine without a GPU: header, binding and
exports agree, the header is plain C99 and stands alone, the entry refuses bad arguments without a device, ``compare``
judges its arguments and the two models before any device work, the reference (tests/compare_ref.py) gives the
hand-computed values on every branch of ``d`` and ``rel``, and the host's list agreement equals plain set logic."""
import re

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _compare, _lib, _model, _neighbors, _query
from tests import companion_abi as A
from tests import compare_ref as R
from tests.test_cluster_cpu import _Spec, boom, guarded_estimator

INF, NAN = float("inf"), float("nan")


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_compare) == _compare.VERSION == 1
    text = A.header(_compare)
    assert re.search(r"#define SIMRANK_COMPARE_MAX_TOL %d\b" % _compare.MAX_TOL, text) and _compare.MAX_TOL == 8
    assert re.search(r"#define SIMRANK_COMPARE_BINS %d\b" % _compare.BINS, text) and _compare.BINS == R.BINS == 2048
    assert re.search(r"#define SIMRANK_COMPARE_MAX_GRID %d\b" % _compare.MAX_GRID, text)
    assert sorted(_compare.PROTOTYPES) == ["simrank_compare_last_error", "simrank_compare_sweep", "simrank_compare_version"]
    A.assert_header_stands_alone(_compare)


def test_the_layout_codes_are_the_shared_ones():
    assert A.layout_codes(_compare) == A.layout_codes(_query) and len(A.layout_codes(_compare)) == 4


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_compare)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_compare)


def test_the_main_library_is_unchanged():
    version, names, exports = A.main_library(_compare)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_the_entry_refuses_bad_arguments_without_a_device(tmp_path):
    assert "compare 1 ok" in A.run_c99(_compare, tmp_path, r'''
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "simrank_compare.h"
#define BAD(call, code, word) do { if ((call) != SIMRANK_COMPARE_ERR_INVALID) return code; \
                                   if (!strstr(simrank_compare_last_error(), word)) return 100 + code; } while (0)
#define SWEEP(A, la, sa, B, lb, sb, rows, cols, tol, n_tol, floor, d1, i1, d2, i2, over, hist) \
    simrank_compare_sweep(A, la, sa, B, lb, sb, rows, cols, tol, n_tol, floor, d1, i1, d2, i2, over, hist, NULL)
int main(void) {
    /* aligned stand-ins for device memory: nothing below may reach a device */
    static double mem[8];
    static int32_t ids[8];
    static uint32_t cnt[8];
    static unsigned long long hist[SIMRANK_COMPARE_BINS];
    const void* S = mem;
    double* d = mem;
    double tol[9] = {0.0, 1e-5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0};
    double bad_tol[2] = {0.5, -1.0};
    const int32_t f32 = SIMRANK_COMPARE_ROWMAJOR_F32, f64 = SIMRANK_COMPARE_ROWMAJOR_F64;
    const int32_t p32 = SIMRANK_COMPARE_PANEL_F32, p16 = SIMRANK_COMPARE_PANEL_F16;
    const int64_t huge = (int64_t)1 << 31;
    if (simrank_compare_version() != SIMRANK_COMPARE_VERSION) return 1;
    /* an unknown layout on either side */
    BAD(SWEEP(S, 4, 4, S, f32, 4, 4, 4, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 2, "A: unknown layout 4");
    BAD(SWEEP(S, f32, 4, S, -1, 4, 4, 4, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 3, "B: unknown layout -1");
    /* a NULL block, a NULL output */
    BAD(SWEEP(NULL, f32, 4, S, f32, 4, 4, 4, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 4, "A is NULL");
    BAD(SWEEP(S, f32, 4, NULL, f32, 4, 4, 4, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 5, "B is NULL");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, 2, 0.0, NULL, ids, d, ids, cnt, hist), 6, "is NULL");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, 2, 0.0, d, NULL, d, ids, cnt, hist), 7, "is NULL");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, 2, 0.0, d, ids, NULL, ids, cnt, hist), 8, "is NULL");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, 2, 0.0, d, ids, d, NULL, cnt, hist), 9, "is NULL");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, 2, 0.0, d, ids, d, ids, NULL, hist), 10, "over is NULL");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, 2, 0.0, d, ids, d, ids, cnt, NULL), 11, "hist is NULL");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, NULL, 0, 0.0, d, ids, d, ids, cnt, hist), 12, "over must be NULL");
    /* a stride too small: columns of a row-major block, rows of a panel block, on either side */
    BAD(SWEEP(S, f32, 3, S, f32, 4, 4, 4, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 13, "A: stride 3");
    BAD(SWEEP(S, f32, 4, S, f64, 3, 4, 4, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 14, "B: stride 3");
    BAD(SWEEP(S, p32, 3, S, f32, 2, 4, 2, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 15, "A: stride 3");
    BAD(SWEEP(S, f32, 2, S, p16, 3, 4, 2, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 16, "B: stride 3");
    /* a negative shape, a shape of 2^31 */
    BAD(SWEEP(S, f32, 4, S, f32, 4, -1, 4, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 17, "bad block shape");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, -1, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 18, "bad block shape");
    BAD(SWEEP(S, f32, huge, S, f32, huge, 4, huge, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 19, "bad block shape");
    /* the tolerances */
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, -1, 0.0, d, ids, d, ids, cnt, hist), 20, "n_tol must be 0 .. 8");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, 9, 0.0, d, ids, d, ids, cnt, hist), 21, "n_tol must be 0 .. 8");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, NULL, 2, 0.0, d, ids, d, ids, cnt, hist), 22, "tol is NULL");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, 0, 0.0, d, ids, d, ids, NULL, hist), 23, "tol must be NULL");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, bad_tol, 2, 0.0, d, ids, d, ids, cnt, hist), 24, "tol[1]");
    bad_tol[0] = NAN;
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, bad_tol, 1, 0.0, d, ids, d, ids, cnt, hist), 25, "tol[0]");
    bad_tol[0] = INFINITY;
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, bad_tol, 1, 0.0, d, ids, d, ids, cnt, hist), 26, "tol[0]");
    /* the floor */
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, 2, -0.5, d, ids, d, ids, cnt, hist), 27, "floor");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, 2, NAN, d, ids, d, ids, cnt, hist), 28, "floor");
    BAD(SWEEP(S, f32, 4, S, f32, 4, 4, 4, tol, 2, INFINITY, d, ids, d, ids, cnt, hist), 29, "floor");
    /* a block that does not start on its element's size */
    BAD(SWEEP((const char*)S + 2, f32, 4, S, f32, 4, 4, 4, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 30, "A must start");
    BAD(SWEEP(S, f32, 4, (const char*)S + 4, f64, 4, 4, 4, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 31, "B must start");
    /* one workgroup's 32-bit bins: 2^31 - 1 rows of 2^31 - 1 columns are too many for one call */
    BAD(SWEEP(S, f32, huge, S, f32, huge, huge - 1, huge - 1, tol, 2, 0.0, d, ids, d, ids, cnt, hist), 32, "bands of fewer rows");
    /* no rows: nothing to queue */
    if (SWEEP(NULL, f32, 4, NULL, p16, 0, 0, 4, NULL, 0, 0.0, NULL, NULL, NULL, NULL, NULL, NULL) != SIMRANK_COMPARE_OK)
        return 33;
    printf("compare %d ok\n", simrank_compare_version());
    return 0;
}
''')


def test_band_rows_keep_a_workgroup_below_2_32_elements():
    for n_cols in (1, 1000, 65536, 2 ** 20, 2 ** 31 - 1):
        rows = _compare.band_rows(n_cols)
        turns = -(-rows // (_compare.WAVES * _compare.MAX_GRID))
        assert rows >= 1 and min(rows, turns * _compare.WAVES) * n_cols < 2 ** 32


# ---- compare: everything judged before any device work -------------------------------------------------------------------
class _Ops:
    synchronize = _malloc = put = staticmethod(boom)

    def __init__(self, device=0):
        self.device = device


class _Block:
    def __init__(self, n, storage="f32"):
        self.n, self.storage, self.nbytes, self.ptr = n, storage, 0, None

    def free(self):
        pass


def dense_estimator(labels=("a", "b", "c"), device=0, cls=SRA.SimRank, groups=1):
    """An estimator holding an unpruned model whose device no argument check may reach."""
    sides = [(j, list(labels)) for j in range(groups)]
    solver = _model.DetachedSolver(_Ops(device), [_Spec] * groups, [_Block(len(labels)) for _ in range(groups)])
    solver._make_reader = boom
    solver.one_block = boom
    return cls()._keep(solver, sides)


@pytest.fixture
def no_device(monkeypatch):
    for name in ("load", "sweep_blocks", "compare_readers", "callers_readers", "select_ids"):
        monkeypatch.setattr(_compare, name, boom)
    monkeypatch.setattr(_neighbors, "select", boom)
    monkeypatch.setattr(_model, "detach", boom)


def test_compare_refuses_models_that_do_not_match(no_device):
    est = dense_estimator()
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().compare(est)
    with pytest.raises(RuntimeError, match="no kept model"):
        est.compare(SRA.SimRank())
    for bad in (None, 3, "model", pd.DataFrame()):
        with pytest.raises(ValueError, match="other must be an estimator"):
            est.compare(bad)
    # the labels: the first difference, with its position and the two labels
    with pytest.raises(ValueError, match=r"group 1: the labels differ at position 1: 'b' and 'x'"):
        est.compare(dense_estimator(("a", "x", "y")))
    with pytest.raises(ValueError, match=r"position 0: 'a' and 'c'"):
        est.compare(dense_estimator(("c", "b", "a")))
    with pytest.raises(ValueError, match=r"position 2: 'c' and 2"):
        est.compare(dense_estimator(("a", "b", 2)))
    with pytest.raises(ValueError, match="group 1: the two models have 3 and 4 nodes"):
        est.compare(dense_estimator(("a", "b", "c", "d")))
    # the groups
    two = dense_estimator(cls=SRA.BipartiteSimRank, groups=2)
    with pytest.raises(ValueError, match="1 and 2 node groups"):
        est.compare(two)
    with pytest.raises(ValueError, match="2 and 1 node groups"):
        two.compare(est)
    other = dense_estimator(cls=SRA.BipartiteSimRank, groups=2)
    other._model[1][1] = (1, ["a", "b", "z"])
    with pytest.raises(ValueError, match=r"group 2: the labels differ at position 2: 'c' and 'z'"):
        two.compare(other)
    # the device
    with pytest.raises(ValueError, match=r"different devices \(0 and 1\)"):
        est.compare(dense_estimator(device=1))
    # a pruned model on either side
    pruned = guarded_estimator()
    with pytest.raises(ValueError, match="the other model was pruned to kept_neighbors = 2.*compare before prune"):
        est.compare(pruned)
    with pytest.raises(ValueError, match="this model was pruned to kept_neighbors = 2"):
        pruned.compare(est)
    # a released model on either side
    gone = dense_estimator()
    gone.release()
    with pytest.raises(RuntimeError, match="released"):
        gone.compare(est)
    with pytest.raises(RuntimeError, match="released"):
        est.compare(gone)


BAD_TOLERANCES = [None, 1e-5, "1e-5", [-1.0], [NAN], [INF], [0.1, -0.0 - 1e-300], [True], ["x"], [None], [0.1] * 8, [[0.1]],
                  [1 + 2j], [np.nan], [np.True_]]
BAD_TOP_K = [0, -1, 2.5, True, "3", [3], np.True_]
BAD_FLOOR = [None, -1.0, NAN, INF, -INF, "0", True, [0.0], 1j]


def test_compare_argument_checks_need_no_device(no_device):
    est, other = dense_estimator(), dense_estimator()
    for bad in BAD_TOLERANCES:
        with pytest.raises(ValueError, match="toleranc"):
            est.compare(other, tolerances=bad)
    for bad in BAD_TOP_K:
        with pytest.raises(ValueError, match="top_k must be None or a positive integer"):
            est.compare(other, top_k=bad)
    for bad in BAD_FLOOR:
        with pytest.raises(ValueError, match="floor must be a finite number >= 0"):
            est.compare(other, floor=bad)
    # top_k is clamped to N - 1 first: above the selection's limit only on a model that large
    big, big2 = dense_estimator(range(5000)), dense_estimator(range(5000))
    with pytest.raises(ValueError, match="top_k = 4097 on 5000 nodes is more than the 4096"):
        big.compare(big2, top_k=4097)
    assert _compare.check_top_k(10 ** 6, [3]) == 10 ** 6 and _compare.check_top_k(None, [3]) is None
    assert _compare.check_tolerances(()) == () and _compare.check_tolerances([0, 1e-5, 0.0]) == (0.0, 1e-5, 0.0)
    assert _compare.check_tolerances(np.array([0.5] * 7)) == (0.5,) * 7 and _compare.check_floor(np.float32(2)) == 2.0
    with pytest.raises(ValueError, match="group must be"):
        est.rows(["a"], group=2)                              # (the model is intact)


# ---- the reference on hand-computed cases -----------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def test_the_reference_on_every_branch_of_d_and_rel():
    tiny = 2.0 ** -1074
    #              a      b       d      rel (floor 0)          rel (floor 0.5)
    cases = [(-0.0, 0.0, 0.0, 0.0, 0.0),
             (INF, INF, 0.0, 0.0, 0.0),
             (-INF, -INF, 0.0, 0.0, 0.0),
             (INF, -INF, INF, INF, INF),
             (INF, 1.0, INF, INF, INF),
             (NAN, NAN, 0.0, 0.0, 0.0),
             (NAN, 1.0, INF, INF, INF),
             (0.25, NAN, INF, INF, INF),                          # (the other operand is below the floor: still +inf)
             (1.0, 1.0, 0.0, 0.0, 0.0),
             (1.0, 0.75, 0.25, 0.25, 0.25),
             (0.25, 0.125, 0.125, 0.5, 0.0),                      # max(|a|, |b|) = 0.25 < 0.5
             (-0.5, 0.25, 0.75, 1.5, 1.5),                        # max(|a|, |b|) = 0.5 is not below the floor
             (0.0, tiny, tiny, 1.0, 0.0),
             (1.0, 1.0 + 2.0 ** -52, 2.0 ** -52, 2.0 ** -52 / (1.0 + 2.0 ** -52), 2.0 ** -52 / (1.0 + 2.0 ** -52)),
             (1.5e308, -1.5e308, INF, INF, INF),                  # a finite difference that overflows
             (3.0, -1.0, 4.0, 4.0 / 3.0, 4.0 / 3.0)]
    a, b = np.array([[c[0] for c in cases]]), np.array([[c[1] for c in cases]])
    d = R.distance(a, b)
    assert np.array_equal(bits(d), bits([[c[2] for c in cases]]))
    assert np.array_equal(bits(R.relative(a, b, d, 0.0)), bits([[c[3] for c in cases]]))
    assert np.array_equal(bits(R.relative(a, b, d, 0.5)), bits([[c[4] for c in cases]]))
    assert not np.signbit(d).any()
    # the first rule that applies: below a (finite) floor the overflowed difference of two finite values is still +0.0,
    # a NaN operand is below no floor, an infinite operand neither
    huge = np.array([[1.5e308, NAN, INF, 1.0]]), np.array([[-1.5e308, 1.0, 1.0, 1.0]])
    dh = R.distance(*huge)
    assert np.array_equal(bits(dh), bits([[INF, INF, INF, 0.0]]))
    assert np.array_equal(bits(R.relative(*huge, dh, 1.7e308)), bits([[0.0, INF, INF, 0.0]]))


def test_the_reference_sweep_on_a_hand_made_pair():
    A_ = np.array([[1.0, 2.0, 3.0, 4.0], [0.0, -0.0, NAN, 1.0], [1.0, 1.0, 1.0, 1.0]])
    B_ = np.array([[1.0, 2.5, 2.5, 4.0], [-0.0, 0.0, NAN, NAN], [1.0, 1.0, 1.0, 1.0]])
    max_abs, arg_abs, max_rel, arg_rel, over, hist = R.sweep(A_, B_, (0.0, 0.25, 0.5), 0.0)
    assert np.array_equal(bits(max_abs), bits([0.5, INF, 0.0])) and arg_abs.tolist() == [1, 3, 0]   # a tie: the first column
    assert np.array_equal(bits(max_rel), bits([0.5 / 2.5, INF, 0.0])) and arg_rel.tolist() == [1, 3, 0]
    assert over.dtype == np.uint32 and over.tolist() == [[2, 2, 0], [1, 1, 1], [0, 0, 0]]
    assert hist.dtype == np.uint64 and hist.sum() == 12
    assert hist[0] == 9 and hist[1022] == 2 and hist[2047] == 1                                  # 0.5 = 2^-1: bin 1022
    # the relative maximum may sit elsewhere than the absolute one
    _, aa, _, ar, _, _ = R.sweep(np.array([[8.0, 0.5]]), np.array([[7.0, 0.25]]), (), 0.0)
    assert aa.tolist() == [0] and ar.tolist() == [1]
    _, _, mr, ar, _, _ = R.sweep(np.array([[8.0, 0.5]]), np.array([[7.0, 0.25]]), (), 1.0)     # the floor hides column 1
    assert ar.tolist() == [0] and mr[0] == 0.125
    # an empty row
    ma, aa, mr, ar, ov, h = R.sweep(np.zeros((2, 0)), np.zeros((2, 0)), (0.0,), 0.0)
    assert ma.tolist() == [0.0, 0.0] and aa.tolist() == [-1, -1] and ar.tolist() == [-1, -1] and ov.shape == (2, 1)
    assert h.sum() == 0
    # the bins: subnormal differences in bin 0, 2^(e-1023) <= d < 2^(e-1022) in bin e
    d = np.array([[0.0, 2.0 ** -1074, 2.0 ** -1023, 2.0 ** -1022, 1.0, 1.5, 2.0, np.nextafter(2.0, 1.0)]])
    h = R.sweep(d, np.zeros_like(d))[5]
    assert h[0] == 3 and h[1] == 1 and h[1023] == 3 and h[1024] == 1 and h.sum() == 8


# ---- the host's list agreement ------------------------------------------------------------------------------------------------
def test_list_agreement_on_hand_built_tables():
    a = np.array([[1, 2, 3], [1, 2, 3], [1, 2, 3], [5, -1, -1], [-1, -1, -1], [4, 0, -1], [2, 1, 0], [0, 1, -1]], dtype=np.int32)
    b = np.array([[1, 2, 3], [3, 2, 1], [1, 2, 4], [5, -1, -1], [-1, -1, -1], [4, -1, -1], [7, 8, 9], [0, 1, 2]], dtype=np.int32)
    overlap, prefix = _compare.list_agreement(a, b)
    assert overlap.dtype == np.int64 and prefix.dtype == np.int64
    assert overlap.tolist() == [3, 3, 2, 1, 0, 1, 0, 2]         # (empty slots never match each other)
    assert prefix.tolist() == [3, 0, 2, 1, 0, 1, 0, 2]
    want = R.lists_agreement(a, b)
    assert np.array_equal(overlap, want[0]) and np.array_equal(prefix, want[1])
    rng = np.random.default_rng(5)
    for n, k, pool in ((40, 1, 3), (200, 7, 12), (64, 10, 300), (3, 5, 5)):
        tables = []
        for _ in range(2):
            t = np.array([rng.permutation(pool)[:k] if pool >= k else np.r_[rng.permutation(pool), [-1] * (k - pool)]
                          for _ in range(n)])
            cut = rng.integers(0, k + 1, size=n)                # a row's valid entries come first
            t[np.arange(k)[None, :] >= cut[:, None]] = -1
            tables.append(t)
        overlap, prefix = _compare.list_agreement(*tables)
        want = R.lists_agreement(*tables)
        assert np.array_equal(overlap, want[0]) and np.array_equal(prefix, want[1]), (n, k)
    for shape in ((0, 3), (4, 0)):
        overlap, prefix = _compare.list_agreement(np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32))
        assert overlap.tolist() == [0] * shape[0] and prefix.tolist() == [0] * shape[0]


def test_the_frames_of_compare_from_hand_made_arrays():
    """``_compare_frames`` is host arithmetic on the sweep's arrays: equal to the reference's ``model`` on a hand-made pair."""
    index = pd.Index(["a", "b", "c"])
    SA = np.array([[1.0, 0.5, 0.0], [0.5, 1.0, 0.25], [0.0, 0.25, 1.0]])
    SB = np.array([[1.0, 0.5, 0.0], [0.25, 1.0, 0.5], [0.0, 0.25, 1.0 - 2.0 ** -20]])
    tols, swept = (0.1, 0.0, 1e-7), (0.0, 1e-7, 0.1)
    ids_a, ids_b = np.array([[1, 2], [0, 2], [1, 0]]), np.array([[1, 2], [2, 0], [1, 0]])
    max_abs, arg_abs, max_rel, arg_rel, over, hist = R.sweep(SA, SB, swept, 0.0)
    overlap, prefix = _compare.list_agreement(ids_a, ids_b)
    got = dict(max_abs=max_abs, arg_abs=arg_abs, max_rel=max_rel, arg_rel=arg_rel, over=over, hist=hist.astype(np.int64),
               overlap=overlap, same_prefix=prefix, k=2)
    summary, nodes, histogram = SRA.SimRank._compare_frames(index, got, swept, tols)
    want_s, want_n, want_h = R.model(SA, SB, index, tols, 0.0, (ids_a, ids_b, 2))
    assert nodes.index.equals(index) and nodes.columns.tolist() == list(want_n)
    assert nodes.columns.tolist() == ["max_abs", "at", "max_rel", "at_rel", "differing", "over@0.1", "over@0.0", "over@1e-07",
                                      "overlap", "same_prefix"]
    for name, col in want_n.items():
        assert nodes[name].tolist() == col.tolist(), name
    assert nodes["at"].tolist() == ["a", "a", "c"] and nodes["differing"].tolist() == [0, 2, 1]
    assert len(summary) == 1 and summary.columns.tolist() == list(want_s)
    for name, value in want_s.items():
        assert summary[name][0] == value, name
    assert summary["node"][0] == "b" and summary["neighbor"][0] == "a" and summary["entries"][0] == 9   # 0.25 twice: the first
    assert summary["identical_lists"][0] == 2 and summary["mean_overlap"][0] == 2.0
    assert summary["entries"].dtype == np.int64 and summary["differing"].dtype == np.int64
    assert histogram.dtype == np.int64 and histogram.index.tolist() == list(range(2048)) and histogram.index.name == "bin"
    assert np.array_equal(histogram.to_numpy(), want_h) and histogram.sum() == 9
