"""libsimrank_select.so (include/simrank_select.h) on a machine without a GPU: header, binding and exports agree, the
header is plain C, the threshold conversion is exact, argument checks need no device, the host merge orders the hits
as the dense frame's masked ``np.nonzero``, and ``fit(min_similarity=...)`` refuses bad thresholds before any device
work.  The main library's ABI stays at version 8 with 117 entry points."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from simrank_amd import _select
from tests import companion_abi as A


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_select) == _select.VERSION == 1


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_select)


def test_main_library_abi_is_unchanged():
    version, names, exports = A.main_library(_select)
    assert version == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_a_c_program_links(tmp_path):
    assert "select 1 ok" in A.run_c99(_select, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_select.h"
int main(void) {
    float t32 = 0.f;
    int64_t off[3];
    int32_t counts[2] = {1, 2};
    int64_t total = -1;
    if (simrank_select_version() != SIMRANK_SELECT_VERSION) return 1;
    if (simrank_select_threshold_f32(0.1, &t32) != SIMRANK_SELECT_OK || !((double)t32 >= 0.1)) return 2;
    if (simrank_select_threshold_f32(-1.0, &t32) != SIMRANK_SELECT_ERR_INVALID) return 3;
    if (!strlen(simrank_select_last_error())) return 4;
    if (simrank_select_count(NULL, SIMRANK_SELECT_PANEL_F32, 8, 4, 4, NULL, NULL, 0.5f, NULL, NULL)
        != SIMRANK_SELECT_ERR_INVALID) return 5;
    if (simrank_select_offsets(counts, 2, off, &total) != SIMRANK_SELECT_OK || total != 3 || off[2] != 3) return 6;
    printf("select %d ok\n", simrank_select_version());
    return 0;
}
''')


def _smallest_f32_at_least(t):
    """NumPy: the smallest float32 x with float64(x) >= t, by walking from the nearest float32."""
    with np.errstate(over="ignore"):
        x = np.float32(t)
    while float(x) < t:
        x = np.nextafter(x, np.float32(np.inf))
    while float(np.nextafter(x, np.float32(0))) >= t:
        x = np.nextafter(x, np.float32(0))
    return x


@pytest.mark.parametrize("t", [0.1, 1 / 3, 0.05000000001, 0.5, 1.0, 2.0 ** -20, 1e-40, 0.7999999999999999, 3.9,
                               float(np.float32(0.1)), float(np.float32(1 / 3)), 1e39])
def test_threshold_conversion_is_exact(t):
    t32 = _select.threshold_f32(t)
    want = _smallest_f32_at_least(t)
    assert np.float32(t32).view(np.uint32) == want.view(np.uint32), (t, t32, want)
    # the f32 compare is the float64 compare on every float32 around t
    around = [np.float32(t32)]
    for _ in range(3):
        around.append(np.nextafter(around[-1], np.float32(np.inf)))
        around.insert(0, np.nextafter(around[0], np.float32(0)))
    for v in around:
        assert (v >= np.float32(t32)) == (float(v) >= t), (t, v)


def test_threshold_ties_are_hits():
    """t equal to a stored float32 value: that value is a hit, the one below it is not."""
    for v in np.float32([0.1, 0.25, 1 / 3, 0.8, 1.0, 1e-30]):
        t32 = np.float32(_select.threshold_f32(float(v)))
        assert t32 == v
        assert not float(np.nextafter(v, np.float32(0))) >= float(v)


@pytest.mark.parametrize("bad", [0, 0.0, -1, -1e-300, float("nan"), float("inf"), -float("inf"), True, "0.5", None])
def test_threshold_refuses_what_is_not_a_positive_finite_number(bad):
    with pytest.raises(ValueError, match="min_similarity"):
        _select.threshold_f32(bad)


def test_null_and_out_of_range_arguments_fail_with_a_message():
    lib = _select.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    aligned = p if p % 16 == 0 else p + (16 - p % 16)
    calls = {
        "NULL S": lambda: lib.simrank_select_count(None, 0, 8, 4, 4, None, None, 0.5, p, None),
        "unknown layout": lambda: lib.simrank_select_count(aligned, 7, 8, 4, 4, None, None, 0.5, p, None),
        "stride < rows": lambda: lib.simrank_select_count(aligned, 0, 2, 4, 4, None, None, 0.5, p, None),
        "ld < cols": lambda: lib.simrank_select_count(aligned, 1, 3, 4, 4, None, None, 0.5, p, None),
        "no rows": lambda: lib.simrank_select_count(aligned, 0, 8, 0, 4, None, None, 0.5, p, None),
        "2^31 columns": lambda: lib.simrank_select_count(aligned, 1, 1 << 31, 1, 1 << 31, None, None, 0.5, p, None),
        "NULL counts": lambda: lib.simrank_select_count(aligned, 0, 8, 4, 4, None, None, 0.5, None, None),
        "threshold 0": lambda: lib.simrank_select_count(aligned, 0, 8, 4, 4, None, None, 0.0, p, None),
        "threshold nan": lambda: lib.simrank_select_count(aligned, 0, 8, 4, 4, None, None, float("nan"), p, None),
        "unaligned panels": lambda: lib.simrank_select_count(aligned + 4, 0, 8, 4, 4, None, None, 0.5, p, None),
        "emit NULL offsets": lambda: lib.simrank_select_emit(aligned, 0, 8, 4, 4, None, None, 0.5, None, 4, p, p, None),
        "emit NULL outputs": lambda: lib.simrank_select_emit(aligned, 0, 8, 4, 4, None, None, 0.5, p, 4, None, None, None),
        "emit capacity < 0": lambda: lib.simrank_select_emit(aligned, 0, 8, 4, 4, None, None, 0.5, p, -1, p, p, None),
        "offsets NULL": lambda: lib.simrank_select_offsets(None, 4, p, None),
        "threshold NULL out": lambda: lib.simrank_select_threshold_f32(0.5, None),
        "merge no pieces": lambda: lib.simrank_select_merge(0, None, None, None, 4, None, None, None, None, 0),
    }
    for what, call in calls.items():
        assert call() == -1, what
        assert lib.simrank_select_last_error(), what


def _pieces_from_dense(S, ord_, blocks, t):
    """What the emit pass writes for a dense S held in the solver's order (rows and columns permuted by ord_), split in
    column blocks: per block, per solver row, the hits in solver-column order with caller ids."""
    n = S.shape[0]
    Ssolver = S[np.ix_(ord_, ord_)]
    pieces = []
    for lo, hi in blocks:
        off, ids, vals = [0], [], []
        for r in range(n):
            cols = [c for c in range(lo, hi) if float(Ssolver[r, c]) >= t and ord_[c] != ord_[r]]
            ids += [int(ord_[c]) for c in cols]
            vals += [Ssolver[r, c] for c in cols]
            off.append(len(ids))
        pieces.append((np.array(off, np.int64), np.array(ids, np.int32), np.array(vals, np.float32)))
    return pieces


@pytest.mark.parametrize("n,blocks", [(1, [(0, 1)]), (37, [(0, 37)]), (300, [(0, 64), (64, 128), (128, 300)]),
                                      (50, [(0, 0), (0, 50)])])
def test_host_merge_gives_the_masked_nonzero_of_the_dense_matrix(n, blocks):
    rng = np.random.default_rng(n)
    S = rng.random((n, n)).astype(np.float32)
    S = np.minimum(S, S.T)
    S[rng.random((n, n)) < 0.5] = 0
    np.fill_diagonal(S, 1)
    ord_ = rng.permutation(n).astype(np.int32)
    t = 0.6
    pieces = _pieces_from_dense(S, ord_, blocks, t)
    for threads in (1, 3, 0):
        off, ids, vals = _select.merge(pieces, ord_, threads)
        mask = S.astype(np.float64) >= t
        np.fill_diagonal(mask, False)
        r, c = np.nonzero(mask)
        assert np.array_equal(np.repeat(np.arange(n), np.diff(off)), r)
        assert np.array_equal(ids, c)
        assert np.array_equal(vals.view(np.uint32), S[r, c].view(np.uint32))


def test_host_merge_refuses_an_order_that_is_not_a_permutation():
    off = np.array([0, 0, 0], np.int64)
    with pytest.raises(_select.SelectError, match="permutation"):
        _select.merge([(off, np.zeros(0, np.int32), np.zeros(0, np.float32))], np.array([0, 0], np.int32))
    with pytest.raises(_select.SelectError, match="same id"):
        _select.merge([(np.array([0, 2], np.int64), np.array([3, 3], np.int32), np.zeros(2, np.float32))],
                      np.array([0], np.int32))


@pytest.mark.parametrize("cls", ["SimRank", "SimRankPP", "AprioriSimRank", "BipartiteSimRank", "BipartiteSimRankPP",
                                 "BipartitleAprioriSimRank", "BipartitleSimRank", "BipartiteAprioriSimRank"])
@pytest.mark.parametrize("t", [0, -1, float("nan"), float("inf")])
def test_fit_refuses_a_bad_threshold_before_any_device_work(cls, t):
    """ValueError names the keyword; it comes before the library's "no CPU fallback" error (or any device call)."""
    import simrank_amd.SimRank as SRA
    est = getattr(SRA, cls)()
    if cls.startswith("Bipart"):
        df = pd.DataFrame({"user": [1, 2], "item": [3, 3]})
        args = (df, np.eye(2), np.eye(1)) if "Apriori" in cls else (df,)
    else:
        df = pd.DataFrame({"from": [1, 2], "to": [2, 1]})
        args = (df, np.eye(2)) if "Apriori" in cls else (df,)
    with pytest.raises(ValueError, match="min_similarity"):
        est.fit(*args, verbose=False, min_similarity=t)


@pytest.mark.parametrize("m", [0, -5, 2.5, True])
def test_fit_refuses_a_bad_max_pairs(m):
    import simrank_amd.SimRank as SRA
    with pytest.raises(ValueError, match="max_pairs"):
        SRA.SimRank().fit(pd.DataFrame({"from": [1, 2], "to": [2, 1]}), verbose=False, min_similarity=0.5, max_pairs=m)


def test_keywords_are_keyword_only_and_default_off():
    import inspect
    import simrank_amd.SimRank as SRA
    for name in ("SimRank", "SimRankPP", "AprioriSimRank", "BipartiteSimRank", "BipartiteSimRankPP",
                 "BipartitleAprioriSimRank"):
        sig = inspect.signature(getattr(SRA, name).fit)
        for kw, default in (("min_similarity", None), ("max_pairs", 2 ** 27)):
            assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY, (name, kw)
            assert sig.parameters[kw].default == default, (name, kw)
