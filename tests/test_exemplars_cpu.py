"""libsimrank_exemplars.so (include/simrank_exemplars.h) and ``exemplars`` on a machine without a GPU: header, binding and
exports agree, the header is plain C99 and stands alone, the entries refuse bad arguments without a device, the method's
arguments are judged before any device work, the lazy loop returns what plain greedy returns on matrices built to break
it, the reference's ordered sum is monotone under cover raises and stays inside its bound, the host path of a pruned
model equals greedy on the dense P, and the dyadic fit the GPU test uses does hold exact ties."""
import math
import re

import numpy as np
import pandas as pd
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _exemplars, _lib, _neighbors, _query
from tests import companion_abi as A
from tests import exact as X
from tests import exemplars_ref as ER
from tests.test_cluster_cpu import HostOps, _FullSpec, boom, guarded_estimator
from tests.test_groups_cpu import same, table_cases
from tests.test_kmedoids_cpu import matrix_p


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_exemplars) == _exemplars.VERSION == 1
    text = A.header(_exemplars)
    assert re.search(r"#define SIMRANK_EXEMPLARS_THREADS %d\b" % _exemplars.THREADS, text) and ER.T == _exemplars.THREADS
    assert re.search(r"#define SIMRANK_EXEMPLARS_GRID_CAP %d\b" % _exemplars.GRID_CAP, text)
    assert sorted(_exemplars.PROTOTYPES) == ["simrank_exemplars_cover", "simrank_exemplars_gains",
                                             "simrank_exemplars_last_error", "simrank_exemplars_version"]
    A.assert_header_stands_alone(_exemplars)
    A.assert_prototypes_match_the_header_argument_counts(_exemplars)
    assert A.layout_codes(_exemplars) == A.layout_codes(_query) and len(A.layout_codes(_exemplars)) == 4


def test_companion_links_nothing_of_the_main_library_which_is_unchanged():
    A.assert_links_nothing_of_the_main_library(_exemplars)
    version, names, exports = A.main_library(_exemplars)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_the_entries_refuse_bad_arguments_without_a_device(tmp_path):
    assert "exemplars 1 ok" in A.run_c99(_exemplars, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_exemplars.h"
#define BAD(call, code) do { if ((call) != SIMRANK_EXEMPLARS_ERR_INVALID) return code; \
                             if (!strlen(simrank_exemplars_last_error())) return 100 + code; } while (0)
int main(void) {
    /* aligned stand-ins for device memory: nothing below may reach a device */
    static double mem[8];
    static int32_t ids[8];
    static uint32_t count[8];
    const void* S = mem;
    double* d = mem;
    const int32_t f32 = SIMRANK_EXEMPLARS_ROWMAJOR_F32;
    const int64_t huge = (int64_t)1 << 31;
    if (simrank_exemplars_version() != SIMRANK_EXEMPLARS_VERSION) return 1;
    /* gains: NULL pointers, one at a time (rows may be NULL) */
    BAD(simrank_exemplars_gains(NULL, f32, 4, 4, 4, ids, 2, d, d, NULL), 2);
    BAD(simrank_exemplars_gains(S, f32, 4, 4, 4, ids, 2, NULL, d, NULL), 3);
    BAD(simrank_exemplars_gains(S, f32, 4, 4, 4, ids, 2, d, NULL, NULL), 4);
    /* without rows the list is every row */
    BAD(simrank_exemplars_gains(S, f32, 4, 4, 4, NULL, 3, d, d, NULL), 5);
    if (!strstr(simrank_exemplars_last_error(), "n_list")) return 6;
    /* a bad list length */
    BAD(simrank_exemplars_gains(S, f32, 4, 4, 4, ids, -1, d, d, NULL), 7);
    BAD(simrank_exemplars_gains(S, f32, 4, 4, 4, ids, huge, d, d, NULL), 8);
    /* an unknown layout */
    BAD(simrank_exemplars_gains(S, 4, 4, 4, 4, ids, 2, d, d, NULL), 10);
    BAD(simrank_exemplars_gains(S, -1, 4, 4, 4, ids, 2, d, d, NULL), 11);
    /* a stride too small: columns of a row-major block, rows of a panel block */
    BAD(simrank_exemplars_gains(S, f32, 3, 4, 4, ids, 2, d, d, NULL), 12);
    BAD(simrank_exemplars_gains(S, SIMRANK_EXEMPLARS_ROWMAJOR_F64, 3, 4, 4, ids, 2, d, d, NULL), 13);
    BAD(simrank_exemplars_gains(S, SIMRANK_EXEMPLARS_PANEL_F32, 3, 4, 2, ids, 2, d, d, NULL), 14);
    BAD(simrank_exemplars_gains(S, SIMRANK_EXEMPLARS_PANEL_F16, 3, 4, 2, ids, 2, d, d, NULL), 15);
    /* a negative shape, a shape of 2^31 */
    BAD(simrank_exemplars_gains(S, f32, 4, -1, 4, ids, 2, d, d, NULL), 16);
    BAD(simrank_exemplars_gains(S, f32, 4, 4, -1, ids, 2, d, d, NULL), 17);
    BAD(simrank_exemplars_gains(S, f32, huge, 4, huge, ids, 2, d, d, NULL), 18);
    BAD(simrank_exemplars_gains(S, SIMRANK_EXEMPLARS_PANEL_F32, huge, huge, 4, ids, 2, d, d, NULL), 19);
    /* a block that does not start on a multiple of its element's size; a cover off 8 bytes */
    BAD(simrank_exemplars_gains((const char*)S + 2, f32, 4, 4, 4, ids, 2, d, d, NULL), 20);
    BAD(simrank_exemplars_gains((const char*)S + 4, SIMRANK_EXEMPLARS_ROWMAJOR_F64, 4, 1, 4, ids, 2, d, d, NULL), 21);
    BAD(simrank_exemplars_gains((const char*)S + 1, SIMRANK_EXEMPLARS_PANEL_F16, 4, 1, 4, ids, 2, d, d, NULL), 22);
    if (!strstr(simrank_exemplars_last_error(), "element")) return 23;
    BAD(simrank_exemplars_gains(S, f32, 4, 4, 4, ids, 2, (const double*)((const char*)d + 4), d, NULL), 24);
    if (!strstr(simrank_exemplars_last_error(), "cover")) return 25;
    /* no listed rows: nothing to queue */
    if (simrank_exemplars_gains(S, f32, 4, 4, 4, ids, 0, d, NULL, NULL) != SIMRANK_EXEMPLARS_OK) return 26;
    if (simrank_exemplars_gains(NULL, f32, 4, 0, 4, NULL, 0, d, NULL, NULL) != SIMRANK_EXEMPLARS_OK) return 27;
    /* cover: NULL pointers, one at a time; an empty list; the block checks */
    BAD(simrank_exemplars_cover(NULL, f32, 4, 4, 4, ids, 2, d, count, NULL), 30);
    BAD(simrank_exemplars_cover(S, f32, 4, 4, 4, NULL, 2, d, count, NULL), 31);
    BAD(simrank_exemplars_cover(S, f32, 4, 4, 4, ids, 2, NULL, count, NULL), 32);
    BAD(simrank_exemplars_cover(S, f32, 4, 4, 4, ids, 2, d, NULL, NULL), 33);
    BAD(simrank_exemplars_cover(S, f32, 4, 4, 4, ids, 0, d, count, NULL), 34);
    BAD(simrank_exemplars_cover(S, f32, 4, 4, 4, ids, -2, d, count, NULL), 35);
    BAD(simrank_exemplars_cover(S, 7, 4, 4, 4, ids, 2, d, count, NULL), 36);
    BAD(simrank_exemplars_cover(S, f32, 3, 4, 4, ids, 2, d, count, NULL), 37);
    BAD(simrank_exemplars_cover(S, SIMRANK_EXEMPLARS_PANEL_F16, 3, 4, 2, ids, 2, d, count, NULL), 38);
    BAD(simrank_exemplars_cover((const char*)S + 2, f32, 4, 4, 4, ids, 2, d, count, NULL), 39);
    BAD(simrank_exemplars_cover(S, f32, 4, 4, 4, ids, 2, (double*)((char*)d + 4), count, NULL), 40);
    /* no columns: nothing to queue */
    if (simrank_exemplars_cover(NULL, f32, 4, 4, 0, ids, 2, NULL, count, NULL) != SIMRANK_EXEMPLARS_OK) return 41;
    printf("exemplars %d ok\n", simrank_exemplars_version());
    return 0;
}
''')


# ---- the arguments: judged before any device work ---------------------------------------------------------------------------
INDEX = pd.Index(["a", "b", "c"])
BAD_GIVEN = [["a", "a"], ["a", "b", "a"], pd.Series(["b", "b"]), np.array(["c", "c"]),              # a repeated label
             "abc", "a", b"a", 7, 1.5, {"a": 0}, pd.DataFrame({"x": ["a"]}), np.array([["a"]]),      # no sequence of labels
             iter(["a"]), (x for x in "ab"), {"a", "b"}]
BAD_K = [0, -1, True, False, np.True_, 1.5, 2.0, None, "2", [2], 4, 10 ** 30]


def test_what_the_argument_checks_refuse_and_accept():
    for bad in BAD_GIVEN:
        with pytest.raises(ValueError, match="given"):
            _exemplars.check_given(bad, INDEX)
    for unknown in (["a", "z"], ["z"], pd.Series(["b", "z"], index=[4, 5]), [0]):
        with pytest.raises(KeyError):
            _exemplars.check_given(unknown, INDEX)
    for none in (None, [], (), np.array([], dtype=object)):
        got = _exemplars.check_given(none, INDEX)
        assert got.dtype == np.int64 and got.size == 0
    for good in (["c", "a"], ("c", "a"), np.array(["c", "a"]), pd.Series(["c", "a"], index=[7, -2]), pd.Index(["c", "a"])):
        got = _exemplars.check_given(good, INDEX)
        assert got.dtype == np.int64 and got.tolist() == [2, 0], good
    for bad in BAD_K:
        with pytest.raises(ValueError, match="k "):
            _exemplars.check_k(bad, 3, 0)
    for bad in (3, 2 ** 40):
        with pytest.raises(ValueError, match="too large"):
            _exemplars.check_k(bad, 3, 1)
    assert _exemplars.check_k(np.int64(3), 3, 0) == 3 and _exemplars.check_k(1, 3, 2) == 1
    for bad in (0, 1, None, "yes", [True], 1.0):
        with pytest.raises(ValueError, match="lazy"):
            _exemplars.check_lazy(bad)
    assert _exemplars.check_lazy(np.True_) is True and _exemplars.check_lazy(False) is False


def test_argument_checks_need_no_device(monkeypatch):
    for name in ("exemplars", "load", "greedy", "DeviceEvaluator", "ListsEvaluator"):
        monkeypatch.setattr(_exemplars, name, boom)
    with pytest.raises(RuntimeError, match="no kept model"):
        SRA.SimRank().exemplars(1)
    est = guarded_estimator()
    for bad in BAD_K:
        with pytest.raises(ValueError, match="k "):
            est.exemplars(bad)
    with pytest.raises(ValueError, match="too large"):
        est.exemplars(3, given=["b"])
    for bad in BAD_GIVEN:
        with pytest.raises(ValueError, match="given"):
            est.exemplars(1, given=bad)
    with pytest.raises(KeyError, match="z"):
        est.exemplars(1, given=["a", "z"])
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="lazy"):
            est.exemplars(1, lazy=bad)
    for bad in (2, 0, "1"):
        with pytest.raises(ValueError, match="group"):
            est.exemplars(1, group=bad)
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.exemplars(1)


# ---- the reference by hand -------------------------------------------------------------------------------------------------------
def test_the_reference_by_hand():
    nan, inf = float("nan"), float("inf")
    cover = np.array([0.0, 0.5, 0.5, 0.25, 0.0, 1.0, 0.0])
    row = np.array([0.25, 0.5, 0.75, nan, -1.0, inf, -0.0])
    t = ER.terms(row, cover)
    assert same(t, [0.25, 0.0, 0.25, 0.0, 0.0, inf, 0.0]) and not np.signbit(t).any()      # (equal: the strict >)
    assert ER.gain(row, cover) == inf and ER.gain(row[:5], cover[:5]) == 0.5 == ER.exact_sum(t[:5])
    c = cover.copy()
    assert ER.apply(row, c) == 3 and same(c, [0.25, 0.5, 0.75, 0.25, 0.0, inf, 0.0])
    assert ER.apply(row, c) == 0                                                            # (inf > inf is false)
    assert ER.gain(row, c) == 0.0
    assert same(ER.coverage(np.array([row, [0.5, nan, 0.0, 0.125, -2.0, 2.0, 0.0]])), [0.5, 0.5, 0.75, 0.125, 0.0, inf, 0.0])
    A_ = np.array([[0.5, 0.25, 0.0], [0.25, 0.5, 0.5], [0.0, 0.5, 0.5]])
    assert same(ER.block_gains(A_, [1, -1, 3, 0, 1], np.zeros(3)), [1.25, nan, nan, 0.75, 1.25])
    cov, raised = ER.block_cover(A_, [0, 5, 1, 0, -2], np.zeros(3), [0, 7, 0, 0, 1])
    assert same(cov, [0.5, 0.5, 0.5]) and raised.tolist() == [2, 7, 2, 0, 1]
    # rows 1 and 2 tie at 1.25 on the empty cover: the smaller position wins; then row 0 gains 0.5 - 0.25, row 2 nothing
    picks, gains, raised, cov = ER.greedy(A_, 3)
    assert picks.tolist() == [1, 0, 2] and gains.tolist() == [1.25, 0.25, 0.0] and raised.tolist() == [3, 1, 0]
    picks, gains, raised, cov = ER.greedy(A_, 1, given=[1])
    assert picks.tolist() == [0] and gains.tolist() == [0.25] and same(cov, [0.5, 0.5, 0.5])


def test_the_ordered_sum_is_exact_on_dyadic_terms_and_inside_its_bound_on_others():
    rng = np.random.default_rng(3)
    for n in (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4097, 9000):
        t = rng.integers(0, 4096, size=n) * 2.0 ** -8
        assert ER.ordered_sum(t) == ER.exact_sum(t) == float(t.sum())
        t = rng.random(n) * 2.0 ** rng.integers(-40, 3, size=n)
        got, exact = ER.ordered_sum(t), ER.exact_fraction(t)
        assert abs(got - exact) <= (n + 1) * 2.0 ** -52 * exact and abs(got - ER.exact_sum(t)) <= ER.bound(t)
    # the order is not the left-to-right one: a sum that tells them apart
    t = np.zeros(1025)
    t[[0, 4, 1024]] = [2.0 ** -53, 1.0, 2.0 ** -53]                      # columns 0 and 1024 share a running sum
    left_to_right = 0.0
    for x in t:
        left_to_right += x
    assert ER.ordered_sum(t) == 1.0 + 2.0 ** -52 and left_to_right == 1.0


def test_the_ordered_sum_is_monotone_under_cover_raises():
    """What lazy evaluation relies on: raise any part of the cover and no gain rises, in floating point."""
    rng = np.random.default_rng(8)
    for n in (37, 300, 1100):
        for _ in range(6):
            row = rng.random(n) * 2.0 ** rng.integers(-30, 1, size=n)
            row[rng.random(n) < 0.05] = np.nan
            cover = np.where(rng.random(n) < 0.5, 0.0, rng.random(n) * 0.5)
            last = ER.gain(row, cover)
            for step in range(12):
                at = rng.random(n) < 0.2
                tiny = rng.random(n) < 0.5                             # raises of one ulp and large ones
                cover = np.where(at, np.where(tiny, np.nextafter(cover, 2.0), cover + rng.random(n) * 0.1), cover)
                now = ER.gain(row, cover)
                assert now <= last, (n, step, now, last)
                last = now


# ---- lazy against plain, through the NumPy evaluator -------------------------------------------------------------------------------
def hostile_matrices():
    rng = np.random.default_rng(17)
    nan, inf = float("nan"), float("inf")
    out = {"all zeros": np.zeros((40, 40))}
    out["identical rows"] = np.tile(rng.integers(0, 9, size=60) / 8.0, (60, 1))
    # plateaus of exact ties: blocks of nodes whose rows are permutations within the block, so whole groups tie
    n = 120
    S = np.zeros((n, n))
    for lo in range(0, n, 8):
        S[lo:lo + 8, lo:lo + 8] = 0.5 - 0.125 * ((lo // 8) % 3)
    S[np.arange(n), np.arange(n)] = 1.0
    out["plateaus"] = S
    S = rng.random((150, 150)) * (rng.random((150, 150)) < 0.1)
    S[[3, 70]] = nan
    S[rng.random(S.shape) < 0.02] = nan
    out["nan rows and entries"] = S
    S = rng.integers(-8, 9, size=(90, 90)) / 8.0
    out["negative entries"] = S
    S = rng.random((64, 64))
    S[5, 9] = S[40, 2] = S[41, 2] = inf
    out["inf"] = S
    out["random, not square-symmetric"] = rng.random((300, 300)) ** 6
    return out


@pytest.mark.parametrize("name", list(hostile_matrices()))
def test_lazy_returns_what_plain_greedy_returns(name):
    S = hostile_matrices()[name]
    n = len(S)
    k = min(n, 25)
    want = ER.greedy(S, k)
    plain = _exemplars.greedy(ER.DenseEvaluator(S), n, k, (), lazy=False)
    assert plain[0].tolist() == want[0].tolist() and same(plain[1], want[1]) and plain[2].tolist() == want[2].tolist()
    assert plain[3].tolist() == [n - p for p in range(k)] and plain[4] == k
    for batch in (1, 2, 3, n):
        ev = ER.DenseEvaluator(S)
        got = _exemplars.greedy(ev, n, k, (), lazy=True, batch=batch)
        assert got[0].tolist() == want[0].tolist(), (name, batch)
        assert same(got[1], want[1]) and got[2].tolist() == want[2].tolist(), (name, batch)
        assert same(ev.cover, want[3])
        assert got[3][0] == n and (got[3][1:] >= 1).all() and got[4] == len(ev.calls)
        assert all(c is None or (1 <= c.size <= batch and np.unique(c).size == c.size) for c in ev.calls)
        assert got[3].sum() == n + sum(c.size for c in ev.calls if c is not None)
        if name == "random, not square-symmetric" and batch == 3:
            assert got[3][1:].sum() < (k - 1) * n // 2                  # lazy does evaluate fewer rows
    if name == "plateaus":
        assert (np.diff(want[0][:5]) > 0).all() and len(set(want[1][:5])) == 1    # exact ties: positions ascend


def test_given_rows_come_first_and_are_never_picked():
    S = hostile_matrices()["random, not square-symmetric"]
    n = len(S)
    given = [7, 250, 3]
    want = ER.greedy(S, 10, given)
    assert not set(want[0]) & set(given) and not same(want[0], ER.greedy(S, 10)[0])
    for lazy in (False, True):
        ev = ER.DenseEvaluator(S)
        got = _exemplars.greedy(ev, n, 10, np.array(given), lazy=lazy, batch=3)
        assert got[0].tolist() == want[0].tolist() and same(got[1], want[1]) and got[2].tolist() == want[2].tolist()
        assert got[3][0] == n - 3 and same(ev.cover, want[3])
    # given covering everything: every gain is +0.0, the picks are the first candidates in the frame's order
    S2 = S.copy()
    S2[11] = 2.0
    for lazy in (False, True):
        got = _exemplars.greedy(ER.DenseEvaluator(S2), n, n - 1, [11], lazy=lazy, batch=2)
        assert got[0].tolist() == [m for m in range(n) if m != 11] and not got[1].any() and not got[2].any()
        assert not np.signbit(got[1]).any()
    # every node picked
    got = _exemplars.greedy(ER.DenseEvaluator(S[:40, :40]), 40, 40, (), lazy=True, batch=3)
    assert sorted(got[0].tolist()) == list(range(40))


def test_a_gain_above_its_bound_is_an_error():
    class Liar(ER.DenseEvaluator):
        def gains(self, rows):
            g = super().gains(rows)
            return g if rows is None else g + 100.0
    with pytest.raises(_exemplars.ExemplarsError, match="bound"):
        _exemplars.greedy(Liar(np.eye(64) + 0.25), 64, 5, (), lazy=True, batch=2)


# ---- the host path of a pruned model ------------------------------------------------------------------------------------------------
def test_the_host_path_of_pruned_lists_equals_greedy_on_the_dense_p():
    for ids, vals, _ in table_cases():
        n = len(ids)
        diag = 1.0 - 0.125 * (np.arange(n) % 3)
        P = matrix_p(ids, vals, diag)
        for given in ((), (2,), (n - 1, 0)):
            k = n - len(given)
            want = ER.greedy(P, k, given, total=ER.exact_sum)
            for lazy in (False, True):
                ev = _exemplars.ListsEvaluator(ids, vals, diag)
                got = _exemplars.greedy(ev, n, k, np.array(given, dtype=np.int64), lazy=lazy, batch=2)
                assert got[0].tolist() == want[0].tolist() and same(got[1], want[1]), (given, lazy)
                assert got[2].tolist() == want[2].tolist() and same(ev.cover(), want[3])


def test_the_method_on_a_pruned_model(monkeypatch):
    monkeypatch.setattr(_exemplars, "load", boom)             # (a pruned model needs no library)
    ops = HostOps()
    ids, vals, _ = table_cases()[0]
    names = list("abcdefg")
    diag = np.array([1.0, 0.5, 1.0, 1.0, 0.75, 1.0, 1.0])
    solver = _neighbors.NeighborSolver(ops, [_FullSpec(7)], [_neighbors.Tables.from_host(ops, ids, vals, diag)])
    est = SRA.SimRank()._keep(solver, [(0, names)])
    P = matrix_p(ids, vals, diag)
    for given, at in ((None, []), (["e", "b"], [4, 1])):
        want = ER.greedy(P, 4, at, total=ER.exact_sum)
        out = {}
        for lazy in (False, True):
            picks, coverage = est.exemplars(4, given=given, lazy=lazy)
            assert picks.index.tolist() == [0, 1, 2, 3] and picks.index.name == "rank"
            assert picks.columns.tolist() == ["exemplar", "gain", "raised", "evaluated"]
            assert picks.dtypes.tolist()[1:] == [np.float64, np.int64, np.int64]
            assert picks["exemplar"].tolist() == [names[m] for m in want[0]] and same(picks["gain"], want[1])
            assert picks["raised"].tolist() == want[2].tolist()
            assert coverage.name == "coverage" and coverage.dtype == np.float64 and coverage.index.tolist() == names
            assert same(coverage, want[3])
            assert same(coverage, ER.coverage(P[at + want[0].tolist()]))
            out[lazy] = picks
        assert out[False]["evaluated"].tolist() == [7 - len(at) - p for p in range(4)]
        assert out[True].drop(columns="evaluated").equals(out[False].drop(columns="evaluated"))
    labels, clusters, _ = est.kmedoids(picks["exemplar"])     # a Series of labels seeds kmedoids
    assert len(clusters) == 4 and labels.index.tolist() == names
    assert est.kept_neighbors == 2                            # the model is as it was
    est.release()
    with pytest.raises(RuntimeError, match="released"):
        est.exemplars(1)
    assert not ops.live


DYADIC_K = 60            # picks on the dyadic fit, here and in tests/test_gpu_exemplars.py


# ---- the dyadic fit of the GPU test holds exact ties ------------------------------------------------------------------------------------
def test_the_reference_meets_exact_ties_on_the_dyadic_fit():
    """regular_graph(256, 4) with C = 0.5, as tests/test_gpu_exemplars.py fits it: every sum of its elements is exact, so
    the ordered sum is the exact one, and from the 52nd pick on the best candidates do tie exactly: within ``DYADIC_K``
    picks the rule (smaller position first) decides some."""
    from oracle import simrank_oracle as O
    df = X.regular_graph(256, 4, seed=260)
    _, G = O.directed_graph(df)
    updates = X.exact_updates(G, 0.5, None, mantissa=24, limit=8).updates
    assert updates >= 2
    S = np.asarray(O.fit_simrank(df, C=0.5, iterations=updates, eps=1e-30, verbose=False)["S"], dtype=np.float64)
    zero = np.zeros(256)
    first = ER.block_gains(S, None, zero)
    assert same(first, ER.block_gains(S, None, zero, total=ER.exact_sum))
    assert same(first, [float(ER.exact_fraction(ER.terms(r, zero))) for r in S])
    picks, gains, raised, cover = ER.greedy(S, DYADIC_K)
    tied, cov = 0, np.zeros(256)
    for p in picks:
        g = ER.block_gains(S, None, cov, total=ER.exact_sum)
        g[picks[:list(picks).index(p)]] = -1.0
        assert g.argmax() == p
        tied += int((g == g[p]).sum() > 1)
        ER.apply(S[p], cov)
    assert tied >= 2
