"""tests/evidence_ref.py checked on the host: the reference against a brute-force dense product, and every pattern of
tests/test_gpu_evidence_edges.py for what the GPU tests rely on — the hub count by the rule, the planted counts before
clipping, which side of column 65 536 each planted row lies on, and a walk short enough for a test.  The NumPy double
(tests/cpu_ops.py) is held to the same reference where a dense square fits."""
import numpy as np
import pytest

from tests import evidence_ref as E
from tests.cpu_ops import NumpyOps

BIG = [65535, 65536, 65537, 65632]
WALK_MAX = 5 * 10 ** 8


@pytest.fixture(scope="module")
def big():
    return {n: E.big_case(n) for n in BIG}


def brute(p):
    dense = np.zeros((p.n_rows, p.n_cols), dtype=np.int64)
    for a in range(p.n_rows):
        if np.float32(p.rowscale[a]) > 0:
            dense[a, p.col[p.rowptr[a]:p.rowptr[a + 1]]] = 1
    return dense @ dense.T


@pytest.mark.parametrize("M,K,avg,seed", [(1, 1, 1, 0), (7, 3, 2, 1), (40, 300, 280, 2), (130, 65, 9, 3), (64, 700, 500, 4)])
def test_counts_equal_a_dense_product(M, K, avg, seed):
    rng = np.random.default_rng(seed)
    rows = [rng.choice(K, size=min(K, int(rng.poisson(avg))), replace=False) for _ in range(M)]
    scale = rng.random(M) + 0.1
    scale[rng.random(M) < 0.2] = 0.0
    scale[M // 2] = 1e-60                                         # positive in float64, zero in float32: a dead row
    p = E.from_rows(rows, K, scale)
    want = brute(p)
    assert not want[M // 2].any() and not want[:, M // 2].any()
    assert np.array_equal(E.raw_counts(p).toarray(), want)
    R = E.counts(p)
    assert np.array_equal(R.toarray(), np.minimum(want, 255))
    if seed in (2, 4):
        assert want.max() > 255
    r0, r1, c0, c1 = M // 3, M, M // 4, M - M // 5
    b = E.band(R, r0, r1, c0, c1)
    assert b.dtype == np.uint8 and np.array_equal(b, np.minimum(want, 255)[r0:r1, c0:c1])
    assert np.array_equal(E.live_refs(p), brute(E.from_rows(_transposed(p), M, np.ones(K))).diagonal())


def _transposed(p):
    cols = [[] for _ in range(p.n_cols)]
    for a in range(p.n_rows):
        if np.float32(p.rowscale[a]) > 0:
            for i in p.col[p.rowptr[a]:p.rowptr[a + 1]]:
                cols[i].append(a)
    return cols


def test_hub_rule_threshold_order_and_caps():
    """The rule on patterns small enough to read: the threshold is max(48, ceil(n_rows ev_hub / 1000)) on LIVE references,
    the order is references descending then column ascending, the cut is at 4096 and fewer than 8 candidates are none."""
    M = 100
    refs = [100, 60, 60, 48, 47, 99, 48, 55, 70, 50]              # per column; row a holds column i iff a < refs[i]
    rows = [[i for i, d in enumerate(refs) if a < d] for a in range(M)]
    p = E.from_rows(rows, len(refs), np.ones(M))
    assert list(E.live_refs(p)) == refs
    assert list(E.hubs(p, 1)) == [0, 5, 8, 1, 2, 7, 9, 3, 6]      # 47 is below the floor of 48
    assert list(E.hubs(p, 480)) == [0, 5, 8, 1, 2, 7, 9, 3, 6]    # ceil(100 * 480 / 1000) = 48 still
    assert E.hubs(p, 481).size == 0                               # ceil(48.1) = 49: seven candidates, no hub part
    assert E.hubs(p, 0).size == 0
    dead = np.ones(M)
    dead[:53] = 0                                                 # live references drop by 53 where a row below 53 held the column
    assert E.hubs(E.from_rows(rows, len(refs), dead), 1).size == 0
    wide = E.from_rows([np.arange(5000)] * 50 + [np.arange(10)], 5000, np.ones(51))
    h = E.hubs(wide, 1)
    assert h.size == 4096 and list(h[:12]) == list(range(12)) and h[-1] == 4095


def test_hub_rule_rounds_the_threshold_up():
    refs = [50] * 8 + [49] * 3
    p = E.from_rows([[i for i, d in enumerate(refs) if a < d] for a in range(100)], len(refs), np.ones(100))
    assert E.hubs(p, 490).size == 11                               # threshold 49
    assert list(E.hubs(p, 491)) == list(range(8)) == list(E.hubs(p, 500))    # ceil(49.1) = 50 = 50.0
    assert E.hubs(p, 501).size == 0                                # 51


def _check_planted(case):
    raw = E.raw_counts(case.pattern)
    for (a, b), want in case.planted.items():
        assert raw[a, b] == want == raw[b, a], (a, b, raw[a, b], want)
    assert E.walk_cost(case.pattern) < WALK_MAX
    assert raw.diagonal().sum() == E.live_pattern(case.pattern).nnz


def _check_double(case, blocks):
    """tests/cpu_ops.py's evidence_counts on the same blocks the GPU runs."""
    p = case.pattern
    ops, R = NumpyOps(), E.counts(p)
    g = ops.graph(p)
    for c0, L in blocks:
        out = ops.matrix(p.n_rows, L, np.uint8)
        ops.evidence_counts(g, c0, out)
        assert np.array_equal(out.a[:p.n_rows, :L], E.band(R, 0, p.n_rows, c0, c0 + L))


def test_cap_case_plants_the_counts_at_the_counter_caps():
    case = E.cap_case()
    p = case.pattern
    assert (p.n_rows, p.n_cols) == (48, 65600)
    raw = E.raw_counts(p)
    planted = sorted({raw[0, b] for b in range(10)}, reverse=True)
    assert planted == [65536, 65535, 16384, 16383, 255, 254, 0]
    _check_planted(case)
    assert E.live_refs(p).max() < E.MIN_REFS and all(E.hubs(p, h).size == 0 for h in (1, 14, 1000))
    R = E.counts(p)
    assert list(E.band(R, 0, 1, 0, 10)[0]) == [255, 255, 255, 255, 255, 255, 255, 254, 0, 0]
    # the counts beside the capped ones are small and not all alike: a carry out of a capped counter would show there
    assert R[0, 10:].toarray().max() < 30 and len(set(R[0, 10:].toarray().ravel())) > 5
    _check_double(case, [(0, 48), (1, 47), (2, 5)])


def test_cap_case_with_hub_rows_fills_the_hub_list():
    case = E.cap_case(hub_rows=64)
    p = case.pattern
    assert (p.n_rows, p.n_cols) == (112, 65600)
    _check_planted(case)
    refs = E.live_refs(p)
    assert int((refs >= E.MIN_REFS).sum()) == 5000 and not (refs[5000:] >= E.MIN_REFS).any()
    h = E.hubs(p, case.ev_hub)
    assert h.size == 4096 == E.MAX_HUBS and h.max() < 5000
    hubs01 = 4096                                                 # rows 0 and 1 hold every hub column
    assert hubs01 >= 255 and E.raw_counts(p)[0, 1] - hubs01 > 60000
    assert E.hubs(p, 0).size == 0
    _check_double(case, [(0, 112), (1, 111), (2, 5)])


@pytest.mark.parametrize("n_planted,want", [(7, 0), (8, 8)])
def test_few_hubs_cases_sit_on_either_side_of_eight(n_planted, want):
    case = E.few_hubs_case(n_planted)
    p = case.pattern
    assert (p.n_rows, p.n_cols) == (600, 900)
    assert int((E.live_refs(p) >= E.MIN_REFS).sum()) == n_planted
    h = E.hubs(p, case.ev_hub)
    assert h.size == want and set(h) == set(range(900 - want, 900))
    _check_planted(case)
    assert (np.asarray(p.rowscale, dtype=np.float32) == 0).any()
    _check_double(case, [(0, 600)])


def test_wide_case_has_its_hubs_above_the_line():
    case = E.wide_case()
    p = case.pattern
    assert (p.n_rows, p.n_cols) == (300, 70000)
    h = E.hubs(p, case.ev_hub)
    assert h.size == 16 and h.min() > E.LINE
    assert p.col.max() > E.LINE + 3000
    _check_planted(case)
    assert E.counts(p)[0, 1] == 255
    _check_double(case, [(0, 300)])


@pytest.mark.parametrize("n", BIG)
def test_big_cases(big, n):
    case = big[n]
    p = case.pattern
    assert p.n_rows == p.n_cols == n
    assert 2.5 < p.col.size / n < 3.6
    dead = np.asarray(p.rowscale, dtype=np.float32) == 0
    assert 0.04 < dead.mean() < 0.06
    thr = -(-n // 1000)
    assert thr in (66,) and thr > E.MIN_REFS
    h = E.hubs(p, case.ev_hub)
    refs = E.live_refs(p)
    assert 38 <= h.size <= 40 and refs[h].min() > 250 and np.sort(refs)[-h.size - 1] < 30
    assert h.min() == 0 and h.max() == n - 1
    _check_planted(case)
    assert all(v > 255 for v in case.planted.values())
    sides = [(a < E.LINE, b < E.LINE) for a, b in case.planted]
    assert any(a < 100 and b < 100 for a, b in case.planted) and any(a >= n - 100 and b >= n - 100 for a, b in case.planted)
    if n > E.LINE:
        assert {(True, True), (True, False)} <= set(sides) and ((False, False) in sides) == (n >= E.LINE + 8)
        assert (E.LINE - 1, E.LINE) in case.planted
        # the shared neighbourhoods lie on both sides of the line too
        a, b = E.LINE - 1, E.LINE
        common = np.intersect1d(p.col[p.rowptr[a]:p.rowptr[a + 1]], p.col[p.rowptr[b]:p.rowptr[b + 1]])
        assert common.min() < E.LINE <= common.max()
    else:
        assert all(s == (True, True) for s in sides)
