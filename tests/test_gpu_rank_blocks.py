"""libsimrank_rank.so at its C interface, on bands the test writes itself: values drawn from a handful (+0.0, -0.0, a
subnormal, +-1, +inf, NaN, -inf), so that most comparisons are ties and the id decides; a leading dimension larger than
the row with +inf in the padding and in a guard row (a kernel that read them would count them before everything); ids
that are the columns and ids that are a non-monotone permutation; target lists that are empty, single, repeated, one
more than the local-memory tile, every column, and one whose column is in another block.  Every counter is pre-filled:
the library ADDS.  Everything is compared for equality with the NumPy statement (tests/rank_ref.py)."""
import numpy as np
import pytest

from simrank_amd import _rank
from simrank_amd.engine import HipOps
from tests import rank_ref as K

pytestmark = pytest.mark.gpu

VALUES = np.array([0.0, -0.0, 5e-324, 1.0, -1.0, np.inf, np.nan, -np.inf])
ORDERED = VALUES[:6]                              # neither NaN nor -inf: every column is a candidate
ELSEWHERE_SCORE, ELSEWHERE_ID = 0.0, 5            # the target whose column is in another block: its score is given


class Dev:
    """Device memory of one test through HipOps: freed together at the end."""

    def __init__(self):
        self.ops, self.held = HipOps(0), []

    def put(self, host):
        host = np.ascontiguousarray(host)
        ptr = self.ops._malloc(host.nbytes + 16)
        self.held.append(ptr)
        if host.nbytes:
            self.ops.h2d(ptr, host)
        return ptr

    def get(self, ptr, like):
        out = np.empty_like(like)
        self.ops.d2h(out, ptr)
        self.ops.synchronize()
        return out

    def release(self):
        self.ops.synchronize()
        for p in self.held:
            self.ops._free(p)
        self.held = []

    def close(self):
        self.release()
        self.ops.close()


@pytest.fixture(scope="module")
def device():
    d = Dev()
    yield d
    d.close()


@pytest.fixture
def dev(device):
    yield device
    device.release()


def target_lists(rng, n_out):
    """Columns per basket, -1 = a column of another block: none, one, the same one twice, one more than the tile, every
    column (twice: a general row, and a row without NaN and -inf), and a list with a column elsewhere in its middle."""
    one = int(rng.integers(0, n_out))
    return [[], [one], [one, one], rng.integers(0, n_out, size=_rank.TILE + 1).tolist(), list(range(n_out)),
            [int(rng.integers(0, n_out)), -1, int(rng.integers(0, n_out))], list(range(n_out))]


def permuted_ids(rng, n):
    """Distinct ids that are no column numbers, in an order that neither ascends nor descends (three columns and up)."""
    ids = (rng.permutation(n + 7)[:n] * 3 + 1).astype(np.int32)
    if n >= 3:
        ids[:3] = np.sort(ids[:3])[[0, 2, 1]]
    return ids


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n_out", [1, 3, 4, 1023, 1024, 1025, 1100])
def test_gather_and_count_are_the_statement(dev, n_out):
    lib, st = _rank.load(), dev.ops.stream
    rng = np.random.default_rng(n_out)
    lists = target_lists(rng, n_out)
    n_sets = len(lists)
    assert (_rank.TILE + 1) % _rank.TILE and len(lists[3]) == _rank.TILE + 1
    tptr = np.zeros(n_sets + 1, dtype=np.int64)
    np.cumsum([len(l) for l in lists], out=tptr[1:])
    tcol = np.concatenate([np.asarray(l, dtype=np.int32) for l in lists])
    n_t = int(tcol.size)
    for pad in (3, 4):                            # (one of the two leading dimensions is even: rows on 16 bytes)
        ld = n_out + pad
        band = np.full((n_sets + 1, ld), np.inf)
        band[:n_sets, :n_out] = rng.choice(VALUES, size=(n_sets, n_out))
        band[6, :n_out] = rng.choice(ORDERED, size=n_out)
        band_dev = dev.put(band)
        for ids in (None, permuted_ids(rng, n_out)):
            what = (n_out, pad, ids is None)
            col_id = np.arange(n_out, dtype=np.int32) if ids is None else ids
            assert ids is None or n_out < 3 or (np.diff(ids) < 0).any() and (np.diff(ids) > 0).any()
            tid = np.where(tcol >= 0, col_id[np.maximum(tcol, 0)], ELSEWHERE_ID).astype(np.int32)
            # gather: the targets of this block get the band's value, the one elsewhere keeps what it had
            score0 = np.where(tcol >= 0, 123.0, ELSEWHERE_SCORE)
            basket = np.repeat(np.arange(n_sets), np.diff(tptr))
            want_score = np.where(tcol >= 0, band[basket, np.maximum(tcol, 0)], score0)
            tptr_dev, tcol_dev, tid_dev, score_dev = dev.put(tptr), dev.put(tcol), dev.put(tid), dev.put(score0)
            _rank.check(lib.simrank_rank_gather(band_dev, ld, n_sets, n_out, tptr_dev, tcol_dev, score_dev, st), "gather")
            score = dev.get(score_dev, score0)
            assert np.array_equal(bits(score), bits(want_score)), what
            # count: ADDED to what the counters held; a basket without targets adds nothing, to its candidates either
            before0 = 1000 + np.arange(n_t, dtype=np.int64)
            cand0 = 77 + np.arange(n_sets + 1, dtype=np.int64)
            want_before, want_cand = before0.copy(), cand0.copy()
            for q in range(n_sets):
                for x in range(tptr[q], tptr[q + 1]):
                    b, c = K.count(band[q, :n_out], col_id, want_score[x], tid[x])
                    want_before[x] += b
                if tptr[q + 1] > tptr[q]:
                    want_cand[q] += c
            before_dev, cand_dev = dev.put(before0), dev.put(cand0)
            _rank.check(lib.simrank_rank_count(band_dev, ld, n_sets, n_out, None if ids is None else dev.put(ids),
                                               tptr_dev, score_dev, tid_dev, before_dev, cand_dev, st), "count")
            before, cand = dev.get(before_dev, before0), dev.get(cand_dev, cand0)
            assert np.array_equal(before, want_before), (what, np.flatnonzero(before != want_before)[:5])
            assert np.array_equal(cand, want_cand), what
            assert cand[0] == cand0[0] and cand[n_sets] == cand0[n_sets]
            # every column a target and every column a candidate: the ranks are a permutation of 1 .. n_out
            ranks = _rank.ranks_of(score[tptr[6]:tptr[7]], before[tptr[6]:tptr[7]] - before0[tptr[6]:tptr[7]])
            assert sorted(ranks.tolist()) == list(range(1, n_out + 1)), what
            # the general row: NaN and -inf targets are no candidates, the others' ranks are 1 .. candidates
            sl = slice(tptr[4], tptr[5])
            ranks = _rank.ranks_of(score[sl], before[sl] - before0[sl])
            n_cand = int(cand[4] - cand0[4])
            assert n_cand == int((band[4, :n_out] > -np.inf).sum())
            assert sorted(ranks[ranks > 0].tolist()) == list(range(1, n_cand + 1)) and (ranks == 0).sum() == n_out - n_cand
            # a band of the baskets 3 and 4 alone, as a caller that cuts its baskets passes them: the same counts again
            _rank.check(lib.simrank_rank_count(band_dev + 8 * 3 * ld, ld, 2, n_out, None if ids is None else dev.put(ids),
                                               tptr_dev + 8 * 3, score_dev, tid_dev, before_dev, cand_dev + 8 * 3, st), "count")
            twice = dev.get(before_dev, before0)
            sl = slice(tptr[3], tptr[5])
            assert np.array_equal(twice[sl] - before[sl], before[sl] - before0[sl]), what
            rest = np.ones(n_t, dtype=bool)
            rest[sl] = False
            assert np.array_equal(twice[rest], before[rest]), what
            assert np.array_equal(dev.get(cand_dev, cand0) - cand, np.where(np.isin(np.arange(n_sets + 1), (3, 4)), cand - cand0, 0))
