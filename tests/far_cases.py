"""The inputs of tests/test_gpu_far_exemplars.py and tests/test_gpu_far_candidates.py on the 70 x 1100 far block, and the
expected outputs as a function of the logical matrix alone, so that tests/test_far_cpu.py can evaluate the very same
calls on ``narrowed(g, A, bits)``: the matrix a kernel would see whose element offsets were cut to 32 bits.  If those
outputs equalled the ones on ``A``, the GPU tests could not tell a narrowed address from a right one.

Rows, lists, covers and ``k`` depend on the block and on a counter ``i`` (the place of (geometry, kind) in
``far_blocks``' order), never on the stride.  Nothing here touches a device; the references are those of
tests/exemplars_ref.py and tests/candidates_ref.py."""
import numpy as np

from tests import blocks as B
from tests import candidates_ref as CR
from tests import exemplars_ref as ER
from tests import far as F

KINDS = ("dyadic", "wide")
# simrank_candidates_staged per layout (the GPU test asserts that the library says the same)
STAGED = {B.PANEL_F32: 16384, B.ROWMAJOR_F32: 16384, B.PANEL_F16: 16384, B.ROWMAJOR_F64: 8192}
STAGED_KS = (1, 10, F.N_COLS)
LONG_KS = (3, 4096)
N_Q = 10


def counter(g, kind):
    """The place of (geometry, kind) in the order ``far_blocks`` yields them for the layout."""
    tags = [x.tag for x in F.geometries(g.layout)]
    return tags.index(g.tag) * len(KINDS) + KINDS.index(kind)


def widened_filler(layout):
    return float(B.widen(layout, F.filler(layout))[0])


def narrowed(g, A, bits):
    """``A`` as a kernel reads it that keeps ``bits`` = "int32" (sign-wrapped) or "uint32" of every element offset of
    geometry ``g``: an element whose offset changes holds the widened filler -> (the matrix, how many elements moved)."""
    off = F.live_offsets(g, *A.shape)
    kept = off.astype(np.int32).astype(np.int64) if bits == "int32" else off & ((1 << 32) - 1)
    moved = kept != off
    return np.where(moved, widened_filler(g.layout), A), int(moved.sum())


# ---- exemplars -------------------------------------------------------------------------------------------------------------
def exemplar_inputs(blk, i):
    """-> dict: ``gain_rows`` [None, a shuffled list of every edge row with one twice, n_rows, -1 and 2^31 - 1];
    ``covers`` name -> cover (zeros, the positive elements of a far row, mixed), each below the widened filler in every
    column; ``cover_runs`` [(rows, start name, first counters)]: lists of 1, 2 and 7 rows drawn from the edge rows, the
    last row among them, and a row outside; the starts are zeros and mixed, the counters start non-zero."""
    A, n_rows, n_cols = blk.A, F.N_ROWS, F.N_COLS
    rng = np.random.default_rng([blk.layout, i, 61])
    listed = np.array(list(F.EDGE_ROWS) + [F.EDGE_ROWS[4], n_rows, -1, 2 ** 31 - 1], dtype=np.int64)
    rng.shuffle(listed)
    r0 = F.EDGE_ROWS[4 + i % 2]                                             # row 64 or the last row
    pick = np.abs(A[rng.integers(0, n_rows, size=n_cols), np.arange(n_cols)])
    covers = {"zeros": np.zeros(n_cols), "a row": np.where(A[r0] > 0, A[r0], 0.0),
              "mixed": np.where(rng.random(n_cols) < 0.5, 0.0, pick)}
    fill = widened_filler(blk.layout)
    for c in covers.values():
        assert (c >= 0).all() and (c < fill).all()                          # a misread element rises above every cover
    runs = []
    for j, m in enumerate((1, 2, 7)):
        rows = rng.choice(F.EDGE_ROWS, size=m).astype(np.int64)
        rows[m // 2] = F.EDGE_ROWS[(4, 5, 4)[j]]                            # a row that every narrowing moves
        rows = np.insert(rows, int(rng.integers(m + 1)), (n_rows, -1, 2 ** 31 - 1)[j])
        runs.append((rows, ("mixed", "zeros", "mixed")[(i + j) % 3], rng.integers(1, 1000, size=rows.size)))
    return {"gain_rows": [None, listed], "covers": covers, "cover_runs": runs, "r0": r0}


def exemplar_outputs(A, inp):
    """(gains: (cover name, rows is None) -> float64 in the header's order, covers: [(cover, counters)] per cover run)."""
    gains = {(name, rows is None): ER.block_gains(A, rows, c) for name, c in inp["covers"].items() for rows in inp["gain_rows"]}
    return gains, [ER.block_cover(A, rows, inp["covers"][start], first) for rows, start, first in inp["cover_runs"]]


# ---- candidates ------------------------------------------------------------------------------------------------------------
def candidate_inputs(blk, i):
    """-> dict: ``row_pos`` (``edge_rows``), ``col_ids`` (a permutation-like map) and ``runs``: [(name, cand_pos,
    cand_ids or None, row_ids, k)].  Staged: every column in ascending-id order ("all": what simrank_neighbors_select
    answers) and the edge columns plus 40 random ones with -1 and n_cols inside the list ("edges").  Not staged
    ("long"): ``STAGED + 1`` entries, every column once and then columns drawn with repeats, the edge columns among
    them, with distinct ids and without.  ``row_ids`` name one listed candidate per row."""
    from tests.test_gpu_far_blocks import edge_rows                          # (importing it needs no device)
    layout, n_cols = blk.layout, F.N_COLS
    rng = np.random.default_rng([layout, i, 67])
    row_pos = edge_rows(rng, N_Q)
    col_ids = (rng.permutation(n_cols + 7)[:n_cols] * 3 + 1).astype(np.int32)
    own = (row_pos.astype(np.int64) * 5 + 1) % n_cols                       # a column per row
    runs = []
    by_id = np.argsort(col_ids, kind="stable")
    some = np.concatenate([F.EDGE_COLS, rng.permutation(np.setdiff1d(np.arange(n_cols), F.EDGE_COLS))[:40]])
    rng.shuffle(some)
    edges = np.concatenate([some[:9], [-1], some[9:30], [n_cols], some[30:]]).astype(np.int64)
    edge_ids = np.where((edges >= 0) & (edges < n_cols), col_ids[np.clip(edges, 0, n_cols - 1)], 3 * (n_cols + 9) + 2 + edges)
    own_edge = some[(row_pos.astype(np.int64) * 5 + 1) % some.size]         # a listed column per row
    for k in STAGED_KS:
        runs.append(("all", by_id, col_ids[by_id], col_ids[own], k))
        runs.append(("all", np.arange(n_cols), None, own, k))
        runs.append(("edges", edges, edge_ids, col_ids[own_edge], k))
        runs.append(("edges", edges, None, own_edge, k))
    m = STAGED[layout] + 1
    repeats = rng.integers(0, n_cols, size=m - n_cols)
    repeats[rng.permutation(repeats.size)[:len(F.EDGE_COLS)]] = F.EDGE_COLS
    long = np.concatenate([rng.permutation(n_cols), repeats]).astype(np.int64)
    long_ids = (rng.permutation(m + 11)[:m] * 2 + 1).astype(np.int32)       # distinct: a candidate is a list index
    own_long = (row_pos.astype(np.int64) * 977 + 13) % m                    # a list index per row
    for k in LONG_KS:
        runs.append(("long", long, long_ids, long_ids[own_long], k))
        runs.append(("long", long, None, long[own_long], k))
    return {"row_pos": row_pos, "col_ids": col_ids, "runs": runs}


def candidate_outputs(A, inp):
    """[(ids, values)] per run: ``candidates_ref.ref_topk``."""
    return [CR.ref_topk(A, inp["row_pos"], row_ids, pos, ids, k) for _, pos, ids, row_ids, k in inp["runs"]]


def ties_at_k(A, inp, run):
    """How many rows of the run have equal values at ranks k and k + 1 of the full order."""
    _, pos, ids, row_ids, k = run
    idx, val = CR.ref_topk(A, inp["row_pos"], row_ids, pos, ids, k + 1)
    return int(((idx[:, k] >= 0) & (val[:, k - 1] == val[:, k])).sum())
