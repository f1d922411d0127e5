"""The evidence counts restated in NumPy / SciPy, the hub rule of simrank_graph_create restated beside them, and the
patterns of tests/test_evidence_cpu.py and tests/test_gpu_evidence_edges.py.  Nothing of the product is imported:
whatever a test expects of a count byte or of "ev_hubs" comes from here, never from the library.

counts(a, b) = min(|{i : P[a, i] = P[b, i] = 1}|, 255), P the 0/1 pattern of the rows whose float32 scale is positive
(`_cal_Evidence`, SimRank.py:311-320: `Graph.dot(Graph.T)` on `G > 0`).  Integer arithmetic, one right answer."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

# the fields of simrank_amd.ingest.CSR that graph creation reads
Pattern = namedtuple("Pattern", "n_rows n_cols rowptr col rowscale")

LINE = 65536           # columns of one pass of the counting kernel: 16-bit LDS counters, two per word
MAX_HUBS = 4096        # the hub list is cut here ...
MIN_HUBS = 8           # ... and dropped below this many candidates
MIN_REFS = 48          # a hub column has at least this many live references
GUARD = 0xA5           # what the GPU tests pre-fill outputs with


def from_rows(rows, n_cols, rowscale):
    """A pattern from explicit row lists (each: distinct column ids, any order)."""
    rows = [np.unique(np.asarray(r, dtype=np.int64)) for r in rows]
    for r in rows:
        assert r.size == 0 or (r[0] >= 0 and r[-1] < n_cols)
    rowptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    col = (np.concatenate(rows) if rowptr[-1] else np.empty(0)).astype(np.int32)
    rowscale = np.asarray(rowscale, dtype=np.float64)
    assert rowscale.shape == (len(rows),)
    return Pattern(len(rows), int(n_cols), rowptr, col, rowscale)


def live_pattern(p):
    """P: 0/1, int64, the rows without positive float32 scale emptied."""
    live = p.rowscale.astype(np.float32) > 0
    deg = np.diff(p.rowptr)
    keep = np.repeat(live, deg)
    rows = np.repeat(np.arange(p.n_rows), deg)[keep]
    return sp.csr_matrix((np.ones(rows.size, dtype=np.int64), (rows, p.col[keep])), shape=(p.n_rows, p.n_cols))


def raw_counts(p):
    """P P^T before clipping, sparse int64."""
    P = live_pattern(p)
    R = (P @ P.T).tocsr()
    R.sort_indices()
    return R


def counts(p):
    """min(P P^T, 255), sparse (never a dense n x n array of 8-byte elements)."""
    R = raw_counts(p)
    R.data = np.minimum(R.data, 255)
    return R


def band(R, r0, r1, c0, c1):
    """Rows [r0, r1) x columns [c0, c1) of the counts as a dense uint8 array."""
    return R[r0:r1][:, c0:c1].astype(np.uint8).toarray()


def live_refs(p):
    """Per column: how many live rows hold it."""
    return np.asarray(live_pattern(p).sum(axis=0)).ravel()


def hubs(p, ev_hub):
    """The hub columns simrank_graph_create chooses under tuning ev_hub (thousandths of the row count; 0: none), in its
    order: columns with at least max(48, ceil(n_rows ev_hub / 1000)) live references, most referenced first and the
    lower id first among equals, at most 4096 of them, none at all below 8."""
    if ev_hub <= 0 or p.col.size == 0:
        return np.empty(0, dtype=np.int64)
    thr = max(MIN_REFS, -(-p.n_rows * int(ev_hub) // 1000))
    refs = live_refs(p)
    cand = np.flatnonzero(refs >= thr)
    cand = cand[np.lexsort((cand, -refs[cand]))][:MAX_HUBS]
    return cand if cand.size >= MIN_HUBS else np.empty(0, dtype=np.int64)


def walk_cost(p):
    """sum over columns of (live references)^2: the 2-hop paths the LDS-counter walk takes without a hub part."""
    d = live_refs(p).astype(np.int64)
    return int((d * d).sum())


# ---------------------------------------------------------------------------------------------------------------------
# patterns
# ---------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "pattern ev_hub planted")     # planted: {(row a, row b): common neighbours before clipping}

CAP_K = 65600
CAP_ROWS = 48


def cap_case(hub_rows=0):
    """Counter cap.  48 rows over 65 600 columns: rows 0, 1, 2 hold all of [0, 65536) — every pair of them and each of
    their diagonals has exactly 65 536 common neighbours, where an uncapped 16-bit counter wraps to 0 and carries into
    its neighbour — then one row each on [0, 65535), [0, 16384), [0, 16383), [0, 255), [0, 254), one holding column
    65 599 alone, one WITHOUT weight holding every column, and 38 short random rows.  47 live rows: no column reaches
    48 references, no hub part under any ev_hub.
    hub_rows = 64: that many live rows more, each holding [0, 5000) — 5000 columns with at least 48 references, of which
    4096 become hubs and 904 stay in the walk; the hub product of rows 0 and 1 is 4096 (stored as 255) when the walk
    starts and the walk adds 61 440 to it."""
    rng = np.random.default_rng(48)
    K = CAP_K
    rows = [np.arange(LINE)] * 3 + [np.arange(LINE - 1), np.arange(16384), np.arange(16383), np.arange(255),
                                    np.arange(254), np.array([K - 1]), np.arange(K)]
    rows += [rng.choice(K, size=int(rng.integers(3, 25)), replace=False) for _ in range(CAP_ROWS - len(rows))]
    scale = 0.1 + rng.random(CAP_ROWS)
    scale[9] = 0.0
    planted = {(0, 0): LINE, (0, 1): LINE, (0, 2): LINE, (1, 2): LINE, (2, 2): LINE, (0, 3): LINE - 1, (3, 3): LINE - 1,
               (0, 4): 16384, (0, 5): 16383, (4, 5): 16383, (0, 6): 255, (0, 7): 254, (6, 7): 254, (0, 8): 0, (8, 8): 1,
               (0, 9): 0, (9, 9): 0}
    if hub_rows:
        rows += [np.arange(5000)] * hub_rows
        scale = np.concatenate([scale, 0.1 + rng.random(hub_rows)])
        planted.update({(0, CAP_ROWS): 5000, (CAP_ROWS, CAP_ROWS + 1): 5000, (6, CAP_ROWS): 255, (7, CAP_ROWS): 254})
    return Case(from_rows(rows, K, scale), 1, planted)


def few_hubs_case(n_planted):
    """600 rows over 900 columns, about 2 references per column, and n_planted columns (the last ones) that 60 rows hold
    each: 7 of them are no hub part at all, 8 are one of 8 columns in an image of 32."""
    rng = np.random.default_rng(600 + n_planted)
    M, K = 600, 900
    rows = [rng.choice(K - 16, size=int(rng.poisson(3)), replace=False) for _ in range(M)]
    for h in range(n_planted):
        for a in rng.choice(M, size=60, replace=False):
            rows[a] = np.append(rows[a], K - 1 - h)
    scale = 0.1 + rng.random(M)
    scale[rng.random(M) < 0.05] = 0.0
    scale[:4] = 1.0
    return Case(from_rows(rows, K, scale), 14, {})


def wide_case():
    """Wide operand, small output: 300 rows over 70 000 columns (the bipartite shape) — the transposed pattern has ids
    above 65 535 — with 16 hub columns above 65 536 that half of the rows hold each."""
    rng = np.random.default_rng(300)
    M, K = 300, 70000
    hub_cols = LINE + 1000 + 200 * np.arange(16)
    rows = []
    for a in range(M):
        rest = rng.choice(K, size=int(rng.poisson(30)), replace=False)
        rows.append(np.concatenate([rest, hub_cols[rng.random(16) < 0.5]]))
    rows[0] = np.concatenate([np.arange(LINE - 150, LINE + 150), hub_cols])     # rows 0 and 1: 300 common neighbours across the line
    rows[1] = np.concatenate([np.arange(LINE - 150, LINE + 150), hub_cols[:8]])
    scale = 0.1 + rng.random(M)
    scale[rng.random(M) < 0.05] = 0.0
    scale[:2] = 1.0
    return Case(from_rows(rows, K, scale), 14, {(0, 1): 308, (0, 0): 316})


def big_case(n):
    """n x n, mean degree about 3, 5 % of the rows without weight; 40 planted columns that about 300 rows drawn from
    all of [0, n) hold each (hubs at ev_hub = 1, threshold ceil(n / 1000)); two rows among the first 100 ids and two among
    the last 100 that share 300 neighbours, and — where n lies beyond 65 536 — a pair across that line, one below it and (where more than a few ids lie beyond it) one
    above it.  The shared neighbourhoods lie on both sides of the line as well."""
    rng = np.random.default_rng(n)
    deg = rng.poisson(3, size=n)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    col = rng.integers(0, n, size=int(rowptr[-1]))
    rows = [col[rowptr[a]:rowptr[a + 1]] for a in range(n)]
    hub_cols = rng.choice(n, size=40, replace=False)
    hub_cols[0], hub_cols[1] = 0, n - 1
    hub_cols = np.unique(hub_cols)
    for h in hub_cols:
        for a in rng.choice(n, size=300, replace=False):
            rows[a] = np.append(rows[a], h)
    scale = 0.1 + rng.random(n)
    scale[rng.random(n) < 0.05] = 0.0
    pairs = [(3, 97), (n - 90, n - 5)]
    if n > LINE:
        pairs += [(LINE - 1, LINE), (LINE - 40, LINE - 3)] + ([(LINE + 1, n - 2)] if n >= LINE + 8 else [])
    free = np.setdiff1d(np.arange(n), hub_cols)
    planted = {}
    for k, (a, b) in enumerate(pairs):
        lo = free[free < min(n, LINE) - 1000]
        shared = np.concatenate([rng.choice(lo, size=150, replace=False), free[-750:][k::5]])
        rows[a] = shared if k % 2 else np.append(shared, hub_cols[-3:])
        rows[b] = np.append(shared, hub_cols[-5:])
        scale[a] = scale[b] = 1.0
        planted[(a, b)] = 300 if k % 2 else 303
    return Case(from_rows(rows, n, scale), 1, planted)
