"""Child process of tests/test_gpu_leg2_short.py, started with SIMRANK_POOL_POISON=1 (every block the library hands out is
NaN until written): five updates of engine.Plan per (graph, plan options) with tuning leg2_short = 0, 8 and 16, once with
the exact count and once with count_any (one case: 18 updates with eps = 1e-4).

    python tests/leg2_short_worker.py ROOT

Asserts nothing: prints one JSON object, case name -> what was seen (bit equality of result() across the three settings,
the counts of every update, the error against the float64 oracle, "leg2_short_groups" of the plan and the same number
recomputed from the rule in NumPy); the tests assert on it."""
import json
import sys

import numpy as np

sys.path.insert(0, sys.argv[1])
from oracle import simrank_oracle as O  # noqa: E402
from simrank_amd import ingest, synth  # noqa: E402
from simrank_amd.engine import HipOps, Plan  # noqa: E402
from simrank_amd.ingest import CSR  # noqa: E402

UPDATES = 5
CONVERGE_UPDATES = 18
WIDTHS = (0, 8, 16)
# the two-launch leg 2 on the plain pattern (the one-launch leg 2 and the dense-block part are other kernels), the stable
# length order (the rule below needs the sorted lengths only)
BASE = dict(fuse=1, fuse_sym=0, dense_sym=0, ids16=1, restrict_support=0, leg1_skip=1, leg1_order=0, balance=2)


def from_frame(df):
    return ingest.directed(df, False, "from", "to", "weight")[1]


def from_lengths(lengths, seed):
    """Rows of exactly these lengths, columns drawn without repetition; the plan keeps the order (reorder = False)."""
    n = len(lengths)
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32) for k in lengths]
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(lengths)
    col = np.concatenate(rows + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    deg = np.asarray(lengths, dtype=np.float64)
    return CSR(n, n, rowptr, col, np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0))


def boundary_graph():
    """Groups of four 32-row tiles (one workgroup each) at the edges of both widths, then a ragged last tile:
    0: rows of 0..8 entries, one tile wholly empty            short at 8 and at 16
    1: three tiles of <= 8, one tile with rows of exactly 9   general path at 8, short at 16
    2: rows of exactly 16 and fewer                           short at 16 only
    3: three tiles of <= 8, one tile with a row of 17         never short
    4: rows of exactly 8                                      short at both
    5: 20 rows of <= 8 (the ragged last tile)                 short at both"""
    rng = np.random.default_rng(21)
    g0 = np.concatenate([rng.integers(0, 9, 32), np.full(32, 8), np.zeros(32, int), rng.integers(0, 9, 32)])
    # (no 32-row block above 256 entries: build_tiles would cut it, and a cut tile is never short)
    g1 = np.concatenate([rng.integers(0, 9, 64), np.full(16, 9), rng.integers(1, 9, 48)])
    g2 = np.concatenate([np.full(8, 16), rng.integers(0, 9, 24), rng.integers(0, 9, 96)])
    g2[40] = 16
    t17 = rng.integers(0, 9, 32)
    t17[5] = 17
    g3 = np.concatenate([rng.integers(0, 9, 32), t17, rng.integers(0, 9, 64)])
    g4 = np.full(128, 8)
    g5 = rng.integers(0, 9, 20)
    return from_lengths(np.concatenate([g0, g1, g2, g3, g4, g5]).astype(int).tolist(), 22)


def heavy_row_graph():
    """One row of 400 entries among rows of <= 8: its 32-row block is cut into pieces (tuning balance), which shifts the
    groups of four tiles behind it off the 128-row grid; the groups of cut tiles take the general path, their neighbours
    the short one."""
    rng = np.random.default_rng(23)
    lengths = rng.integers(0, 9, 700)
    lengths[200] = 400
    return from_lengths(lengths.astype(int).tolist(), 24)


def tiles_of(rowptr, n, balance=2):
    """api.hip build_tiles: 32-row blocks, those heavier than balance x the mean cut into halves."""
    nnz = int(rowptr[-1])
    if nnz <= 0:
        return []
    nblk = (n + 31) // 32
    limit = max(balance * ((nnz + nblk - 1) // nblk), 256)
    out = []
    for b in range(nblk):
        stack = [(b * 32, min(n, b * 32 + 32))]
        while stack:
            lo, hi = stack.pop()
            if rowptr[hi] - rowptr[lo] <= limit or hi - lo <= 1:
                out.append(lo)
            else:
                mid = lo + (hi - lo + 1) // 2
                stack.append((mid, hi))
                stack.append((lo, mid))
    out.append(n)
    return out


def short_groups(lengths, width):
    """The rule: a group of four consecutive tiles is short when each tile is a whole 32-row block (or the ragged last one)
    and no row of it has more than `width` entries."""
    n = len(lengths)
    if width == 0 or n < 64:
        return 0
    rowptr = np.concatenate([[0], np.cumsum(lengths)])
    t = tiles_of(rowptr, n)
    n_tiles = len(t) - 1
    count = 0
    for k in range((n_tiles + 3) // 4):
        ok = True
        for i in range(4 * k, min(4 * k + 4, n_tiles)):
            lo, hi = t[i], t[i + 1]
            ok = ok and lo % 32 == 0 and hi == min(n, lo + 32) and (hi == lo or max(lengths[lo:hi]) <= width)
        count += int(ok)
    return count


def oracle(csr, scale, evidence, apriori, lbd, coef, updates=UPDATES):
    W = csr.dense(scale.astype(np.float32).astype(np.float64))
    E = O.evidence(csr.dense(np.ones(csr.n_rows))) if evidence else None
    S = np.eye(csr.n_rows)
    for _ in range(updates):
        S = O.update(W, S, coef, E, None if apriori is None else apriori.astype(np.float64), lbd)
    return S


def run_plan(ops, csr, scale, width, tuning, exact, updates=UPDATES, eps=0.0, **kw):
    ops.set_tuning(**{**BASE, **tuning, "leg2_short": width})
    p = Plan(ops, csr, scale, **kw)
    counts = [p.step(eps, exact_count=exact) for _ in range(updates)]
    groups = p.get("leg2_short_groups")
    got = p.result()
    p.free()
    return got, counts, groups


def case(ops, out, name, csr, tuning, want=None, rtol=1e-5, updates=UPDATES, eps=0.0, **kw):
    scale = kw.pop("rowscale", csr.rowscale)
    lengths = np.diff(csr.rowptr).astype(np.int64)
    if kw.get("reorder", True):
        lengths = np.sort(lengths, kind="stable")
    runs = {(w, exact): run_plan(ops, csr, scale, w, tuning, exact, updates, eps, **kw) for w in WIDTHS for exact in (True, False)}
    ref, ref_counts, _ = runs[(0, True)]
    rec = {
        "finite": bool(all(np.isfinite(r[0]).all() for r in runs.values())),
        "bit_equal": bool(all(np.array_equal(r[0], ref) for r in runs.values())),
        "counts_exact": {str(w): runs[(w, True)][1] for w in WIDTHS},
        # (count_any: a count that stops at the first difference a wave sees; its VALUE depends on the order the waves ran
        # in, what it says is "zero or not")
        "counts_any_nonzero": {str(w): [c != 0 for c in runs[(w, False)][1]] for w in WIDTHS},
        "groups": {str(w): [runs[(w, True)][2], runs[(w, False)][2]] for w in WIDTHS},
        "rule": {str(w): short_groups(lengths.tolist(), w) for w in WIDTHS},
    }
    n_tiles = len(tiles_of(np.concatenate([[0], np.cumsum(lengths)]), len(lengths))) - 1
    rec["tiles"], rec["blocks"], rec["tile_groups"] = n_tiles, (len(lengths) + 31) // 32, (n_tiles + 3) // 4
    if want is not None:
        rec["within_parity"] = bool(all(np.allclose(r[0], want, rtol=rtol, atol=1e-30) for r in runs.values()))
        rec["max_rel_err"] = float(np.max(np.abs(ref - want) / np.maximum(np.abs(want), 1e-300)))
    out[name] = rec


def main():
    ops = HipOps(0)
    out = {}
    graphs = {
        "pl520": (from_frame(synth.powerlaw_directed(520, 6, seed=1)), {}),
        "pl1031": (from_frame(synth.powerlaw_directed(1031, 6, seed=2)), {}),
        "pl2100": (from_frame(synth.powerlaw_directed(2100, 6, seed=3)), {}),
        "er500": (from_frame(synth.er_directed(500, 0.012, seed=5)), {}),
        "boundary": (boundary_graph(), dict(reorder=False)),
        "heavy_row": (heavy_row_graph(), dict(reorder=False)),
    }
    for gname, (csr, kw) in graphs.items():
        case(ops, out, f"{gname}/plain", csr, {}, oracle(csr, csr.rowscale, False, None, None, 0.8), coef=0.8, **kw)
    # to convergence with the fit's eps: the counts fall from nearly everything to a handful to zero, so a wrong row of the
    # early previous-iterate loads (a stale or a neighbouring row compared) shows in them
    csr = graphs["pl520"][0]
    case(ops, out, "pl520/to_convergence", csr, {}, oracle(csr, csr.rowscale, False, None, None, 0.8, CONVERGE_UPDATES),
         updates=CONVERGE_UPDATES, eps=1e-4, coef=0.8)
    # SimRank++ (evidence; leg 2 restricted to its support and not), priors, 32-bit ids, fp16-held matrices: one graph
    csr = graphs["pl1031"][0]
    n = csr.n_rows
    spread = ingest.spread(csr) * csr.rowscale
    rng = np.random.default_rng(7)
    sym = rng.random((n, n)).astype(np.float32)             # (the plan holds a prior in f32: the oracle gets the same values)
    sym = ((sym + sym.T) / 2).astype(np.float32)
    asym = rng.random((n, n)).astype(np.float32)
    want_pp = oracle(csr, spread, True, None, None, 0.8)
    case(ops, out, "pp/unrestricted", csr, dict(restrict_support=0), want_pp, rowscale=spread, evidence=True)
    case(ops, out, "pp/restricted", csr, dict(restrict_support=1), want_pp, rowscale=spread, evidence=True)
    case(ops, out, "prior/symmetric", csr, {}, oracle(csr, spread, True, sym, 0.3, 0.8), rowscale=spread, evidence=True,
         apriori=sym, lbd=0.3)
    case(ops, out, "prior/asymmetric", csr, {}, oracle(csr, spread, True, asym, 0.3, 0.8), rowscale=spread, evidence=True,
         apriori=asym, lbd=0.3)
    case(ops, out, "ids32", csr, dict(ids16=0), oracle(csr, csr.rowscale, False, None, None, 0.8), coef=0.8)
    case(ops, out, "fp16", csr, {}, None, coef=0.8, storage="fp16")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
