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
from tests.leg2_rule import boundary_lengths, from_lengths, heavy_row_lengths, short_groups, tiles_of  # noqa: E402

UPDATES = 5
CONVERGE_UPDATES = 18
WIDTHS = (0, 8, 16)
# the two-launch leg 2 on the plain pattern (the one-launch leg 2 and the dense-block part are other kernels), the stable
# length order (the rule below needs the sorted lengths only)
BASE = dict(fuse=1, fuse_sym=0, dense_sym=0, ids16=1, restrict_support=0, leg1_skip=1, leg1_order=0, balance=2)


def from_frame(df):
    return ingest.directed(df, False, "from", "to", "weight")[1]


def boundary_graph():
    """tests/leg2_rule.py boundary_lengths: groups at the edges of both widths, a ragged last tile of 20 rows."""
    return from_lengths(boundary_lengths(), 22)


def heavy_row_graph():
    """tests/leg2_rule.py heavy_row_lengths: one row of 400 entries among rows of <= 8."""
    return from_lengths(heavy_row_lengths(), 24)


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
