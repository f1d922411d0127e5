"""Child process of tests/test_gpu_leg1_skip.py, started with SIMRANK_POOL_POISON=1 (every block the library hands out is
NaN until written): five updates of engine.Plan per (graph, tuning, plan options) with tuning leg1_skip = 1 and = 0.

    python tests/leg1_skip_worker.py ROOT [big]

Asserts nothing: prints one JSON object, case name -> what was seen (bit equality of result() and of every step's count
between the two settings, the error against the float64 oracle, the skipped-unit counts, the dead-block count of the
node order recomputed in NumPy); the tests assert on it.  ``big``: the one graph large enough for GROUPED units to
survive (build_fused_plan keeps a group only where a panel still gets 64 units), bit equality of sampled rows only."""
import json
import sys

import numpy as np

sys.path.insert(0, sys.argv[1])
from oracle import simrank_oracle as O  # noqa: E402
from simrank_amd import ingest, synth  # noqa: E402
from simrank_amd.engine import HipOps, Plan  # noqa: E402
from simrank_amd.ingest import CSR  # noqa: E402

UPDATES = 5
BASE = dict(fuse=1, fuse_min=2, fuse_steps=1, fuse_unit=48, fuse_group=3, fuse_rows=8192, fuse_order=0, fuse_sym=-1, ids16=1,
            restrict_support=-1, leg1_skip=1, leg1_order=1)       # (leg1_order: the refined node order at these small sizes too)
VARIANTS = {
    "default": {},
    "split": dict(fuse_min=3, fuse_steps=2, fuse_unit=4, fuse_rows=400),
    "grouped": dict(fuse_group=4),
    "no_set": dict(fuse_steps=1 << 20),
    "ids32": dict(ids16=0),
    "one_launch_leg2": dict(fuse_sym=1),
}


def from_frame(df):
    return ingest.directed(df, False, "from", "to", "weight")[1]


def from_lists(n, rows):
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate([np.sort(np.asarray(r, dtype=np.int32)) for r in rows] + [np.zeros(0, dtype=np.int32)])
    deg = np.diff(rowptr).astype(np.float64)
    return CSR(n, n, rowptr, col.astype(np.int32), np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0))


def row0_sees_all(n=520):
    """Row 0 of the caller's order references every node (the plan keeps that order: reorder = False): first(i) = 0."""
    rng = np.random.default_rng(11)
    rows = [list(range(n))] + [sorted(set(rng.integers(0, n, size=rng.integers(0, 9)).tolist())) for _ in range(n - 1)]
    return from_lists(n, rows)


def last_block_only(n=700, live=50):
    """Only `live` rows have entries: the ascending order puts them last, inside the last 128-row block."""
    rng = np.random.default_rng(12)
    who = set(rng.choice(n, size=live, replace=False).tolist())
    rows = [sorted(set(rng.integers(0, n, size=rng.integers(3, 40)).tolist())) if a in who else [] for a in range(n)]
    return from_lists(n, rows)


def dead_blocks(csr, reorder=True):
    """planprep.hip in NumPy: the order (stable length order, two passes by (length, first referencing row)), then
    sum over the panels of min(first_block, blocks) = the (128-row block, panel) units no triangle-form leg 2 reads."""
    n = csr.n_rows
    length = np.diff(csr.rowptr).astype(np.int64)
    rows = np.repeat(np.arange(n), length)
    col = csr.col.astype(np.int64)

    def first_under(order):
        inv = np.empty(n, dtype=np.int64)
        inv[order] = np.arange(n)
        first = np.full(n, n, dtype=np.int64)
        np.minimum.at(first, col, inv[rows])
        return inv, first
    order = np.arange(n)
    if reorder:
        order = np.argsort(length, kind="stable")
        for _ in range(2):
            _, first = first_under(order)
            order = order[np.argsort(length[order] * (n + 1) + first[order], kind="stable")]
    inv, first = first_under(order)
    nblk, npan = (n + 127) // 128, (n + 31) // 32
    fb = np.full(npan, nblk, dtype=np.int64)
    ref = first < n
    np.minimum.at(fb, inv[ref] // 32, first[ref] // 128)
    return int(fb.sum()), int(nblk * npan)


def oracle(csr, scale, evidence, apriori, lbd, coef):
    W = csr.dense(scale.astype(np.float32).astype(np.float64))
    E = O.evidence(csr.dense(np.ones(csr.n_rows))) if evidence else None
    S = np.eye(csr.n_rows)
    for _ in range(UPDATES):
        S = O.update(W, S, coef, E, None if apriori is None else apriori.astype(np.float64), lbd)
    return S


def run_plan(ops, csr, scale, skip, tuning, sample=None, **kw):
    ops.set_tuning(**{**BASE, **tuning, "leg1_skip": skip})
    p = Plan(ops, csr, scale, **kw)
    counts = [p.step(0.0, exact_count=True) for _ in range(UPDATES)]
    units, skipped = p.get("leg1_units"), p.get("leg1_skipped")
    got = p.result() if sample is None else p.rows(sample)
    p.free()
    return got, counts, units, skipped


def case(ops, out, name, csr, tuning, want=None, sample=None, **kw):
    scale = kw.pop("rowscale", csr.rowscale)
    on, c_on, units, skipped = run_plan(ops, csr, scale, 1, tuning, sample, **kw)
    off, c_off, units_off, skipped_off = run_plan(ops, csr, scale, 0, tuning, sample, **kw)
    rec = {"bit_equal": bool(np.array_equal(on, off)), "finite": bool(np.isfinite(on).all() and np.isfinite(off).all()),
           "counts_equal": c_on == c_off, "counts": c_on, "units": units, "skipped": skipped, "units_off": units_off,
           "skipped_off": skipped_off}
    rec["dead_blocks"], rec["blocks"] = dead_blocks(csr, kw.get("reorder", True))
    if want is not None:
        rec["within_parity"] = bool(np.allclose(on, want, rtol=1e-5, atol=1e-30) and np.allclose(off, want, rtol=1e-5, atol=1e-30))
        rec["max_rel_err"] = float(np.max(np.abs(on - want) / np.maximum(np.abs(want), 1e-300)))
    out[name] = rec


def main():
    ops = HipOps(0)
    out = {}
    if len(sys.argv) > 2 and sys.argv[2] == "big":
        csr = from_frame(synth.powerlaw_directed(16500, 6, seed=4))
        sample = np.sort(np.random.default_rng(0).choice(csr.n_rows, size=192, replace=False)).astype(np.int32)
        case(ops, out, "big/grouped", csr, dict(fuse=1, fuse_min=0, fuse_steps=-1, fuse_group=4, leg1_order=-1), sample=sample, coef=0.8)
        print(json.dumps(out))
        return
    graphs = {
        "pl520": (from_frame(synth.powerlaw_directed(520, 5, seed=1)), {}),
        "pl1031": (from_frame(synth.powerlaw_directed(1031, 5, seed=2)), {}),
        "pl2100": (from_frame(synth.powerlaw_directed(2100, 6, seed=3)), {}),
        "er500": (from_frame(synth.er_directed(500, 0.012, seed=5)), {}),
        "row0_all": (row0_sees_all(), dict(reorder=False)),
        "last_block": (last_block_only(), {}),
    }
    for gname, (csr, kw) in graphs.items():
        want = oracle(csr, csr.rowscale, False, None, None, 0.8)
        for vname, tuning in VARIANTS.items():
            case(ops, out, f"{gname}/{vname}", csr, tuning, want, coef=0.8, **kw)
    # SimRank++ (evidence, restricted to its support and not) and priors, on one graph
    csr = graphs["pl1031"][0]
    n = csr.n_rows
    spread = ingest.spread(csr) * csr.rowscale
    rng = np.random.default_rng(7)
    sym = rng.random((n, n)).astype(np.float32)             # (the plan holds a prior in f32: the oracle gets the same values)
    sym = ((sym + sym.T) / 2).astype(np.float32)
    asym = rng.random((n, n)).astype(np.float32)
    want_pp = oracle(csr, spread, True, None, None, 0.8)
    case(ops, out, "pp/restricted", csr, dict(restrict_support=1), want_pp, rowscale=spread, evidence=True)
    case(ops, out, "pp/unrestricted", csr, dict(restrict_support=0), want_pp, rowscale=spread, evidence=True)
    case(ops, out, "prior/symmetric", csr, {}, oracle(csr, spread, True, sym, 0.3, 0.8), rowscale=spread, evidence=True,
         apriori=sym, lbd=0.3)
    case(ops, out, "prior/asymmetric", csr, {}, oracle(csr, spread, True, asym, 0.3, 0.8), rowscale=spread, evidence=True,
         apriori=asym, lbd=0.3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
