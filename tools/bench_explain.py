#!/usr/bin/env python3
"""explain (libsimrank_explain.so) on compact f32 and fp16-held models at BASELINE config 4 (N = 32768 power-law, mean
degree 32), for two workloads: "small", every one of --nodes random nodes against its --top most similar nodes (tens of
thousands of pairs of about degree x degree terms), and "hub", the node with the most in-neighbours against one of about
--hub-other (one pair).  Warm,
medians and the spread (min .. max) over --reps; one JSON line per measurement on stdout, all of them also in --out:

  what="explain"  the three device stages (HIP events: the gather from the iterate in place, the sums, the selection), the
                  whole explain call (wall, frames included), the pairs, the terms and the bytes of the band; next to the
                  gather a device-to-device copy of terms x 8 bytes (what the memory system gives a pure stream of the
                  bytes the gather WRITES; it reads one stored element, in the worst case one cache line, per term)
  what="parent"   (--parent) the route the public methods offered before, timed in the same run on the first
                  --parent-pairs pairs: rows(I(a)) over PCIe, NumPy's sub-matrix, sums and top-k; and whether it gives
                  the same integers and top-k (exactly) and the same sums (within the bound the header states)

    python tools/bench_explain.py [--workloads pl32768d32] [--reps 5] [--updates 3] [--nodes 1024] [--top 10] [--k 10]
                                  [--hub-other 1000] [--parent] [--parent-pairs 64] [--out profiles/bench_explain.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simrank_amd.SimRank as SRA                         # noqa: E402
from simrank_amd import _explain, synth                   # noqa: E402
from simrank_amd._driver import Scratch                   # noqa: E402

LINES = []
ELEMENT_BYTES = {0: 4, 1: 4, 2: 2, 3: 8}


def emit(**row):
    LINES.append(row)
    print(json.dumps(row), flush=True)


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def parent_route(model, index, spec, ia, ib, k):
    """Per pair rows(I(a)) and NumPy: (raw, contributors, best (i, j, value) per pair as ids, row sums), milliseconds."""
    rowptr, col = np.asarray(spec.csr.rowptr, dtype=np.int64), np.asarray(spec.csr.col, dtype=np.int64)
    ms = dict(rows_ms=0.0, numpy_ms=0.0)
    out = []
    for a, b in zip(ia.tolist(), ib.tolist()):
        la, lb = np.sort(col[rowptr[a]:rowptr[a + 1]]), np.sort(col[rowptr[b]:rowptr[b + 1]])
        t0 = time.perf_counter()
        rows = model.rows(index[la]).to_numpy() if la.size else np.zeros((0, len(index)))
        t1 = time.perf_counter()
        piece = rows[:, lb]
        r_sum, c_sum, raw, count = _explain.reduce_host(piece)
        bi, bj, bv = _explain.best_host(piece, k)
        t2 = time.perf_counter()
        ms["rows_ms"] += (t1 - t0) * 1e3
        ms["numpy_ms"] += (t2 - t1) * 1e3
        out.append((raw, count, np.where(bi >= 0, la[np.maximum(bi, 0)] if la.size else -1, -1),
                    np.where(bj >= 0, lb[np.maximum(bj, 0)] if lb.size else -1, -1), bv, float(np.abs(piece).sum())))
        del rows
    return out, ms


def one_model(a, name, model, storage):
    solver = model._model[0]
    reader = solver._reader(0)
    ops, n, b = reader.ops, reader.n, reader.blocks[0]
    index = pd.Index(model._model[1][0][1])               # the dense frame's labels
    spec = solver.specs[0]
    deg = np.diff(np.asarray(spec.csr.rowptr, dtype=np.int64))
    nodes = np.sort(np.random.default_rng(0).choice(n, a.nodes, replace=False))
    near = model.most_similar(index[nodes], a.top)
    small = (index.get_indexer(near["node"]), index.get_indexer(near["neighbor"]))
    hub = int(np.argmax(deg))                             # the longest list against one of about --hub-other entries
    other = int(np.argmin(np.where(np.arange(n) == hub, np.iinfo(np.int64).max, np.abs(deg - a.hub_other))))
    workloads = {"small": small, "hub": (np.array([other]), np.array([hub]))}      # (the parent route reads rows(I(a)))
    for wname, (ia, ib) in workloads.items():
        ia, ib = np.asarray(ia, dtype=np.int64), np.asarray(ib, dtype=np.int64)
        ptr_a, ids_a = _explain.lists_of(spec.csr, ia)
        ptr_b, ids_b = _explain.lists_of(spec.csr, ib)
        terms = int((np.diff(ptr_a) * np.diff(ptr_b)).sum())
        sorted_a, sorted_b = _explain.sorted_lists(ptr_a, ids_a)[0], _explain.sorted_lists(ptr_b, ids_b)[0]
        copy = []
        with Scratch(ops) as scratch:
            src, dst = scratch.malloc(8 * max(terms, 1)), scratch.malloc(8 * max(terms, 1))
            for _ in range(a.reps + 1):
                copy.append(ops.timed(lambda: ops.copy_bytes(dst, src, 8 * max(terms, 1))))
        stages, wall, out = [], [], None
        for _ in range(a.reps + 1):
            timing = {}
            _explain.run(reader, ptr_a, sorted_a, ptr_b, sorted_b, a.k, timing)
            stages.append(timing)
            t0 = time.perf_counter()
            out = model.explain(index[ia], index[ib], k=a.k)
            wall.append((time.perf_counter() - t0) * 1e3)
        pairs, top, _ = out
        emit(what="explain", workload=name, pairs_of=wname, n=n, storage=storage, pairs=int(ia.size), k=a.k, terms=terms,
             largest_pair=[int(np.diff(ptr_a).max()), int(np.diff(ptr_b).max())], band_bytes=8 * terms,
             stored_bytes=terms * ELEMENT_BYTES[b["layout"]], copy_ms=spread(copy[1:]), explain_wall_ms=spread(wall[1:]),
             stages_ms={key: spread([s[key] for s in stages[1:]]) for key in stages[0]})
        if a.parent:
            m = min(a.parent_pairs, int(ia.size))
            t0 = time.perf_counter()
            got, ms = parent_route(model, index, spec, ia[:m], ib[:m], a.k)
            parent_ms = (time.perf_counter() - t0) * 1e3
            raw = pairs["raw"].to_numpy()[:m]
            same_sums = all(abs(g[0] - r) <= 2.0 * t * 2.0 ** -52 * g[5]
                            for g, r, t in zip(got, raw, pairs["terms"].to_numpy()[:m].tolist()))
            same_counts = [g[1] for g in got] == pairs["contributors"].tolist()[:m]
            src_index = index
            want_top = [(p, src_index[i], src_index[j], float(v)) for p, g in enumerate(got)
                        for i, j, v in zip(g[2], g[3], g[4]) if i >= 0]
            mine = top[top["pair"] < m]
            same_top = want_top == list(zip(mine["pair"], mine["via_a"], mine["via_b"], mine["similarity"]))
            emit(what="parent", how="rows(I(a)) + NumPy sub-matrix, sums and top-k", workload=name, pairs_of=wname, n=n,
                 storage=storage, pairs=m, wall_ms=round(parent_ms, 1), per_pair_ms={key: round(v / m, 3) for key, v in ms.items()},
                 rows_bytes=int(np.diff(ptr_a)[:m].sum()) * n * 8, same_sums=bool(same_sums), same_counts=bool(same_counts),
                 same_topk=bool(same_top))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pl32768d32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--hub-other", type=int, default=1000, help="in-neighbours of the hub pair's second node, about")
    ap.add_argument("--parent", action="store_true", help="also time rows(I(a)) plus NumPy, on the first pairs")
    ap.add_argument("--parent-pairs", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name in [w for w in a.workloads.split(",") if w]:
        df = synth.WORKLOADS[name][0]()
        for storage in ("f32", "fp16"):
            model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True)
            try:
                model.compact("fp16" if storage == "fp16" else None)
                one_model(a, name, model, storage)
            finally:
                model.release()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(LINES, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
