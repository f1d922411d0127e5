#!/usr/bin/env python3
"""simrank_candidates_topk (libsimrank_candidates.so) at BASELINE config 4 (N = 32768 power-law, mean degree 32) on a
compact f32 model and an fp16-held one: --queries query rows, k in --ks, the candidates |among| = N / 64, N / 8, N / 2 and
N drawn at random, and one contiguous range of N / 8 labels.  Warm; medians and the spread (min .. max) over --reps timed
windows of --inner launches each (HIP events), the routes alternating window by window in the same run.  One JSON line per
point on stdout, and all of them in --out (profiles/bench_candidates.json):

  what="topk"   new_ms:    simrank_candidates_topk
                route2_ms: what the kernels before it allow: simrank_query_rows with col_pos = the candidates into a float64
                           band, then simrank_sets_topk on the band (rows_ms and band_topk_ms are its two parts).  Both
                           routes are given no own id to drop (the band selection cannot), and the tool checks that they
                           return the same ids and the same bits: same_result.
                copy_ms:   a device-to-device copy of the bytes the gather touches (queries x candidates x element size):
                           the floor.
                select_ms: at |among| = N, simrank_neighbors_select on the same rows and k (its result is compared too).
  what="sets"   score_ms and topk_ms of score_sets(top_k=10) over --baskets baskets of 20 members, unfiltered and with
                among = N / 8 (``_sets.run``'s ``timing``): information only.
  what="summary" per model and k the crossover, if any: the points at which the new kernel loses to route 2.

    python tools/bench_candidates.py [--workload pl32768d32] [--ks 10,100] [--queries 1024] [--reps 5] [--inner 4]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simrank_amd.SimRank as SRA                                          # noqa: E402
from simrank_amd import _candidates, _neighbors, _query, _sets, synth      # noqa: E402
from simrank_amd.engine import check                                       # noqa: E402

ELEMENT_BYTES = {_query.PANEL_F32: 4, _query.ROWMAJOR_F32: 4, _query.PANEL_F16: 2, _query.ROWMAJOR_F64: 8}


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def alternate(ops, launches, reps, inner):
    """name -> milliseconds per launch of each timed window; one warm-up window each, then the routes take turns."""
    window = lambda f: ops.timed(lambda: [f() for _ in range(inner)]) / inner
    for f in launches.values():
        window(f)
    out = {name: [] for name in launches}
    for _ in range(reps):
        for name, f in launches.items():
            out[name].append(window(f))
    return out


def candidate_sets(n, rng):
    sets = [("random", n // d, np.sort(rng.permutation(n)[:n // d]).astype(np.int32)) for d in (64, 8, 2, 1)]
    lo = int(rng.integers(0, n - n // 8))
    return sets + [("range", n // 8, np.arange(lo, lo + n // 8, dtype=np.int32))]


def topk_points(a, model, tag, records):
    solver = model._model[0]
    reader = solver._reader(0)
    (b,) = reader.blocks
    ops, n = reader.ops, reader.n
    rng = np.random.default_rng(a.seed)
    n_q = min(a.queries, n)
    nodes = np.sort(rng.permutation(n)[:n_q]).astype(np.int32)
    block = (b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"])
    held = []
    put = lambda host: held.append(ops.put(np.ascontiguousarray(host))) or held[-1]
    malloc = lambda nbytes: held.append(ops._malloc(nbytes)) or held[-1]
    try:
        pos_dev, none_dev = put(reader.inv[nodes]), put(np.full(n_q, -1, dtype=np.int32))
        for kind, m, cand in candidate_sets(n, rng):
            cpos_dev, cids_dev = put(reader.inv[cand]), put(cand)
            band = malloc(8 * n_q * m)
            nbytes = n_q * m * ELEMENT_BYTES[b["layout"]]
            src, dst = malloc(nbytes), malloc(nbytes)
            for k in [min(int(x), m) for x in a.ks.split(",")]:
                out = [(malloc(4 * n_q * k), malloc(8 * n_q * k)) for _ in range(3)]
                rows = lambda: _query.check(_query.load().simrank_query_rows(
                    *block, pos_dev, n_q, cpos_dev, m, band, m, ops.stream), "simrank_query_rows")
                band_topk = lambda: _sets.check(_sets.load().simrank_sets_topk(
                    band, m, n_q, m, cids_dev, k, out[1][0], out[1][1], ops.stream), "simrank_sets_topk")
                launches = {
                    "new_ms": lambda: _candidates.check(_candidates.load().simrank_candidates_topk(
                        *block, pos_dev, none_dev, n_q, cpos_dev, cids_dev, m, k, out[0][0], out[0][1], ops.stream),
                        "simrank_candidates_topk"),
                    "route2_ms": lambda: (rows(), band_topk()),
                    "rows_ms": rows,
                    "band_topk_ms": band_topk,
                    "copy_ms": lambda: check(ops.lib.simrank_memcpy_d2d(C.c_void_p(dst), C.c_void_p(src), nbytes,
                                                                        ops.stream), "simrank_memcpy_d2d"),
                }
                if m == n:
                    launches["select_ms"] = lambda: _neighbors.check(_neighbors.load().simrank_neighbors_select(
                        *block, pos_dev, none_dev, n_q, b.get("col_ids"), k, out[2][0], out[2][1], ops.stream),
                        "simrank_neighbors_select")
                ms = alternate(ops, launches, a.reps, a.inner)
                routes = 3 if "select_ms" in launches else 2
                got = [(np.empty((n_q, k), dtype=np.int32), np.empty((n_q, k), dtype=np.float64)) for _ in range(routes)]
                for (hi, hv), (di, dv) in zip(got, out):
                    ops.d2h(hi, di)
                    ops.d2h(hv, dv)
                ops.synchronize()
                same = bool(all(np.array_equal(got[0][0], g[0]) and np.array_equal(got[0][1].view(np.uint64), g[1].view(np.uint64))
                                for g in got[1:]))
                med = {name: statistics.median(v) for name, v in ms.items()}
                rec = dict(what="topk", model=tag, n=n, layout=b["layout"], queries=n_q, among=kind, candidates=m, k=k,
                           staged=bool(m <= _candidates.staged(b["layout"])), same_result=same,
                           route2_over_new=round(med["route2_ms"] / med["new_ms"], 2),
                           new_over_copy=round(med["new_ms"] / med["copy_ms"], 2),
                           **{name: spread(v) for name, v in ms.items()})
                records.append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        ops.synchronize()
        for p in held:
            ops._free(p)


def sets_points(a, model, tag, records):
    solver = model._model[0]
    reader = solver._reader(0)
    n = reader.n
    rng = np.random.default_rng(a.seed + 1)
    lists = [rng.permutation(n)[:20].astype(np.int32) for _ in range(a.baskets)]
    ptr = np.arange(a.baskets + 1, dtype=np.int64) * 20
    ids, w = np.concatenate(lists), np.ones(20 * a.baskets)
    among = np.sort(rng.permutation(n)[:n // 8]).astype(np.int32)
    for name, cand in (("unfiltered", None), ("among", among)):
        runs = []
        for _ in range(a.reps + 1):
            timing = {}
            _sets.run(reader, ptr, ids, w, 10, (ptr, ids), timing, among=cand)
            runs.append(timing)
        runs = runs[1:]
        rec = dict(what="sets", model=tag, n=n, baskets=a.baskets, k=10, candidates=n if cand is None else int(cand.size),
                   filter=name, score_ms=spread([t["score_ms"] for t in runs]), topk_ms=spread([t["topk_ms"] for t in runs]))
        records.append(rec)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="pl32768d32")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--baskets", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "bench_candidates.json"))
    a = ap.parse_args()
    df = synth.WORKLOADS[a.workload][0]()
    records = []
    for tag, precision in (("compact-f32", None), ("compact-fp16", "fp16")):
        model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True)
        try:
            model.compact() if precision is None else model.compact(precision=precision)
            topk_points(a, model, tag, records)
            sets_points(a, model, tag, records)
        finally:
            model.release()
    lost = [dict(model=r["model"], among=r["among"], candidates=r["candidates"], k=r["k"], route2_over_new=r["route2_over_new"])
            for r in records if r["what"] == "topk" and r["route2_over_new"] < 1.0]
    summary = dict(what="summary", workload=a.workload, all_same=all(r["same_result"] for r in records if r["what"] == "topk"),
                   points_lost_to_route2=lost, not_measured=["N = 65536", "float64", "LocalWorld(P)", "pruned"])
    records.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
