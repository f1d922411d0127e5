#!/usr/bin/env python3
"""prune(k) (libsimrank_neighbors.so) at BASELINE config 4 (N = 32768 power-law, mean degree 32) and at N = 65536, f32.
Warm, medians and the spread (min .. max) over --reps; one JSON line per measurement on stdout:

  what="select"  over ALL rows of the kept model, read in place, into tables that are already allocated (HIP events):
                 select_ms: simrank_neighbors_select; topk_ms: simrank_query_topk on the same rows and k, the yardstick
                 (one warm-up run; when that run takes more than --slow-ms, ONE further run is timed instead of --reps);
                 copy_ms: a device-to-device copy of the matrix's N^2 x 4 bytes in the same run, the floor of anything
                 that reads the matrix once.  -> topk_over_select = topk / select.  The two results are compared.
  what="file"    wall time of prune(100), then save() / load_model() of the pruned model and the file's size, next to the
                 dense (compact) model's when its bytes are at most --dense-file-limit.
  what="recall"  MovieLens-shaped bipartite SimRank++: the share of recommend(users, 10) blocks that the model pruned to
                 k = 50 and k = 100 returns identically to the dense model (information: no threshold).

    python tools/bench_prune.py [--workloads pl32768d32,pl65536] [--ks 10,100,1000] [--reps 3] [--updates 3] [--dir D]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simrank_amd                                        # noqa: E402
import simrank_amd.SimRank as SRA                         # noqa: E402
from simrank_amd import _neighbors, _query, synth         # noqa: E402
from simrank_amd.engine import check                      # noqa: E402


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def d2d_ms(ops, nbytes, reps):
    src, dst = ops._malloc(nbytes), ops._malloc(nbytes)
    try:
        copy = lambda: check(ops.lib.simrank_memcpy_d2d(C.c_void_p(dst), C.c_void_p(src), nbytes, ops.stream), "simrank_memcpy_d2d")
        return [ops.timed(copy) for _ in range(reps + 1)][1:]
    finally:
        ops._free(src), ops._free(dst)


def timed_runs(ops, launch, reps, slow_ms):
    first = ops.timed(launch)                               # warm-up
    if first > slow_ms:
        return [ops.timed(launch)]
    return [ops.timed(launch) for _ in range(reps)]


def select_rows(a, name, model):
    solver = model._model[0]
    reader = solver._reader(0)
    (b,) = reader.blocks
    ops, n = reader.ops, reader.n
    nodes = np.arange(n, dtype=np.int32)
    pos_dev, ids_dev = ops.put(reader.inv[nodes]), ops.put(nodes)
    copy = d2d_ms(ops, n * n * 4, a.reps)
    try:
        for k in [int(x) for x in a.ks.split(",")]:
            k = min(k, n - 1)
            out = [(ops._malloc(4 * n * k), ops._malloc(8 * n * k)) for _ in range(2)]
            try:
                new = lambda: _neighbors.check(_neighbors.load().simrank_neighbors_select(
                    b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], pos_dev, ids_dev, n, b.get("col_ids"), k,
                    out[0][0], out[0][1], ops.stream), "simrank_neighbors_select")
                old = lambda: _query.check(_query.load().simrank_query_topk(
                    b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], pos_dev, ids_dev, n, b.get("col_ids"), k,
                    out[1][0], out[1][1], ops.stream), "simrank_query_topk")
                sel = timed_runs(ops, new, a.reps, a.slow_ms)
                top = timed_runs(ops, old, a.reps, a.slow_ms) if k <= 1024 else None
                same = None
                if top is not None:
                    got = [(np.empty((n, k), dtype=np.int32), np.empty((n, k), dtype=np.float64)) for _ in range(2)]
                    for (hi, hv), (di, dv) in zip(got, out):
                        ops.d2h(hi, di)
                        ops.d2h(hv, dv)
                    ops.synchronize()
                    same = bool(np.array_equal(got[0][0], got[1][0])
                                and np.array_equal(got[0][1].view(np.uint64), got[1][1].view(np.uint64)))
                print(json.dumps(dict(what="select", workload=name, n=n, k=k, layout=b["layout"], select_ms=spread(sel),
                                      topk_ms=None if top is None else spread(top), copy_ms=spread(copy),
                                      select_over_copy=round(statistics.median(sel) / statistics.median(copy), 2),
                                      topk_over_select=None if top is None else round(statistics.median(top) / statistics.median(sel), 2),
                                      same_result=same)), flush=True)
            finally:
                for p in out:
                    ops._free(p[0]), ops._free(p[1])
    finally:
        ops._free(pos_dev), ops._free(ids_dev)


def file_times(model, path, reps):
    save_ms, load_ms = [], []
    try:
        for _ in range(reps):
            t = time.perf_counter()
            model.save(path)
            save_ms.append((time.perf_counter() - t) * 1e3)
            size = os.path.getsize(path)
            t = time.perf_counter()
            loaded = simrank_amd.load_model(path)
            load_ms.append((time.perf_counter() - t) * 1e3)
            loaded.release()
    finally:
        if os.path.exists(path):
            os.remove(path)
    return dict(save_ms=spread(save_ms), load_ms=spread(load_ms), file_bytes=size)


def recall(a):
    df = synth.WORKLOADS["ml1m"][0]()
    dense = SRA.BipartiteSimRankPP().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True, strict_reference=False)
    users = sorted(set(df["user"]))[:a.users]
    want = dense.recommend(users, 10, group=1)
    blocks = {u: g[["neighbor", "score"]].to_numpy().tolist() for u, g in want.groupby("node", sort=False)}
    dense.release()
    for k in (50, 100):
        model = SRA.BipartiteSimRankPP().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True, strict_reference=False)
        t = time.perf_counter()
        model.prune(k)
        prune_ms = (time.perf_counter() - t) * 1e3
        got = model.recommend(users, 10, group=1)
        mine = {u: g[["neighbor", "score"]].to_numpy().tolist() for u, g in got.groupby("node", sort=False)}
        same = sum(mine.get(u) == rows for u, rows in blocks.items())
        same_items = sum([r[0] for r in mine.get(u, [])] == [r[0] for r in rows] for u, rows in blocks.items())
        print(json.dumps(dict(what="recall", workload="ml1m", k=k, users=len(blocks), identical_blocks=same,
                              identical_share=round(same / max(1, len(blocks)), 4),
                              same_items_share=round(same_items / max(1, len(blocks)), 4),
                              prune_wall_ms=round(prune_ms, 1), device_bytes=model.device_bytes)), flush=True)
        model.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pl32768d32,pl65536")
    ap.add_argument("--ks", default="10,100,1000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--slow-ms", type=float, default=1500.0)
    ap.add_argument("--dense-file-limit", type=int, default=6 << 30)
    ap.add_argument("--users", type=int, default=2000)
    ap.add_argument("--no-recall", action="store_true")
    ap.add_argument("--dir", default=tempfile.gettempdir(), help="where the saved models are written (and removed)")
    a = ap.parse_args()
    path = os.path.join(a.dir, f"bench_prune_{os.getpid()}.simrank")
    for name in [w for w in a.workloads.split(",") if w]:
        df = synth.WORKLOADS[name][0]()
        model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True)
        select_rows(a, name, model)
        n = len(model._model[1][0][1])
        dense = None
        if n * n * 4 <= a.dense_file_limit:
            model.compact()
            dense = dict(file_times(model, path, 1), device_bytes=model.device_bytes)
        t = time.perf_counter()
        model.prune(100)
        prune_ms = (time.perf_counter() - t) * 1e3
        pruned = dict(file_times(model, path, a.reps), device_bytes=model.device_bytes)
        print(json.dumps(dict(what="file", workload=name, n=n, k=100, prune_wall_ms=round(prune_ms, 1),
                              prune_from="compact" if dense else "kept", pruned=pruned, dense=dense)), flush=True)
        model.release()
    if not a.no_recall:
        recall(a)


if __name__ == "__main__":
    main()
