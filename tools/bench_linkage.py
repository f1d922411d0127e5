#!/usr/bin/env python3
"""linkage (libsimrank_linkage.so) on compact f32 and fp16-held models at BASELINE config 4 (N = 32768 power-law, mean
degree 32).  Warm, medians and the spread (min .. max) over --reps (HIP events for the stages, wall time for whole calls);
one JSON line per measurement on stdout, all of them also in --out:

  what="rounds"   the Boruvka rounds of one forest and the milliseconds of every pick sweep, hook and flatten call; next
                  to them ONE union sweep of components at the threshold that leaves about --clusters clusters (the same
                  bytes read once, by the kernel linkage shares its walk with) and a device-to-device copy of the
                  matrix's bytes (what the memory system gives a pure stream: it reads AND writes them)
  what="call"     model.linkage() as a whole (wall), the rows it returns, and cut(Z, n_clusters=--clusters)
  what="bisect"   the route through components alone: an 8-ary search for the threshold that leaves --clusters clusters
                  or, where ties skip that count, the next count above it; calls made, wall time, the threshold found
  what="parent"   (--parent; f32 only; host memory 2 x N^2 x 8) frame() over PCIe plus a dense Prim's algorithm over
                  max(S, S.T) on the host, then the same canonical table and cut
  what="agree"    cut(Z, t) of linkage at the threshold the bisection found == components(t) == the host route's cut

    python tools/bench_linkage.py [--workloads pl32768d32] [--reps 5] [--updates 3] [--clusters 500] [--parent]
                                  [--out profiles/bench_linkage.json]
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
from simrank_amd import _cluster, _linkage, _model, synth  # noqa: E402
from simrank_amd._driver import Scratch                   # noqa: E402

LINES = []


def emit(**row):
    LINES.append(row)
    print(json.dumps(row), flush=True)


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def wall(f, reps):
    """(the last result, milliseconds of every run after a warm one)"""
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms[1:]


def search_threshold(model, clusters):
    """(t, components there, calls made): the threshold found through components alone, 8 levels per call, that leaves
    ``clusters`` components or the fewest above that number."""
    n = len(model._model[1][0][1])
    lo, hi = 0.0, float(np.nextafter(model.threshold_for(1)[0], 2.0)) if np.isfinite(model.threshold_for(1)[0]) else 1.0
    best, calls = (hi, n), 0                               # above every value: every node alone
    for _ in range(24):
        ts = [lo + (hi - lo) * (i + 1) / 9 for i in range(8)]
        counts = (model.components(ts).max(axis=0) + 1).tolist()
        calls += 1
        for t, c in zip(ts, counts):                       # (counts rise with t)
            if clusters <= c < best[1] or (c == best[1] and t < best[0]):
                best = (t, c)
        below = [t for t, c in zip(ts, counts) if c < clusters]
        above = [t for t, c in zip(ts, counts) if c >= clusters]
        lo, hi = (max(below) if below else lo), (min(above) if above else hi)
        if best[1] == clusters or hi <= np.nextafter(lo, hi):
            break
    return best[0], best[1], calls


def host_forest(S):
    """Dense Prim's algorithm over w = max(S, S.T) (NaN: no entry) -> (a, b, value): what a user writes for the frame."""
    n = len(S)
    St = np.ascontiguousarray(S.T)
    key, link, done = np.full(n, -np.inf), np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=bool)
    a, b, v = [], [], []
    for start in range(n):
        if done[start]:
            continue
        i = start
        while True:
            done[i] = True
            with np.errstate(invalid="ignore"):
                w = np.fmax(S[i], St[i])
            better = ~done & (w > key)
            key[better], link[better] = w[better], i
            open_ = np.where(done, -np.inf, key)
            j = int(np.argmax(open_))
            if not open_[j] > -np.inf:
                break
            a.append(int(link[j])), b.append(j), v.append(float(key[j]))
            i = j
    return np.array(a, dtype=np.int64), np.array(b, dtype=np.int64), np.array(v)


def one_model(a, name, model, storage):
    reader = model._model[0]._reader(0)
    ops, n, blocks = reader.ops, reader.n, reader.blocks
    nbytes = sum(_model.block_bytes(b) for b in blocks)
    # the whole call, and the cut
    Z, call_ms = wall(model.linkage, a.reps)
    labels_k, cut_ms = wall(lambda: model.cut(Z, n_clusters=a.clusters), a.reps)
    emit(what="call", workload=name, n=n, storage=storage, matrix_bytes=nbytes, rows=len(Z), heights=int(Z["similarity"].nunique()),
         linkage_wall_ms=spread(call_ms), cut_wall_ms=spread(cut_ms), clusters=int(labels_k.max()) + 1)
    # the route through components alone
    (t, found, calls), bisect_ms = wall(lambda: search_threshold(model, a.clusters), 1)
    emit(what="bisect", workload=name, n=n, storage=storage, t=t, components=found, calls=calls, wall_ms=round(bisect_ms[0], 1))
    # the stages
    runs = []
    for _ in range(a.reps + 1):
        ms = []
        *_, rounds = _linkage.forest_blocks(ops, blocks, n, None, timing=ms)
        runs.append(ms)
    per = len(blocks) + 2                                  # (f32 and fp16-held: one pick per block, a hook, a flatten per round)
    picks = [[sum(ms[r * per:r * per + len(blocks)]) for ms in runs[1:]] for r in range(rounds)]
    union = []
    for _ in range(a.reps + 1):
        ms = []
        _cluster.roots_blocks(ops, blocks, n, [t], timing=ms)
        union.append(sum(ms[:len(blocks)]))
    copy = []
    with Scratch(ops) as scratch:
        dst = [scratch.malloc(_model.block_bytes(b)) for b in blocks]
        for _ in range(a.reps + 1):
            copy.append(ops.timed(lambda: [ops.copy_bytes(d, b["ptr"], _model.block_bytes(b)) for d, b in zip(dst, blocks)]))
    emit(what="rounds", workload=name, n=n, storage=storage, matrix_bytes=nbytes, rounds=rounds,
         pick_ms_per_round=[spread(p) for p in picks], hook_flatten_ms=spread([sum(ms) - sum(ms[r * per + i] for r in range(rounds)
                                                                                            for i in range(len(blocks)))
                                                                              for ms in runs[1:]]),
         forest_ms=spread([sum(ms) for ms in runs[1:]]), union_sweep_ms=spread(union[1:]), union_t=t, copy_ms=spread(copy[1:]))
    # the three routes agree at the threshold the bisection found
    mine = model.cut(Z, t=t).to_numpy()
    agree = dict(linkage_cut_equals_components=bool(np.array_equal(mine, model.components(t).to_numpy())))
    if a.parent and storage == "f32":
        t0 = time.perf_counter()
        S = model.frame().to_numpy()
        frame_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        rows = _linkage.canonical(n, *host_forest(S))
        host_ms = (time.perf_counter() - t0) * 1e3
        Zh = pd.DataFrame(dict(zip(_linkage.COLUMNS, rows)))
        emit(what="parent", how="frame() + dense Prim on the host", workload=name, n=n, frame_wall_ms=round(frame_ms, 1),
             host_wall_ms=round(host_ms, 1), host_bytes=int(S.nbytes), rows=len(Zh))
        agree["host_table_equals_linkage"] = bool(Zh.equals(Z))
        agree["host_cut_equals_components"] = bool(np.array_equal(model.cut(Zh, t=t).to_numpy(), mine))
        del S
    emit(what="agree", workload=name, n=n, storage=storage, t=t, **agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pl32768d32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--clusters", type=int, default=500)
    ap.add_argument("--parent", action="store_true", help="also time frame() plus a host spanning tree (f32, host memory 2 N^2 x 8)")
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
