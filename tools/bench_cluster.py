#!/usr/bin/env python3
"""components (libsimrank_cluster.so) on compact f32 and fp16-held models at BASELINE config 4 (N = 32768 power-law, mean
degree 32) and at N = 65536 where memory allows.  Warm, medians and the spread (min .. max) over --reps (HIP events); one
JSON line per measurement on stdout, all of them also in --out:

  what="components" per threshold (threshold_for(10 N), threshold_for(N^2 / 100), 0.0): the union sweeps plus the labels
                    call of ONE level, the components found and the largest one; count_ms: one count_pairs sweep at the
                    same threshold, which reads the same bytes once -> components_over_count; and all three levels in one
                    sweep
  what="parent"     what a user does without the call (--parent; f32 only; needs SciPy): pairs(t) + SciPy's connected
                    components of the rows where the pairs fit --max-pairs; where they do not, frame() (the N x N float64
                    hand-back) + a frontier search over its rows and columns on the host; wall times, components found

    python tools/bench_cluster.py [--workloads pl32768d32,pl65536] [--reps 5] [--updates 3] [--parent]
                                  [--max-pairs 134217728] [--out profiles/bench_cluster.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simrank_amd.SimRank as SRA                         # noqa: E402
from simrank_amd import _cluster, _model, _profile, synth  # noqa: E402

LINES = []


def emit(**row):
    LINES.append(row)
    print(json.dumps(row), flush=True)


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def timed_roots(reader, ts, reps):
    ms = []
    for _ in range(reps + 1):
        t = []
        roots = _cluster.roots_blocks(reader.ops, reader.blocks, reader.n, ts, timing=t)
        ms.append(sum(t))
    return roots, ms[1:]


def sweeps(a, name, model, storage):
    reader = model._model[0]._reader(0)
    ops, n = reader.ops, reader.n
    nbytes = sum(_model.block_bytes(b) for b in reader.blocks)
    levels = [("threshold_for(10 N)", model.threshold_for(10 * n)[0]), ("threshold_for(N^2 / 100)", model.threshold_for(n * n // 100)[0]),
              ("0.0", 0.0)]
    levels = [(tag, float(t)) for tag, t in levels if np.isfinite(t)]
    for tag, t in levels:
        roots, ms = timed_roots(reader, [t], a.reps)
        sizes = np.bincount(np.unique(roots[0], return_inverse=True)[1].reshape(-1))
        count = []
        for _ in range(a.reps + 1):
            c = []
            pairs = _profile.count_blocks(ops, reader.blocks, [t], timing=c)
            count.append(sum(c))
        row = dict(what="components", workload=name, n=n, storage=storage, level=tag, t=t, matrix_bytes=nbytes, pairs=int(pairs[0]),
                   components=int(sizes.size), largest=int(sizes.max()), components_ms=spread(ms), count_ms=spread(count[1:]))
        row["components_over_count"] = round(row["components_ms"]["median"] / row["count_ms"]["median"], 2)
        emit(**row)
    _, ms = timed_roots(reader, [t for _, t in levels], a.reps)
    emit(what="components", workload=name, n=n, storage=storage, level="all of them in one sweep", t=[t for _, t in levels],
         matrix_bytes=nbytes, components_ms=spread(ms))
    return levels


def host_components_of_pairs(n, src, dst):
    """What a user writes for the rows of pairs(t): SciPy's connected components of the edge list."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    graph = coo_matrix((np.ones(src.size, dtype=np.int8), (src, dst)), shape=(n, n))
    return connected_components(graph, directed=False)[0]


def host_components_of_frame(S, t):
    """What a user writes for the dense frame: a frontier search, one row and one column of S per node taken off the
    frontier, over the nodes not yet reached (no N x N boolean copy, no edge list: at a dense level that would be N^2
    entries).  Returns the number of components."""
    n = len(S)
    todo = np.ones(n, dtype=bool)
    count = 0
    for start in range(n):
        if not todo[start]:
            continue
        count += 1
        todo[start] = False
        frontier = [start]
        while frontier:
            i = frontier.pop()
            near = todo & ((S[i] >= t) | (S[:, i] >= t))
            if near.any():
                todo &= ~near
                frontier.extend(np.flatnonzero(near).tolist())
    return count


def parent(a, name, model, levels):
    labels = model._model[1][0][1]
    n = len(labels)
    for tag, t in levels:
        pairs = int(model.count_pairs([t])[0])
        if pairs <= a.max_pairs and t > 0:
            t0 = time.perf_counter()
            df = model.pairs(t, max_pairs=a.max_pairs)
            pairs_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            index = {lab: i for i, lab in enumerate(labels)}
            src, dst = df["node"].map(index).to_numpy(), df["neighbor"].map(index).to_numpy()
            found = host_components_of_pairs(n, src, dst)
            host_ms = (time.perf_counter() - t0) * 1e3
            emit(what="parent", how="pairs(t) + SciPy connected_components", workload=name, level=tag, t=t, pairs=pairs,
                 pairs_wall_ms=round(pairs_ms, 1), host_wall_ms=round(host_ms, 1), components=int(found))
        else:
            t0 = time.perf_counter()
            S = model.frame().to_numpy()
            frame_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            found = host_components_of_frame(S, t)
            host_ms = (time.perf_counter() - t0) * 1e3
            emit(what="parent", how="frame() + host frontier search", workload=name, level=tag, t=t, pairs=pairs,
                 frame_wall_ms=round(frame_ms, 1), host_wall_ms=round(host_ms, 1), host_bytes=int(S.nbytes), components=int(found))
            del S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pl32768d32,pl65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--max-pairs", type=int, default=2 ** 27)
    ap.add_argument("--parent", action="store_true", help="also time what a user does without the call (f32, host memory N^2 x 8)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name in [w for w in a.workloads.split(",") if w]:
        df = synth.WORKLOADS[name][0]()
        for storage in ("f32", "fp16"):
            model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True)
            try:
                model.compact("fp16" if storage == "fp16" else None)
                levels = sweeps(a, name, model, storage)
                if a.parent and storage == "f32":
                    parent(a, name, model, levels)
            finally:
                model.release()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(LINES, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
