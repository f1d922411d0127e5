#!/usr/bin/env python3
"""kmedoids (libsimrank_kmedoids.so) on compact f32 and fp16-held models at BASELINE config 4 (N = 32768 power-law, mean
degree 32), from --seeds random seeds and from the medoids of cut(linkage(), n_clusters=--seeds).  Warm, medians and the
spread (min .. max) over --reps; one JSON line per measurement on stdout, all of them also in --out:

  what="loop"     per start: the iterations to convergence, the whole kmedoids call (wall), and per iteration (the sums of a
                  timed loop over its iterations) the assign kernel, the sweep and the pick (HIP events), the copy of the N
                  labels to the host, the host regroup and the copy of the lists back (host clock); next to the assign
                  kernel a device-to-device copy of K x N stored elements (what the memory system gives a pure stream of
                  the bytes the kernel reads: the copy reads AND writes them)
  what="parent"   (--parent) the route the public methods offered before, timed in the same run: per iteration
                  rows(medoids) over PCIe, a NumPy argmax with the stay rule, cluster_quality and the pick on the host;
                  and whether it gives the same labels, medoids and history

    python tools/bench_kmedoids.py [--workloads pl32768d32] [--reps 5] [--updates 3] [--seeds 500] [--max-iter 20]
                                   [--parent] [--out profiles/bench_kmedoids.json]
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
from simrank_amd import _kmedoids, synth                  # noqa: E402
from simrank_amd._driver import Scratch                   # noqa: E402

LINES = []
ELEMENT_BYTES = {0: 4, 1: 4, 2: 2, 3: 8}


def emit(**row):
    LINES.append(row)
    print(json.dumps(row), flush=True)


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def parent_route(model, index, seeds, max_iter):
    """The loop over the public methods: (cluster, medoids, [(moved, changed)], milliseconds of the stages)."""
    ms = dict(rows_ms=0.0, argmax_ms=0.0, cluster_quality_ms=0.0, pick_ms=0.0)

    def clocked(name, f):
        t0 = time.perf_counter()
        out = f()
        ms[name] += (time.perf_counter() - t0) * 1e3
        return out
    medoids, cluster, steps = np.array(seeds, dtype=np.int64), None, []
    for _ in range(max_iter):
        V = clocked("rows_ms", lambda: model.rows(index[medoids]).to_numpy())
        cluster, _, moved = clocked("argmax_ms", lambda: _kmedoids.assign_rows(V, medoids, cluster))
        del V
        own = clocked("cluster_quality_ms", lambda: model.cluster_quality(cluster)["own"].to_numpy())
        medoids, _, changed = clocked("pick_ms", lambda: _kmedoids.pick_members(own, cluster, medoids))
        steps.append((moved, changed))
        if changed == 0:
            break
    return cluster, medoids, steps, ms


def one_model(a, name, model, storage):
    reader = model._model[0]._reader(0)
    ops, n, b = reader.ops, reader.n, reader.blocks[0]
    index = pd.Index(model._model[1][0][1])               # the dense frame's labels
    starts = {f"random{a.seeds}": np.sort(np.random.default_rng(0).choice(n, a.seeds, replace=False))}
    cut = model.cut(model.linkage(), n_clusters=a.seeds)
    starts[f"cut{a.seeds}"] = index.get_indexer(model.medoids(cut).to_numpy())
    for sname, seeds in starts.items():
        seeds = np.asarray(seeds, dtype=np.int64)
        k = int(seeds.size)
        nbytes = k * n * ELEMENT_BYTES[b["layout"]]
        copy = []
        with Scratch(ops) as scratch:
            dst = scratch.malloc(nbytes)
            for _ in range(a.reps + 1):
                copy.append(ops.timed(lambda: ops.copy_bytes(dst, b["ptr"], nbytes)))
        stages, wall, out = [], [], None
        for _ in range(a.reps + 1):
            timing = {}
            got = _kmedoids.loop_reader(reader, seeds, a.max_iter, timing)
            stages.append({key: v / len(got[5]) for key, v in timing.items()})
            t0 = time.perf_counter()
            out = model.kmedoids(index[seeds], max_iter=a.max_iter)
            wall.append((time.perf_counter() - t0) * 1e3)
        labels, clusters, history = out
        emit(what="loop", workload=name, n=n, storage=storage, start=sname, k=k, iterations=len(history),
             converged=bool(history["changed"].iloc[-1] == 0), moved=history["moved"].tolist(),
             changed=history["changed"].tolist(), objective=history["objective"].tolist(),
             largest=int(clusters["size"].max()), singletons=int((clusters["size"] == 1).sum()), assign_bytes=nbytes,
             copy_ms=spread(copy[1:]), kmedoids_wall_ms=spread(wall[1:]),
             per_iteration_ms={key: spread([s[key] for s in stages[1:]]) for key in stages[0]})
        if a.parent:
            t0 = time.perf_counter()
            cluster, medoids, steps, ms = parent_route(model, index, seeds, a.max_iter)
            parent_ms = (time.perf_counter() - t0) * 1e3
            emit(what="parent", how="rows(medoids) + NumPy argmax + cluster_quality + host pick", workload=name, n=n,
                 storage=storage, start=sname, k=k, iterations=len(steps), wall_ms=round(parent_ms, 1),
                 per_iteration_ms={key: round(v / len(steps), 2) for key, v in ms.items()},
                 rows_bytes_per_iteration=k * n * 8,
                 same_labels=bool(np.array_equal(cluster, labels["cluster"].to_numpy())),
                 same_medoids=bool(np.array_equal(index[medoids], clusters["medoid"].to_numpy())),
                 same_history=bool(steps == list(zip(history["moved"].tolist(), history["changed"].tolist()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pl32768d32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=500)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--parent", action="store_true", help="also time the loop over rows() and cluster_quality")
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
