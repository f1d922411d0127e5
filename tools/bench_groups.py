#!/usr/bin/env python3
"""cluster_quality (libsimrank_groups.so) on compact f32 and fp16-held models at BASELINE config 4 (N = 32768 power-law,
mean degree 32).  Warm, medians and the spread (min .. max) over --reps (HIP events for the kernel, wall time for whole
calls); one JSON line per measurement on stdout, all of them also in --out:

  what="sweep"    per labelling (K = 2; K = --clusters from cut(linkage()) and drawn at random: members a stride of K
                  apart, the gather at its worst; N / 4 small clusters; N singletons) the
                  kernel's milliseconds and the whole cluster_quality call (wall); next to them a device-to-device copy
                  of the matrix's bytes (what the memory system gives a pure stream: it reads AND writes them)
  what="sets"     score_sets with the --clusters clusters as baskets, dense form (wall): the transposed orientation, the
                  node itself included, a K x N float64 band over PCIe
  what="parent"   (--parent; f32 only; host memory 2 x N^2 x 8) the route the call replaces at the --clusters point:
                  frame() over PCIe plus the NumPy group-by of tests/groups_ref.py's vectorised twin; and whether its
                  `nearest` is the device's

    python tools/bench_groups.py [--workloads pl32768d32] [--reps 5] [--updates 3] [--clusters 500] [--parent]
                                 [--out profiles/bench_groups.json]
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
from simrank_amd import _groups, _model, synth             # noqa: E402
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


def labellings(model, n, clusters):
    rng = np.random.default_rng(0)
    Z = model.linkage()
    return {"k2": (np.arange(n) % 2).astype(np.int64), f"cut{clusters}": model.cut(Z, n_clusters=clusters).to_numpy(),
            f"random{clusters}": rng.integers(0, clusters, size=n), "small": rng.permutation(n) // 4, "singletons": np.arange(n, dtype=np.int64)}


def one_model(a, name, model, storage):
    reader = model._model[0]._reader(0)
    ops, n, b = reader.ops, reader.n, reader.blocks[0]
    nbytes = _model.block_bytes(b)
    copy = []
    with Scratch(ops) as scratch:
        dst = scratch.malloc(nbytes)
        for _ in range(a.reps + 1):
            copy.append(ops.timed(lambda: ops.copy_bytes(dst, b["ptr"], nbytes)))
    labs = labellings(model, n, a.clusters)
    quality = {}
    for lname, lab in labs.items():
        clusters, gidx, sizes = _groups.groups_of(lab)
        kernel = []
        for _ in range(a.reps + 1):
            ms = []
            _groups.scores_reader(reader, gidx, sizes, False, timing=ms)
            kernel.append(sum(ms))
        quality[lname], call_ms = wall(lambda: model.cluster_quality(lab), a.reps)
        emit(what="sweep", workload=name, n=n, storage=storage, labelling=lname, clusters=int(clusters.size),
             largest=int(sizes.max()), matrix_bytes=nbytes, kernel_ms=spread(kernel[1:]), copy_ms=spread(copy[1:]),
             cluster_quality_wall_ms=spread(call_ms), silhouette_mean=float(np.nanmean(quality[lname]["silhouette"])))
    lname = f"cut{a.clusters}"
    lab = labs[lname]
    index = quality[lname].index
    baskets = [index[lab == g].tolist() for g in np.unique(lab)]
    try:
        band, sets_ms = wall(lambda: model.score_sets(baskets), 1)
        emit(what="sets", workload=name, n=n, storage=storage, labelling=lname, baskets=len(baskets),
             band_bytes=int(np.asarray(band).nbytes), wall_ms=round(sets_ms[0], 1))
        del band
    except ValueError as e:                                # (a limit of score_sets: reported, not worked around)
        emit(what="sets", workload=name, n=n, storage=storage, labelling=lname, baskets=len(baskets), refused=str(e)[:200])
    if a.parent and storage == "f32":
        from tests import groups_ref
        t0 = time.perf_counter()
        S = model.frame().to_numpy()
        frame_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        own, nearest, other = groups_ref.quality_fast(S, lab)
        host_ms = (time.perf_counter() - t0) * 1e3
        q = quality[lname]
        emit(what="parent", how="frame() + NumPy group-by on the host", workload=name, n=n, labelling=lname,
             frame_wall_ms=round(frame_ms, 1), host_wall_ms=round(host_ms, 1), host_bytes=int(S.nbytes),
             nearest_equal=float(np.mean(nearest == q["nearest"].to_numpy())),
             own_max_abs_diff=float(np.nanmax(np.abs(own - q["own"].to_numpy()))),
             other_max_abs_diff=float(np.nanmax(np.abs(other - q["other"].to_numpy()))))
        del S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pl32768d32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--clusters", type=int, default=500)
    ap.add_argument("--parent", action="store_true", help="also time frame() plus a host group-by (f32, host memory 2 N^2 x 8)")
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
