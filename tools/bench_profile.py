#!/usr/bin/env python3
"""count_pairs / threshold_for (libsimrank_profile.so) on compact f32 and fp16-held models at BASELINE config 4 (N = 32768
power-law, mean degree 32) and at N = 65536 where memory allows.  Warm, medians and the spread (min .. max) over --reps
(HIP events); one JSON line per measurement on stdout, all of them also in --out:

  what="count"      one count sweep at 1, 32 and 1024 thresholds, with the ballot rounds and (SIMRANK_PROFILE_PLAIN=1)
                    without them; copy_ms: a device-to-device copy of the matrix's bytes in the same run, the floor of
                    anything that reads the matrix once -> count_over_copy
  what="digits"     every digit sweep of one threshold_for (per sweep, in order), both ways, and the call end to end
                    (wall time around work that ends synchronised)
  what="parent"     what a user does without these calls (--parent; f32 only): bisection of t with pairs(t, max_pairs=M)
                    until the bracket is 1e-6 relative, probes counted and timed; frame() + np.partition for the counts

    python tools/bench_profile.py [--workloads pl32768d32,pl65536] [--reps 5] [--updates 3] [--max-pairs 10000000]
                                  [--parent] [--out profiles/profile_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simrank_amd.SimRank as SRA                         # noqa: E402
from simrank_amd import _model, _profile, synth           # noqa: E402
from simrank_amd.engine import check                      # noqa: E402

LINES = []


def emit(**row):
    LINES.append(row)
    print(json.dumps(row), flush=True)


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def d2d_ms(ops, nbytes, reps):
    src, dst = ops._malloc(nbytes), ops._malloc(nbytes)
    try:
        copy = lambda: check(ops.lib.simrank_memcpy_d2d(C.c_void_p(dst), C.c_void_p(src), nbytes, ops.stream), "simrank_memcpy_d2d")
        return [ops.timed(copy) for _ in range(reps + 1)][1:]
    finally:
        ops._free(src), ops._free(dst)


def plain(on):
    if on:
        os.environ["SIMRANK_PROFILE_PLAIN"] = "1"
    else:
        os.environ.pop("SIMRANK_PROFILE_PLAIN", None)


def sweeps(a, name, model, storage):
    solver = model._model[0]
    reader = solver._reader(0)
    ops, n = reader.ops, reader.n
    nbytes = sum(_model.block_bytes(b) for b in reader.blocks)
    try:
        copy = d2d_ms(ops, nbytes, a.reps)
    except Exception as e:                                   # (no room for two more copies of the matrix)
        copy = None
        print(f"# no device-to-device yardstick at {name} {storage}: {e}", file=sys.stderr)
    rng = np.random.default_rng(0)
    for m in (1, 32, 1024):
        ts = np.sort(10.0 ** rng.uniform(-6, 0, size=m))
        row = dict(what="count", workload=name, n=n, storage=storage, thresholds=m, matrix_bytes=nbytes)
        for tag, off in (("ballot", False), ("plain", True)):
            plain(off)
            ms = []
            for _ in range(a.reps + 1):
                t = []
                counts = _profile.count_blocks(ops, reader.blocks, ts, timing=t)
                ms.append(sum(t))
            row[tag + "_ms"] = spread(ms[1:])
            row[tag + "_counts_head"] = counts[:3].tolist()
        plain(False)
        row["same_counts"] = row["ballot_counts_head"] == row["plain_counts_head"]
        if copy is not None:
            row["copy_ms"] = spread(copy)
            row["count_over_copy"] = round(row["ballot_ms"]["median"] / statistics.median(copy), 2)
        emit(**row)
    row = dict(what="digits", workload=name, n=n, storage=storage, max_pairs=a.max_pairs, matrix_bytes=nbytes)
    for tag, off in (("ballot", False), ("plain", True)):
        plain(off)
        per, wall = [], []
        for _ in range(a.reps + 1):
            t = []
            answer = _profile.threshold_blocks(ops, reader.blocks, a.max_pairs, timing=t)
            per.append(t)
            t0 = time.perf_counter()
            model.threshold_for(a.max_pairs)
            wall.append((time.perf_counter() - t0) * 1e3)
        row[tag + "_sweep_ms"] = [spread([p[i] for p in per[1:]]) for i in range(len(per[0]))]
        row[tag + "_end_to_end_ms"] = spread(wall[1:])
        row[tag + "_answer"] = [answer[0], answer[1]]
    plain(False)
    if copy is not None:
        row["copy_ms"] = spread(copy)
        row["first_sweep_over_copy"] = round(row["ballot_sweep_ms"][0]["median"] / statistics.median(copy), 2)
    emit(**row)
    return row["ballot_answer"]


def parent(a, name, model, answer):
    """Bisection with pairs() for the cut of --max-pairs, and frame() + np.partition for a count."""
    lo, hi, probes, t0 = 0.0, 1.0, 0, time.perf_counter()      # count(lo) > M >= count(hi): S lies in [0, 1] off the diagonal
    rows = None
    while hi - lo > 1e-6 * hi and probes < 60:
        mid = (lo + hi) / 2
        probes += 1
        try:
            rows = len(model.pairs(mid, max_pairs=a.max_pairs))
            hi = mid
        except ValueError:
            lo = mid
    bisect_ms = (time.perf_counter() - t0) * 1e3
    emit(what="parent", how="bisect pairs()", workload=name, max_pairs=a.max_pairs, probes=probes, wall_ms=round(bisect_ms, 1),
         t=hi, rows=rows, threshold_for=answer)
    t0 = time.perf_counter()
    S = model.frame().to_numpy()
    frame_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    np.fill_diagonal(S, -np.inf)
    flat = S.reshape(-1)
    kth = flat.size - a.max_pairs
    t = float(np.partition(flat, kth)[kth])
    part_ms = (time.perf_counter() - t0) * 1e3
    emit(what="parent", how="frame() + np.partition", workload=name, max_pairs=a.max_pairs, frame_wall_ms=round(frame_ms, 1),
         partition_wall_ms=round(part_ms, 1), host_bytes=int(S.nbytes), kth_value=t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pl32768d32,pl65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--max-pairs", type=int, default=10_000_000)
    ap.add_argument("--parent", action="store_true", help="also time what a user does without these calls (f32, host memory 2 N^2 x 8)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name in [w for w in a.workloads.split(",") if w]:
        df = synth.WORKLOADS[name][0]()
        for storage in ("f32", "fp16"):
            model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True)
            try:
                model.compact("fp16" if storage == "fp16" else None)
                answer = sweeps(a, name, model, storage)
                if a.parent and storage == "f32":
                    parent(a, name, model, answer)
            finally:
                model.release()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(LINES, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
