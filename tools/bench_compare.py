#!/usr/bin/env python3
"""model.compare (libsimrank_compare.so) at BASELINE config 4 (N = 32768 power-law, mean degree 32): a compact f32 model
against ``compact(precision="fp16")`` of the same fit, and against a second f32 fit with fewer iterations.  Warm, medians
and the spread (min .. max) over --reps (HIP events for the kernels, wall time for whole calls); one JSON line per
measurement on stdout, all of them also in --out:

  what="sweep"    per pair the sweep's milliseconds, next to a device-to-device copy whose read-plus-write traffic equals
                  the bytes the sweep reads (half of them copied), and the sweep's ratio to that copy; the milliseconds of
                  the two selections of top_k; the wall time of compare; the statistics themselves
  what="parent"   (--parent; host memory 2 x N^2 x 8 plus bands) the route the call replaces: two frame() calls over PCIe
                  plus tests/compare_ref.py in bands of rows, in the same run, and whether both routes give the same numbers

--workloads pl32768d32,pl65536 adds N = 65536 (config 5's graph) where memory allows: the three compact models are 17 GB
(f32) and 8.6 GB (fp16-held) each next to the plan of the fit in progress; --parent there needs 69 GB of host memory.

    python tools/bench_compare.py [--workloads pl32768d32] [--reps 5] [--updates 4] [--fewer 2] [--top-k 10] [--parent]
                                  [--out profiles/bench_compare.json]
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
from simrank_amd import _compare, _model, synth            # noqa: E402
from simrank_amd._driver import Scratch                   # noqa: E402

LINES = []
TOLERANCES = (1e-5, 1e-3)


def emit(**row):
    LINES.append(row)
    print(json.dumps(row), flush=True)


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def fit(df, updates, precision=None):
    model = SRA.SimRank().fit(df, verbose=False, iterations=updates, eps=0, keep=True)
    model.compact(precision)
    return model


def host_route(a, b, tolerances, floor, band=2048):
    """Two frame() calls plus the NumPy statement in bands of rows -> (frame seconds, NumPy seconds, the numbers)."""
    from tests import compare_ref
    t0 = time.perf_counter()
    SA, SB = a.frame().to_numpy(), b.frame().to_numpy()
    frames_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    tol = tuple(sorted(set(tolerances) | {0.0}))
    parts = [compare_ref.sweep(SA[r:r + band], SB[r:r + band], tol, floor) for r in range(0, len(SA), band)]
    max_abs, arg_abs, max_rel, arg_rel, over = (np.concatenate([p[i] for p in parts]) for i in range(5))
    hist = sum(p[5] for p in parts).astype(np.int64)
    return frames_s, time.perf_counter() - t0, (max_abs, arg_abs, max_rel, arg_rel, over.astype(np.int64), hist, tol)


def one_pair(a, name, pair, ma, mb):
    ra, rb = ma._model[0]._reader(0), mb._model[0]._reader(0)
    ops, n = ra.ops, ra.n
    (ba,), (bb,) = ra.blocks, rb.blocks
    read_bytes = _model.block_bytes(ba) + _model.block_bytes(bb)
    swept = tuple(sorted(set(TOLERANCES) | {0.0}))
    copy, sweep, select = [], [], []
    with Scratch(ops) as scratch:
        dst = scratch.malloc(read_bytes // 2)
        for _ in range(a.reps + 1):
            copy.append(ops.timed(lambda: ops.copy_bytes(dst, ba["ptr"], read_bytes // 2)))
    for _ in range(a.reps + 1):
        ms = []
        _compare.sweep_blocks(ops, ba, bb, swept, 0.0, timing=ms)
        sweep.append(sum(ms))
        ms = []
        _compare.select_ids(ra, a.top_k, timing=ms)
        _compare.select_ids(rb, a.top_k, timing=ms)
        select.append(sum(ms))
    wall = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        summary, nodes, histogram = ma.compare(mb, tolerances=TOLERANCES, top_k=a.top_k)
        wall.append((time.perf_counter() - t0) * 1e3)
    s = {k: summary[k].iloc[0] for k in summary.columns}       # (column by column: a row would turn the integers into floats)
    stats = {k: (float(v) if isinstance(v, (float, np.floating)) else int(v) if isinstance(v, (int, np.integer)) else str(v))
             for k, v in s.items()}
    filled = histogram[histogram > 0]
    emit(what="sweep", workload=name, pair=pair, n=n, read_bytes=read_bytes, sweep_ms=spread(sweep[1:]),
         copy_ms=spread(copy[1:]), sweep_over_copy=round(statistics.median(sweep[1:]) / statistics.median(copy[1:]), 3),
         select_ms=spread(select[1:]), compare_wall_ms=spread(wall[1:]), top_k=a.top_k, summary=stats,
         histogram={int(k): int(v) for k, v in filled.items()},
         largest_finite_exponent=int(max([e for e in filled.index if 0 < e < 2047], default=0)) - 1023)
    if a.parent:
        from tests import compare_ref
        frames_s, numpy_s, (max_abs, arg_abs, max_rel, arg_rel, over, hist, tol) = host_route(ma, mb, TOLERANCES, 0.0)
        index = nodes.index
        same = (np.array_equal(max_abs.view(np.uint64), nodes["max_abs"].to_numpy().view(np.uint64))
                and np.array_equal(max_rel.view(np.uint64), nodes["max_rel"].to_numpy().view(np.uint64))
                and np.array_equal(index.take(arg_abs).to_numpy(), nodes["at"].to_numpy())
                and np.array_equal(index.take(arg_rel).to_numpy(), nodes["at_rel"].to_numpy())
                and np.array_equal(over[:, tol.index(0.0)], nodes["differing"].to_numpy())
                and all(np.array_equal(over[:, tol.index(t)], nodes[f"over@{t!r}"].to_numpy()) for t in TOLERANCES)
                and np.array_equal(hist, histogram.to_numpy()))
        r, r2 = int(np.argmax(max_abs)), int(np.argmax(max_rel))
        same_summary = (float(s["max_abs"]) == max_abs[r] and s["node"] == index[r] and s["neighbor"] == index[arg_abs[r]]
                        and float(s["max_rel"]) == max_rel[r2] and s["node_rel"] == index[r2]
                        and s["neighbor_rel"] == index[arg_rel[r2]] and int(s["entries"]) == n * n
                        and int(s["differing"]) == int(over[:, tol.index(0.0)].sum())
                        and all(int(s[f"over@{t!r}"]) == int(over[:, tol.index(t)].sum()) for t in TOLERANCES))
        ids = [compare_ref.id_table(m.most_similar(list(index[:256]), a.top_k), index, a.top_k)[:256] for m in (ma, mb)]
        overlap, prefix = compare_ref.lists_agreement(*ids)
        same_lists = (np.array_equal(overlap, nodes["overlap"].to_numpy()[:256])
                      and np.array_equal(prefix, nodes["same_prefix"].to_numpy()[:256]))
        emit(what="parent", how="two frame() calls + NumPy in bands of rows", workload=name, pair=pair, n=n,
             frames_wall_s=round(frames_s, 2), numpy_wall_s=round(numpy_s, 2), host_bytes=2 * n * n * 8,
             same_numbers=bool(same), same_summary=bool(same_summary), same_lists_first_256_nodes=bool(same_lists))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pl32768d32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=4)
    ap.add_argument("--fewer", type=int, default=2)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--parent", action="store_true", help="also time two frame() calls plus NumPy (host memory 2 N^2 x 8)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name in [w for w in a.workloads.split(",") if w]:
        df = synth.WORKLOADS[name][0]()
        base = fit(df, a.updates)
        try:
            for pair, make in (("f32 | fp16-held", lambda: fit(df, a.updates, "fp16")),
                               (f"f32 {a.updates} updates | f32 {a.fewer} updates", lambda: fit(df, a.fewer))):
                other = make()
                try:
                    one_pair(a, name, pair, base, other)
                finally:
                    other.release()
        finally:
            base.release()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(LINES, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
