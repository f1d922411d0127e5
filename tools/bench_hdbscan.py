#!/usr/bin/env python3
"""core_similarity, linkage(min_samples=) and hdbscan (libsimrank_hdbscan.so) on compact f32 and fp16-held models at
BASELINE config 4 (N = 32768 power-law, mean degree 32), at min_samples 5 and 50.  Warm, medians and the spread
(min .. max) over --reps (HIP events); one JSON line per measurement on stdout, all of them also in --out.  Everything of
one storage is timed in the same run:

  what="copy"      a device copy of the matrix's bytes (reads them once, writes them once)
  what="degrees8"  one simrank_density_degrees sweep with 8 levels: the yardstick of a count sweep (the same bytes in the
                   same tile-pair shape)
  what="select"    per min_samples: the select as a whole (init, every count sweep and step, finish) and per count sweep;
                   the ratio of a count sweep to the degrees sweep and to the copy
  what="picks"     per min_samples: the clamped pick per round next to simrank_linkage_pick per round on the same
                   block (each its own Boruvka run: the rounds of both are reported), and their ratio
  what="hdbscan"   per min_samples: hdbscan() as a whole (wall clock), split into the device part (select and rounds, with
                   the 20 N bytes back) and the host part (the canonical table, the condensed tree and the selection);
                   clusters, noise and the largest cluster, for "eom" and "leaf"
  what="host"      the route it replaces (--host-n N, f32 only, a power-law graph of N nodes that fits the host): frame()
                   plus sklearn.cluster.HDBSCAN(metric="precomputed", cluster_selection_method="leaf") on
                   1 - max(S, S^T), against hdbscan(selection="leaf"): wall times, and how far the partitions agree
                   (adjusted Rand index over all nodes, and over the nodes neither calls noise).  Information, not a
                   check: ties are broken differently there

    python tools/bench_hdbscan.py [--workloads pl32768d32] [--reps 3] [--updates 3] [--min-cluster-size 5]
                                  [--host-n 8192] [--out profiles/bench_hdbscan.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simrank_amd.SimRank as SRA                                   # noqa: E402
from simrank_amd import _density, _hdbscan, _linkage, _model, synth  # noqa: E402
from simrank_amd._driver import Scratch                              # noqa: E402

LINES = []
MIN_SAMPLES = (5, 50)
HOST_MIN_SAMPLES = (2, 5, 50)                # of the comparison with scikit-learn


def emit(**row):
    LINES.append(row)
    print(json.dumps(row), flush=True)


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def select_stepwise(ops, b, n, rank):
    """The select entry by entry -> (core float64 [n], ms of every count sweep, ms of everything else)."""
    lib = _hdbscan.load()
    S, layout, stride = b["ptr"], b["layout"], b["stride"]
    core = np.empty(n, dtype=np.float64)
    counts, rest = [], 0.0
    with Scratch(ops) as scratch:
        prefix, remaining, hist = scratch.malloc(8 * n), scratch.malloc(4 * n), scratch.malloc(4 * _hdbscan.BINS * n)
        core64, core_cmp = scratch.malloc(8 * n), scratch.malloc(_hdbscan.cmp_bytes(layout) * n)
        rest += ops.timed(lambda: _hdbscan.check(lib.simrank_hdbscan_select_init(prefix, remaining, hist, n, rank, ops.stream), "init"))
        for p in range(_hdbscan.select_passes(layout)):
            counts.append(ops.timed(lambda: _hdbscan.check(lib.simrank_hdbscan_select_count(
                S, layout, stride, n, b.get("row_ids"), p, prefix, hist, ops.stream), "count")))
            rest += ops.timed(lambda: _hdbscan.check(lib.simrank_hdbscan_select_step(layout, p, prefix, remaining, hist, n,
                                                                                    ops.stream), "step"))
        rest += ops.timed(lambda: _hdbscan.check(lib.simrank_hdbscan_select_finish(layout, prefix, remaining, n, core64, core_cmp,
                                                                                  ops.stream), "finish"))
        ops.d2h(core, core64)
        ops.synchronize()
    return core, counts, rest


def summary(labels):
    sizes = np.bincount(labels[labels >= 0]) if (labels >= 0).any() else np.zeros(1, dtype=np.int64)
    return dict(clusters=int((sizes > 0).sum()), noise=int((labels < 0).sum()), largest=int(sizes.max()))


def measure(a, name, model, storage):
    solver = model._model[0]
    reader = solver._reader(0)
    ops, n = reader.ops, reader.n
    (b,) = reader.blocks
    nbytes = _model.block_bytes(b)
    spare = ops._malloc(nbytes)
    try:
        copy = [ops.timed(lambda: ops.copy_bytes(spare, b["ptr"], nbytes)) for _ in range(a.reps + 1)][1:]
    finally:
        ops.synchronize()
        ops._free(spare)
    copy_ms = statistics.median(copy)
    emit(what="copy", workload=name, n=n, storage=storage, matrix_bytes=nbytes, copy_ms=spread(copy),
         copy_gb_per_s=round(2 * nbytes / copy_ms / 1e6, 1))
    lo, hi = float(model.threshold_for(100 * n)[0]), float(model.threshold_for(10 * n)[0])
    ts = [hi, lo, (lo + hi) / 2, lo / 2, hi * 2, lo / 4, (3 * lo + hi) / 4, (lo + 3 * hi) / 4]
    d8 = []
    for _ in range(a.reps + 1):
        timing = {}
        _density.degrees_block(ops, b, n, ts, timing=timing)
        d8.append(timing["degrees_ms"])
    degrees_ms = statistics.median(d8[1:])
    emit(what="degrees8", workload=name, n=n, storage=storage, degrees_ms=spread(d8[1:]),
         degrees_over_copy=round(degrees_ms / copy_ms, 2))
    for m in MIN_SAMPLES:
        rank = m - 1
        whole, sweeps, others = [], [], []
        for _ in range(a.reps + 1):
            timing = {}
            core = _hdbscan.core_block(ops, b, n, rank, timing=timing)
            whole.append(timing["select_ms"])
            core2, counts, rest = select_stepwise(ops, b, n, rank)
            assert np.array_equal(core.view(np.uint64), core2.view(np.uint64))
            sweeps.append(counts)
            others.append(rest)
        per_sweep = [x for run in sweeps[1:] for x in run]
        sweep_ms = statistics.median(per_sweep)
        emit(what="select", workload=name, n=n, storage=storage, min_samples=m, passes=len(sweeps[0]),
             select_ms=spread(whole[1:]), count_sweep_ms=spread(per_sweep),
             count_sweep_by_pass_ms=[round(statistics.median(run[p] for run in sweeps[1:]), 4) for p in range(len(sweeps[0]))],
             steps_init_finish_ms=spread(others[1:]), count_over_degrees8=round(sweep_ms / degrees_ms, 2),
             count_over_copy=round(sweep_ms / copy_ms, 2), count_read_gb_per_s=round(nbytes / sweep_ms / 1e6, 1),
             core_finite=int(np.isfinite(core).sum()), core_median=float(np.median(core[np.isfinite(core)])))
        clamped, plain = [], []
        for _ in range(a.reps + 1):
            t1, t2 = {}, {}
            _, _, _, _, r1 = _hdbscan.forest_blocks(ops, b, [b], n, rank, None, timing=t1)
            _, _, _, r2 = _linkage.forest_blocks(ops, [b], n, None, timing=t2)
            clamped.append((t1["pick_ms"] / r1, r1))
            plain.append((t2["pick_ms"] / r2, r2))
        row = dict(what="picks", workload=name, n=n, storage=storage, min_samples=m,
                   clamped_pick_ms_per_round=spread([x for x, _ in clamped[1:]]), clamped_rounds=clamped[-1][1],
                   plain_pick_ms_per_round=spread([x for x, _ in plain[1:]]), plain_rounds=plain[-1][1])
        row["clamped_over_plain"] = round(row["clamped_pick_ms_per_round"]["median"] / row["plain_pick_ms_per_round"]["median"], 2)
        row["clamped_over_copy"] = round(row["clamped_pick_ms_per_round"]["median"] / copy_ms, 2)
        emit(**row)
        device, canon, condense, wall = [], [], [], []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            core, x, y, v, _ = _hdbscan.forest_blocks(ops, b, [b], n, rank, None)
            t1 = time.perf_counter()
            table = _linkage.canonical(n, x, y, v)
            t2 = time.perf_counter()
            _hdbscan.condense(n, *table, a.min_cluster_size, "eom", False)
            t3 = time.perf_counter()
            labels, clusters = model.hdbscan(a.min_cluster_size, m)
            t4 = time.perf_counter()
            device.append((t1 - t0) * 1e3)
            canon.append((t2 - t1) * 1e3)
            condense.append((t3 - t2) * 1e3)
            wall.append((t4 - t3) * 1e3)
        leaf, _ = model.hdbscan(a.min_cluster_size, m, selection="leaf")
        emit(what="hdbscan", workload=name, n=n, storage=storage, min_cluster_size=a.min_cluster_size, min_samples=m,
             hdbscan_wall_ms=spread(wall[1:]), device_wall_ms=spread(device[1:]), host_canonical_ms=spread(canon[1:]),
             host_condense_ms=spread(condense[1:]), table_rows=len(table[0]), condensed_clusters=len(clusters),
             eom=summary(labels["cluster"].to_numpy()), leaf=summary(leaf["cluster"].to_numpy()))


def host(a):
    """frame() + scikit-learn's HDBSCAN at an N the host holds, against hdbscan(selection="leaf")."""
    from sklearn.cluster import HDBSCAN
    from sklearn.metrics import adjusted_rand_score
    n = a.host_n
    df = synth.powerlaw_directed(n, 32, n, exact=True)
    model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True)
    try:
        model.compact()
        for m in HOST_MIN_SAMPLES:
            model.hdbscan(a.min_cluster_size, m, selection="leaf")           # warm
            t0 = time.perf_counter()
            ours, _ = model.hdbscan(a.min_cluster_size, m, selection="leaf")
            ours_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            S = model.frame().to_numpy()
            frame_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            D = 1.0 - np.fmax(S, S.T)
            np.fill_diagonal(D, 0.0)
            fit = HDBSCAN(min_cluster_size=a.min_cluster_size, min_samples=m, metric="precomputed",
                          cluster_selection_method="leaf").fit(D)
            host_ms = (time.perf_counter() - t0) * 1e3
            mine, theirs = ours["cluster"].to_numpy(), fit.labels_
            both = (mine >= 0) & (theirs >= 0)
            emit(what="host", how="frame() + sklearn.cluster.HDBSCAN(metric='precomputed', cluster_selection_method='leaf')",
                 n=len(S), min_cluster_size=a.min_cluster_size, min_samples=m, hdbscan_leaf_wall_ms=round(ours_ms, 1),
                 frame_wall_ms=round(frame_ms, 1), host_wall_ms=round(host_ms, 1), host_bytes=int(S.nbytes + D.nbytes),
                 ours=summary(mine), sklearn=summary(theirs), adjusted_rand_all=round(float(adjusted_rand_score(theirs, mine)), 4),
                 adjusted_rand_where_neither_is_noise=round(float(adjusted_rand_score(theirs[both], mine[both])), 4) if both.any() else None,
                 same_noise_flags=round(float(((mine < 0) == (theirs < 0)).mean()), 4))
            del S, D
    finally:
        model.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pl32768d32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--min-cluster-size", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=0, help="also time the route it replaces at this N (0: not)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:
        for name in [w for w in a.workloads.split(",") if w]:
            df = synth.WORKLOADS[name][0]()
            for storage in ("f32", "fp16"):
                model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True)
                try:
                    model.compact("fp16" if storage == "fp16" else None)
                    measure(a, name, model, storage)
                finally:
                    model.release()
        if a.host_n:
            host(a)
    finally:
        if a.out and LINES:
            with open(a.out, "w") as f:
                json.dump(LINES, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
