#!/usr/bin/env python3
"""degrees and dbscan (libsimrank_density.so) on compact f32 and fp16-held models at BASELINE config 4 (N = 32768
power-law, mean degree 32).  Warm, medians and the spread (min .. max) over --reps (HIP events); one JSON line per
measurement on stdout, all of them also in --out:

  what="copy"      a device copy of the matrix's bytes (reads them once, writes them once): the yardstick of a sweep
  what="sweeps"    per level (threshold_for(10 N), threshold_for(100 N)): the degrees sweep with 1 level; the union sweep
                   and the labels call of dbscan(t, --min-samples); simrank_cluster_union at the same level in the same
                   run (the other yardstick); dbscan as a whole (wall clock of the method: the three sweeps, 8 N bytes
                   back, the numbering); clusters / border nodes / noise nodes found; the ratios to the copy
  what="degrees8"  the degrees sweep with 8 levels at once (the two levels and six between and around them)
  what="host"      the route the methods replace (--host; f32 only): frame() (the N x N float64 hand-back) plus the host:
                   the OR-symmetrised graph as a sparse matrix, then scikit-learn's DBSCAN(metric="precomputed") on it
                   where it imports, tests/density_ref.py where not; wall times; checked to give the same core flags and
                   the same partition of the core nodes as dbscan

    python tools/bench_density.py [--workloads pl32768d32] [--reps 5] [--updates 3] [--min-samples 5] [--host]
                                  [--out profiles/bench_density.json]
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
from simrank_amd import _cluster, _density, _model, synth  # noqa: E402

LINES = []


def emit(**row):
    LINES.append(row)
    print(json.dumps(row), flush=True)


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def repeat(reps, run):
    """``run(timing)`` once to warm up and ``reps`` times more: (the last result, the timing dicts of the timed runs)."""
    out, got = [], None
    for _ in range(reps + 1):
        timing = {}
        got = run(timing)
        out.append(timing)
    return got, out[1:]


def first_member(labels):
    """Per node the first node with its label: equal arrays = the same partition."""
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    return first[inverse.reshape(-1)]


def sweeps(a, name, model, storage):
    reader = model._model[0]._reader(0)
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
    levels = [("threshold_for(10 N)", model.threshold_for(10 * n)[0]), ("threshold_for(100 N)", model.threshold_for(100 * n)[0])]
    levels = [(tag, float(t)) for tag, t in levels if np.isfinite(t)]
    found = {}
    for tag, t in levels:
        deg, d1 = repeat(a.reps, lambda timing: _density.degrees_block(ops, b, n, [t], timing=timing))
        (_, roots), db = repeat(a.reps, lambda timing: _density.dbscan_blocks(ops, b, [b], n, t, a.min_samples - 1, timing=timing))
        _, cl = repeat(a.reps, lambda timing: _cluster.roots_blocks(ops, [b], n, [t], timing=timing))
        wall = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            frame = model.dbscan(t, a.min_samples)
            wall.append((time.perf_counter() - t0) * 1e3)
        core = frame["core"].to_numpy()
        assert np.array_equal(frame["neighbors"].to_numpy(), deg[0]) and np.array_equal(roots >= 0, frame["cluster"].to_numpy() >= 0)
        found[t] = frame
        row = dict(what="sweeps", workload=name, n=n, storage=storage, level=tag, t=t, min_samples=a.min_samples,
                   matrix_bytes=nbytes, neighbour_pairs=int(deg[0].sum()) // 2, core=int(core.sum()),
                   clusters=int(frame["cluster"].max()) + 1, border=int(((frame["cluster"] >= 0) & ~frame["core"]).sum()),
                   noise=int((frame["cluster"] < 0).sum()),
                   degrees_ms=spread([x["degrees_ms"] for x in d1]), union_ms=spread([x["union_ms"] for x in db]),
                   labels_ms=spread([x["labels_ms"] for x in db]), cluster_union_ms=spread([x["union_ms"] for x in cl]),
                   dbscan_wall_ms=spread(wall[1:]))
        row["degrees_over_copy"] = round(row["degrees_ms"]["median"] / copy_ms, 2)
        row["union_over_copy"] = round(row["union_ms"]["median"] / copy_ms, 2)
        row["union_over_cluster_union"] = round(row["union_ms"]["median"] / row["cluster_union_ms"]["median"], 2)
        row["degrees_read_gb_per_s"] = round(nbytes / row["degrees_ms"]["median"] / 1e6, 1)
        emit(**row)
    if levels:
        lo, hi = sorted(t for _, t in levels)
        ts = [hi, lo, (lo + hi) / 2, lo / 2, hi * 2, lo / 4, (3 * lo + hi) / 4, (lo + 3 * hi) / 4]
        _, d8 = repeat(a.reps, lambda timing: _density.degrees_block(ops, b, n, ts, timing=timing))
        ms = spread([x["degrees_ms"] for x in d8])
        emit(what="degrees8", workload=name, n=n, storage=storage, t=ts, matrix_bytes=nbytes, degrees_ms=ms,
             degrees_over_copy=round(ms["median"] / copy_ms, 2))
    return levels, found


def host_dbscan(S, t, min_samples):
    """(how, core bool [n], labels [n]) on the host from the dense float64 matrix."""
    from scipy import sparse
    n = len(S)
    hit = S >= t
    hit |= hit.T
    np.fill_diagonal(hit, True)                             # (a stored 0 on the diagonal: the node counts itself)
    graph = sparse.csr_matrix(hit)
    del hit
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        from tests import density_ref
        dense = graph.toarray()
        np.fill_diagonal(dense, False)
        cluster, core, _, _ = density_ref.dbscan_of_graph(dense, min_samples)
        return "tests/density_ref.py", core, cluster
    dist = graph.astype(np.float64) * 0.25                  # every neighbour at distance 0.25 <= eps = 0.5
    fit = DBSCAN(eps=0.5, min_samples=min_samples, metric="precomputed").fit(dist)
    core = np.zeros(n, dtype=bool)
    core[fit.core_sample_indices_] = True
    return "scikit-learn DBSCAN(metric='precomputed') on the sparse graph", core, fit.labels_


def host(a, name, model, levels, found):
    for tag, t in levels:
        t0 = time.perf_counter()
        S = model.frame().to_numpy()
        frame_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        how, core, labels = host_dbscan(S, t, a.min_samples)
        host_ms = (time.perf_counter() - t0) * 1e3
        ours = found[t]
        same_core = bool(np.array_equal(core, ours["core"].to_numpy()))
        same_partition = bool(np.array_equal(first_member(labels[core]), first_member(ours["cluster"].to_numpy()[core])))
        same_noise = bool(np.array_equal(labels < 0, ours["cluster"].to_numpy() < 0))
        emit(what="host", how="frame() + " + how, workload=name, level=tag, t=t, min_samples=a.min_samples,
             frame_wall_ms=round(frame_ms, 1), host_wall_ms=round(host_ms, 1), host_bytes=int(S.nbytes), same_core_flags=same_core,
             same_partition_of_the_core_nodes=same_partition, same_noise=same_noise)
        assert same_core and same_partition and same_noise
        del S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pl32768d32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--min-samples", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="also time the route the methods replace (f32, host memory N^2 x 8 and more)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:
        for name in [w for w in a.workloads.split(",") if w]:
            df = synth.WORKLOADS[name][0]()
            for storage in ("f32", "fp16"):
                model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True)
                try:
                    model.compact("fp16" if storage == "fp16" else None)
                    levels, found = sweeps(a, name, model, storage)
                    if a.host and storage == "f32":
                        host(a, name, model, levels, found)
                finally:
                    model.release()
    finally:
        if a.out and LINES:
            with open(a.out, "w") as f:
                json.dump(LINES, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
