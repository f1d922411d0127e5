#!/usr/bin/env python3
"""``exemplars`` (libsimrank_exemplars.so) at BASELINE config 4 (N = 32768 power-law, mean degree 32) on a compact f32
model and an fp16-held one.  Warm; kernel times are medians and the spread (min .. max) over --reps timed windows of
--inner launches each (HIP events), the routes alternating window by window in the same run; loop times are host wall
clock around the whole call, medians over --loop-reps.  One JSON line per point on stdout, and all of them in --out
(profiles/bench_exemplars.json):

  what="sweep"     gains_ms:    one simrank_exemplars_gains call on every row, against the cover after --warm-picks picks
                   copy_ms:     a device-to-device copy of the bytes the sweep reads (N x N elements)
                   operator_ms: simrank_operator_apply at d = 1 on the same block (the ``matmul`` sweep)
                   listed_ms:   a gains call on --listed scattered rows
                   cover_ms:    one simrank_exemplars_cover call with one row
  what="loop"      exemplars(--k) plain and lazy at every BATCH of --batches: wall seconds, ``gains`` calls (rounds), rows
                   evaluated in all; ``same_as_plain``: picks, gains and raised counts equal plain mode's bit for bit
  what="route"     (compact-f32 only) the route the public methods allowed before: per pick ``rows()`` of every candidate
                   in bands of --band rows over PCIe and the NumPy statement of the gain on the host, for --route-k
                   picks; ``same_picks``: they are exemplars' first --route-k picks
  what="kmedoids"  ``kmedoids`` seeded with the --k exemplars against --k random seeds: iterations, the last objective,
                   the largest cluster, wall seconds
  what="summary"   which mode wins, and what was not measured

    python tools/bench_exemplars.py [--workload pl32768d32] [--k 500] [--batches 256,1024,4096] [--reps 5] [--inner 4]
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
import simrank_amd.SimRank as SRA                                          # noqa: E402
from simrank_amd import _exemplars, _operator, _query, synth               # noqa: E402
from simrank_amd._driver import Scratch                                    # noqa: E402
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


def sweep_point(a, model, tag, records):
    solver = model._model[0]
    with solver.one_block(0) as reader, Scratch(reader.ops) as scratch, _operator.Session(reader, 1) as session:
        (b,) = reader.blocks
        ops, n = reader.ops, reader.n
        ev = _exemplars.DeviceEvaluator(reader, scratch)
        _exemplars.greedy(ev, n, a.warm_picks, (), lazy=True)              # a cover that is not all zeros
        lib = _exemplars.load()
        block = (b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"])
        rng = np.random.default_rng(a.seed)
        listed = scratch.put(rng.permutation(n)[:a.listed].astype(np.int32))
        nbytes = n * n * ELEMENT_BYTES[b["layout"]]
        src, dst = scratch.malloc(nbytes), scratch.malloc(nbytes)
        spare_cover, word = scratch.put(np.zeros(n)), scratch.put(np.array([int(rng.integers(n)), 0], dtype=np.int32))
        session.put(np.ones((n, 1)))
        launches = {
            "gains_ms": lambda: _exemplars.check(lib.simrank_exemplars_gains(
                *block, None, n, ev.cover_dev, ev.gain_dev, ops.stream), "simrank_exemplars_gains"),
            "copy_ms": lambda: check(ops.lib.simrank_memcpy_d2d(C.c_void_p(dst), C.c_void_p(src), nbytes, ops.stream),
                                     "simrank_memcpy_d2d"),
            "operator_ms": lambda: session.apply(False, 1.0, 0.0),
            "listed_ms": lambda: _exemplars.check(lib.simrank_exemplars_gains(
                *block, listed, a.listed, ev.cover_dev, ev.gain_dev, ops.stream), "simrank_exemplars_gains"),
            "cover_ms": lambda: _exemplars.check(lib.simrank_exemplars_cover(
                *block, word, 1, spare_cover, word + 4, ops.stream), "simrank_exemplars_cover"),
        }
        ms = alternate(ops, launches, a.reps, a.inner)
        med = {name: statistics.median(v) for name, v in ms.items()}
        rec = dict(what="sweep", model=tag, n=n, layout=b["layout"], bytes_read=nbytes, warm_picks=a.warm_picks,
                   listed=a.listed, gains_over_copy=round(med["gains_ms"] / med["copy_ms"], 2),
                   gains_over_operator=round(med["gains_ms"] / med["operator_ms"], 2),
                   gains_gb_per_s=round(nbytes / med["gains_ms"] / 1e6, 1), **{name: spread(v) for name, v in ms.items()})
        records.append(rec)
        print(json.dumps(rec), flush=True)


def same(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
                and np.array_equal(a[2], b[2]))


def loop_points(a, model, tag, records):
    solver = model._model[0]
    n = solver._reader(0).n
    none = np.empty(0, dtype=np.int64)
    modes = [("plain", False, None)] + [("lazy", True, int(x)) for x in a.batches.split(",")]
    plain, default = None, _exemplars.BATCH
    try:
        for name, lazy, batch in modes:
            _exemplars.BATCH = default if batch is None else batch
            seconds, stats = [], {}
            for _ in range(a.loop_reps + 1):                               # (the first run is the warm-up)
                t0 = time.perf_counter()
                out = _exemplars.exemplars(solver, 0, a.k, none, lazy, stats)
                seconds.append(time.perf_counter() - t0)
            plain = out if plain is None else plain
            rec = dict(what="loop", model=tag, n=n, k=a.k, mode=name, batch=batch, seconds=spread(seconds[1:]),
                       rounds=int(stats["rounds"]), rows_evaluated=int(out[3].sum()),
                       rows_over_one_sweep=round(float(out[3].sum()) / n, 2), same_as_plain=same(out, plain))
            records.append(rec)
            print(json.dumps(rec), flush=True)
    finally:
        _exemplars.BATCH = default
    return plain


def route_point(a, model, tag, picks, records):
    """Greedy through the public methods alone: ``rows()`` of every candidate, in bands, for every pick."""
    index = model.frame().index if a.route_frame else None
    solver = model._model[0]
    reader = solver._reader(0)
    n = reader.n
    cover, out, got = np.zeros(n), np.zeros(n, dtype=bool), []
    t0 = time.perf_counter()
    for _ in range(a.route_k):
        gain = np.full(n, -1.0)
        for lo in range(0, n, a.band):
            ids = np.arange(lo, min(n, lo + a.band), dtype=np.int32)
            R = reader.rows(ids) if index is None else model.rows(index[ids]).to_numpy()
            gain[ids] = np.where(R > cover, R - cover, 0.0).sum(axis=1)
        gain[out] = -1.0
        c = int(np.argmax(gain))
        row = reader.rows(np.array([c], dtype=np.int32))[0]
        cover = np.where(row > cover, row, cover)
        out[c] = True
        got.append(c)
    seconds = time.perf_counter() - t0
    rec = dict(what="route", model=tag, n=n, k=a.route_k, band=a.band, seconds=round(seconds, 2),
               seconds_per_pick=round(seconds / a.route_k, 2), same_picks=bool(got == picks[0][:a.route_k].tolist()))
    records.append(rec)
    print(json.dumps(rec), flush=True)


def kmedoids_points(a, model, tag, picks, records):
    index = model.frame().index
    n = len(index)
    rng = np.random.default_rng(a.seed + 2)
    for name, seeds in (("exemplars", index[picks[0]]), ("random", index[rng.permutation(n)[:a.k]])):
        t0 = time.perf_counter()
        labels, clusters, history = model.kmedoids(list(seeds), max_iter=a.max_iter)
        seconds = time.perf_counter() - t0
        rec = dict(what="kmedoids", model=tag, n=n, k=a.k, seeds=name, iterations=len(history),
                   converged=bool(history["changed"].iloc[-1] == 0), first_objective=float(history["objective"].iloc[0]),
                   objective=float(history["objective"].iloc[-1]), largest_cluster=int(clusters["size"].max()),
                   singletons=int((clusters["size"] == 1).sum()), seconds=round(seconds, 2))
        records.append(rec)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="pl32768d32")
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--batches", default="256,1024,4096")
    ap.add_argument("--listed", type=int, default=1024)
    ap.add_argument("--warm-picks", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--route-k", type=int, default=2)
    ap.add_argument("--route-frame", action="store_true", help="go through model.rows(labels) instead of the reader")
    ap.add_argument("--band", type=int, default=1024)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "bench_exemplars.json"))
    a = ap.parse_args()
    df = synth.WORKLOADS[a.workload][0]()
    records = []
    for tag, precision in (("compact-f32", None), ("compact-fp16", "fp16")):
        model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True)
        try:
            model.compact() if precision is None else model.compact(precision=precision)
            sweep_point(a, model, tag, records)
            picks = loop_points(a, model, tag, records)
            if precision is None and a.route_k > 0:
                route_point(a, model, tag, picks, records)
            kmedoids_points(a, model, tag, picks, records)
        finally:
            model.release()
    loops = [r for r in records if r["what"] == "loop"]
    best = {tag: min((r for r in loops if r["model"] == tag), key=lambda r: r["seconds"]["median"])
            for tag in ("compact-f32", "compact-fp16")}
    summary = dict(what="summary", workload=a.workload, all_same=all(r["same_as_plain"] for r in loops),
                   fastest={tag: dict(mode=r["mode"], batch=r["batch"], seconds=r["seconds"]["median"]) for tag, r in best.items()},
                   lazy_wins=all(r["mode"] == "lazy" for r in best.values()),
                   not_measured=["N = 65536", "float64", "LocalWorld(P)", "pruned"])
    records.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
