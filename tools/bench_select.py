#!/usr/bin/env python3
"""fit(min_similarity=t): the two passes of libsimrank_select.so at BASELINE config 4 (N = 32768, SimRank, f32) and
config 5 (N = 65536, SimRank++, f32 and fp16-held), on the C plan's own iterate.

Per configuration: the count-pass and emit-pass times from HIP events on the plan's stream (best of --reps), the bytes
each pass reads (the whole block of the iterate: N^2 x 4 or x 2 bytes) over that time, next to the measured copy rate
of DESIGN.md (6.29 TB/s, float4 copy), and the pairs found.  At config 4 also the wall time of fit(min_similarity=t)
next to fit().  One JSON line per measurement on stdout.

    python tools/bench_select.py [--configs 4,5] [--reps 5] [--updates 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simrank_amd import ingest, synth                     # noqa: E402
from simrank_amd.engine import HipOps, Plan               # noqa: E402

COPY_TBS = 6.29          # MI355X_MICROARCH / DESIGN: float4 copy, measured


def threshold_for(plan, n, quantile):
    """A threshold at this quantile of the off-diagonal values of 64 sampled rows."""
    rows = np.random.default_rng(1).choice(n, 64, replace=False)
    R = plan.rows(rows).astype(np.float64)
    R[np.arange(rows.size), rows] = 0
    return float(np.quantile(R[R > 0], quantile))


def passes(name, ops, plan, n, storage, reps, quantile):
    t = threshold_for(plan, n, quantile)
    best_c, best_e, total = float("inf"), float("inf"), 0
    for i in range(reps + 1):                            # (the first is a warm-up)
        sel = plan.selection(t, timing=True)
        sel.emit()
        if i:
            best_c, best_e = min(best_c, sel.count_ms), min(best_e, sel.emit_ms)
        total = sel.total
    nbytes = n * n * (2 if storage == "fp16" else 4)
    out = dict(config=name, storage=storage, n=n, t=t, pairs=total, bytes_read_per_pass=nbytes,
               count_ms=round(best_c, 4), emit_ms=round(best_e, 4),
               count_tbs=round(nbytes / best_c / 1e9, 3), emit_tbs=round(nbytes / best_e / 1e9, 3),
               copy_tbs=COPY_TBS, count_share_of_copy=round(nbytes / best_c / 1e9 / COPY_TBS, 3),
               emit_share_of_copy=round(nbytes / best_e / 1e9 / COPY_TBS, 3))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4,5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--quantile", type=float, default=0.999)
    ap.add_argument("--no-fit", action="store_true", help="skip the fit() wall-time comparison at config 4")
    a = ap.parse_args()
    ops = HipOps(0)
    configs = a.configs.split(",")
    if "4" in configs:
        df = synth.WORKLOADS["pl32768"][0]()
        _, csr = ingest.directed(df, False, "from", "to", "weight")
        plan = Plan(ops, csr, coef=0.8)
        plan.run(a.updates, 0.0)
        passes("4", ops, plan, csr.n_rows, "f32", a.reps, a.quantile)
        t = threshold_for(plan, csr.n_rows, a.quantile)
        plan.free()
        if not a.no_fit:
            import simrank_amd.SimRank as SRA
            SRA.SimRank().fit(df, verbose=False, iterations=2)              # warm-up: code objects, pools
            for kw in ({}, {"min_similarity": t}):
                t0 = time.perf_counter()
                res = SRA.SimRank().fit(df, verbose=False, **kw)
                wall = time.perf_counter() - t0
                print(json.dumps(dict(config="4", fit=("min_similarity" if kw else "dense"), t=kw.get("min_similarity"),
                                      wall_s=round(wall, 3), rows=int(len(res)))), flush=True)
                del res
    if "5" in configs:
        df = synth.WORKLOADS["pl65536"][0]()
        _, csr = ingest.directed(df, False, "from", "to", "weight")
        scale = ingest.spread(csr) * csr.rowscale
        for storage in ("f32", "fp16"):
            plan = Plan(ops, csr, scale, coef=0.8, evidence=True, storage=storage)
            plan.run(a.updates, 0.0)
            passes("5", ops, plan, csr.n_rows, storage, a.reps, a.quantile)
            plan.free()
    ops.close()


if __name__ == "__main__":
    main()
