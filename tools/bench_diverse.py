#!/usr/bin/env python3
"""score_sets / recommend with diversity= : greedy maximal-marginal-relevance picks on a kept model
(libsimrank_diverse.so), against the plain selection and against the route it replaces.

  N = 32768 SimRank, compact f32 and fp16-held; the baskets of recommend for the first 1024 nodes (their CSR rows with the
  fit's weights, the seen nodes excluded); k = 10, d = 0.3.

Per model, warm, medians and the spread (min .. max) over --reps:
  pick_ms        (a) the pick kernel alone (HIP events, `_sets.run`'s timing hook), and score_ms of the same call
  topk_ms        (b) `simrank_sets_topk` on the same band with the same k (`score_sets(top_k=k)`'s selection), in this run
  copy_ms        (c) a device copy that moves the bytes the pick kernel moves by its own count (`moved_bytes`: per
                 candidate and sweep the score, the pen and the row element read; the pen store is counted apart as
                 `pen_store_bytes_at_most`, it happens only where a pen rose), scaled from a copy of --copy-mib MiB
  call_ms        the whole device half (`score_diverse`: arrays in, k x 28 bytes per basket out)
  host_ms        (d) the route it replaces on the first --host baskets: the dense score rows over PCIe, `rows(pick)` per
                 pick, NumPy; scaled to all baskets; `routes_agree`: it gave the same four arrays bit for bit
One JSON line per model on stdout; --out also writes the list to a file.

    python tools/bench_diverse.py [--reps 5] [--updates 3] [--host 64] [--baskets 1024] [--k 10] [--d 0.3] [--out FILE]
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
from simrank_amd import _sets, synth                      # noqa: E402


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def wall(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def host_route(reader, ptr, ids, w, excl, k, d, first):
    """The picks of the first ``first`` baskets the way a caller without the library gets them -> ((idx, score, pen,
    value) [first, k], wall ms)."""
    t0 = time.perf_counter()
    sub = ptr[:first + 1]
    dense = _sets.run(reader, sub, ids[:sub[-1]], w[:sub[-1]])
    xp, xi = excl
    rel_w = 1.0 - d
    idx = np.full((first, k), -1, dtype=np.int32)
    score, pen_out, val = (np.zeros((first, k)) for _ in range(3))
    for q in range(first):
        s = dense[q].copy()
        s[xi[xp[q]:xp[q + 1]]] = -np.inf
        live = ~np.isnan(s) & (s != -np.inf)
        pen = np.zeros(s.size)
        for t in range(k):
            with np.errstate(invalid="ignore"):
                v = (rel_w * s) - (d * pen)
            cand = np.flatnonzero(live & ~np.isnan(v))
            if not cand.size:
                break
            b = int(cand[np.argmax(v[cand] + 0.0)])
            idx[q, t], score[q, t], pen_out[q, t], val[q, t] = b, s[b], pen[b], v[b]
            live[b] = False
            x = reader.rows(np.array([b], dtype=np.int32))[0]
            pen = np.where(x > pen, x, pen)
    return (idx, score, pen_out, val), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--host", type=int, default=64)
    ap.add_argument("--baskets", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--d", type=float, default=0.3)
    ap.add_argument("--copy-mib", type=int, default=1024)
    ap.add_argument("--workload", default="pl32768")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    df = synth.WORKLOADS[a.workload][0]()
    model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True).compact()
    results = []
    for form, elem in (("compact f32", 4), ("compact fp16-held", 2)):
        if form != "compact f32":
            model.compact(precision="fp16")
        solver, sides = model._model
        reader = solver._reader(0)
        ops, n = reader.ops, reader.n
        spec = solver.specs[0]
        nodes = np.arange(min(a.baskets, n))
        ptr, ids, w, excl = _sets.csr_baskets(spec.csr, spec.rowscale, nodes, True, True)
        n_sets = int(ptr.size - 1)
        k = min(a.k, n)
        stages = {"score_ms": [], "pick_ms": []}
        for i in range(a.reps + 1):                                        # (the first turn warms up)
            t = {}
            got = solver.score_diverse(0, ptr, ids, w, k, excl, a.d, timing=t)
            if i:
                for name in stages:
                    stages[name].append(t.get(name, 0.0))
        call = wall(lambda: solver.score_diverse(0, ptr, ids, w, k, excl, a.d), a.reps)
        plain = {"score_ms": [], "topk_ms": []}
        for i in range(a.reps + 1):
            t = {}
            top = _sets.run(reader, ptr, ids, w, k, excl, timing=t)
            if i:
                for name in plain:
                    plain[name].append(t.get(name, 0.0))
        plain_call = wall(lambda: _sets.run(reader, ptr, ids, w, k, excl), a.reps)
        picks = (got[0] >= 0).sum(axis=1)
        sweeps = int(picks.sum() + (picks < k).sum())                      # (a basket that runs dry sweeps once more to see it)
        pen = 4                                                            # (f32 and fp16-held blocks keep their pens as f32)
        moved = sweeps * n * (8 + pen + elem)                              # score, pen and row element per candidate and sweep
        copy_bytes = a.copy_mib << 20
        src, dst = ops._malloc(copy_bytes), ops._malloc(copy_bytes)
        try:
            copies = [ops.timed(lambda: ops.copy_bytes(dst, src, copy_bytes)) for _ in range(a.reps + 1)][1:]
        finally:
            ops.synchronize()
            ops._free(src)
            ops._free(dst)
        copy_gbs = 2 * copy_bytes / (statistics.median(copies) * 1e-3) / 1e9   # (a copy reads and writes every byte)
        first = min(a.host, n_sets)
        by_host, host_ms = host_route(reader, ptr, ids, w, excl, k, a.d, first)
        agree = all(np.array_equal(np.ascontiguousarray(g[:first]).view(np.uint8), np.ascontiguousarray(h).view(np.uint8))
                    for g, h in zip(got, by_host))
        pick = statistics.median(stages["pick_ms"])
        out = dict(model=form, n=n, baskets=n_sets, members=int(ids.size), k=k, d=a.d, sweeps=sweeps,
                   pick_ms=spread(stages["pick_ms"]), score_ms=spread(stages["score_ms"]), call_ms=spread(call),
                   topk_ms=spread(plain["topk_ms"]), plain_score_ms=spread(plain["score_ms"]), plain_call_ms=spread(plain_call),
                   moved_bytes=moved, pen_store_bytes_at_most=sweeps * n * pen,
                   pick_gbs=round(moved / (pick * 1e-3) / 1e9, 1), copy_gbs=round(copy_gbs, 1),
                   copy_ms=round(moved / copy_gbs / 1e6, 3), host_ms_scaled=round(host_ms * n_sets / max(1, first), 1),
                   host_baskets_timed=first, routes_agree=bool(agree), differs_from_plain=int((got[0] != top[0]).sum()),
                   picks_with_penalty=int((got[2] > 0).sum()))
        out["pick_over_topk"] = round(pick / statistics.median(plain["topk_ms"]), 3)
        out["pick_over_copy"] = round(pick / out["copy_ms"], 3)
        print(json.dumps(out), flush=True)
        results.append(out)
    model.release()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
