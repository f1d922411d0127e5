#!/usr/bin/env python3
"""rank_sets / rank_recommended: held-out ranks on a kept model (libsimrank_rank.so), against the two ways the same ranks
are obtained without it.

  N = 32768 SimRank, compact f32 and fp16-held; the baskets of recommend for the first 1024 nodes (their CSR rows with the
  fit's weights, the seen nodes excluded); 1, 16 and 256 random targets per basket.

Per point, warm, medians and the spread (min .. max) over --reps:
  score_ms / gather_ms / count_ms   the stages of the rank call alone (HIP events, `_sets.run`'s timing hook)
  call_ms        the whole device half (`score_ranks`: arrays in, three small arrays out)
  dense_ms       route 1: the dense score rows to the host (`score_sets(sets)`'s device half: n_sets x N float64 over PCIe)
  host_rank_ms   ... plus a vectorised NumPy count per basket on them, over the first --host baskets, scaled to all
  topk_n_ms      route 2: the selection with k = N (`score_sets(top_k=N)`'s device half), once; topk_2048_ms the same
                 with k = 2048, from which k = N is projected first and skipped above --topk-limit seconds
and whether the three routes gave the same ranks on the baskets all of them ranked.  One JSON line per point on stdout;
--out also writes the list to a file.

    python tools/bench_rank.py [--reps 5] [--updates 3] [--host 32] [--baskets 1024] [--no-topk] [--topk-limit 120] [--out FILE]
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
from simrank_amd import _rank, _sets, synth               # noqa: E402


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def wall(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def host_ranks(dense, excl, tptr, tids, first):
    """(ranks of the targets of the first ``first`` baskets, wall ms): the exclusion and one broadcast comparison per
    basket on the dense rows."""
    xp, xi = excl
    ids = np.arange(dense.shape[1])
    out = []
    t0 = time.perf_counter()
    for q in range(first):
        row = dense[q].copy()
        row[xi[xp[q]:xp[q + 1]]] = -np.inf
        t = tids[tptr[q]:tptr[q + 1]]
        s = row[t]
        cand = row > -np.inf
        before = (cand & ((row > s[:, None]) | ((row == s[:, None]) & (ids < t[:, None])))).sum(axis=1)
        out.append(np.where(s > -np.inf, before + 1, 0))
    ms = (time.perf_counter() - t0) * 1e3
    return (np.concatenate(out) if out else np.empty(0, dtype=np.int64)), ms


def topk_ranks(idx, tptr, tids, first):
    """The targets' ranks read off the k = N selection: the position of the target's id in its basket's row, 0 if absent."""
    out = []
    for q in range(first):
        place = np.zeros(idx.shape[1] + 1, dtype=np.int64)
        got = idx[q][idx[q] >= 0]
        place[got] = np.arange(1, got.size + 1)
        out.append(place[tids[tptr[q]:tptr[q + 1]]])
    return np.concatenate(out) if out else np.empty(0, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--host", type=int, default=32)
    ap.add_argument("--baskets", type=int, default=1024)
    ap.add_argument("--no-topk", action="store_true")
    ap.add_argument("--topk-limit", type=float, default=120.0, help="seconds the k = N selection may be projected to take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    df = synth.WORKLOADS["pl32768"][0]()
    model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True).compact()
    results = []
    for form in ("compact f32", "compact fp16-held"):
        if form != "compact f32":
            model.compact(precision="fp16")
        solver, sides = model._model
        reader = solver._reader(0)
        n = reader.n
        spec = solver.specs[0]
        nodes = np.arange(min(a.baskets, n))
        ptr, ids, w, excl = _sets.csr_baskets(spec.csr, spec.rowscale, nodes, True, True)
        n_sets = int(ptr.size - 1)
        first = min(a.host, n_sets)
        dense_ms = wall(lambda: _sets.run(reader, ptr, ids, w), max(2, a.reps // 2))
        dense = _sets.run(reader, ptr, ids, w)
        # route 2 sweeps a row once per pick: k = 2048 first, and k = N only when 16 x that stays below --topk-limit
        topk_ms = idx = None
        t = time.perf_counter()
        _sets.run(reader, ptr, ids, w, 2048, excl)
        topk_2048_ms = round((time.perf_counter() - t) * 1e3, 1)
        if not a.no_topk and topk_2048_ms * (n / 2048) <= a.topk_limit * 1e3:
            t = time.perf_counter()
            idx, _ = _sets.run(reader, ptr, ids, w, n, excl)
            topk_ms = round((time.perf_counter() - t) * 1e3, 1)
        rng = np.random.default_rng(4)
        for per in (1, 16, 256):
            tptr = np.arange(n_sets + 1, dtype=np.int64) * per
            tids = rng.integers(0, n, size=n_sets * per).astype(np.int32)
            stages = {"score_ms": [], "gather_ms": [], "count_ms": []}
            for i in range(a.reps + 1):
                t = {}
                score, before, _ = solver.score_ranks(0, ptr, ids, w, excl, tptr, tids, timing=t)
                if i:
                    for name in stages:
                        stages[name].append(t.get(name, 0.0))
            call = wall(lambda: solver.score_ranks(0, ptr, ids, w, excl, tptr, tids), a.reps)
            ranks = _rank.ranks_of(score, before)[:first * per]
            by_host, host_ms = host_ranks(dense, excl, tptr, tids, first)
            agree = bool(np.array_equal(ranks, by_host))
            if idx is not None:
                agree = agree and bool(np.array_equal(ranks, topk_ranks(idx, tptr, tids, first)))
            out = dict(model=form, n=n, baskets=n_sets, members=int(ids.size), targets_per_basket=per,
                       comparisons=int(n_sets) * per * n, call_ms=spread(call), dense_ms=spread(dense_ms),
                       host_rank_ms_scaled=round(host_ms * n_sets / max(1, first), 1), host_baskets_timed=first,
                       topk_n_ms=topk_ms, topk_2048_ms=topk_2048_ms, dense_bytes=8 * n_sets * n, rank_bytes=16 * n_sets * per + 8 * n_sets,
                       routes_agree=agree, **{name: spread(v) for name, v in stages.items()})
            out["count_ns_per_comparison"] = round(statistics.median(stages["count_ms"]) * 1e6 / out["comparisons"], 5)
            print(json.dumps(out), flush=True)
            results.append(out)
        del dense, idx
    model.release()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
