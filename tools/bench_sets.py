#!/usr/bin/env python3
"""score_sets / recommend: basket queries on a kept model (libsimrank_sets.so).

  config 3  MovieLens-shaped BipartiteSimRankPP (6040 x 3706), compact f32: recommend(users, 10, group=1) for 1024 and for
            all group-1 nodes; the score kernel in both grid orders
  config 4  N = 32768 SimRank, f32, kept and compact: 1024 baskets of 8, 32 and 128 random members, dense form and top-10

Per point, warm, medians and the spread (min .. max) over --reps:
  score_ms    the score kernels alone (HIP events), per grid order -> ns per source KiB
  topk_ms     the selection kernels alone
  copy_ms     a device-to-device copy of the bytes the score kernel reads, sum|set| x N x elem, in the SAME run
              (hipMemcpyDtoD of that many bytes, in pieces of at most 1 GiB)
  rows_kernel_ms  the `rows` kernel on the first 8192 of the same member ids (reads the same lines, writes 8 bytes per
              element), SAME run; compared per source KiB
  call_ms     the whole call (labels in, DataFrame out): top-10 and, at config 4, the dense form
  today_ms    today's route: model.rows(members) per basket plus the NumPy statement (weighted sum, exclusion, stable
              sort), over the first --today baskets, scaled to all of them
One JSON line per measurement on stdout.

    python tools/bench_sets.py [--configs 3,4] [--reps 5] [--updates 3] [--today 16]
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
from simrank_amd import _sets, synth                      # noqa: E402
from simrank_amd.engine import check                      # noqa: E402


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def wall(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def copy_ms(ops, nbytes, reps):
    """Milliseconds of device-to-device copies of ``nbytes`` in all (pieces of at most 1 GiB between two buffers)."""
    piece = int(min(nbytes, 1 << 30))
    src, dst = ops._malloc(piece + 16), ops._malloc(piece + 16)
    out = []
    try:
        for i in range(reps + 1):
            def go():
                left = nbytes
                while left > 0:
                    m = min(piece, left)
                    check(ops.lib.simrank_memcpy_d2d(C.c_void_p(dst), C.c_void_p(src), m, ops.stream), "simrank_memcpy_d2d")
                    left -= m
            ms = ops.timed(go)
            if i:
                out.append(ms)
    finally:
        ops._free(src), ops._free(dst)
    return out


def kernels(reader, ptr, ids, w, k, excl, order, reps):
    score, topk = [], []
    for i in range(reps + 1):
        t = {}
        _sets.run(reader, ptr, ids, w, k, excl, timing=t, grid_order=order)
        if i:
            score.append(t.get("score_ms", 0.0)), topk.append(t.get("topk_ms", 0.0))
    return score, topk


ROWS_SAMPLE = 8192       # member ids the `rows` kernel is timed on (its output, 8 bytes per element, has to fit somewhere)


def rows_kernel(reader, ids, reps):
    """The `rows` kernel on the first ``ROWS_SAMPLE`` member ids, in pieces of 1024 (HIP events)."""
    ids = ids[:ROWS_SAMPLE]
    out = []
    for i in range(reps + 1):
        ms = []
        for at in range(0, ids.size, 1024):
            got = reader.rows(ids[at:at + 1024], timing=ms)
            del got
        if i:
            out.append(sum(ms))
    return out


def today(model, frame_labels, sets, weights, excluded, k, n_first, **kw):
    """Wall ms per basket of rows() + the NumPy statement + a stable sort, over the first ``n_first`` baskets."""
    at = {lab: i for i, lab in enumerate(frame_labels)}
    t = time.perf_counter()
    for s, w, x in list(zip(sets, weights, excluded))[:n_first]:
        if not len(s):
            continue
        rows = model.rows(s, **kw).values
        acc = np.zeros(rows.shape[1])
        for e in range(rows.shape[0]):
            acc = acc + (w[e] * rows[e])
        acc[[at[v] for v in x]] = -np.inf
        np.argsort(-acc, kind="stable")[:k]
    return (time.perf_counter() - t) * 1e3 / max(1, min(n_first, len(sets)))


def point(tag, model, solver, side, read_side, ptr, ids, w, excl, reps, elem, extra):
    reader = solver._reader(read_side)
    n = reader.n
    src = int(ids.size) * n * elem
    out = dict(tag, n=n, baskets=int(ptr.size - 1), members=int(ids.size), source_bytes=src)
    for name, order in (("basket_major", _sets.BASKET_MAJOR), ("chunk_label", _sets.CHUNK_LABEL)):
        score, topk = kernels(reader, ptr, ids, w, 10, excl, order, reps)
        out["score_ms_" + name] = spread(score)
        out["score_ns_per_kib_" + name] = round(statistics.median(score) * 1e6 / (src / 1024), 4)
        out["topk_ms"] = spread(topk)
    rk = rows_kernel(reader, ids, reps)
    cp = copy_ms(reader.ops, src, reps)
    rows_src = min(int(ids.size), ROWS_SAMPLE) * n * elem
    out.update(rows_kernel_ms=spread(rk), rows_members=min(int(ids.size), ROWS_SAMPLE),
               rows_ns_per_kib=round(statistics.median(rk) * 1e6 / (rows_src / 1024), 4),
               rows_ns_per_kib_min_max=[round(min(rk) * 1e6 / (rows_src / 1024), 4), round(max(rk) * 1e6 / (rows_src / 1024), 4)],
               copy_ms=spread(cp), copy_ns_per_kib=round(statistics.median(cp) * 1e6 / (src / 1024), 4), **extra)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--today", type=int, default=16)
    a = ap.parse_args()
    configs = [int(c) for c in a.configs.split(",")]
    if 3 in configs:
        df = synth.WORKLOADS["ml1m"][0]()
        model = SRA.BipartiteSimRankPP().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True,
                                             strict_reference=False).compact()
        solver, sides = model._model
        users, items = sides[0][1], sides[1][1]
        spec = solver.specs[0]
        for n_u in (1024, len(users)):
            nodes = users[:n_u]
            u = np.arange(n_u)
            ptr, ids, w, excl = _sets.csr_baskets(spec.csr, spec.rowscale, u, False, True)
            model.recommend(nodes, 10, group=1)
            call = wall(lambda: model.recommend(nodes, 10, group=1), a.reps)
            rowptr, col = np.asarray(spec.csr.rowptr), np.asarray(spec.csr.col)
            sets = [[items[c] for c in col[rowptr[x]:rowptr[x + 1]]] for x in u[:a.today]]
            weights = [[spec.rowscale[x]] * len(s) for x, s in zip(u, sets)]
            per = today(model, items, sets, weights, sets, 10, a.today, group=2)
            point(dict(config=3, model="compact f32", what="recommend(k=10, group=1)"), model, solver, 0, 1, ptr, ids, w, excl,
                  a.reps, 4, dict(call_top10_ms=spread(call), today_ms_per_basket=round(per, 3),
                                  today_ms_scaled=round(per * n_u, 1), today_baskets_timed=min(a.today, n_u)))
        model.release()
    if 4 in configs:
        df = synth.WORKLOADS["pl32768"][0]()
        for form in ("kept", "compact"):
            model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True)
            if form == "compact":
                model.compact()
            solver, sides = model._model
            labels = sides[0][1]
            n = len(labels)
            rng = np.random.default_rng(4)
            for m in (8, 32, 128):
                lists = [rng.integers(0, n, size=m).astype(np.int32) for _ in range(1024)]
                ptr, ids = _sets.join(lists)
                w = rng.normal(size=ids.size)
                sets = [[labels[i] for i in l] for l in lists]
                weights = [list(w[ptr[q]:ptr[q + 1]]) for q in range(1024)]
                model.score_sets(sets[:4], weights=weights[:4], top_k=10)
                top = wall(lambda: model.score_sets(sets, weights=weights, top_k=10), a.reps)
                dense = wall(lambda: model.score_sets(sets, weights=weights), max(2, a.reps // 2))
                per = today(model, labels, sets, weights, sets, 10, a.today)
                point(dict(config=4, model=form + " f32", what="score_sets, %d members" % m), model, solver, 0, 0, ptr, ids, w,
                      (ptr, ids), a.reps, 4, dict(call_top10_ms=spread(top), call_dense_ms=spread(dense),
                                                  today_ms_per_basket=round(per, 3), today_ms_scaled=round(per * 1024, 1),
                                                  today_baskets_timed=a.today))
            model.release()


if __name__ == "__main__":
    main()
