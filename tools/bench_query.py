#!/usr/bin/env python3
"""fit(keep=True): node queries on a kept model (libsimrank_query.so) at BASELINE config 4 (N = 32768, SimRank) and
config 5 (N = 65536, SimRank++), f32 and fp16-held, for |Q| random nodes.

Per (config, storage, |Q|), warm, medians and the spread (min .. max) over --reps:
  kernel_ms   the `rows` kernels alone (HIP events on the engine's stream)
  copy_ms     a device-to-device copy of the bytes that kernel must read plus write, |Q| x N x (4 or 2 + 8), in the
              SAME run (hipMemcpyDtoD of half of them: a copy reads and writes each byte) -> kernel_share_of_copy
  rows_ms     `rows` end to end (labels in, DataFrame out); rows_minor_faults = the host pages first touched per call
  d2h_ms      a plain device-to-host copy of |Q| x N x 8 bytes into the same kind of host block, in the SAME run
              -> rows_over_d2h
  top10_ms    `most_similar(Q, 10)` end to end
and at config 4 the wall time of fit(keep=True) (the first answer is that plus rows_ms) next to a plain fit() with its
dense hand-back.  One JSON line per measurement on stdout.

    python tools/bench_query.py [--configs 4,5] [--storages f32,fp16] [--q 1,64,1024,16384] [--reps 5] [--updates 3]
"""
import argparse
import ctypes as C
import json
import os
import resource
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simrank_amd.SimRank as SRA                         # noqa: E402
from simrank_amd import _query, hostpool, synth           # noqa: E402
from simrank_amd.engine import check                      # noqa: E402

CONFIGS = {4: ("pl32768", "SimRank"), 5: ("pl65536", "SimRankPP")}


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def wall(fn, reps, faults=None):
    """Wall milliseconds of ``reps`` calls; ``faults`` receives each call's minor page faults (first touches of host pages)."""
    out = []
    for _ in range(reps):
        f0 = resource.getrusage(resource.RUSAGE_SELF).ru_minflt
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
        if faults is not None:
            faults.append(resource.getrusage(resource.RUSAGE_SELF).ru_minflt - f0)
    return out


def device_copies(ops, n_q, n, elem, reps):
    """(d2d ms list, d2h ms list): the copy of the rows kernel's bytes, and |Q| x N x 8 bytes to the host."""
    moved = n_q * n * (elem + 8)
    src, dst = ops._malloc(moved // 2 + 16), ops._malloc(moved // 2 + 16)
    host = hostpool.empty_f64(n_q, n)
    host[:] = 0                                           # (pages touched, as a recycled frame's are)
    d2d, d2h = [], []
    try:
        for i in range(reps + 1):
            a, b = ops.event(), ops.event()
            ops.record(a)
            check(ops.lib.simrank_memcpy_d2d(C.c_void_p(dst), C.c_void_p(src), moved // 2, ops.stream), "simrank_memcpy_d2d")
            ops.record(b)
            ops.event_synchronize(b)
            if i:
                d2d.append(ops.elapsed_ms(a, b))
            ops.event_destroy(a), ops.event_destroy(b)
            band = min(n_q * n * 8, moved // 2)
            t = time.perf_counter()
            for off in range(0, n_q * n * 8, band):
                m = min(band, n_q * n * 8 - off)
                check(ops.lib.simrank_memcpy_d2h(host.ctypes.data + off, C.c_void_p(src), m, ops.stream), "simrank_memcpy_d2h")
            ops.synchronize()
            if i:
                d2h.append((time.perf_counter() - t) * 1e3)
    finally:
        ops._free(src), ops._free(dst)
    return d2d, d2h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4,5")
    ap.add_argument("--storages", default="f32,fp16")
    ap.add_argument("--q", default="1,64,1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--no-fit", action="store_true", help="skip the fit() wall-time comparison at config 4")
    a = ap.parse_args()
    for cfg in [int(c) for c in a.configs.split(",")]:
        workload, cls = CONFIGS[cfg]
        df = synth.WORKLOADS[workload][0]()
        for storage in a.storages.split(","):
            fit = lambda **kw: getattr(SRA, cls)().fit(df, verbose=False, iterations=a.updates, eps=0,
                                                       storage_precision=storage, **kw)
            fit(top_k=1)                                  # warm: code objects, pools, the engine of this thread
            t0 = time.perf_counter()
            kept = fit(keep=True)
            fit_keep_ms = (time.perf_counter() - t0) * 1e3
            solver = kept._model[0]
            labels = kept._model[1][0][1]
            n, ops, elem = len(labels), solver.ops[0], 2 if storage == "fp16" else 4
            rng = np.random.default_rng(1)
            for n_q in [int(q) for q in a.q.split(",")]:
                nodes = [labels[i] for i in rng.integers(0, n, n_q)]
                ids = np.asarray(kept._ids(0, labels, nodes)[1])
                reader = solver._reader(0)
                out = hostpool.empty_f64(n_q, n)
                kernel = []
                for i in range(a.reps + 1):
                    ms = []
                    reader.rows(ids, out=out, timing=ms)
                    if i:
                        kernel.append(sum(ms))
                del out                                   # (one answer-sized host frame alive at a time, as in a user's loop)
                kept.rows(nodes), kept.most_similar(nodes, 10)
                faults = []
                rows_ms = wall(lambda: kept.rows(nodes), a.reps, faults)
                top_ms = wall(lambda: kept.most_similar(nodes, 10), max(1, a.reps if n_q <= 1024 else 2))
                d2d, d2h = device_copies(ops, n_q, n, elem, a.reps)
                moved = n_q * n * (elem + 8)
                k_med, c_med = statistics.median(kernel), statistics.median(d2d)
                print(json.dumps(dict(
                    config=cfg, cls=cls, storage=storage, n=n, q=n_q, bytes_moved=moved, kernel_ms=spread(kernel),
                    copy_ms=spread(d2d), kernel_tbs=round(moved / k_med / 1e9, 3), copy_tbs=round(moved / c_med / 1e9, 3),
                    kernel_share_of_copy=round(c_med / k_med, 3), rows_ms=spread(rows_ms), d2h_ms=spread(d2h),
                    rows_over_d2h=round(statistics.median(rows_ms) / statistics.median(d2h), 3), top10_ms=spread(top_ms),
                    rows_minor_faults=faults, slab_bytes=_query.SLAB_BYTES)), flush=True)
            kept.release()
            if cfg == 4 and not a.no_fit:
                t0 = time.perf_counter()
                dense = fit()
                plain_ms = (time.perf_counter() - t0) * 1e3
                del dense
                print(json.dumps(dict(config=cfg, storage=storage, fit_keep_ms=round(fit_keep_ms, 1),
                                      plain_fit_with_dense_handback_ms=round(plain_ms, 1), updates=a.updates)), flush=True)


if __name__ == "__main__":
    main()
