#!/usr/bin/env python3
"""compact() / save() / load_model() (libsimrank_model.so) at BASELINE config 4 (N = 32768, SimRank) and config 5
(N = 65536, SimRank++), f32 and fp16-held.  Warm, medians and the spread (min .. max) over --reps; one JSON line per
measurement on stdout:

  what="pack"   pack_ms: the pack kernel of compact() alone (HIP events), into a block that is already allocated;
                copy_ms: a hipMemcpy device-to-device of the same N^2 x (4 | 2) bytes in the SAME run (both read and
                write every byte once) -> pack_share_of_copy = copy / pack.  For an f32 model also the converting pack
                (f32 -> fp16-held), against the copy of its own bytes, N^2 x (4 + 2) / 2.
  what="rows"   kernel_ms of `rows` for |Q| random nodes on the KEPT model (the plan's order: a column-map gather) and on
                the COMPACT model (the caller's order: contiguous rows) in the same run, each against the copy of the
                kernel's bytes, |Q| x N x (4 | 2 + 8) -> share_of_copy, and compact_over_kept = kept / compact.
  what="file"   wall time of compact(), save() and load_model(), next to a plain device-to-host and host-to-device copy
                of the same bytes in the same 256 MiB bands.

    python tools/bench_compact.py [--configs 4,5] [--storages f32,fp16] [--q 1024,16384] [--reps 5] [--updates 3] [--dir D]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simrank_amd                                        # noqa: E402
import simrank_amd.SimRank as SRA                         # noqa: E402
from simrank_amd import _model, hostpool, synth           # noqa: E402
from simrank_amd.engine import check                      # noqa: E402

CONFIGS = {4: ("pl32768", "SimRank"), 5: ("pl65536", "SimRankPP")}


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def d2d_ms(ops, nbytes, reps):
    """HIP-event milliseconds of a device-to-device copy of ``nbytes``."""
    src, dst = ops._malloc(nbytes), ops._malloc(nbytes)
    try:
        copy = lambda: check(ops.lib.simrank_memcpy_d2d(C.c_void_p(dst), C.c_void_p(src), nbytes, ops.stream), "simrank_memcpy_d2d")
        return [ops.timed(copy) for _ in range(reps + 1)][1:]
    finally:
        ops._free(src), ops._free(dst)


def host_copies(ops, nbytes, reps):
    """(d2h ms list, h2d ms list): ``nbytes`` between the device and a host block, in save()'s bands."""
    dev = ops._malloc(nbytes)
    stage = np.zeros(min(nbytes, _model.BAND_BYTES), dtype=np.uint8)
    down, up = [], []
    try:
        for i in range(reps + 1):
            for out, move in ((down, lambda at, m: ops.d2h(stage[:m], dev + at, m)), (up, lambda at, m: ops.h2d(dev + at, stage[:m]))):
                t = time.perf_counter()
                for at in range(0, nbytes, _model.BAND_BYTES):
                    move(at, min(_model.BAND_BYTES, nbytes - at))
                    ops.synchronize()
                if i:
                    out.append((time.perf_counter() - t) * 1e3)
    finally:
        ops._free(dev)
    return down, up


def rows_kernel_ms(solver, ids, n, reps):
    reader = solver._reader(0)
    out = hostpool.empty_f64(ids.size, n)
    got = []
    for i in range(reps + 1):
        ms = []
        reader.rows(ids, out=out, timing=ms)
        if i:
            got.append(sum(ms))
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4,5")
    ap.add_argument("--storages", default="f32,fp16")
    ap.add_argument("--q", default="1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--dir", default=tempfile.gettempdir(), help="where the saved model is written (and removed)")
    a = ap.parse_args()
    qs = [int(q) for q in a.q.split(",")]
    for cfg in [int(c) for c in a.configs.split(",")]:
        workload, cls = CONFIGS[cfg]
        df = synth.WORKLOADS[workload][0]()
        for storage in a.storages.split(","):
            base = dict(config=cfg, cls=cls, storage=storage)
            kept = getattr(SRA, cls)().fit(df, verbose=False, iterations=a.updates, eps=0, storage_precision=storage, keep=True)
            solver, labels = kept._model[0], kept._model[1][0][1]
            n, ops, elem = len(labels), solver.ops[0], 2 if storage == "fp16" else 4
            rng = np.random.default_rng(1)
            ids = {q: rng.integers(0, n, q).astype(np.int32) for q in qs}
            kept_rows = {q: rows_kernel_ms(solver, ids[q], n, a.reps) for q in qs}
            # (a) the pack kernel against the copy of the same bytes
            reader = solver._reader(0)
            for target in ([storage, "fp16"] if storage == "f32" else [storage]):
                dst = _model.Block(ops, target, n)
                count = ops.put(np.zeros(1, dtype=np.int64)) if target != storage else None
                try:
                    pack = []
                    for i in range(a.reps + 1):
                        ms = []
                        _model.pack_reader(reader, dst, count, timing=ms)
                        if i:
                            pack.append(sum(ms))
                    moved = n * n * elem + dst.nbytes
                finally:
                    dst.free()
                    if count is not None:
                        ops._free(count)
                copy = d2d_ms(ops, moved // 2, a.reps)
                p, c = statistics.median(pack), statistics.median(copy)
                print(json.dumps(dict(base, what="pack", to=target, n=n, bytes_moved=moved, pack_ms=spread(pack),
                                      copy_ms=spread(copy), pack_tbs=round(moved / p / 1e9, 3),
                                      copy_tbs=round(moved / c / 1e9, 3), pack_share_of_copy=round(c / p, 3))), flush=True)
            # (c) compact, save, load against plain copies
            t = time.perf_counter()
            kept.compact()
            compact_ms = (time.perf_counter() - t) * 1e3
            nbytes = kept.device_bytes
            # (b) the rows kernel on the compact model against the kept model's, same ids, same run
            for q in qs:
                got = rows_kernel_ms(kept._model[0], ids[q], n, a.reps)
                moved = q * n * (elem + 8)
                copy = d2d_ms(ops, moved // 2, a.reps)
                k, m, c = (statistics.median(x) for x in (kept_rows[q], got, copy))
                print(json.dumps(dict(base, what="rows", n=n, q=q, bytes_moved=moved, kept_kernel_ms=spread(kept_rows[q]),
                                      compact_kernel_ms=spread(got), copy_ms=spread(copy),
                                      kept_share_of_copy=round(c / k, 3), compact_share_of_copy=round(c / m, 3),
                                      compact_over_kept=round(k / m, 3))), flush=True)
            path = os.path.join(a.dir, f"bench_compact_{os.getpid()}.simrank")
            try:
                save_ms, load_ms = [], []
                for _ in range(max(1, min(3, a.reps))):
                    t = time.perf_counter()
                    kept.save(path)
                    save_ms.append((time.perf_counter() - t) * 1e3)
                    t = time.perf_counter()
                    loaded = simrank_amd.load_model(path)
                    load_ms.append((time.perf_counter() - t) * 1e3)
                    loaded.release()
            finally:
                if os.path.exists(path):
                    os.remove(path)
            down, up = host_copies(ops, nbytes, min(3, a.reps))
            print(json.dumps(dict(base, what="file", n=n, bytes=nbytes, compact_wall_ms=round(compact_ms, 1),
                                  save_ms=spread(save_ms), load_ms=spread(load_ms), d2h_ms=spread(down), h2d_ms=spread(up),
                                  save_over_d2h=round(statistics.median(save_ms) / statistics.median(down), 3),
                                  load_over_h2d=round(statistics.median(load_ms) / statistics.median(up), 3))), flush=True)
            kept.release()


if __name__ == "__main__":
    main()
