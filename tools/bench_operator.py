#!/usr/bin/env python3
"""matmul / embed: a kept model as a linear operator (libsimrank_operator.so), against a device copy of the matrix's
bytes and against the two routes it replaces.

  N = 32768 SimRank, compact f32 and fp16-held; X standard normal, d in {1, 8, 32, 64}, both directions.

Per model and product, warm, medians and the spread (min .. max) over --reps:
  apply_ms       (a) `simrank_operator_apply` alone (HIP events: the product kernel and the kernel that adds the parts)
  copy_ms        (b) a device copy of the same bytes of S, timed in this run; `apply_over_copy` = (a) / (b).  A copy
                 reads AND writes every byte, the product only reads them: half a copy is the floor of a sweep
  call_ms        the whole `apply_operator`: X up, the product, the result down
  sets_ms        (c) the `score_sets` route on the same inputs in this run: d dense baskets of all N members with the
                 column's weights (it gives S.T @ X and sweeps the matrix d times), the whole call, and `sets_kernel_ms`
                 its score kernel alone (HIP events); `sets_agree`: within the bound
  numpy_ms       (d) `frame()` (timed once per model: `frame_ms`) plus NumPy on the host; `numpy_agree`: within the bound
and per model `embed(32)` as a whole with its split into device, PCIe and host (QR, eigh and the small products).
One JSON line per record on stdout; --out also writes the list to a file.

    python tools/bench_operator.py [--reps 5] [--updates 3] [--out profiles/bench_operator.json]
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
from simrank_amd import _model, _operator, _sets, synth   # noqa: E402

DS = (1, 8, 32, 64)
U = 2.0 ** -52


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def wall(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--workload", default="pl32768")
    ap.add_argument("--embed-dim", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    df = synth.WORKLOADS[a.workload][0]()
    model = SRA.SimRank().fit(df, verbose=False, iterations=a.updates, eps=0, keep=True).compact()
    results = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        results.append(rec)

    for form in ("compact f32", "compact fp16-held"):
        if form != "compact f32":
            model.compact(precision="fp16")
        solver, _ = model._model
        reader = solver._reader(0)
        ops, n = reader.ops, reader.n
        (block,) = reader.blocks
        s_bytes = _model.block_bytes(block)
        rng = np.random.default_rng(0)
        X = rng.standard_normal((n, max(DS)))
        # (b) a device copy of the matrix's bytes
        dst = ops._malloc(s_bytes)
        try:
            copies = [ops.timed(lambda: ops.copy_bytes(dst, block["ptr"], s_bytes)) for _ in range(a.reps + 1)][1:]
        finally:
            ops.synchronize()
            ops._free(dst)
        copy_ms = statistics.median(copies)
        # (d) the host route's matrix, once
        t0 = time.perf_counter()
        S = model.frame().values
        frame_ms = (time.perf_counter() - t0) * 1e3
        absX = np.abs(X)
        want, bound, numpy_ms = {}, {}, {}
        for transpose in (False, True):
            A = S.T if transpose else S
            for d in DS:
                t0 = time.perf_counter()
                got = A @ X[:, :d]
                numpy_ms[(transpose, d)] = (time.perf_counter() - t0) * 1e3
            want[transpose] = got                                            # (d = 64: its first columns are the smaller d's)
            bound[transpose] = n * U * (np.abs(A) @ absX)
        del S
        ids = np.tile(np.arange(n, dtype=np.int32), max(DS))
        for d in DS:
            Xd = np.ascontiguousarray(X[:, :d])
            # (c) score_sets with d dense baskets: basket q holds every node with column q's weights -> row q = (S.T @ X)[:, q]
            ptr = np.arange(d + 1, dtype=np.int64) * n
            w = np.ascontiguousarray(Xd.T).ravel()
            by_sets = _sets.run(reader, ptr, ids[:d * n], w)
            sets_ms = wall(lambda: _sets.run(reader, ptr, ids[:d * n], w), a.reps)
            sets_kernel = []
            for _ in range(a.reps):
                t = {}
                _sets.run(reader, ptr, ids[:d * n], w, timing=t)
                sets_kernel.append(t.get("score_ms", 0.0))
            sets_agree = bool((np.abs(by_sets.T - want[True][:, :d]) <= bound[True][:, :d]).all())
            for transpose in (False, True):
                stages = []
                for i in range(a.reps + 1):                                  # (the first turn warms up)
                    t = {}
                    got = _operator.product(reader, Xd, transpose, timing=t)
                    if i:
                        stages.append(t["apply_ms"])
                call = wall(lambda: solver.apply_operator(0, Xd, transpose), a.reps)
                again = solver.apply_operator(0, Xd, transpose)
                apply_ms = statistics.median(stages)
                rec = dict(model=form, n=n, d=d, transpose=transpose, s_bytes=s_bytes, apply_ms=spread(stages),
                           copy_ms=spread(copies), apply_over_copy=round(apply_ms / copy_ms, 3),
                           s_gbs=round(s_bytes / (apply_ms * 1e-3) / 1e9, 1),
                           gflops=round(2.0 * n * n * d / (apply_ms * 1e-3) / 1e9, 1), call_ms=spread(call),
                           numpy_ms=round(numpy_ms[(transpose, d)], 1), frame_ms=round(frame_ms, 1),
                           numpy_agree=bool((np.abs(got - want[transpose][:, :d]) <= bound[transpose][:, :d]).all()),
                           same_bits_twice=bool(np.array_equal(got.view(np.uint64), again.view(np.uint64))))
                if transpose:
                    rec.update(sets_ms=spread(sets_ms), sets_kernel_ms=spread(sets_kernel), sets_agree=sets_agree,
                               sets_over_apply=round(statistics.median(sets_ms) / statistics.median(call), 2),
                               sets_kernel_over_apply=round(statistics.median(sets_kernel) / apply_ms, 2))
                emit(rec)
        # embed as a whole, and where its time goes
        runs = []
        for i in range(min(a.reps, 3) + 1):
            t = {}
            with solver.one_block(0) as r:
                _operator.embed(r, a.embed_dim, min(a.embed_dim + 8, n), 2, 0, timing=t)
            if i:
                runs.append(t)
        med = lambda name: round(statistics.median(t.get(name, 0.0) for t in runs), 2)
        total, device, pcie = med("total_ms"), med("apply_ms"), round(med("h2d_ms") + med("d2h_ms"), 2)
        emit(dict(model=form, n=n, embed_dim=a.embed_dim, p=min(a.embed_dim + 8, n), power_iterations=2, total_ms=total,
                  device_ms=device, pcie_ms=pcie, host_ms=round(total - device - pcie, 2)))
    model.release()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
