#!/usr/bin/env python3
"""fold_in on a kept model (libsimrank_foldin.so) at BASELINE config 4 (N = 32768, SimRank, f32) and config 5
(N = 65536, SimRank++, fp16-held), for n_new new nodes whose lists are existing nodes' lists.

Per (config, n_new), warm, alternating IN THE SAME RUN, enough repeats to pass --seconds per figure:
  foldin_ms        ``model.fold_in(lists)`` end to end (labels in, DataFrame out)
  gather_ms, apply_ms (member_ms)   the stages alone (HIP events on the engine's stream), and the bytes of DESIGN.md
                   section 4.16 over those times (GB/s)
  host_route_ms    what a user has without fold_in: ``model.rows(union of the neighbours)`` plus the two products with
                   scipy.sparse on the host's CPUs (float64; the evidence counts too for SimRank++); W and its pattern
                   are built once per config, outside the timed calls, as fold_in's CSR upload is
One JSON line per measurement on stdout.

    python tools/bench_foldin.py [--configs 4,5] [--new 1,32,1024] [--seconds 0.5] [--updates 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simrank_amd.SimRank as SRA                         # noqa: E402
from simrank_amd import synth                             # noqa: E402

CONFIGS = {4: ("pl32768", "SimRank", "f32"), 5: ("pl65536", "SimRankPP", "fp16")}


def host_operands(csr, scale, evidence):
    """What a user of the host route builds ONCE after the fit (as fold_in uploads its CSR once): W and, for the
    SimRank++ classes, its 0/1 pattern, as scipy.sparse matrices."""
    W = sp.csr_matrix((np.repeat(scale, np.diff(csr.rowptr)), csr.col, csr.rowptr), shape=(csr.n_rows, csr.n_cols))
    Wp = sp.csr_matrix((np.ones(csr.col.size), csr.col, csr.rowptr), shape=(csr.n_rows, csr.n_cols)) if evidence else None
    return W, Wp


def host_route(model, labels, W, Wp, coef, lists):
    """rows(union) over PCIe, then T = G_new . S[union] and out = coef . T . W^T with scipy.sparse (float64)."""
    n = len(labels)
    union = np.unique(np.concatenate(lists))
    rows = model.rows([labels[i] for i in union]).values
    where = np.full(n, -1, dtype=np.int64)
    where[union] = np.arange(union.size)
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(l) for l in lists], out=ptr[1:])
    vals = np.repeat(1.0 / np.maximum(1, np.diff(ptr)), np.diff(ptr))
    G = sp.csr_matrix((vals, where[np.concatenate(lists)], ptr), shape=(len(lists), union.size))
    T = G @ rows                                                       # [n_new, N] dense
    out = coef * (W @ T.T).T
    if Wp is not None:
        Gp = sp.csr_matrix((np.ones(ptr[-1]), np.concatenate(lists), ptr), shape=(len(lists), n))
        out = out * (1 - 0.5 ** np.asarray((Gp @ Wp.T).todense()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4,5")
    ap.add_argument("--new", default="1,32,1024")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--updates", type=int, default=3)
    args = ap.parse_args()
    for cfg in [int(c) for c in args.configs.split(",")]:
        workload, cls, storage = CONFIGS[cfg]
        df = synth.WORKLOADS[workload][0]()
        t = time.perf_counter()
        model = getattr(SRA, cls)().fit(df, verbose=False, iterations=args.updates, eps=0, storage_precision=storage,
                                        keep=True)
        fit_s = time.perf_counter() - t
        solver, sides = model._model
        labels = sides[0][1]
        csr, spec = model._csr, solver.specs[0]
        n, nnz, elem = csr.n_rows, csr.nnz, 2 if storage == "fp16" else 4
        evidence = spec.evidence_from is not None
        rng = np.random.default_rng(cfg)
        W, Wp = host_operands(csr, spec.rowscale, evidence)
        print(json.dumps(dict(config=cfg, cls=cls, storage=storage, n=n, nnz=nnz, fit_keep_s=round(fit_s, 3))), flush=True)
        for n_new in [int(x) for x in args.new.split(",")]:
            pick = rng.choice(np.nonzero(np.diff(csr.rowptr) > 0)[0], n_new, replace=n_new > n)
            lists = [csr.col[csr.rowptr[a]:csr.rowptr[a + 1]].astype(np.int64) for a in pick]
            lab_lists = [[labels[i] for i in l] for l in lists]
            run = lambda: model.fold_in(lab_lists)
            other = lambda: host_route(model, labels, W, Wp, spec.coef, lists)
            got, want = run().values, other()                          # warm both; the two routes agree
            err = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300) * (want != 0)))
            fold, host = [], []
            while sum(fold) < args.seconds * 1e3 or len(fold) < 3:     # alternating
                t = time.perf_counter(); run(); fold.append((time.perf_counter() - t) * 1e3)
                if sum(host) < args.seconds * 1e3 or len(host) < 3:
                    t = time.perf_counter(); other(); host.append((time.perf_counter() - t) * 1e3)
            stages, reps = {}, 0
            w = 1.0 / np.array([len(l) for l in lists], dtype=np.float64)
            ids = [l.astype(np.int32) for l in lists]
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < args.seconds or reps < 3:
                solver.fold_in(0, ids, w, timing=stages)
                reps += 1
            tiles = -(-n_new // 32)
            gathered = elem * sum(len(l) for l in lists) * n + tiles * 128 * n
            applied = tiles * (nnz * (4 + 128 + (4 if evidence else 0)) + 4 * (n + 1)) + 8 * n_new * n
            g_ms, a_ms = stages["gather_ms"] / reps, stages["apply_ms"] / reps
            print(json.dumps(dict(
                config=cfg, n_new=n_new, list_entries=int(sum(len(l) for l in lists)),
                foldin_ms=round(statistics.median(fold), 3), foldin_min=round(min(fold), 3), foldin_max=round(max(fold), 3),
                foldin_reps=len(fold), host_route_ms=round(statistics.median(host), 3), host_route_min=round(min(host), 3),
                host_route_max=round(max(host), 3), host_reps=len(host),
                speedup=round(statistics.median(host) / statistics.median(fold), 2),
                gather_ms=round(g_ms, 4), apply_ms=round(a_ms, 4), member_ms=round(stages.get("member_ms", 0.0) / reps, 4),
                gather_bytes=int(gathered), apply_bytes=int(applied), gather_gbs=round(gathered / g_ms / 1e6, 1),
                apply_gbs=round(applied / a_ms / 1e6, 1), max_rel_diff_of_the_routes=err)), flush=True)
        model.release()


if __name__ == "__main__":
    main()
