#!/usr/bin/env python3
"""fit(storage_precision="f64") next to the default f32 loop: ms per update of both, in the same run, at BASELINE configs
2 (ER N = 8192, SimRank), 3 (MovieLens-shaped 6040 x 3706, BipartiteSimRankPP, Evidence_N2), 4 (power-law N = 32768,
SimRank) and 5 (power-law N = 65536, SimRank++).

f64: the plan of libsimrank_f64.so with HIP events around leg A, leg B and the mirror / epilogue pass (summed over the
timed updates, one synchronised step per update, as fit() runs it).  f32: the C plan of libsimrank_hip.so (simrank_plan_*
/ simrank_biplan_*), wall time of ``run(K, eps=0)``, and its own leg times where it has them.  The roofline fraction is
algorithmic bytes over time against the measured copy rate (DESIGN.md §6, 6.29 TB/s): f64, per matrix update, 16 N^2 per
leg (read the gathered matrix once, write the product) plus 8 N^2 for the old iterate of the convergence test, the mirror
pass (8 N^2) and the CSR; f32 the same with 4-byte values.  One JSON line per configuration on stdout.

    python tools/bench_f64.py [--configs 2,3,4,5] [--updates 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simrank_amd import cdouble, ingest, synth             # noqa: E402
from simrank_amd.driver import LocalWorld, SideSpec        # noqa: E402
from simrank_amd.engine import BiPlan, HipOps, Plan        # noqa: E402

COPY_TBS = 6.29


def side_bytes(n_w, n_y, nnz, value):
    """Algorithmic bytes of one matrix update: leg A reads Y (n_y^2) and writes T (n_w n_y), leg B reads T and writes
    X' (n_w^2) and reads the old X (n_w^2); the mirror pass of a symmetric update moves half of X' twice; the CSR once
    per leg."""
    csr = 2 * (4 * (n_w + 1) + 4 * nnz + 8 * n_w)
    legs = value * (n_y * n_y + n_w * n_y) + value * (n_w * n_y + 2 * n_w * n_w)
    return legs + value * n_w * n_w + csr


def workload(cfg):
    if cfg == "2":
        df = synth.WORKLOADS["er8192"][0]()
        _, csr = ingest.directed(df, False, "from", "to", "weight")
        return "SimRank", [SideSpec(csr, csr.rowscale, 0.8)]
    if cfg == "3":
        df = synth.WORKLOADS["ml1m"][0]()
        _, _, _, _, g12, g21 = ingest.bipartite(df, False, "user", "item", "weight")
        w1, w2 = ingest.spread(g12) * g12.rowscale, ingest.spread(g21) * g21.rowscale
        return "BipartiteSimRankPP", [SideSpec(g12, w1, 0.8, evidence_from=g12), SideSpec(g21, w2, 0.8, evidence_from=g21)]
    name = {"4": "pl32768", "5": "pl65536"}[cfg]
    df = synth.WORKLOADS[name][0]()
    _, csr = ingest.directed(df, False, "from", "to", "weight")
    if cfg == "4":
        return "SimRank", [SideSpec(csr, csr.rowscale, 0.8)]
    return "SimRankPP", [SideSpec(csr, ingest.spread(csr) * csr.rowscale, 0.8, evidence_from=csr)]


def f32_plan(ops, specs):
    if len(specs) == 2:
        a, b = specs
        return BiPlan(ops, a.csr, a.rowscale, b.rowscale, evidence=True)
    (s,) = specs
    return Plan(ops, s.csr, s.rowscale, coef=s.coef, evidence=s.evidence_from is not None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3,4,5")
    ap.add_argument("--updates", type=int, default=5)
    a = ap.parse_args()
    ops = HipOps(0)
    K = a.updates
    for cfg in a.configs.split(","):
        cls, specs = workload(cfg)
        total_bytes = {8: 0, 4: 0}
        for s in specs:
            for v in total_bytes:
                total_bytes[v] += side_bytes(s.csr.n_rows, s.csr.n_cols, s.csr.nnz, v)
        # f32: the C plan, a warm-up run, then K updates
        plan = f32_plan(ops, specs)
        plan.run(1, 0.0)
        if hasattr(plan, "set_timing"):
            plan.set_timing(K)
        t0 = time.perf_counter()
        plan.run(K, 0.0)
        f32_ms = (time.perf_counter() - t0) * 1e3 / K
        f32_legs = list(plan.leg_times()[:2]) if hasattr(plan, "leg_times") else None
        plan.free()
        # f64: the fit's solver (counts included), a warm-up step, then K timed steps
        sol = cdouble.F64Solver(ops, LocalWorld(1), [s for s in specs])
        sol.plan.reset()
        sol.plan.step(0.0)
        sol.plan.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(K):
            sol.plan.step(0.0)
        f64_ms = (time.perf_counter() - t0) * 1e3 / K
        legs, steps = sol.plan.leg_times()
        legs = [x / steps for x in legs]
        sol.release()
        del sol
        HipOps.trim_pool(0)
        out = dict(config=cfg, cls=cls, n=[s.csr.n_rows for s in specs], nnz=specs[0].csr.nnz, updates=K,
                   f64_ms_per_update=round(f64_ms, 3), f64_leg_ms=dict(legA=round(legs[0], 3), legB=round(legs[1], 3),
                                                                       mirror_or_epilogue=round(legs[2], 3)),
                   f32_ms_per_update=round(f32_ms, 3),
                   f32_leg_ms=None if f32_legs is None else dict(leg1=round(f32_legs[0], 3), leg2=round(f32_legs[1], 3)),
                   ratio_f64_over_f32=round(f64_ms / f32_ms, 2),
                   f64_bytes=total_bytes[8], f64_roofline=round(total_bytes[8] / (f64_ms * 1e-3) / 1e12 / COPY_TBS, 3),
                   f32_bytes=total_bytes[4], f32_roofline=round(total_bytes[4] / (f32_ms * 1e-3) / 1e12 / COPY_TBS, 3))
        print(json.dumps(out), flush=True)
    ops.close()


if __name__ == "__main__":
    main()
