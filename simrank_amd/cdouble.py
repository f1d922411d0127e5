"""The estimators' solver for ``fit(storage_precision="f64")``: the reference's float64 loop on one GPU.

``F64Plan`` wraps a plan of libsimrank_f64.so (include/simrank_f64.h); ``F64Solver`` gives it the methods ``estimators.py``
asks of a solver — ``run`` with the reference's console hooks, ``result``, ``topk``, ``pairs``, ``evidence``, ``release`` —
as ``cplan.PlanSolver`` does for the f32 plans.  The loop is driven from here, one C call per loop index: an f64 update is
milliseconds to seconds long, so reading its count before the next one costs nothing that matters.

Everything the reference computes in float64 stays float64: the row scales, the prior (not rounded to float32 as the f32
plans do), the products, the epilogue and the convergence test.  The evidence counts come from the main library
(``HipOps.evidence_counts``, u8 saturated at 255: 1 - 0.5**255 is already 1.0 in float64, so they are exact).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _f64, hostpool
from ._f64 import F64MemoryError, check
from .driver import Solver, prior_matrix


def refusal(world, specs, mode, ops_factory) -> str | None:
    """None when the f64 loop can run this fit, else the reason it cannot (checked before any device work)."""
    from .driver import LocalWorld
    if ops_factory is not None:
        return "storage_precision='f64' runs on the HIP engine only (no injected engine)"
    if not isinstance(world, LocalWorld) or world.size != 1:
        return ("storage_precision='f64' runs on one GPU (no world, or LocalWorld(1)); the sharded loops and their "
                "exchanges are float32")
    if mode not in ("auto", "sparse"):
        return "storage_precision='f64' runs the gather legs only (mode 'auto' or 'sparse')"
    if any(s.dense_terms != 3 for s in specs):
        return "storage_precision='f64' computes exact float64 products: dense_precision must be 'f32'"
    return None


class F64Plan:
    """One or two sides (``_f64.Side`` fields as keyword dicts) on the device, S = I."""

    def __init__(self, sides, symmetric: bool, stream):
        self.lib = _f64.load()
        self._keep = sides                       # (the host arrays the descriptors point at)
        arr = self._array(sides)
        self.n = [int(s["n_rows"]) for s in sides]
        h = C.c_void_p()
        opts = _f64.Options(int(bool(symmetric)))
        check(self.lib.simrank_f64_plan_create(arr, len(sides), C.byref(opts), stream, C.byref(h)),
              "simrank_f64_plan_create")
        self.handle = h

    @staticmethod
    def side(csr, rowscale, coef, counts=None, prior=None, lbd=0.0) -> dict:
        """A side descriptor; ``counts`` = (device pointer, ld, n) of u8 counts or None."""
        d = dict(n_rows=csr.n_rows, n_cols=csr.n_cols, nnz=csr.nnz,
                 rowptr=np.ascontiguousarray(csr.rowptr, dtype=np.int32),
                 col=np.ascontiguousarray(csr.col, dtype=np.int32) if csr.nnz else None,
                 rowscale=np.ascontiguousarray(rowscale, dtype=np.float64), coef=float(coef), lbd=float(lbd),
                 prior=prior)
        if counts is not None:
            d.update(counts=counts[0], counts_ld=counts[1], counts_n=counts[2])
        return d

    @staticmethod
    def _array(sides):
        arr = (_f64.Side * len(sides))()
        for i, s in enumerate(sides):
            for k, v in s.items():
                setattr(arr[i], k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        return arr

    @staticmethod
    def bytes_needed(sides) -> int:
        b = C.c_int64(0)
        check(_f64.load().simrank_f64_plan_bytes(F64Plan._array(sides), len(sides), C.byref(b)), "simrank_f64_plan_bytes")
        return b.value

    def step(self, eps: float):
        out = (C.c_int64 * len(self.n))()
        check(self.lib.simrank_f64_plan_step(self.handle, float(eps), out), "simrank_f64_plan_step")
        return list(out)

    def reset(self):
        check(self.lib.simrank_f64_plan_reset(self.handle), "simrank_f64_plan_reset")

    def set_timing(self, on: bool):
        check(self.lib.simrank_f64_plan_set_timing(self.handle, int(bool(on))), "simrank_f64_plan_set_timing")

    def leg_times(self):
        """(ms of leg A, leg B, mirror / epilogue pass summed since set_timing(True), steps)."""
        ms, steps = (C.c_double * 3)(), C.c_int32(0)
        check(self.lib.simrank_f64_plan_leg_times(self.handle, ms, C.byref(steps)), "simrank_f64_plan_leg_times")
        return list(ms), steps.value

    def result(self, side: int) -> np.ndarray:
        n = self.n[side]
        out = hostpool.empty_f64(n, n)
        check(self.lib.simrank_f64_plan_result(self.handle, side, out.ctypes.data, n), "simrank_f64_plan_result")
        return out

    def topk(self, side: int, k: int, exclude_diag: bool = True):
        n = self.n[side]
        idx = np.empty((n, k), dtype=np.int32)
        val = np.empty((n, k), dtype=np.float64)
        check(self.lib.simrank_f64_plan_topk(self.handle, side, int(k), int(bool(exclude_diag)), idx.ctypes.data,
                                             val.ctypes.data), "simrank_f64_plan_topk")
        return idx, val

    def pairs_above(self, side: int, t: float, max_pairs: int):
        """(offsets int64 [n + 1], ids int32, values float64) of the pairs of different nodes with S >= t; ValueError,
        before anything but the counts crosses, when more than ``max_pairs`` qualify."""
        from ._select import too_many
        n = self.n[side]
        off = np.empty(n + 1, dtype=np.int64)
        check(self.lib.simrank_f64_plan_count_above(self.handle, side, float(t), off.ctypes.data),
              "simrank_f64_plan_count_above")
        total = int(off[-1])
        if max_pairs is not None and total > int(max_pairs):
            raise too_many(total, max_pairs)
        ids = np.empty(total, dtype=np.int32)
        vals = np.empty(total, dtype=np.float64)
        check(self.lib.simrank_f64_plan_emit_above(self.handle, side, float(t), total,
                                                   ids.ctypes.data if total else None,
                                                   vals.ctypes.data if total else None), "simrank_f64_plan_emit_above")
        return off, ids, vals

    def get(self, side: int, key: str) -> int:
        """Where side ``side``'s current matrix is (simrank_f64_plan_get): "iterate", "iterate_ld", "iterate_rows"."""
        v = C.c_int64(0)
        check(self.lib.simrank_f64_plan_get(self.handle, int(side), key.encode(), C.byref(v)), f"simrank_f64_plan_get({key})")
        return v.value

    def trim(self):
        if self.handle:
            check(self.lib.simrank_f64_plan_trim(self.handle), "simrank_f64_plan_trim")

    def free(self):
        if getattr(self, "handle", None):
            self.lib.simrank_f64_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class F64Solver(Solver):
    """``cplan.PlanSolver``'s surface over an ``F64Plan``."""

    def __init__(self, ops, world, specs):
        from .engine import HipOps
        self._describe(world, specs)
        self.ops = {0: ops}
        self.plan = None
        self._counts = {}                        # id(csr) -> (csr, u8 Matrix): what gates the updates
        priors = [prior_matrix(s, np.float64) for s in specs]
        patterns = []
        for s in specs:
            e = s.evidence_from
            if e is not None and all(e is not p for p in patterns):
                patterns.append(e)
        # device memory: the plan's matrices + the counts, checked before anything is allocated
        sides = [F64Plan.side(s.csr, s.rowscale, s.coef, None, priors[j], s.lbd) for j, s in enumerate(specs)]
        need = F64Plan.bytes_needed(sides) + sum(p.n_rows * ops.pitch(p.n_rows, np.uint8) for p in patterns)
        free, total = C.c_int64(0), C.c_int64(0)
        check(_f64.load().simrank_f64_mem_info(C.byref(free), C.byref(total)), "simrank_f64_mem_info")
        if free.value < need:
            rest = HipOps.pool_stats(ops.device)[0]
            if free.value + rest < need:
                gib = 1 << 30
                raise F64MemoryError(
                    f"storage_precision='f64' at {' x '.join(str(n) for n in self.n)} nodes needs {need / gib:.2f} GiB "
                    f"of device memory (three float64 matrices per side, priors and counts); "
                    f"{(free.value + rest) / gib:.2f} GiB of {total.value / gib:.2f} GiB are free")
            HipOps.trim_pool(ops.device)
        for p in patterns:
            self._counts[id(p)] = (p, self._evidence_counts(ops, p))
        ops.synchronize()
        for j, s in enumerate(specs):
            e = s.evidence_from
            if e is None:
                continue
            m = self._counts[id(e)][1]
            if e.n_rows == s.csr.n_rows:
                sides[j].update(counts=m.ptr, counts_ld=m.ld, counts_n=e.n_rows)
            elif e.n_rows == 1:
                sides[j].update(counts=m.ptr, counts_ld=m.ld, counts_n=1)        # a 1 x 1 Evidence broadcasts
            # (otherwise the broadcast error above ends the fit before this side's first update)
        self.plan = F64Plan(sides, all(s.symmetric for s in specs), ops.stream)

    @staticmethod
    def _evidence_counts(ops, csr):
        """u8 [n, n] common in-neighbour counts of ``csr``'s pattern (rows with rowscale > 0), row-major, on the device."""
        from .engine import check as hip_check
        n = csr.n_rows
        m = ops.matrix(n, n, np.uint8)
        hip_check(ops.lib.simrank_memset(C.c_void_p(m.ptr), 0, m.nbytes, ops.stream), "simrank_memset")
        g = ops.graph(csr)
        ops.evidence_counts(g, 0, m)
        ops.synchronize()
        g.free()
        return m

    def run(self, iterations, eps, on_iteration=None, on_converged=None):
        """The loop of SimRank.py:124-140 / :280-302, as simrank_plan_run_cb runs it: loop index k tests the counts of
        update k (index 0: S_0 = I against the zero matrix, "converged" unless 1 > eps), then goes on to update k + 1.
        Returns k, or None when ``iterations`` updates were applied."""
        self.plan.reset()
        self._refuse_run(iterations, eps, on_iteration)
        if iterations > 0 and not (1.0 > eps):
            if on_converged:
                on_converged(0)
            return 0
        for k in range(iterations):
            if k > 0 and not any(changed):
                if on_converged:
                    on_converged(k)
                return k
            if on_iteration:
                on_iteration(k)
            changed = self.plan.step(eps)
        return None

    def result(self, j=0):
        return self.plan.result(j)

    def topk(self, j, k, exclude_diag=True):
        return self.plan.topk(j, self._k(j, k, exclude_diag), exclude_diag)

    def pairs(self, j, t, max_pairs):
        """Side j's pairs at least ``t`` similar (float64 comparison), selected on the device: (offsets [n + 1],
        neighbour ids, float64 values) in the caller's order."""
        return self.plan.pairs_above(j, t, max_pairs)

    def evidence(self, j=0):
        """Evidence matrix of side j (1 - 0.5**count, SimRank.py:316) as float64 in the caller's node order."""
        csr = self.specs[j].evidence_from
        cnt = self.ops[0].download(self._counts[id(csr)][1])
        return 1 - 0.5 ** cnt.astype(np.float64)

    def _make_reader(self, j):
        """Node queries on a kept model (``_query.SolverQueries``): side j's matrix as libsimrank_query.so's float64
        row-major layout, rows and columns already in the caller's order (identity maps)."""
        from . import _query
        ptr = self.plan.get(j, "iterate")
        if not ptr:
            raise ValueError("the plan's matrices were released: query before release()")
        n = self.plan.get(j, "iterate_rows")
        block = dict(ptr=ptr, layout=_query.ROWMAJOR_F64, stride=self.plan.get(j, "iterate_ld"), rows=n, cols=n, col_lo=0,
                     col_ids=None)
        return _query.Reader(self.ops[0], [block], np.arange(n, dtype=np.int32))

    def release(self):
        """Free the matrices of the loop; the evidence counts stay (the ``Evidence`` attributes read them lazily)."""
        self._close_readers()
        self.plan.trim()
