"""The estimators' solver on ONE GPU: the loops of ``fit`` behind the C ABI.

``PlanSolver`` gives ``engine.Plan`` (``simrank_plan_*``: SimRank.py:129-141, :351-363, :443-455) and ``engine.BiPlan``
(``simrank_biplan_*``: :288-303, :410-425, :478-493) the few methods ``estimators.py`` asks of a solver — ``run`` with
the reference's console hooks, ``result``, ``topk``, ``pairs``, ``evidence``, ``release`` — so that what a user imports runs the
fastest loop the library has: both legs and the count of an update queued by one C call, update k + 1 queued before the
count of update k is read on small graphs, and a banded hand-back (csrc/handback.hip: full form by default; the
upper-triangle form is opt-in, ``SIMRANK_SYM_HANDBACK=1``, and checks on the device that the result is symmetric).

An asymmetric prior (``SimRank.py:453``: asymmetric iterates) runs in the same plans with leg 2 stored transposed and the
epilogue as a pass of its own.  Several ranks, virtual or real (``LocalWorld(P > 1)``, ``TorchWorld``), run in
``cshard.CShardSolver``.  The same choreography kernel by kernel in Python — the dense / hybrid GEMM modes, non-default
kernel knobs, the NumPy test double of the CPU tests — is ``tests/pydriver.py``, a test double that plugs in through
``estimators.PYTHON_SOLVER``.
"""
from __future__ import annotations

import numpy as np

from .driver import LocalWorld, Solver, lean_knobs, pattern_refusal, prior_matrix


def applies(ops_factory, world, specs, mode) -> bool:
    """Can the C-level plan run these specs?  One rank of this process, the gather legs, symmetric iterates, the HIP
    engine (``ops_factory`` None = the default engine) with its kernel knobs at their defaults."""
    if ops_factory is not None or not isinstance(world, LocalWorld) or world.size != 1:
        return False
    if mode not in ("auto", "sparse"):
        return False
    if not all(s.symmetric for s in specs) and any(s.storage != "f32" for s in specs):
        return False                 # (asymmetric priors: the f32 plans run them un-fused; fp16-held matrices do not)
    if len({s.storage for s in specs}) != 1 or len({s.dense_terms for s in specs}) != 1:
        return False
    if len(specs) == 2:
        a = specs[0]
        if a.storage != "f32" or a.dense_terms != 3:
            return False             # (the two-matrix plan is f32 with exact products only)
    if pattern_refusal(specs) is not None:
        return False
    return len(specs) == 2 or specs[0].csr.n_rows == specs[0].csr.n_cols


class PlanSolver(Solver):
    """The solver surface ``estimators.py`` asks for, over ``engine.Plan`` / ``engine.BiPlan``."""

    def __init__(self, ops, world, specs):
        from .engine import BiPlan, Plan
        if not lean_knobs(ops):
            raise ValueError("the C-level plans need the default kernel knobs")
        self._describe(world, specs)
        self.ops = {0: ops}
        if self.bipartite:
            a, b = specs
            self.plan = BiPlan(ops, a.csr, a.rowscale, b.rowscale, c1=a.coef, c2=b.coef, evidence=self.gated,
                               apriori1=prior_matrix(a, np.float32), apriori2=prior_matrix(b, np.float32), lbd1=a.lbd, lbd2=b.lbd,
                               strict_reference=self.strict)
        else:
            (s,) = specs
            ap = prior_matrix(s, np.float32)
            if ap is not None and s.storage == "fp16" and not (np.isfinite(ap).all() and float(np.abs(ap).max()) < 3.99):
                raise ValueError("storage_precision='fp16' needs prior values below 4 in magnitude")
            self.plan = Plan(ops, s.csr, s.rowscale, coef=s.coef, evidence=self.gated, apriori=ap,
                             lbd=s.lbd, storage=s.storage, dense_terms=s.dense_terms)

    def run(self, iterations, eps, on_iteration=None, on_converged=None):
        """The loop of SimRank.py:129-140 / :288-302.  Returns k (loop index at which the test passed) or None when
        ``iterations`` updates were applied."""
        self._refuse_run(iterations, eps, on_iteration)
        _, k = self.plan.run(iterations, eps, on_iteration, on_converged)
        return k

    def result(self, j=0):
        return self.plan.side(j).result()

    def topk(self, j, k, exclude_diag=True):
        idx, val = self.plan.side(j).topk(self._k(j, k, exclude_diag), exclude_diag)
        return idx, val.astype(np.float64)

    def pairs(self, j, t, max_pairs):
        """Side j's pairs at least ``t`` similar, selected on the device: (offsets [n + 1], neighbour ids, float32 values)
        in the caller's order (``engine._Side.pairs_above``)."""
        return self.plan.side(j).pairs_above(t, max_pairs)

    def evidence(self, j=0):
        """Evidence matrix of side j (1 - 0.5**count, SimRank.py:316) as float64 in the caller's node order."""
        return 1 - 0.5 ** self.plan.side(j).evidence_counts().astype(np.float64)

    def _make_reader(self, j):
        """Node queries on a kept model (``_query.SolverQueries``): libsimrank_query.so on side j's iterate, in place."""
        return self.plan.side(j).reader()

    def release(self):
        """Free the matrices of the loop; the evidence counts stay (the ``Evidence`` attributes read them lazily)."""
        self._close_readers()
        self.plan.trim()
