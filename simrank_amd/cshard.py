"""fp16-held matrices on SHARDS through the reference's class surface: ``fit(storage_precision="fp16", world=...)`` with
more than one rank (BASELINE.json config 5 in its stated form: N = 65536 SimRank++, reduced precision, 8 GPUs).

The Python driver's solver keeps fp16-held matrices to one rank; the sharded loop on such matrices lives behind the C ABI
(``simrank_shardplan_*``, csrc/shardplan.hip: leg 1 and a full-form leg 2 of half.hip on every rank's column block, the fp16
panels themselves on the links).  ``CShardSolver`` gives that loop the few methods the estimators ask of a solver —
``run`` with the reference's progress callbacks (SimRank.py:129-140), ``result``, ``topk``, ``pairs``, ``release`` — over

* ``LocalWorld(P)``: an in-process group of P virtual ranks on one device (tests, single-GPU emulation), or
* ``TorchWorld`` on RCCL ranks: the library's own RCCL communicator, made from an id rank 0 broadcasts through
  ``torch.distributed``; the library is pointed at the RCCL build torch itself loaded, so one process never runs two.

Since round 5 the same solver runs the f32 (parity-grade) sharded fits of an RCCL world as well — every class with
class, the two-matrix ones through ``simrank_shardbiplan_*``, asymmetric priors with a second all-to-all and an un-fused
epilogue — so that what a multi-GPU user's ``fit`` runs is the C loop, not a second choreography in Python;
the Python choreography of ``tests/pydriver.py`` (a test double) keeps the GEMM modes and the CPU rehearsal over gloo.
"""
from __future__ import annotations

import os

import numpy as np

from .driver import LocalWorld, Solver, TorchWorld, pattern_refusal, prior_matrix


def applies(world, specs, mode) -> str | None:
    """None when the C sharded loop can run these specs, else the reason it cannot."""
    if mode not in ("auto", "sparse"):
        return "the sharded C loop runs the gather legs only (mode 'sparse' or 'auto')"
    if not all(s.symmetric for s in specs):
        # asymmetric iterates: leg 2's product goes round a second all-to-all, the epilogue is a pass of its own (f32 only)
        if any(s.storage != "f32" for s in specs):
            return "an asymmetric prior needs f32 matrices"
    if len({s.storage for s in specs}) != 1 or any(s.dense_terms != 3 for s in specs):
        return "one storage precision for every matrix, exact products on the matrix cores"
    fp16 = specs[0].storage == "fp16"
    if isinstance(world, TorchWorld) and world.dist.get_backend(world.group) != "nccl":
        return "the sharded C loop exchanges over RCCL (one GPU per process)"
    if len(specs) == 2:
        return "the bipartite classes keep fp16-held matrices to one GPU" if fp16 else pattern_refusal(specs)
    s = specs[0]
    why = pattern_refusal(specs)
    if why is not None:
        return why
    if fp16 and s.apriori is not None:
        return "a prior keeps fp16-held matrices to one GPU"
    if fp16 and s.csr.n_rows % (64 * world.size):
        return f"fp16-held matrices on {world.size} ranks need the node count to be a multiple of {64 * world.size}"
    return None


def _rccl_comm(world, ops):
    """The library's communicator for this torch world (made once per world)."""
    comm = getattr(world, "_c_comm", None)
    if comm is not None:
        return comm
    from .engine import ShardPlans
    if "SIMRANK_RCCL_LIB" not in os.environ:
        import torch
        bundled = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if os.path.exists(bundled):              # the RCCL torch runs on (and the HIP runtime it was built for)
            os.environ["SIMRANK_RCCL_LIB"] = bundled
    box = [ShardPlans.rccl_unique_id(ops.lib) if world.rank == 0 else None]
    world.dist.broadcast_object_list(box, src=0, group=world.group)
    # (RCCL prints a version banner on STDOUT when a communicator is made outside torch; a program that promised one JSON
    # line there — bench.py — must not carry it: the banner goes to stderr)
    import sys
    sys.stdout.flush()
    saved = os.dup(1)
    try:
        os.dup2(2, 1)
        comm = ShardPlans.rccl_comm(ops.lib, box[0], world.rank, world.size)
    finally:
        os.dup2(saved, 1)
        os.close(saved)
    world._c_comm = comm
    return comm


class CShardSolver(Solver):
    """The estimators' view of ``engine.ShardPlans`` / ``engine.ShardBiPlans``: the sharded loops behind the C ABI
    (csrc/shardplan.hip) — every class, f32 (the parity path) or, for SimRank / SimRank++ without a prior, fp16-held
    matrices."""

    def __init__(self, make_ops, world, specs):
        from .engine import ShardBiPlans, ShardPlans
        if not isinstance(specs, (list, tuple)):
            specs = [specs]
        self._describe(world, specs)
        self.ops = {r: make_ops(r) for r in world.local_ranks}
        ops = self.ops[world.local_ranks[0]]
        if self.storage == "fp16" and not getattr(ops, "supports_half_storage", False):
            raise ValueError("storage_precision='fp16' needs the HIP engine (matrices held in fp16: csrc/half.hip)")
        local = isinstance(world, LocalWorld)
        sym = getattr(world, "symmetric_shards", True)
        form = -1 if sym == "auto" else (1 if sym else 0)
        if self.storage == "fp16" or not all(s.symmetric for s in specs):
            form = 0                 # (no mirror image to share: fp16-held blocks, asymmetric iterates)
        if form == 1 and all(n % (32 * world.size) for n in self.n):
            form = 0
        common = dict(world=world.size, comm=None if local else _rccl_comm(world, ops), leg2_form=form,
                      stages=0 if local else getattr(world, "stages", 0),
                      wire_fp16=getattr(world, "exchange_precision", "f32") == "fp16")
        if self.bipartite:
            a, b = specs
            self.plans = ShardBiPlans(ops, a.csr, a.rowscale, b.rowscale, c1=a.coef, c2=b.coef, evidence=self.gated,
                                      apriori1=prior_matrix(a, np.float32), apriori2=prior_matrix(b, np.float32), lbd1=a.lbd, lbd2=b.lbd,
                                      strict_reference=self.strict, **common)
        else:
            (s,) = specs
            self.plans = ShardPlans(ops, s.csr, rowscale=s.rowscale, coef=s.coef, evidence=self.gated,
                                    apriori=prior_matrix(s, np.float32), lbd=s.lbd, storage=self.storage, **common)
        self.root = local or world.rank == 0

    def run(self, iterations, eps, on_iteration=None, on_converged=None):
        """The loop of SimRank.py:129-140 / :288-302 (the count of every update is read before the next one is queued)."""
        self._refuse_run(iterations, eps, on_iteration)
        self.plans.reset()
        changed = sum(self.n) if 1.0 > eps else 0
        for k in range(iterations):
            if changed == 0:
                if on_converged:
                    on_converged(k)
                return k
            if on_iteration:
                on_iteration(k)
            c = self.plans.step(eps, exact_count=False)
            changed = sum(c) if self.bipartite else c
        return None

    def _share(self, value):
        """Root's hand-back to the ranks that asked for one (TorchWorld(handback="all"), top-k)."""
        box = [value]
        self.world.dist.broadcast_object_list(box, src=0, group=self.world.group)
        return box[0]

    def _deliver(self, value):
        """Root's ``value`` as the world hands results back: to rank 0 alone (the other ranks are told why they hold
        None), or with ``TorchWorld(handback="all")`` to every rank."""
        if isinstance(self.world, LocalWorld) or getattr(self.world, "handback", "root") == "root":
            if not self.root:
                self._warn_root_only()
            return value
        return self._share(value)

    def result(self, j=0):
        return self._deliver(self.plans.side(j).result(root=0, i_am_root=self.root))

    def topk(self, j, k, exclude_diag=True):
        idx, val = self.plans.side(j).topk(self._k(j, k, exclude_diag), exclude_diag, root=0, i_am_root=self.root)
        if not isinstance(self.world, LocalWorld):
            idx, val = self._share((idx, val))
        return idx, val.astype(np.float64)

    def pairs(self, j, t, max_pairs):
        """Side j's pairs at least ``t`` similar (``engine.Selection``): every rank counts and emits the hits of its own
        columns; an in-process group merges them here, an RCCL world agrees on the total (``max_pairs`` is refused on every
        rank alike) and sends the pieces to rank 0, sizes first, which merges them.  Delivered as ``result``."""
        from . import _select
        sel = self.plans.side(j).selection(t)
        if isinstance(self.world, LocalWorld):
            if sel.total > max_pairs:
                raise _select.too_many(sel.total, max_pairs)
            return sel.pairs()
        dist, group = self.world.dist, self.world.group
        sizes = [None] * self.world.size
        dist.all_gather_object(sizes, sel.total, group=group)
        total = sum(sizes)
        if total > max_pairs:
            raise _select.too_many(total, max_pairs)
        pieces = [None] * self.world.size if self.root else None
        dist.gather_object(sel.emit(), pieces, dst=dist.get_global_rank(group, 0) if group is not None else 0,
                           group=group)
        return self._deliver(_select.merge([p for got in pieces for p in got], sel.row_order) if self.root else None)

    def _make_reader(self, j):
        """Node queries on a kept model (``_query.SolverQueries``): libsimrank_query.so on side j's iterate, in place."""
        return self.plans.side(j).reader()

    def release(self):
        self._close_readers()
        self.plans.free()
