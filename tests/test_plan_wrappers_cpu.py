"""The plan wrappers of ``simrank_amd.engine`` (``Plan``, ``BiPlan``, ``ShardPlans``, ``ShardBiPlans``, ``Selection``) and the
solvers on top of them (``cplan.PlanSolver``, ``cshard.CShardSolver``) on a machine without a GPU and without a library:
``Lib`` stands in for every library (each entry point records its name and arguments and returns 0) and ``Ops`` for the
engine's ``HipOps``; all of them write one log, so the tests read the sequence of C calls, their scalar arguments and
the order of synchronise and free straight off it."""
import ctypes as C
import sys
import warnings

import numpy as np
import pytest

from simrank_amd import _query, _select, cplan, cshard
from simrank_amd.driver import LocalWorld, SideSpec, TorchWorld
from simrank_amd.engine import BiPlan, Plan, Selection, ShardBiPlans, ShardPlans
from simrank_amd.ingest import CSR


# (the libraries' doubles fill no output: arrays of ``np.empty`` are widened as they are)
pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered in cast")


class _Ptr:
    """Equals any non-null address."""

    def __eq__(self, other):
        return isinstance(other, int) and not isinstance(other, bool) and other != 0

    def __repr__(self):
        return "PTR"


PTR, CB, STREAM = _Ptr(), "callback", 0x57
OUT32, OUT64, NOCONV, NEWH = ("out", "c_int", 0), ("out", "c_long", 0), ("out", "c_int", -1), ("out", "c_void_p", None)
_BYREF = type(C.byref(C.c_int()))
ITERATE_KEYS = [b"iterate", b"ids", b"iterate_col_lo", b"iterate_layout", b"iterate_stride", b"iterate_rows",
                b"iterate_col_hi"]


def _norm(a):
    if isinstance(a, _BYREF):
        o = a._obj
        if isinstance(o, C.Structure):
            return {k: getattr(o, k) for k, _ in o._fields_}
        return ("out", type(o).__name__, o.value)
    if isinstance(a, C.Array):
        return list(a)
    if isinstance(a, (C.c_void_p, C.c_char_p, C.c_float)):
        return a.value
    if isinstance(a, C._CFuncPtr):
        return CB
    return a


def _read(ptr, dtype, count):
    return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).tolist() if ptr else None


class Lib:
    """Every attribute is an entry point that logs (name, arguments) and returns 0.  Entries that hand something back
    do so as the libraries would: fresh handles, counts of a step, the outcome of a run (``run_result``; a ``_cb`` run
    calls the hook for loop indices 0, 1 and "converged at 2" until it asks to stop), the values of a getter."""

    def __init__(self, log, n=5):
        self.log, self.n, self._handle, self.run_result, self.raises, self.host = log, n, 0x100, (3, -1), {}, []

    def _new(self):
        self._handle += 0x10
        return self._handle

    def __getattr__(self, name):
        if not name.startswith("simrank_"):
            raise AttributeError(name)

        def entry(*args):
            self.log.append((name,) + tuple(_norm(a) for a in args))
            if name in self.raises:
                raise self.raises[name]
            outs = [a._obj for a in args if isinstance(a, _BYREF)]
            if name.endswith("_create") and name != "simrank_comm_create":
                self._seen_create(name, args)
            if name.endswith("_create") or name == "simrank_shardbiplan_side":
                outs[-1].value = self._new()
            elif name == "simrank_comm_local_group":
                for r in range(args[0]):
                    args[1][r] = self._new()
            elif name.endswith("_step"):
                for i, o in enumerate(outs):
                    o.value = 7 - 2 * i
            elif name.endswith(("_run", "_run_cb")):
                if name.endswith("_cb"):
                    cb = next(a for a in args if isinstance(a, C._CFuncPtr))
                    for k, conv in ((0, 0), (1, 0), (2, 1)):
                        if cb(None, k, conv):
                            break
                outs[0].value, outs[1].value = self.run_result
            elif name.endswith("_get"):
                key = next(a for a in args if isinstance(a, bytes))
                outs[-1].value = {b"iterate": 0x7000, b"ids": 0x8000, b"iterate_col_lo": 0, b"iterate_col_hi": self.n,
                                  b"iterate_rows": self.n, b"iterate_layout": 1, b"iterate_stride": 32,
                                  b"restrict_support": 1}[key]
            elif name == "simrank_shardplan_info":
                for o, v in zip(outs, (self.n, 2, 4, 1, 3, 9)):
                    o.value = v
            elif name == "simrank_select_threshold_f32":
                outs[0].value = args[0]
            elif name == "simrank_select_offsets":            # two hits in every row
                np.frombuffer((C.c_int64 * (args[1] + 1)).from_address(args[2]), dtype=np.int64)[:] = \
                    2 * np.arange(args[1] + 1)
            return 0
        return entry

    def _seen_create(self, name, args):
        """The host arrays behind a create call's pointers, read while the call runs."""
        two = "biplan" in name
        dims, (rowptr, col) = args[:2 + two], args[2 + two:4 + two]
        scales = args[4 + two:5 + 2 * two]
        opt = args[5 + 2 * two]._obj
        seen = dict(rowptr=_read(rowptr, np.int32, dims[0] + 1), col=_read(col, np.int32, dims[-1]),
                    scales=[_read(s, np.float32, d) for s, d in zip(scales, dims)])
        for f, d in zip(("apriori1", "apriori2") if two else ("apriori",), dims):
            seen[f] = _read(getattr(opt, f), np.float32, d * d)
        self.host.append(seen)


class Ops:
    supports_half_storage = True

    def __init__(self, log=None, n=5):
        self.log = [] if log is None else log
        self.lib, self.stream, self._next = Lib(self.log, n), C.c_void_p(STREAM), 0x1000

    def _malloc(self, nbytes):
        self._next += 0x100
        self.log.append(("_malloc", self._next, int(nbytes)))
        return self._next

    def _free(self, ptr):
        self.log.append(("_free", ptr))

    def h2d(self, ptr, host):
        assert host.flags.c_contiguous
        self.log.append(("h2d", ptr, host.nbytes))

    def put(self, host):
        ptr = self._malloc(host.nbytes)
        self.h2d(ptr, host)
        return ptr

    def d2h(self, host, ptr, nbytes=None):
        assert host.flags.c_contiguous
        host[...] = 0
        self.log.append(("d2h", ptr, host.nbytes if nbytes is None else nbytes))

    def synchronize(self):
        self.log.append(("synchronize",))

    def timed(self, launch):
        self.log.append(("timed",))
        launch()
        return 1.5

    def take(self, *prefixes):
        """The log so far (entries whose name starts with one of ``prefixes``, or all), which is then cleared."""
        got = [e for e in self.log if not prefixes or e[0].startswith(prefixes)]
        del self.log[:]
        return got


@pytest.fixture
def ops(monkeypatch):
    ops = Ops()
    monkeypatch.setattr(_select, "load", lambda: ops.lib)
    monkeypatch.setattr(_query, "load", lambda: ops.lib)
    return ops


def _csr(n_rows=5, n_cols=5, empty=False):
    """One entry per row (none with ``empty``), held as int64 / float64 Fortran-ish views: the wrappers convert."""
    rowptr = np.zeros(n_rows + 1, dtype=np.int64) if empty else np.arange(n_rows + 1, dtype=np.int64)
    col = np.empty(0, dtype=np.int64) if empty else (np.arange(n_rows, dtype=np.int64) * 3) % n_cols
    return CSR(n_rows, n_cols, rowptr, col, np.arange(1, n_rows + 1, dtype=np.float64) / 8)


def _prior(n):
    return np.asfortranarray(np.arange(n * n, dtype=np.float64).reshape(n, n) / 64)


def _gets(kind, handle, group=None):
    """The getter calls that describe one block of an iterate (``kind``: "plan", "biplan" with its group, "shardplan")."""
    mid = () if group is None else (group,)
    return [(f"simrank_{kind}_get", handle) + mid + (k, OUT64) for k in ITERATE_KEYS]


class PTR_LIST:
    """Equals a list of ``k`` non-null handles."""

    def __init__(self, k):
        self.k = k

    def __eq__(self, other):
        return isinstance(other, list) and len(other) == self.k and all(PTR == x for x in other)


def _options(entry):
    """The options struct of a logged create call."""
    return next(a for a in entry if isinstance(a, dict))


def _selection_calls(blocks, n=5, t=0.5):
    """What ``selection(t)`` + ``emit()`` queue for ``blocks`` column blocks, without synchronises and frees."""
    block = (0x7000, 1, 32, n, n, 0x8000, 0x8000, t)
    count = [("_malloc", PTR, 4 * n)]
    for _ in range(blocks):
        count += [("simrank_select_count",) + block + (PTR, STREAM), ("d2h", PTR, 4 * n),
                  ("simrank_select_offsets", PTR, n, PTR, None)]
    count += [("d2h", 0x8000, 4 * n)]
    emit = []
    for _ in range(blocks):
        emit += [("_malloc", PTR, 8 * (n + 1)), ("_malloc", PTR, 8 * n), ("_malloc", PTR, 8 * n), ("h2d", PTR, 8 * (n + 1)),
                 ("simrank_select_emit",) + block + (PTR, 2 * n, PTR, PTR, STREAM), ("d2h", PTR, 8 * n), ("d2h", PTR, 8 * n)]
    return count, emit


def _quiet(log):
    return [e for e in log if e[0] not in ("synchronize", "_free", "simrank_select_threshold_f32")]


def _assert_read_backs_synchronised_and_blocks_freed_once(log):
    """Every read-back is followed by a synchronise before the next library call, upload, allocation or free; what was
    handed out is freed exactly once."""
    pending = False
    for e in log:
        if e[0] == "d2h":
            pending = True
        elif e[0] == "synchronize":
            pending = False
        else:
            assert not pending, (e, log)
    assert not pending
    assert sorted(e[1] for e in log if e[0] == "_free") == sorted(e[1] for e in log if e[0] == "_malloc")


def _check_queries(ops, obj, gets, blocks, args=(), n=5):
    """``selection`` / ``reader`` / ``pairs_above`` of a plan class (``args``: the group number of a two-matrix one)."""
    count, emit = _selection_calls(blocks, n)
    sel = obj.selection(*args, 0.5)
    assert (sel.total, sel.count_ms, sel.emit_ms, len(sel.offsets), sel.row_order.tolist()) == \
        (2 * n * blocks, 0.0, 0.0, blocks, [0] * n)
    log = ops.take()
    assert _quiet(log) == gets + count
    _assert_read_backs_synchronised_and_blocks_freed_once(log)
    sel = obj.selection(*args, 0.5, timing=True)
    sel.emit()
    assert (sel.count_ms, sel.emit_ms) == (1.5 * blocks, 1.5 * blocks)
    log = ops.take()
    assert [e for e in _quiet(log) if e[0] != "timed"] == gets + count + emit
    assert [e[0] for e in log].count("timed") == 2 * blocks
    _assert_read_backs_synchronised_and_blocks_freed_once(log)
    reader = obj.reader(*args)
    per_block = len(gets) // blocks
    want = []
    for b in range(blocks):
        g = gets[b * per_block:(b + 1) * per_block]
        want += g + [g[2]]                                # ("iterate_col_lo" once more)
    assert ops.take() == want + [("d2h", 0x8000, 4 * n), ("synchronize",)]
    assert isinstance(reader, _query.Reader) and len(reader.blocks) == blocks and reader.n == n
    off, ids, vals = obj.pairs_above(*args, 0.5, 2 * n * blocks)
    log = ops.take()
    assert _quiet(log)[:-1] == gets + count + emit
    assert log[-1][:2] == ("simrank_select_merge", blocks) and log[-1][-1] == 0
    assert (off.dtype, ids.dtype, vals.dtype, ids.size) == (np.int64, np.int32, np.float32, 2 * n * blocks)
    total = 2 * n * blocks
    with pytest.raises(ValueError, match=f"^{total} pairs reach min_similarity, more than max_pairs={total - 1}: raise"):
        obj.pairs_above(*args, 0.5, total - 1)
    assert _quiet(ops.take()) == gets + count             # (refused after the count pass: nothing was emitted)


def _check_hooks(ops, obj, name, handle):
    """``run`` through the ``_cb`` entry: hooks called from inside the C call, their exception raised after it."""
    seen = []
    ops.lib.run_result = (3, 2)
    assert obj.run(7, 0.25, seen.append, lambda k: seen.append(("converged", k))) == (3, 2)
    assert seen == [0, 1, ("converged", 2)]
    assert ops.take() == [(name, handle, 7, 0.25, CB, None, OUT32, NOCONV)]
    assert obj.run(7, 0.25, on_converged=seen.append) == (3, 2) and seen[3:] == [2]

    def bad(k):
        seen.append(("raising", k, len(ops.log)))
        raise KeyError("the hook's")
    ops.take()
    with pytest.raises(KeyError, match="the hook's"):
        obj.run(7, 0.25, bad)
    assert seen[-1] == ("raising", 0, 1)                  # (raised inside the call; the loop was told to stop)
    assert [e[0] for e in ops.take()] == [name]
    ops.lib.run_result = (3, -1)


# ---- Plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior,evidence,storage,terms,empty", [(False, False, "f32", 3, False),
                                                                (True, True, "fp16", 1, False),
                                                                (False, True, "f32", 3, True)])
def test_plan(ops, prior, evidence, storage, terms, empty):
    csr = _csr(empty=empty)
    plan = Plan(ops, csr, coef=0.75, evidence=evidence, apriori=_prior(5) if prior else None, lbd=0.25, reorder=not prior,
                storage=storage, dense_terms=terms)
    H = 0x110
    opt = dict(coef=0.75, lbd=0.25, apriori=PTR if prior else None, ld_apriori=5 if prior else 0, evidence=int(evidence),
               reorder=int(not prior), storage_fp16=int(storage == "fp16"), dense_terms=terms)
    assert ops.take() == [("simrank_plan_create", 5, 0 if empty else 5, PTR, None if empty else PTR, PTR, opt, STREAM, NEWH)]
    assert ops.lib.host == [dict(rowptr=csr.rowptr.tolist(), col=None if empty else csr.col.tolist(),
                                 scales=[csr.rowscale.tolist()], apriori=_prior(5).ravel().tolist() if prior else None)]
    assert plan.n == 5 and plan.handle.value == H
    plan.reset()
    assert plan.step(0.5) == 7 and plan.step(0.125, exact_count=False) == 7
    assert plan.run(7, 0.25) == (3, None)
    ops.lib.run_result = (4, 0)
    assert plan.run(2, 0) == (4, 0)
    ops.lib.run_result = (3, -1)
    assert ops.take() == [("simrank_plan_reset", H), ("simrank_plan_step", H, 0.5, 1, OUT64),
                          ("simrank_plan_step", H, 0.125, 0, OUT64), ("simrank_plan_run", H, 7, 0.25, OUT32, NOCONV),
                          ("simrank_plan_run", H, 2, 0.0, OUT32, NOCONV)]
    _check_hooks(ops, plan, "simrank_plan_run_cb", H)
    out = plan.result()
    idx, val = plan.topk(3)
    plan.topk(2, exclude_diag=False)
    rows = plan.rows([1, 3])
    cnt = plan.evidence_counts()
    assert (out.shape, out.dtype, idx.shape, idx.dtype, val.shape, val.dtype) == \
        ((5, 5), np.float64, (5, 3), np.int32, (5, 3), np.float32)
    assert (rows.shape, rows.dtype, cnt.shape, cnt.dtype) == ((2, 5), np.float32, (5, 5), np.uint8)
    assert ops.take() == [("simrank_plan_result_f64", H, PTR, 5), ("simrank_plan_topk", H, 3, 1, PTR, PTR),
                          ("simrank_plan_topk", H, 2, 0, PTR, PTR), ("simrank_plan_rows_f32", H, PTR, 2, PTR, 5),
                          ("simrank_plan_evidence_u8", H, PTR, 5)]
    assert plan.get("restrict_support") == 1 and plan.graph_handle().value is None
    plan.set_timing(2)
    assert plan.leg_times() == (0.0, 0.0, 0)
    assert [e[:2] for e in ops.take()] == [("simrank_plan_get", H), ("simrank_plan_info", H),
                                           ("simrank_plan_set_timing", H), ("simrank_plan_leg_times", H)]
    _check_queries(ops, plan, _gets("plan", H), 1)
    plan.trim()
    plan.free()
    plan.free()
    plan.trim()
    assert ops.take() == [("simrank_plan_trim", H), ("simrank_plan_destroy", H)]


# ---- BiPlan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("priors,evidence,strict,empty", [((False, False), False, False, False),
                                                          ((True, False), True, True, False),
                                                          ((False, True), True, False, True)])
def test_biplan(ops, priors, evidence, strict, empty):
    csr = _csr(5, 3, empty=empty)
    rs1, rs2 = np.arange(5, dtype=np.float64) / 4, np.arange(6, dtype=np.float64)[::2] / 4
    a1, a2 = (_prior(n) if p else None for n, p in zip((5, 3), priors))
    plan = BiPlan(ops, csr, rs1, rs2, c1=0.75, c2=0.5, evidence=evidence, apriori1=a1, apriori2=a2, lbd1=0.25, lbd2=0.125,
                  reorder=not strict, strict_reference=strict)
    H = 0x110
    opt = dict(c1=0.75, c2=0.5, lbd1=0.25, lbd2=0.125, apriori1=PTR if priors[0] else None, ld_apriori1=5 if priors[0] else 0,
               apriori2=PTR if priors[1] else None, ld_apriori2=3 if priors[1] else 0, evidence=int(evidence),
               reorder=int(not strict), strict_reference=int(strict))
    assert ops.take() == [("simrank_biplan_create", 5, 3, 0 if empty else 5, PTR, None if empty else PTR, PTR, PTR, opt,
                           STREAM, NEWH)]
    assert ops.lib.host == [dict(rowptr=csr.rowptr.tolist(), col=None if empty else csr.col.tolist(),
                                 scales=[rs1.tolist(), rs2.tolist()],
                                 apriori1=_prior(5).ravel().tolist() if priors[0] else None,
                                 apriori2=_prior(3).ravel().tolist() if priors[1] else None)]
    assert (plan.n1, plan.n2) == (5, 3)
    plan.reset()
    assert plan.step(0.5) == (7, 5) and plan.step(0.125, exact_count=False) == (7, 5)
    assert plan.run(7, 0.25) == (3, None)
    assert ops.take() == [("simrank_biplan_reset", H), ("simrank_biplan_step", H, 0.5, 1, OUT64, OUT64),
                          ("simrank_biplan_step", H, 0.125, 0, OUT64, OUT64),
                          ("simrank_biplan_run", H, 7, 0.25, OUT32, NOCONV)]
    _check_hooks(ops, plan, "simrank_biplan_run_cb", H)
    s1, s2 = plan.result()
    assert (s1.shape, s2.shape, s1.dtype) == ((5, 5), (3, 3), np.float64)
    assert ops.take() == [("simrank_biplan_result_f64", H, 1, PTR, 5), ("simrank_biplan_result_f64", H, 2, PTR, 3)]
    for group, n in ((1, 5), (2, 3)):
        ops.lib.n = n
        assert plan.result_group(group).shape == (n, n)
        idx, val = plan.topk(group, 2, exclude_diag=False)
        assert (idx.shape, val.shape, idx.dtype, val.dtype) == ((n, 2), (n, 2), np.int32, np.float32)
        assert plan.rows(group, [2, 0, 1]).shape == (3, n) and plan.evidence_counts(group).shape == (n, n)
        assert plan.get(group, "restrict_support") == 1
        assert ops.take() == [("simrank_biplan_result_f64", H, group, PTR, n), ("simrank_biplan_topk", H, group, 2, 0, PTR, PTR),
                              ("simrank_biplan_rows_f32", H, group, PTR, 3, PTR, n),
                              ("simrank_biplan_evidence_u8", H, group, PTR, n),
                              ("simrank_biplan_get", H, group, b"restrict_support", OUT64)]
        _check_queries(ops, plan, _gets("biplan", H, group), 1, (group,), n)
    plan.get(3, "restrict_support")                       # a group that does not exist is the library's to refuse
    assert ops.take() == [("simrank_biplan_get", H, 3, b"restrict_support", OUT64)]
    plan.trim()
    plan.free()
    plan.free()
    assert ops.take() == [("simrank_biplan_trim", H), ("simrank_biplan_destroy", H)]


# ---- ShardPlans --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,prior,own", [(1, False, True), (3, True, True), (3, False, False)])
def test_shardplans(ops, world, prior, own):
    csr = _csr(empty=not prior and world == 1)
    empty = csr.nnz == 0
    comm = None if own else C.c_void_p(0xC0)
    plans = ShardPlans(ops, csr, world=world, comm=comm, coef=0.75, evidence=prior, apriori=_prior(5) if prior else None,
                       lbd=0.25, reorder=own, leg2_form=0 if prior else -1, stages=2 if prior else 0, wire_fp16=prior,
                       storage="f32" if prior else "fp16")
    P = world if own else 1
    comms = [0x110 + 0x10 * r for r in range(P)] if own else [0xC0]
    hs = [(0x110 if own else 0x100) + 0x10 * (P + r) for r in range(P)]
    opt = dict(coef=0.75, lbd=0.25, apriori=PTR if prior else None, ld_apriori=5 if prior else 0, evidence=int(prior),
               reorder=int(own), leg2_form=0 if prior else -1, stages=2 if prior else 0, wire_fp16=int(prior),
               storage_fp16=int(not prior))
    assert ops.take() == ([("simrank_comm_local_group", world, [None] * world)] if own else []) + [
        ("simrank_shardplan_create", 5, csr.nnz, PTR, None if empty else PTR, PTR, opt, c, STREAM, NEWH) for c in comms]
    assert ops.lib.host == [dict(rowptr=csr.rowptr.tolist(), col=None if empty else csr.col.tolist(),
                                 scales=[csr.rowscale.tolist()], apriori=_prior(5).ravel().tolist() if prior else None)] * P
    assert [h.value for h in plans.plans] == hs and plans.n == 5
    plans.reset()
    assert plans.step(0.5) == 7 and plans.step(0.125, exact_count=False) == 7
    assert plans.run(7, 0.25) == (3, None)
    ops.lib.run_result = (3, 2)
    assert plans.run(7, 0.25) == (3, 2)
    ops.lib.run_result = (3, -1)
    assert ops.take() == [("simrank_shardplan_reset", hs, P), ("simrank_shardplan_step", hs, P, 0.5, 1, OUT64),
                          ("simrank_shardplan_step", hs, P, 0.125, 0, OUT64)] + \
        [("simrank_shardplan_run", hs, P, 7, 0.25, OUT32, NOCONV)] * 2
    out = plans.result()
    idx, val = plans.topk(3)
    assert (out.shape, out.dtype, idx.shape, idx.dtype, val.shape, val.dtype) == \
        ((5, 5), np.float64, (5, 3), np.int32, (5, 3), np.float32)
    assert plans.result(root=1, i_am_root=False) is None
    assert plans.topk(2, exclude_diag=False, root=1, i_am_root=False) == (None, None)
    assert ops.take() == [("simrank_shardplan_result_f64", hs, P, 0, PTR, 5), ("simrank_shardplan_topk", hs, P, 0, 3, 1, PTR, PTR),
                          ("simrank_shardplan_result_f64", hs, P, 1, None, 5),
                          ("simrank_shardplan_topk", hs, P, 1, 2, 0, None, None)]
    i = P - 1
    assert plans.info(i) == dict(n=5, col_lo=2, col_hi=4, half_form=True, stages=3, updates=9, restrict_support=1)
    block, ids = plans.block(i)
    assert (block.shape, block.dtype, ids.shape, ids.dtype) == ((5, 2), np.float64, (2,), np.int32)
    info = [("simrank_shardplan_info", hs[i]) + (OUT64,) * 3 + (OUT32,) * 3,
            ("simrank_shardplan_get", hs[i], b"restrict_support", OUT64)]
    assert ops.take() == info + info + [("simrank_shardplan_block_f64", hs[i], PTR, 2), ("simrank_shardplan_columns", hs[i], PTR)]
    plans.set_timing(4)
    assert plans.timings() == dict.fromkeys(ShardPlans.TIMING_KEYS, 0.0) | {"updates": 0}
    assert ops.take() == [("simrank_shardplan_set_timing", hs[0], 4), ("simrank_shardplan_timings", hs[0], [0.0] * 6, 6, OUT32)]
    _check_queries(ops, plans, [g for h in hs for g in _gets("shardplan", h)], P)
    plans.free()
    plans.free()
    assert ops.take() == [("simrank_shardplan_destroy", h) for h in hs] + \
        ([("simrank_comm_destroy", c) for c in comms] if own else [])
    assert plans.plans == [] and plans.comms == []


def test_rccl_helpers(ops):
    assert ShardPlans.rccl_unique_id(ops.lib) == b"\0" * 128
    assert ShardPlans.rccl_comm(ops.lib, b"id", 2, 4).value == 0x110
    assert [e[0] for e in ops.log] == ["simrank_comm_unique_id", "simrank_comm_create"]
    assert ops.log[1][1:4] == (b"id", 2, 4)


# ---- ShardBiPlans ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own,priors", [(True, (True, False)), (False, (False, False))])
def test_shardbiplans(ops, own, priors):
    csr = _csr(5, 3, empty=not own)
    empty = csr.nnz == 0
    rs1, rs2 = np.arange(5, dtype=np.float64) / 4, np.arange(6, dtype=np.float64)[::2] / 4
    a1, a2 = (_prior(n) if p else None for n, p in zip((5, 3), priors))
    comm = None if own else C.c_void_p(0xC0)
    plans = ShardBiPlans(ops, csr, rs1, rs2, world=2, comm=comm, c1=0.75, c2=0.5, evidence=own, apriori1=a1, apriori2=a2,
                         lbd1=0.25, lbd2=0.125, reorder=own, strict_reference=own, leg2_form=0 if own else -1,
                         stages=3 if own else 0, wire_fp16=own)
    P = 2 if own else 1
    comms = [0x110, 0x120] if own else [0xC0]
    base = 0x110 + 0x10 * P if own else 0x110
    hs = [base + 0x10 * r for r in range(P)]
    sides = {g: [base + 0x10 * (P + (g - 1) * P + r) for r in range(P)] for g in (1, 2)}
    opt = dict(c1=0.75, c2=0.5, lbd1=0.25, lbd2=0.125, apriori1=PTR if priors[0] else None, ld_apriori1=5 if priors[0] else 0,
               apriori2=None, ld_apriori2=0, evidence=int(own), reorder=int(own), strict_reference=int(own))
    assert ops.take() == ([("simrank_comm_local_group", 2, [None, None])] if own else []) + [
        ("simrank_shardbiplan_create", 5, 3, csr.nnz, PTR, None if empty else PTR, PTR, PTR, opt, 0 if own else -1,
         3 if own else 0, int(own), c, STREAM, NEWH) for c in comms] + [
        ("simrank_shardbiplan_side", h, g, NEWH) for g in (1, 2) for h in hs]
    assert ops.lib.host == [dict(rowptr=csr.rowptr.tolist(), col=None if empty else csr.col.tolist(),
                                 scales=[rs1.tolist(), rs2.tolist()],
                                 apriori1=_prior(5).ravel().tolist() if priors[0] else None, apriori2=None)] * P
    assert [h.value for h in plans.pairs] == hs and (plans.n1, plans.n2) == (5, 3)
    plans.reset()
    assert plans.step(0.5) == (7, 5) and plans.step(0.125, exact_count=False) == (7, 5)
    assert plans.run(7, 0.25) == (3, None)
    ops.lib.run_result = (3, 2)
    assert plans.run(7, 0.25) == (3, 2)
    ops.lib.run_result = (3, -1)
    assert ops.take() == [("simrank_shardbiplan_reset", hs, P), ("simrank_shardbiplan_step", hs, P, 0.5, 1, OUT64, OUT64),
                          ("simrank_shardbiplan_step", hs, P, 0.125, 0, OUT64, OUT64)] + \
        [("simrank_shardbiplan_run", hs, P, 7, 0.25, OUT32, NOCONV)] * 2
    for group, n in ((1, 5), (2, 3)):
        ops.lib.n, sp = n, sides[group]
        out = plans.result(group)
        idx, val = plans.topk(group, 2)
        assert (out.shape, out.dtype, idx.shape, idx.dtype, val.shape, val.dtype) == \
            ((n, n), np.float64, (n, 2), np.int32, (n, 2), np.float32)
        assert plans.result(group, root=1, i_am_root=False) is None
        assert plans.topk(group, 3, exclude_diag=False, root=1, i_am_root=False) == (None, None)
        assert ops.take() == [("simrank_shardplan_result_f64", sp, P, 0, PTR, n),
                              ("simrank_shardplan_topk", sp, P, 0, 2, 1, PTR, PTR),
                              ("simrank_shardplan_result_f64", sp, P, 1, None, n),
                              ("simrank_shardplan_topk", sp, P, 1, 3, 0, None, None)]
        assert plans.side_info(group, P - 1) == dict(n=n, col_lo=2, col_hi=4, half_form=True, stages=3, updates=9,
                                                     restrict_support=1)
        assert ops.take() == [("simrank_shardplan_info", sp[-1]) + (OUT64,) * 3 + (OUT32,) * 3,
                              ("simrank_shardplan_get", sp[-1], b"restrict_support", OUT64)]
        _check_queries(ops, plans, [g for h in sp for g in _gets("shardplan", h)], P, (group,), n)
    plans.free()
    plans.free()
    assert ops.take() == [("simrank_shardbiplan_destroy", h) for h in hs] + \
        ([("simrank_comm_destroy", c) for c in comms] if own else [])
    assert plans.pairs == [] and plans.comms == []


# ---- Selection ---------------------------------------------------------------------------------------------------------
def _blocks(k, n=5):
    return [dict(ptr=0x7000, layout=1, stride=32, rows=n, cols=n, row_ids=0x8000, col_ids=0x8000) for _ in range(k)]


def test_selection_queues_the_two_passes_in_order(ops):
    count, emit = _selection_calls(2)
    sel = Selection(ops, _blocks(2), 0.5)
    assert (sel.total, [o.tolist() for o in sel.offsets]) == (20, [list(range(0, 11, 2))] * 2)
    pieces = sel.emit()
    assert [(o.tolist(), i.shape, i.dtype, v.shape, v.dtype) for o, i, v in pieces] == \
        [(list(range(0, 11, 2)), (10,), np.int32, (10,), np.float32)] * 2
    log = ops.take()
    assert _quiet(log) == count + emit
    _assert_read_backs_synchronised_and_blocks_freed_once(log)


def _first_free_follows_a_synchronise_of_the_failed_pass(log, failed):
    at = [e[0] for e in log].index(failed)
    names = [e[0] for e in log[at + 1:]]
    return "synchronize" in names and names.index("synchronize") < names.index("_free")


@pytest.mark.parametrize("failed", ["simrank_select_count", "simrank_select_emit"])
def test_selection_frees_everything_once_after_an_error_and_only_after_a_synchronise(ops, failed):
    ops.lib.raises[failed] = RuntimeError("the pass's")
    with pytest.raises(RuntimeError, match="the pass's"):
        Selection(ops, _blocks(2), 0.5).emit()
    log = ops.take()
    mallocs = [e[1] for e in log if e[0] == "_malloc"]
    assert len(mallocs) == (1 if failed.endswith("count") else 4)
    assert sorted(e[1] for e in log if e[0] == "_free") == sorted(mallocs)       # everything, nothing twice
    assert [e[0] for e in log][-1] == "_free"                                    # (and nothing after the frees)
    # THE INTENDED CHANGE: before Selection took its blocks in a ``_driver.Scratch`` scope, a block went back to the
    # pool while the failed pass's kernel could still be queued; this one assertion fails on that earlier code
    assert _first_free_follows_a_synchronise_of_the_failed_pass(log, failed)


# ---- solvers -----------------------------------------------------------------------------------------------------------
def _spec(csr, evidence_from=None, **kw):
    return SideSpec(csr, csr.rowscale, 0.75, evidence_from=evidence_from, **kw)


def _two(n1=4, n2=3, strict=False, evidence=True):
    a, b = _csr(n1, n2), _csr(n2, n1)
    b = CSR(n2, n1, np.linspace(0, a.nnz, n2 + 1).astype(np.int64), np.zeros(a.nnz, dtype=np.int64), b.rowscale)
    if not evidence:
        return [_spec(a), _spec(b)]
    return [_spec(a, a), _spec(b, a if strict else b)]


class _Dist:
    """torch.distributed for one rank of a made-up world: every collective hands back what it was given."""

    def __init__(self, backend="nccl"):
        self.backend, self.calls = backend, []

    def get_backend(self, group):
        return self.backend

    def broadcast_object_list(self, box, src=0, group=None):
        self.calls.append("broadcast_object_list")

    def all_gather_object(self, out, value, group=None):
        self.calls.append("all_gather_object")
        out[:] = [value] * len(out)

    def gather_object(self, value, out, dst=0, group=None):
        self.calls.append("gather_object")
        if out is not None:
            out[:] = [value] * len(out)


class _World(TorchWorld):
    """A ``TorchWorld`` without torch: the fields a solver reads, and a made-up communicator that no library destroys."""

    def __init__(self):
        pass

    def close(self):
        self._c_comm = None


def _torch_world(rank, size=2, handback="root", backend="nccl"):
    w = _World()
    w.dist, w.group, w.rank, w.size, w.local_ranks, w.handback = _Dist(backend), None, rank, size, [rank], handback
    w.symmetric_shards, w.stages, w.exchange_precision, w._c_comm = "auto", 0, "f32", C.c_void_p(0xC0)
    return w


def _names(ops, *prefixes):
    return [e[0] for e in ops.take(*(prefixes or ("simrank_",))) if not e[0].endswith(("_get", "threshold_f32"))]


def _solvers(ops, specs):
    """(solver, the prefix of its plans' entry points, its local handle count) on one rank and on three virtual ones."""
    two = len(specs) == 2
    yield cplan.PlanSolver(ops, LocalWorld(1), specs), "simrank_biplan" if two else "simrank_plan", None
    yield cshard.CShardSolver(lambda r: ops, LocalWorld(3), specs), "simrank_shardplan", 3


@pytest.mark.parametrize("two", [False, True])
def test_solver_methods_call_the_plans(ops, two):
    specs = _two() if two else [_spec(_csr(4, 4), evidence_from=None)]
    for solver, prefix, P in _solvers(ops, specs):
        sharded = P is not None
        assert (solver.bipartite, solver.n, solver.storage, solver.specs, solver.broadcast_error) == \
            (two, [4, 3] if two else [4], "f32", specs, None)
        assert isinstance((solver.plans if sharded else solver.plan),
                          {(0, 0): Plan, (0, 1): BiPlan, (1, 0): ShardPlans, (1, 1): ShardBiPlans}[sharded, two])
        created = ops.take("simrank_")
        opt = _options(next(e for e in created if e[0].endswith("plan_create")))
        if two:
            assert (opt["c1"], opt["c2"], opt["evidence"], opt["strict_reference"], opt["apriori1"]) == (0.75, 0.75, 1, 0, None)
        else:
            assert (opt["coef"], opt["evidence"], opt["apriori"]) == (0.75, 0, None)
        seen = []
        ops.lib.run_result = (3, 2)
        if sharded:            # the loop is driven from Python: every update's count is read before the next one
            assert solver.run(2, 0.25, seen.append) is None and seen == [0, 1]
            step = "simrank_shardbiplan_step" if two else "simrank_shardplan_step"
            assert ops.take() == [("simrank_shardbiplan_reset" if two else "simrank_shardplan_reset", PTR_LIST(3), 3)] + \
                [(step, PTR_LIST(3), 3, 0.25, 0) + (OUT64,) * (1 + two)] * 2
            assert solver.run(5, 1.0, seen.append, lambda k: seen.append(("converged", k))) == 0
            assert seen[2:] == [("converged", 0)]
        else:
            assert solver.run(9, 0.25) == 2 and solver.run(9, 0.25, seen.append) == 2 and seen == [0, 1]
            assert _names(ops) == [prefix + "_run", prefix + "_run_cb"]
        ops.take()
        for j, n in enumerate(solver.n):
            ops.lib.n = n
            group = ((j + 1,) if two else ())
            assert solver.result(j).shape == (n, n)
            got = ops.take()
            assert len(got) == 1 and got[0][0] == prefix + "_result_f64"
            assert got[0][2:] == ((3, 0, PTR, n) if sharded else group + (PTR, n))
            for k, diag, want in ((2, True, 2), (99, True, n - 1), (99, False, n), (n, True, n - 1)):
                idx, val = solver.topk(j, k, diag)
                assert idx.shape == val.shape == (n, want) and val.dtype == np.float64
                got = ops.take()
                assert len(got) == 1 and got[0][0] == prefix + "_topk"
                assert got[0][2:-2] == ((3, 0, want, int(diag)) if sharded else group + (want, int(diag)))
            off, ids, vals = solver.pairs(j, 0.5, 1000)
            assert _names(ops) == ["simrank_select_count", "simrank_select_offsets"] * (P or 1) + \
                ["simrank_select_emit"] * (P or 1) + ["simrank_select_merge"]
            with pytest.raises(ValueError, match=f"^{2 * n * (P or 1)} pairs reach min_similarity, more than max_pairs=3:"):
                solver.pairs(j, 0.5, 3)
            ops.take()
            assert solver.topk_of(j, [0], 99)[0].shape == (1, n - 1)              # (clamped as ``topk`` clamps)
            assert _names(ops, "simrank_query") == ["simrank_query_topk"] * (P or 1) + \
                (["simrank_query_merge_topk"] if sharded else [])
            if not sharded:
                assert solver.evidence(j).shape == (n, n)
                got = ops.take()
                assert [e[0] for e in got] == [prefix + "_evidence_u8"] and got[0][2:] == group + (PTR, n)
        solver.release()
        got = ops.take("simrank_")
        if sharded:
            assert [e[0] for e in got] == [("simrank_shardbiplan_destroy" if two else "simrank_shardplan_destroy")] * 3 + \
                ["simrank_comm_destroy"] * 3
        else:
            assert [e[0] for e in got] == [prefix + "_trim"]


@pytest.mark.parametrize("two", [False, True])
def test_a_dropped_solver_destroys_its_plans_at_once(ops, two):
    """Not at some later collection: a plan holds the device memory of a fit."""
    import gc
    specs = _two() if two else [_spec(_csr(4, 4))]
    gc.collect()
    gc.disable()
    try:
        for solver, prefix, P in _solvers(ops, specs):
            for j, n in enumerate(solver.n):
                ops.lib.n = n
                solver.result(j), solver.topk(j, 2), solver.pairs(j, 0.5, 1000), solver.topk_of(j, [0], 2)
            ops.take()
            del solver
            assert _names(ops, "simrank_") == (
                [prefix + "_destroy"] if P is None else
                ["simrank_shardbiplan_destroy" if two else "simrank_shardplan_destroy"] * P + ["simrank_comm_destroy"] * P)
    finally:
        gc.enable()


@pytest.mark.parametrize("n,k,diag,want", [(1, 1, True, 1), (1, 5, True, 1), (1, 5, False, 1), (2, 5, True, 1), (2, 5, False, 2),
                                           (2, 1, False, 1)])
def test_topk_clamp(ops, n, k, diag, want):
    for solver, _, _ in _solvers(ops, [_spec(_csr(n, n))]):
        ops.lib.n = n
        ops.take()
        idx, val = solver.topk(0, k, diag)
        assert idx.shape == (n, want)
        (call,) = ops.take("simrank_")
        assert call[-4:-2] == (want, int(diag))
        solver.topk_of(0, [0], k)
        calls = ops.take("simrank_query_topk")
        assert calls and all(c[10] == min(k, max(1, n - 1)) for c in calls)     # (k of each block: its columns = n here)


BROADCAST = r"^operands could not be broadcast together with shapes \(4,4\) \(3,3\) $"


def test_strict_broadcast_error_is_raised_by_run_after_the_first_progress_line(ops):
    for solver, _, _ in _solvers(ops, _two(4, 3, strict=True)):
        created = ops.take("simrank_")
        assert _options(next(e for e in created if e[0].endswith("plan_create")))["strict_reference"] == 1
        assert isinstance(solver.broadcast_error, ValueError)
        seen = []
        with pytest.raises(ValueError, match=BROADCAST):
            solver.run(5, 0.25, seen.append)
        assert seen == [0] and ops.take() == []
        with pytest.raises(ValueError, match=BROADCAST):
            solver.run(5, 0.25)
        # nothing to raise when no update would run (SimRank.py:288-302: the loop body is never entered)
        assert solver.run(0, 0.25) is None
        ops.take()
    # equal sizes, a 1 x 1 first group, or the corrected evidence: no error
    for specs in (_two(3, 3, strict=True), _two(1, 3, strict=True), _two(4, 3, strict=False), _two(4, 3, evidence=False)):
        for solver, _, _ in _solvers(ops, specs):
            assert solver.broadcast_error is None


def _nest(query):
    """(the line of this function that the warning must name, ``query()``'s result): ``query`` is a lambda around the
    solver's method, so the fourth frame counted from that method (``stacklevel=4`` there) is this one."""
    def inner():
        return query()
    line = sys._getframe().f_lineno + 1
    return line, inner()


@pytest.mark.parametrize("two", [False, True])
def test_root_only_warning(ops, two):
    text = ("TorchWorld(handback='root'): only rank 0 receives the similarity matrix, fit() returns "
            "None on this rank (pass handback='all', or fit(top_k=k), to get results on every rank)")
    specs = _two() if two else [_spec(_csr(4, 4))]
    for rank, handback in ((1, "root"), (0, "root"), (1, "all")):
        world = _torch_world(rank, handback=handback)
        solver = cshard.CShardSolver(lambda r: ops, world, specs)
        assert solver.root == (rank == 0)
        for query in (lambda: solver.result(0), lambda: solver.pairs(0, 0.5, 1000)):
            world.dist.calls.clear()
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                line, out = _nest(query)
            if rank == 1 and handback == "root":
                assert out is None and len(caught) == 1
                w = caught[0]
                assert str(w.message) == text and w.category is RuntimeWarning
                assert (w.filename, w.lineno) == (__file__, line)          # stacklevel: three frames above the solver's
            else:
                assert caught == []
            assert ("broadcast_object_list" in world.dist.calls) == (handback == "all")
        if rank == 0:
            idx, val = solver.topk(0, 2)
            assert world.dist.calls[-1] == "broadcast_object_list"         # top-k goes to every rank
        solver.release()
        assert [e[0] for e in ops.take("simrank_comm")] == []               # (the world's communicator is not the plans')


def _applies_cases():
    sq, wide = _csr(4, 4), _csr(4, 6)
    big = _csr(128, 128)
    other = _csr(4, 4)
    a, b = _two(evidence=False)
    ta, tb = a.csr, b.csr
    odd_rows, odd_nnz = CSR(5, 4, tb.rowptr, tb.col, tb.rowscale), CSR(3, 4, tb.rowptr, tb.col[:-1], tb.rowscale)
    one_group = "evidence on one group only"
    foreign = "evidence of a foreign pattern"
    transpose = "the two patterns are not each other's transpose"
    storage = "one storage precision for every matrix, exact products on the matrix cores"
    # (specs, mode, cplan.applies on one rank, cshard.applies on two ranks)
    return [
        ([_spec(sq)], "sparse", True, None),
        ([_spec(sq)], "auto", True, None),
        ([_spec(sq, sq)], "sparse", True, None),
        ([_spec(sq)], "dense", False, "the sharded C loop runs the gather legs only (mode 'sparse' or 'auto')"),
        ([_spec(sq, other)], "hybrid", False, "the sharded C loop runs the gather legs only (mode 'sparse' or 'auto')"),
        ([_spec(sq, symmetric=False)], "sparse", True, None),
        ([_spec(sq, symmetric=False, storage="fp16")], "sparse", False, "an asymmetric prior needs f32 matrices"),
        ([_spec(sq, dense_terms=1)], "sparse", True, storage),
        ([_spec(sq, other)], "sparse", False, foreign),
        ([_spec(wide)], "sparse", False, None),
        ([_spec(wide, other)], "sparse", False, foreign),
        ([_spec(big, storage="fp16")], "sparse", True, None),
        ([_spec(sq, storage="fp16")], "sparse", True,
         "fp16-held matrices on 2 ranks need the node count to be a multiple of 128"),
        ([_spec(big, storage="fp16", apriori=np.eye(128))], "sparse", True, "a prior keeps fp16-held matrices to one GPU"),
        ([_spec(big, other, storage="fp16", apriori=np.eye(128))], "sparse", False, foreign),
        ([_spec(ta), _spec(tb)], "sparse", True, None),
        ([_spec(ta, ta), _spec(tb, tb)], "sparse", True, None),
        ([_spec(ta, ta), _spec(tb, ta)], "sparse", True, None),
        ([_spec(ta), _spec(tb, storage="fp16")], "sparse", False, storage),
        ([_spec(ta, dense_terms=1), _spec(tb, dense_terms=1)], "sparse", False, storage),
        ([_spec(ta, dense_terms=1), _spec(tb)], "sparse", False, storage),
        ([_spec(ta, storage="fp16"), _spec(tb, storage="fp16")], "sparse", False,
         "the bipartite classes keep fp16-held matrices to one GPU"),
        ([_spec(ta, ta), _spec(tb)], "sparse", False, one_group),
        ([_spec(ta), _spec(tb, tb)], "sparse", False, one_group),
        ([_spec(ta, ta), _spec(odd_rows)], "sparse", False, one_group),
        ([_spec(ta, tb), _spec(tb, tb)], "sparse", False, foreign),
        ([_spec(ta, ta), _spec(tb, other)], "sparse", False, foreign),
        ([_spec(ta, other), _spec(odd_nnz, other)], "sparse", False, foreign),
        ([_spec(ta), _spec(odd_rows)], "sparse", False, transpose),
        ([_spec(ta), _spec(odd_nnz)], "sparse", False, transpose),
        ([_spec(ta, ta), _spec(odd_nnz, ta)], "sparse", False, transpose),
        ([_spec(tb), _spec(tb)], "sparse", False, transpose),
    ]


def test_applies_case_by_case():
    for i, (specs, mode, one_rank, why_not_sharded) in enumerate(_applies_cases()):
        assert cplan.applies(None, LocalWorld(1), specs, mode) is one_rank, i
        assert cshard.applies(LocalWorld(2), specs, mode) == why_not_sharded, i
    plain = [_spec(_csr(4, 4))]
    assert cplan.applies(object(), LocalWorld(1), plain, "sparse") is False       # an injected engine
    assert cplan.applies(None, LocalWorld(2), plain, "sparse") is False
    assert cplan.applies(None, _torch_world(0, size=1), plain, "sparse") is False
    assert cshard.applies(_torch_world(0), plain, "sparse") is None
    assert cshard.applies(_torch_world(0, backend="gloo"), plain, "sparse") == \
        "the sharded C loop exchanges over RCCL (one GPU per process)"
    assert cshard.applies(_torch_world(0, backend="gloo"), [_spec(_csr(4, 4), dense_terms=1)], "sparse") == \
        "one storage precision for every matrix, exact products on the matrix cores"
    assert cshard.applies(_torch_world(0, backend="gloo"), _two(evidence=False)[:1] + [_spec(_csr(9, 9))], "sparse") == \
        "the sharded C loop exchanges over RCCL (one GPU per process)"


def test_fp16_prior_bound_and_knobs(ops):
    with pytest.raises(ValueError, match="^storage_precision='fp16' needs prior values below 4 in magnitude$"):
        cplan.PlanSolver(ops, LocalWorld(1), [_spec(_csr(4, 4), storage="fp16", apriori=np.full((4, 4), 4.0))])
    ops.get_tuning = lambda key: 0
    with pytest.raises(ValueError, match="^the C-level plans need the default kernel knobs$"):
        cplan.PlanSolver(ops, LocalWorld(1), [_spec(_csr(4, 4))])
    assert ops.take() == []
