"""ctypes binding of libsimrank_compare.so (include/simrank_compare.h): how far apart two kept models are, on the device.

``model.compare(other)`` answers "is it the same?" for two models of one graph (an f32 fit against its fp16-held or
float64 form, 8 iterations against 16, one rank against ``LocalWorld(4)``): one sweep of both matrices in place, a few
numbers per node back, and the agreement of the neighbour lists.  Every statistic is a maximum or an integer count, so
the answer is a function of the two matrices alone.  The sweep needs both sides as ONE block in the caller's order: a
compact or loaded model is read in place, a side held in several column blocks (``LocalWorld(P)``) or in a plan's own
order is first packed into a temporary block (``_model.detach``).  No CPU fallback: a missing library or device is an
error.

The definitions (include/simrank_compare.h states them for a block).  For the elements ``a = A[r, c]``, ``b = B[r, c]``,
widened as ``rows`` widens them: ``d`` is +0.0 if ``a == b`` or both are NaN, +inf if exactly one is NaN, otherwise
``fabs(a - b)``; ``rel`` is +0.0 if ``d == 0`` or ``max(|a|, |b|) < floor``, +inf if ``d == inf``, otherwise
``d / max(|a|, |b|)``, the first rule that applies (a NaN operand is below no floor).  Per node the largest ``d`` and ``rel`` with the smallest column attaining each, and the number of
columns with ``d`` above each tolerance; over the matrix the histogram of ``bits(d) >> 52``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import numpy as np

from ._checks import is_int
from ._companion import PANEL_F16, PANEL_F32, ROWMAJOR_F32, ROWMAJOR_F64, Companion  # noqa: F401 (a block's layouts)
from ._driver import Scratch, stage

VERSION = 1              # SIMRANK_COMPARE_VERSION of include/simrank_compare.h
MAX_TOL = 8              # SIMRANK_COMPARE_MAX_TOL: tolerances of one sweep (the wrapper's own 0.0 is one of them)
BINS = 2048              # SIMRANK_COMPARE_BINS: exponent bins of the histogram
MAX_GRID = 2048          # SIMRANK_COMPARE_MAX_GRID: workgroups of one sweep
WAVES = 4                # rows one workgroup holds at a time

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_compare_version": [],
    "simrank_compare_last_error": [],
    "simrank_compare_sweep": [_vp, _i32, _i64, _vp, _i32, _i64, _i64, _i64, _vp, _i32, C.c_double, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp],
}
_RESTYPES = {"simrank_compare_last_error": C.c_char_p}


class CompareError(RuntimeError):
    """A call into libsimrank_compare.so failed."""


_c = Companion("compare", VERSION, PROTOTYPES, _RESTYPES, CompareError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- argument checks: nothing touches a device ---------------------------------------------------------------------------
def _finite_nonnegative(x) -> bool:
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_)) \
        and math.isfinite(float(x)) and float(x) >= 0.0


def check_tolerances(tolerances):
    """``tolerances``: 0 to 7 finite numbers >= 0 -> a tuple of floats in the order given (ValueError otherwise)."""
    if isinstance(tolerances, (str, bytes)) or not hasattr(tolerances, "__iter__"):
        raise ValueError(f"tolerances must be a sequence of 0 to {MAX_TOL - 1} finite numbers >= 0, not {tolerances!r}")
    ts = list(tolerances)
    if len(ts) > MAX_TOL - 1:
        raise ValueError(f"tolerances holds {len(ts)} numbers: at most {MAX_TOL - 1} (the sweep counts {MAX_TOL} and 0.0 "
                         "is one of them)")
    for t in ts:
        if not _finite_nonnegative(t):
            raise ValueError(f"a tolerance must be a finite number >= 0, not {t!r}")
    return tuple(float(t) for t in ts)


def check_floor(floor) -> float:
    if not _finite_nonnegative(floor):
        raise ValueError(f"floor must be a finite number >= 0, not {floor!r}")
    return float(floor)


def check_top_k(top_k, ns):
    """``top_k``: None or a positive int whose clamped value (N - 1 per group) the selection can hold -> None or int."""
    from . import _neighbors
    if top_k is None:
        return None
    if not is_int(top_k) or int(top_k) < 1:
        raise ValueError(f"top_k must be None or a positive integer, not {top_k!r}")
    for n in ns:
        if _neighbors.clamp_k(top_k, n) > _neighbors.MAX_K:
            raise ValueError(f"top_k = {top_k} on {n} nodes is more than the {_neighbors.MAX_K} neighbours per node the "
                             "selection holds")
    return int(top_k)


def check_sides(sides_a, sides_b):
    """The two models' [(side, labels)]: the same number of groups and the same labels in the same order per group;
    a ValueError that names the first difference."""
    if len(sides_a) != len(sides_b):
        raise ValueError(f"the two models have {len(sides_a)} and {len(sides_b)} node groups: compare models of one graph")
    for g, ((_, la), (_, lb)) in enumerate(zip(sides_a, sides_b), start=1):
        if len(la) != len(lb):
            raise ValueError(f"group {g}: the two models have {len(la)} and {len(lb)} nodes")
        if la is lb:
            continue
        a, b = np.empty(len(la), dtype=object), np.empty(len(lb), dtype=object)
        a[:], b[:] = list(la), list(lb)
        differ = np.flatnonzero(a != b)
        if differ.size:
            i = int(differ[0])
            raise ValueError(f"group {g}: the labels differ at position {i}: {la[i]!r} and {lb[i]!r} (the two models must "
                             "hold the same nodes in the same order)")


def band_rows(n_cols: int) -> int:
    """The most rows of ``n_cols`` columns one sweep takes: a workgroup's 32-bit bins see fewer than 2^32 elements."""
    n_cols = max(1, int(n_cols))
    turns = (2 ** 32 - 1) // (WAVES * n_cols)
    return turns * WAVES * MAX_GRID if turns else max(1, (2 ** 32 - 1) // n_cols)


# ---- the device path -----------------------------------------------------------------------------------------------------
def _row_base(block, r0: int) -> int:
    """The address of the block that starts at row r0 of ``block`` (same layout, stride and columns)."""
    layout = block["layout"]
    if layout == PANEL_F32:
        return block["ptr"] + r0 * 32 * 4
    if layout == PANEL_F16:
        return block["ptr"] + r0 * 64 * 2
    return block["ptr"] + r0 * block["stride"] * (8 if layout == ROWMAJOR_F64 else 4)


def sweep_blocks(ops, a, b, tols, floor, timing=None):
    """``simrank_compare_sweep`` on two blocks (dicts with ptr, layout, stride, rows, cols) over the same rows and columns,
    in bands of rows where a workgroup's bins require it -> (max_abs float64 [rows], arg_abs int32, max_rel, arg_rel,
    over uint32 [rows, len(tols)], hist int64 [BINS]).  ``timing``: a list that receives the kernels' milliseconds."""
    rows, cols = int(a["rows"]), int(a["cols"])
    assert rows == int(b["rows"]) and cols == int(b["cols"])
    n_tol = len(tols)
    lib = load()
    tol_host = np.ascontiguousarray(tols, dtype=np.float64)
    max_abs, max_rel = np.zeros(rows, dtype=np.float64), np.zeros(rows, dtype=np.float64)
    arg_abs, arg_rel = np.full(rows, -1, dtype=np.int32), np.full(rows, -1, dtype=np.int32)
    over = np.zeros((rows, n_tol), dtype=np.uint32)
    hist = np.zeros(BINS, dtype=np.uint64)
    if rows == 0:
        return max_abs, arg_abs, max_rel, arg_rel, over, hist.astype(np.int64)
    with Scratch(ops) as scratch:
        d_abs, d_rel = scratch.malloc(8 * rows), scratch.malloc(8 * rows)
        d_aabs, d_arel = scratch.malloc(4 * rows), scratch.malloc(4 * rows)
        d_over = scratch.malloc(4 * rows * n_tol) if n_tol else None
        d_hist = scratch.put(hist)
        step = band_rows(cols)
        for r0 in range(0, rows, step):
            m = min(step, rows - r0)
            stage(ops, timing, "sweep_ms", lambda: check(lib.simrank_compare_sweep(
                _row_base(a, r0), a["layout"], a["stride"], _row_base(b, r0), b["layout"], b["stride"], m, cols,
                tol_host.ctypes.data if n_tol else None, n_tol, floor, d_abs + 8 * r0, d_aabs + 4 * r0, d_rel + 8 * r0,
                d_arel + 4 * r0, d_over + 4 * r0 * n_tol if n_tol else None, d_hist, ops.stream), "simrank_compare_sweep"))
        for host, dev in ((max_abs, d_abs), (max_rel, d_rel), (arg_abs, d_aabs), (arg_rel, d_arel), (hist, d_hist)):
            ops.d2h(host, dev)
        if n_tol:
            ops.d2h(over, d_over)
        ops.synchronize()
    return max_abs, arg_abs, max_rel, arg_rel, over, hist.astype(np.int64)


def _in_callers_order(reader) -> bool:
    """Whether the reader's one block holds rows and columns in the caller's order (host arrays only)."""
    assert len(reader.blocks) == 1
    return bool(np.array_equal(reader.order, np.arange(reader.n, dtype=np.int32)))


@contextlib.contextmanager
def callers_readers(solver):
    """The readers of every side of ``solver``, each over ONE block in the caller's order with identity column ids: the
    solver's own where they are such (a compact or loaded model), else those of a temporary ``_model.detach(solver)``,
    packed at most once and released at the end of the scope.  A model that is packed costs one more copy of its
    matrices (N^2 x 4 | 2 | 8 bytes per side) while the scope is open."""
    from . import _model
    with contextlib.ExitStack() as scope:
        readers = scope.enter_context(solver.one_block())
        if not all(_in_callers_order(r) for r in readers):
            scope.close()                                  # (one block in the plan's own order: that scope packed nothing)
            temp = _model.detach(solver)
            scope.callback(temp.release)
            readers = [temp._reader(j) for j in range(len(solver.n))]
        yield readers


def select_ids(reader, k: int, timing=None) -> np.ndarray:
    """int32 [n, k]: every node's k best OTHER nodes in the project's total order (``_neighbors.select``), -1 in the
    empty slots; only the ids are downloaded, the tables are freed."""
    from . import _neighbors
    t = _neighbors.select(reader, k, timing)
    try:
        ids = np.empty((t.n, t.k), dtype=np.int32)
        if ids.size:
            reader.ops.d2h(ids, t.ids)
        reader.ops.synchronize()
    finally:
        t.free()
    return ids


def list_agreement(ids_a, ids_b):
    """Two id tables int [n, k] (-1: an empty slot, ignored) -> (overlap int64 [n]: the nodes both lists of a row name;
    same_prefix int64 [n]: the leading ranks at which both name the same valid node).  No loop over the rows."""
    ids_a, ids_b = np.asarray(ids_a, dtype=np.int64), np.asarray(ids_b, dtype=np.int64)
    assert ids_a.shape == ids_b.shape and ids_a.ndim == 2
    n, k = ids_a.shape
    if n == 0 or k == 0:
        return np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    # both lists of a row sorted together: a node named by both shows as two equal neighbours (a list names a node once)
    both = np.sort(np.concatenate([np.where(ids_a >= 0, ids_a, -1), np.where(ids_b >= 0, ids_b, -2)], axis=1), axis=1)
    overlap = ((both[:, 1:] == both[:, :-1]) & (both[:, 1:] >= 0)).sum(axis=1).astype(np.int64)
    same = (ids_a == ids_b) & (ids_a >= 0)
    same_prefix = np.logical_and.accumulate(same, axis=1).sum(axis=1).astype(np.int64)
    return overlap, same_prefix


def compare_readers(ra, rb, tols, floor, k=None, timing=None):
    """One side of two models through their readers (``callers_readers``): the sweep and, with ``k``, the two selections
    -> a dict of host arrays in the caller's order."""
    (a,), (b,) = ra.blocks, rb.blocks
    max_abs, arg_abs, max_rel, arg_rel, over, hist = sweep_blocks(ra.ops, a, b, tols, floor, timing)
    out = dict(max_abs=max_abs, arg_abs=arg_abs, max_rel=max_rel, arg_rel=arg_rel, over=over, hist=hist)
    if k is not None:
        ids_a = select_ids(ra, k, timing)
        ids_b = ids_a if rb is ra else select_ids(rb, k, timing)
        out["k"] = int(ids_a.shape[1])
        out["overlap"], out["same_prefix"] = list_agreement(ids_a, ids_b)
    return out
