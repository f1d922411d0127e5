"""ctypes binding of libsimrank_exemplars.so (include/simrank_exemplars.h): greedy facility location on a kept model.

``exemplars(k)`` picks, k times, the node whose row raises ``sum_a max over the picked m of S[m, a]`` the most.  The two
device steps read the iterate in place (the block a solver's ``_query.Reader`` describes): ``simrank_exemplars_gains``
gives the marginal gain of listed rows against the running vector of column maxima ``cover``, which stays on the device,
and ``simrank_exemplars_cover`` applies a picked row to it.  The loop (``greedy``) lives here, on the host, over a small
evaluator interface: ``gains(rows) -> float64 array`` (``rows``: frame positions, or None for all of them in the
frame's order) and ``apply(row) -> raised``.  The device path (``DeviceEvaluator``) and the host path of a pruned model
(``ListsEvaluator``) share it, and a test can drive it with a NumPy evaluator.  A side held in several column blocks
(``LocalWorld(P)``) is packed into one temporary block once per call (the solver's ``one_block`` scope).  No CPU
fallback for the matrices: a missing library or device is an error.

The definitions (include/simrank_exemplars.h states them for a block; ``_kept.exemplars`` for a model).  ``cover`` starts
at +0.0 and only rises; ``term(m, a) = v(m, a) - cover[a]`` where ``v(m, a) > cover[a]`` and +0.0 elsewhere; a gain is
the float64 sum of a row's terms in an order that depends on the number of columns alone.  Rounded subtraction and
rounded addition in a fixed tree are monotone, so a gain computed against an older cover is an upper bound of the gain
now: ``lazy`` evaluation keeps such bounds, refreshes only the candidates that could still win, and returns the bits of
the plain loop.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._checks import is_int
from ._companion import Companion
from ._driver import Scratch, stage

VERSION = 1              # SIMRANK_EXEMPLARS_VERSION of include/simrank_exemplars.h
THREADS = 256            # SIMRANK_EXEMPLARS_THREADS: the T of the header's order of additions
GRID_CAP = 2048          # SIMRANK_EXEMPLARS_GRID_CAP: workgroups of one gains call at most
BATCH = 1024             # stale candidates one lazy round refreshes (measured: profiles/bench_exemplars.json)

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_exemplars_version": [],
    "simrank_exemplars_last_error": [],
    "simrank_exemplars_gains": [_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp],
    "simrank_exemplars_cover": [_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp],
}
_RESTYPES = {"simrank_exemplars_last_error": C.c_char_p}


class ExemplarsError(RuntimeError):
    """A call into libsimrank_exemplars.so failed, or the loop met a gain above its bound."""


_c = Companion("exemplars", VERSION, PROTOTYPES, _RESTYPES, ExemplarsError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- argument checks: nothing touches a device ---------------------------------------------------------------------------
def check_given(given, index) -> np.ndarray:
    """The ``given`` argument of ``exemplars`` -> int64 [G], G >= 0: the positions in ``index`` (a pandas Index: the dense
    frame's labels) of distinct fitted labels, in the order given.  None: no given rows.  A sequence of labels; of a pandas
    Series the values are taken.  ValueError for a str, a scalar, anything that is no sequence and a repeated label;
    KeyError for an unknown label."""
    import pandas as pd
    if given is None:
        return np.empty(0, dtype=np.int64)
    if isinstance(given, pd.Series):
        given = given.tolist()
    if isinstance(given, (str, bytes, dict, set, frozenset, pd.DataFrame)) or not hasattr(given, "__len__") or not hasattr(given, "__iter__"):
        raise ValueError(f"given must be None or a sequence of fitted labels, not {type(given).__name__}")
    if getattr(given, "ndim", 1) != 1:
        raise ValueError(f"given must be one-dimensional, not of shape {given.shape}")
    given = list(given)
    if not given:
        return np.empty(0, dtype=np.int64)
    try:
        at = index.get_indexer(pd.Index(given, dtype=object) if index.dtype == object else pd.Index(given))
    except TypeError:
        raise ValueError("given must hold labels (hashable values)") from None
    if (at < 0).any():
        raise KeyError(given[int(np.argmax(at < 0))])
    if np.unique(at).size != at.size:
        raise ValueError("given repeats a label: the given nodes must be distinct")
    return at.astype(np.int64)


def check_k(k, n, n_given) -> int:
    if not is_int(k) or k < 1:
        raise ValueError(f"k must be a positive integer, not {k!r}")
    if k > n - n_given:
        raise ValueError(f"k = {k} is too large: {n} fitted nodes, {n_given} of them given, leave {n - n_given} to pick from")
    return int(k)


def check_lazy(lazy) -> bool:
    if not isinstance(lazy, (bool, np.bool_)):
        raise ValueError(f"lazy must be True or False, not {lazy!r}")
    return bool(lazy)


# ---- the loop ----------------------------------------------------------------------------------------------------------------
def _first(bound, candidate) -> int:
    """The first candidate in the order (bound descending, position ascending).  A bound is a sum of terms >= +0.0 and
    never NaN, so -1.0 stands for "no candidate"."""
    return int(np.argmax(np.where(candidate, bound, -1.0)))


def _first_stale(bound, stale, batch) -> np.ndarray:
    """The first ``batch`` of the positions where ``stale`` holds, in the order (bound descending, position ascending)."""
    at = np.flatnonzero(stale)
    if at.size > batch:
        b = bound[at]
        kth = np.partition(b, at.size - batch)[at.size - batch]          # the batch-th largest
        above = at[b > kth]
        at = np.concatenate([above, at[b == kth][:batch - above.size]])   # (positions ascend within the tie)
    return at[np.lexsort((at, -bound[at]))]


def greedy(ev, n, k, given=(), lazy=True, batch=None):
    """Greedy facility location over an evaluator -> (picks int64 [k], gain float64 [k], raised int64 [k], evaluated
    int64 [k], rounds): the picked frame positions, each pick's fresh gain, the columns it raised, the rows whose gain was
    computed for it, and the number of ``gains`` calls.

    The rows of ``given`` are applied first, in order, and are never picked.  Plain mode: one ``gains(None)`` sweep per
    pick.  Lazy mode: the first pick is a sweep; from then on, with every candidate's last computed gain kept as a bound
    and stamped with the pick it was computed at, let c be the first candidate in the order (bound descending, position
    ascending): a fresh c is the pick; otherwise the first ``batch`` stale candidates in that same order are refreshed
    with one ``gains`` call.  The order is total, so a stale candidate that ties c at a smaller position is refreshed
    before c can be accepted; with bounds that never lie below the gain, lazy mode returns what plain mode returns."""
    batch = BATCH if batch is None else int(batch)
    candidate = np.ones(n, dtype=bool)
    candidate[np.asarray(given, dtype=np.int64)] = False
    for g in given:
        ev.apply(int(g))
    bound, stamp = np.zeros(n, dtype=np.float64), np.full(n, -1, dtype=np.int64)
    picks, gain = np.empty(k, dtype=np.int64), np.empty(k, dtype=np.float64)
    raised, evaluated = np.empty(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
    rounds = 0
    for p in range(k):
        if not lazy or p == 0:
            bound[:] = ev.gains(None)
            stamp[:] = p
            evaluated[p], rounds = int(candidate.sum()), rounds + 1
        else:
            while stamp[_first(bound, candidate)] != p:
                rows = _first_stale(bound, candidate & (stamp != p), batch)
                fresh = np.asarray(ev.gains(rows), dtype=np.float64)
                if not (fresh <= bound[rows]).all():
                    raise ExemplarsError("a refreshed gain lies above its bound: the evaluator is not monotone")
                bound[rows], stamp[rows] = fresh, p
                evaluated[p] += rows.size
                rounds += 1
        c = _first(bound, candidate)
        picks[p], gain[p] = c, bound[c]
        raised[p] = ev.apply(c)
        candidate[c] = False
    return picks, gain, raised, evaluated, rounds


# ---- the device path -----------------------------------------------------------------------------------------------------
class DeviceEvaluator:
    """The evaluator of a reader whose one block holds every row and column: ``cover`` and the gains live in ``scratch``
    (a ``_driver.Scratch`` the caller keeps open), in the block's order; rows go in and gains come out in the frame's."""

    def __init__(self, reader, scratch, timing=None):
        (self.b,), self.ops, self.n, self.inv = reader.blocks, reader.ops, reader.n, reader.inv
        self.lib, self.timing = load(), timing
        n = self.n
        self.cover_dev = scratch.put(np.zeros(n, dtype=np.float64))
        self.gain_dev, self.rows_dev = scratch.malloc(8 * n), scratch.malloc(4 * n)
        self.word_dev = scratch.malloc(8)                             # int32 row, uint32 raised
        self.gain_host, self.word = np.empty(n, dtype=np.float64), np.zeros(2, dtype=np.int32)

    def _gains(self, rows_dev, m):
        b, ops = self.b, self.ops
        stage(ops, self.timing, "gains_ms", lambda: check(self.lib.simrank_exemplars_gains(
            b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], rows_dev, m, self.cover_dev, self.gain_dev,
            ops.stream), "simrank_exemplars_gains"))
        ops.d2h(self.gain_host, self.gain_dev, 8 * m)
        ops.synchronize()
        return self.gain_host[:m]

    def gains(self, rows):
        if rows is None:
            return self._gains(None, self.n)[self.inv]
        pos = np.ascontiguousarray(self.inv[rows], dtype=np.int32)
        self.ops.h2d(self.rows_dev, pos)
        return self._gains(self.rows_dev, int(pos.size)).copy()

    def apply(self, row) -> int:
        b, ops = self.b, self.ops
        self.word[:] = (self.inv[row], 0)
        ops.h2d(self.word_dev, self.word)
        stage(ops, self.timing, "cover_ms", lambda: check(self.lib.simrank_exemplars_cover(
            b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], self.word_dev, 1, self.cover_dev,
            self.word_dev + 4, ops.stream), "simrank_exemplars_cover"))
        ops.d2h(self.word, self.word_dev)
        ops.synchronize()
        return int(self.word.view(np.uint32)[1])

    def cover(self) -> np.ndarray:
        """float64 [n]: the cover in the frame's order."""
        out = np.empty(self.n, dtype=np.float64)
        self.ops.d2h(out, self.cover_dev)
        self.ops.synchronize()
        return out[self.inv]


# ---- the host path of a pruned model ---------------------------------------------------------------------------------------
class ListsEvaluator:
    """The evaluator of the matrix P of a pruned model, on the host: a row's kept entries and its stored diagonal
    element; absent entries are +0.0 and never gain.  A gain is ``math.fsum`` of the row's terms: the correctly rounded
    exact sum, which is monotone in the cover as well."""

    def __init__(self, ids, vals, diag):
        ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64)
        self.n = int(ids.shape[0])
        self.rows = []
        for m in range(self.n):
            kept = (ids[m] >= 0) & (ids[m] != m)
            self.rows.append((np.append(ids[m][kept], m).astype(np.int64), np.append(vals[m][kept], float(diag[m]))))
        self._cover = np.zeros(self.n, dtype=np.float64)

    def _gain(self, m) -> float:
        cols, v = self.rows[m]
        with np.errstate(invalid="ignore"):
            up = v > self._cover[cols]
        return math.fsum((v[up] - self._cover[cols[up]]).tolist())

    def gains(self, rows):
        return np.array([self._gain(m) for m in (range(self.n) if rows is None else np.asarray(rows).tolist())],
                        dtype=np.float64)

    def apply(self, row) -> int:
        cols, v = self.rows[int(row)]
        with np.errstate(invalid="ignore"):
            up = v > self._cover[cols]
        self._cover[cols[up]] = v[up]
        return int(up.sum())

    def cover(self) -> np.ndarray:
        return self._cover.copy()


# ---- a solver's side ---------------------------------------------------------------------------------------------------------
def exemplars(solver, j, k, given, lazy, stats=None):
    """(picks int64 [k] frame positions, gain float64 [k], raised int64 [k], evaluated int64 [k], cover float64 [N] in the
    frame's order) of side j.  ``stats``: a dict that receives ``rounds`` (the ``gains`` calls); where it holds a dict
    under ``"timing"``, that one receives the milliseconds of the two kernels on the device path (HIP events, which
    serialises them)."""
    lists = solver.lists(j)
    if lists is not None:
        ev = ListsEvaluator(*lists)
        out = greedy(ev, ev.n, k, given, lazy)
        cover = ev.cover()
    else:
        with solver.one_block(j) as reader, Scratch(reader.ops) as scratch:
            ev = DeviceEvaluator(reader, scratch, None if stats is None else stats.get("timing"))
            out = greedy(ev, ev.n, k, given, lazy)
            cover = ev.cover()
    if stats is not None:
        stats["rounds"] = out[4]
    return out[:4] + (cover,)
