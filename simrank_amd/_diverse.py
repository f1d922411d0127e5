"""ctypes binding of libsimrank_diverse.so (include/simrank_diverse.h): diversified selection on a model that stays on
the device.  Greedy maximal-marginal-relevance picks per basket,

    value(b) = ((1 - d) * score(b)) - (d * pen(b)),      pen(b) = max(+0.0, S[p, b] over the earlier picks p)

three IEEE double operations per candidate and pick, ROW p of the matrix the scores were read from.  A companion of
libsimrank_hip.so with its own header, version and binding, as ``_sets.py`` is.  ``check_diversity`` checks the keyword on
the host (no device); ``run`` is ``_sets.run``'s band loop with a consumer that picks where the score band lies, so the
band never leaves the device: per basket k x (4 + 3 x 8) bytes cross to the host.  No CPU fallback: a missing library or
device is an error.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np

from ._companion import Companion
from ._driver import Scratch

VERSION = 1              # SIMRANK_DIVERSE_VERSION of include/simrank_diverse.h
CHUNK = 1024             # SIMRANK_DIVERSE_CHUNK: candidates one workgroup visits per turn of a sweep
MAX_BLOCKS = 1 << 24     # SIMRANK_DIVERSE_MAX_BLOCKS: workgroups (baskets) of one call

_vp, _i64, _i32, _f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_diverse_version": [],
    "simrank_diverse_last_error": [],
    "simrank_diverse_blocks": [_i64, _i64],
    "simrank_diverse_workspace_bytes": [_i64, _i64],
    "simrank_diverse_pick": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _f64, _f64, _vp, _vp, _vp,
                             _vp, _vp, _vp],
    "simrank_diverse_pick_lists": [_vp, _vp, _vp, _i64, _i32, _vp, _i64, _i64, _i32, _f64, _f64, _vp, _vp, _vp, _vp, _vp,
                                   _vp],
}
_RESTYPES = {"simrank_diverse_last_error": C.c_char_p, "simrank_diverse_blocks": C.c_int64,
             "simrank_diverse_workspace_bytes": C.c_int64}


class DiverseError(RuntimeError):
    """A call into libsimrank_diverse.so failed."""


_c = Companion("diverse", VERSION, PROTOTYPES, _RESTYPES, DiverseError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- the host half: arguments ----------------------------------------------------------------------------------------
def check_diversity(diversity, top_k):
    """``diversity=`` of ``score_sets`` / ``recommend`` checked on the host, before any device work: None, or a finite
    real number in [0, 1] (no bool) given together with ``top_k`` -> None or float (ValueError otherwise)."""
    if diversity is None:
        return None
    if isinstance(diversity, (bool, np.bool_)) or not isinstance(diversity, numbers.Real):
        raise ValueError(f"diversity must be None or a real number in [0, 1], not {diversity!r}")
    d = float(diversity)
    if math.isnan(d) or not 0.0 <= d <= 1.0:
        raise ValueError(f"diversity must lie in [0, 1], not {diversity!r}")
    if top_k is None:
        raise ValueError("diversity re-ranks a selection: give top_k as well")
    return d


# ---- the device half -------------------------------------------------------------------------------------------------
def run(reader, ptr, ids, w, k, excl, d, timing=None, among=None):
    """The baskets (``ptr``, ``ids``, ``w``, ``excl`` as ``_sets.run`` takes them) scored on ``reader``'s iterate, one
    block holding every row and column (``_query.Reader``; a solver's ``one_block`` scope), or the
    ``_neighbors.NeighborReader`` of a pruned model, and of each the ``k`` picks at diversity ``d`` -> (ids int32
    [n_sets, k]: caller ids, -1 past the last pick; score, penalty, value float64 [n_sets, k]: zeros there).  Per band of
    ``_sets.run``: the score kernel, then one pick kernel on the band where it lies; ``reader.inv`` tells the block row of
    a candidate, the block's column map its column.  ``timing`` also receives ``pick_ms``.  ``among``: the caller ids
    (int32, sorted, each once) of the only candidates, as ``_sets.run`` takes them: the band then has one column per
    candidate, in id order, candidate b's row and column are those of node ``among[b]``, and the picks come back as band
    columns and are mapped to caller ids on the host (a pruned model's band keeps every column, the others marked)."""
    from . import _sets
    lib, ops, n = load(), reader.ops, reader.n
    n_sets = int(ptr.size - 1)
    tables = reader._tables() if hasattr(reader, "score_band") else None
    if among is not None:
        among = np.ascontiguousarray(among, dtype=np.int32)
    narrowed = among is not None and tables is None        # the band holds the candidates' columns only
    nc = int(among.size) if narrowed else n                # columns of the band
    k = int(min(k, max(1, nc if among is None else among.size)))
    d = float(d)
    rel_w = 1.0 - d
    idx = np.full((n_sets, k), -1, dtype=np.int32)
    score, pen, val = (np.zeros((n_sets, k), dtype=np.float64) for _ in range(3))
    if n_sets == 0 or nc == 0 or (among is not None and among.size == 0):
        return idx, score, pen, val
    (b,) = reader.blocks
    assert b["cols"] == n and b.get("col_lo", 0) == 0
    with Scratch(ops) as scratch:
        row_pos = None if tables is not None else scratch.put(reader.inv[among] if narrowed else reader.inv)
        col_pos = row_pos if narrowed else None if tables is not None else reader._col_map(0)[0]
        held = {}

        def consume(q0, m, pieces, stage):
            ((_, band, cols, _),) = pieces
            if not held:                                     # (the first band is the largest)
                held.update(m=m, work=scratch.malloc(lib.simrank_diverse_workspace_bytes(m, nc)),
                            idx=scratch.malloc(4 * m * k), **{x: scratch.malloc(8 * m * k) for x in ("score", "pen", "val")})
            assert m <= held["m"] <= MAX_BLOCKS and cols == nc
            outs = (held["idx"], held["score"], held["pen"], held["val"])
            if tables is not None:
                stage("pick_ms", lambda: check(lib.simrank_diverse_pick_lists(
                    tables[0], tables[1], tables[2], n, tables[4], band, n, m, k, rel_w, d, *outs, held["work"],
                    ops.stream), "simrank_diverse_pick_lists"))
            else:
                stage("pick_ms", lambda: check(lib.simrank_diverse_pick(
                    b["ptr"], b["layout"], b["stride"], b["rows"], n, row_pos, col_pos, nc, band, nc, m, k,
                    rel_w, d, *outs, held["work"], ops.stream), "simrank_diverse_pick"))
            for host, dev in zip((idx, score, pen, val), outs):
                ops.d2h(host[q0:q0 + m], dev, host.itemsize * m * k)
            ops.synchronize()                                # (the next band's picks overwrite the four outputs)

        _sets.run(reader, ptr, ids, w, None, excl, timing, consumer=consume, among=among)
    if narrowed:
        idx[idx >= 0] = among[idx[idx >= 0]]
    return idx, score, pen, val
