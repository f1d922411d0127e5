"""ctypes binding of libsimrank_select.so (include/simrank_select.h): pairs above a threshold, selected on the device.

A companion of libsimrank_hip.so with its own header, version and binding, so that the main library's C ABI stays as it
is; it reads the iterate a plan reports through ``simrank_plan_get`` & co.  No CPU fallback: a missing library or device
is an error.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

from ._companion import PANEL_F16, PANEL_F32, ROWMAJOR_F32, Companion  # noqa: F401 (the layouts a block may have)

VERSION = 1              # SIMRANK_SELECT_VERSION of include/simrank_select.h

_vp, _i64, _i32, _f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_select_version": [],
    "simrank_select_last_error": [],
    "simrank_select_threshold_f32": [C.c_double, C.POINTER(_f32)],
    "simrank_select_count": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _f32, _vp, _vp],
    "simrank_select_offsets": [_vp, _i64, _vp, C.POINTER(_i64)],
    "simrank_select_emit": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _f32, _vp, _i64, _vp, _vp, _vp],
    "simrank_select_merge": [_i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i32],
}
_RESTYPES = {"simrank_select_last_error": C.c_char_p}


class SelectError(RuntimeError):
    """A call into libsimrank_select.so failed."""


_c = Companion("select", VERSION, PROTOTYPES, _RESTYPES, SelectError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


def check_threshold(t, max_pairs=None):
    """``fit(min_similarity=t, max_pairs=m)``'s arguments: t a finite real number > 0, m a positive integer
    (ValueError otherwise; nothing touches a device)."""
    if isinstance(t, bool) or not isinstance(t, numbers.Real) or not math.isfinite(float(t)) or not float(t) > 0:
        raise ValueError(f"min_similarity must be a finite number > 0, not {t!r}")
    if max_pairs is not None and (isinstance(max_pairs, bool) or not isinstance(max_pairs, numbers.Integral)
                                  or int(max_pairs) < 1):
        raise ValueError(f"max_pairs must be a positive integer, not {max_pairs!r}")


def threshold_f32(t) -> float:
    """The smallest float32 t32 with float64(t32) >= t: ``S >= t32`` in f32 is ``float64(S) >= t`` exactly."""
    check_threshold(t)
    out = C.c_float(0)
    check(load().simrank_select_threshold_f32(float(t), C.byref(out)), "simrank_select_threshold_f32")
    return out.value


def too_many(total: int, max_pairs: int) -> ValueError:
    return ValueError(f"{total} pairs reach min_similarity, more than max_pairs={max_pairs}: raise max_pairs or the "
                      "threshold (nothing was transferred)")


def merge(pieces, row_order, threads: int = 0):
    """Host: pieces [(offsets int64 [n + 1], ids int32, values float32)] over the same n rows (rows in the order
    ``row_order`` maps to the caller's) -> (offsets int64 [n + 1] by caller row, ids, values) with each row's ids
    ascending."""
    import numpy as np
    row_order = np.ascontiguousarray(row_order, dtype=np.int32)
    n = row_order.size
    pieces = [(np.ascontiguousarray(o, dtype=np.int64), np.ascontiguousarray(i, dtype=np.int32),
               np.ascontiguousarray(v, dtype=np.float32)) for o, i, v in pieces]
    total = int(sum(int(o[-1]) for o, _, _ in pieces))
    out_off = np.empty(n + 1, dtype=np.int64)
    out_ids = np.empty(total, dtype=np.int32)
    out_val = np.empty(total, dtype=np.float32)
    P = len(pieces)
    offs = (C.c_void_p * P)(*[o.ctypes.data for o, _, _ in pieces])
    ids = (C.c_void_p * P)(*[i.ctypes.data if i.size else None for _, i, _ in pieces])
    vals = (C.c_void_p * P)(*[v.ctypes.data if v.size else None for _, _, v in pieces])
    check(load().simrank_select_merge(P, offs, ids, vals, n, row_order.ctypes.data if n else None, out_off.ctypes.data,
                                      out_ids.ctypes.data if total else None, out_val.ctypes.data if total else None,
                                      int(threads)), "simrank_select_merge")
    return out_off, out_ids, out_val
