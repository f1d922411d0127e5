"""ctypes binding of libsimrank_profile.so (include/simrank_profile.h): the distribution of a kept model's similarities,
counted on the device.

``count_pairs`` answers "how many pairs lie above each of these thresholds?" with one sweep of the iterate per side and
``threshold_for`` answers "which threshold gives me at most M pairs?" with a global radix select whose number of sweeps
depends only on the stored type (3 for f32, 2 for fp16-held, 6 for float64).  Both read the blocks a solver's
``_query.Reader`` describes in place and add over them (one block on one GPU, one per virtual rank of a
``LocalWorld(P)``).  A pruned model (a solver with ``lists``) is answered on the host from its lists: N x k values
plus the absent +0.0 entries, added by arithmetic.  No CPU fallback for the matrices: a missing library or device is an
error.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np

from ._checks import is_finite_real, is_int
from ._companion import PANEL_F16, PANEL_F32, ROWMAJOR_F32, ROWMAJOR_F64, Companion  # noqa: F401 (a block's layouts)
from ._driver import Scratch, stage

VERSION = 1              # SIMRANK_PROFILE_VERSION of include/simrank_profile.h
MAX_EDGES = 1024         # SIMRANK_PROFILE_MAX_EDGES: thresholds of one count sweep
MAX_DIGIT_BITS = 11      # SIMRANK_PROFILE_MAX_DIGIT_BITS: 2048 bins of a digit sweep

# digits of the radix select per key width: the sweeps of ``threshold_for``
DIGIT_PLAN = {32: (11, 11, 10), 16: (8, 8), 64: (11, 11, 11, 11, 11, 9)}

_vp, _i64, _i32, _u64, _u32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_profile_version": [],
    "simrank_profile_last_error": [],
    "simrank_profile_key_bits": [_i32],
    "simrank_profile_count": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _i32, _vp, _vp],
    "simrank_profile_digits": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _u64, _i32, _i32, _vp, _vp, _vp],
    "simrank_profile_key_f32": [C.c_float],
    "simrank_profile_unkey_f32": [_u32],
    "simrank_profile_key_f64": [C.c_double],
    "simrank_profile_unkey_f64": [_u64],
    "simrank_profile_key_f16": [C.c_uint16],
    "simrank_profile_unkey_f16": [_u32],
    "simrank_profile_pick": [_vp, _i32, _u64, _u64, C.POINTER(_i32), C.POINTER(_u64)],
}
_RESTYPES = {"simrank_profile_last_error": C.c_char_p, "simrank_profile_key_f32": _u32,
             "simrank_profile_unkey_f32": C.c_float, "simrank_profile_key_f64": _u64,
             "simrank_profile_unkey_f64": C.c_double, "simrank_profile_key_f16": _u32,
             "simrank_profile_unkey_f16": C.c_double}


class ProfileError(RuntimeError):
    """A call into libsimrank_profile.so failed."""


_c = Companion("profile", VERSION, PROTOTYPES, _RESTYPES, ProfileError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- argument checks: nothing touches a device ---------------------------------------------------------------------------
def check_thresholds(thresholds) -> np.ndarray:
    """``count_pairs(thresholds)``: 1 to ``MAX_EDGES`` finite real numbers -> float64 array (ValueError otherwise)."""
    if isinstance(thresholds, (str, bytes)) or isinstance(thresholds, numbers.Real):
        raise ValueError(f"thresholds must be a sequence of finite numbers, not {thresholds!r}")
    try:
        items = list(thresholds)
    except TypeError:
        raise ValueError(f"thresholds must be a sequence of finite numbers, not {thresholds!r}") from None
    if not 1 <= len(items) <= MAX_EDGES:
        raise ValueError(f"count_pairs takes 1 to {MAX_EDGES} thresholds, not {len(items)}")
    for t in items:
        if not is_finite_real(t):
            raise ValueError(f"every threshold must be a finite number, not {t!r}")
    return np.array([float(t) for t in items], dtype=np.float64)


def check_max_pairs(max_pairs) -> int:
    """``threshold_for(max_pairs)``: an integer >= 1 (ValueError otherwise)."""
    if not is_int(max_pairs) or int(max_pairs) < 1:
        raise ValueError(f"max_pairs must be a positive integer, not {max_pairs!r}")
    return int(max_pairs)


# ---- host helpers ---------------------------------------------------------------------------------------------------------
def edges_f32(ts) -> np.ndarray:
    """Per threshold the smallest float32 e with float64(e) >= t: ``v >= e`` in f32 is ``float64(v) >= t`` exactly
    (t above the largest float gives +inf, t below the smallest the smallest finite one)."""
    ts = np.asarray(ts, dtype=np.float64)
    with np.errstate(over="ignore"):
        e = ts.astype(np.float32)
    low = e.astype(np.float64) < ts
    e[low] = np.nextafter(e[low], np.float32(np.inf))
    return e


def key_bits(layout: int) -> int:
    got = load().simrank_profile_key_bits(int(layout))
    if got < 0:
        check(got, "simrank_profile_key_bits")
    return got


def unkey(bits: int, key: int) -> float:
    """The float64 value of a key of ``bits`` bits (16: the value an fp16-held element means)."""
    lib = load()
    if bits == 32:
        return float(lib.simrank_profile_unkey_f32(key))
    if bits == 16:
        return float(lib.simrank_profile_unkey_f16(key))
    return float(lib.simrank_profile_unkey_f64(key))


def pick(hist, above: int, max_pairs: int):
    """``simrank_profile_pick`` -> (a bin no longer fits, bin, entries above the bin)."""
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    b, out = C.c_int32(0), C.c_uint64(0)
    rc = load().simrank_profile_pick(hist.ctypes.data, hist.size, int(above), int(max_pairs), C.byref(b), C.byref(out))
    if rc < 0:
        check(rc, "simrank_profile_pick")
    return bool(rc), b.value, out.value


def radix_select(sweep, bits: int, max_pairs: int, plan=None):
    """(t, n) of ``threshold_for`` by ``len(plan)`` digit sweeps.  ``sweep(prefix, prefix_bits, digit_bits, want_min)``
    -> (hist uint64 [2^digit_bits] of the keys under the prefix, the smallest key above the prefix or None)."""
    plan = DIGIT_PLAN[bits] if plan is None else plan
    assert sum(plan) == bits
    prefix, pbits, above = 0, 0, 0
    for level, d in enumerate(plan):
        hist, min_above = sweep(prefix, pbits, d, level == len(plan) - 1)
        _, b, above = pick(hist, above, max_pairs)
        if b < 0:
            return math.inf, 0                               # no entry at all
        head, prefix, pbits = prefix, (prefix << d) | b, pbits + d
    here = int(hist[b])                                      # (the last bin is one key: prefix)
    if above + here <= max_pairs:
        return unkey(bits, prefix), above + here             # every entry fits: the smallest value
    if above == 0:
        return math.inf, 0                                   # the largest value alone occurs too often
    higher = np.flatnonzero(hist[b + 1:])
    if higher.size:
        return unkey(bits, (head << d) | (b + 1 + int(higher[0]))), above
    assert min_above is not None and min_above != 2 ** 64 - 1
    return unkey(bits, int(min_above)), above


def select_values(values, zeros: int, max_pairs: int):
    """(t, n) of ``threshold_for`` on the host: ``values`` (float64, NaN ignored) plus ``zeros`` entries of +0.0."""
    v = np.asarray(values, dtype=np.float64).ravel()
    v = v[~np.isnan(v)] + 0.0                                # (-0.0 + 0.0 = +0.0: one value)
    distinct, counts = np.unique(v, return_counts=True)
    if zeros:
        at = int(np.searchsorted(distinct, 0.0))
        if at < distinct.size and distinct[at] == 0.0:
            counts[at] += zeros
        else:
            distinct, counts = np.insert(distinct, at, 0.0), np.insert(counts, at, zeros)
    above = np.cumsum(counts[::-1])[::-1]                    # entries >= distinct[i]
    fit = np.flatnonzero(above <= max_pairs)
    if not fit.size:
        return math.inf, 0
    return float(distinct[fit[0]]), int(above[fit[0]])


# ---- the sweeps over a reader's blocks ---------------------------------------------------------------------------------------
def _kind(blocks) -> int:
    bits = {key_bits(b["layout"]) for b in blocks}
    assert len(bits) == 1, "the blocks of one iterate hold one type"
    return bits.pop()


def count_blocks(ops, blocks, ts, timing=None) -> np.ndarray:
    """int64 [len(ts)]: entries >= ts[i] over ``blocks``, one ``simrank_profile_count`` per block into one set of
    counters.  ``timing``: a list that receives each sweep's milliseconds (HIP events)."""
    ts = np.asarray(ts, dtype=np.float64)
    order = np.argsort(ts, kind="stable")
    edges = ts[order] if _kind(blocks) == 64 else edges_f32(ts[order])
    lib, m = load(), int(ts.size)
    got = np.zeros(m + 1, dtype=np.uint64)
    with Scratch(ops) as scratch:
        edges_dev, counts_dev = scratch.put(edges), scratch.put(got)
        for b in blocks:
            stage(ops, timing, "count_ms", lambda: check(lib.simrank_profile_count(
                b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], b.get("row_ids"), b.get("col_ids"), edges_dev, m,
                counts_dev, ops.stream), "simrank_profile_count"))
        ops.d2h(got, counts_dev)
        ops.synchronize()
    at_least = np.cumsum(got[::-1].astype(np.int64))[::-1][1:]           # interval j holds the entries with j edges <= v
    out = np.empty(m, dtype=np.int64)
    out[order] = at_least
    return out


def threshold_blocks(ops, blocks, max_pairs: int, timing=None):
    """(t float64, n int) of ``threshold_for`` over ``blocks``: ``radix_select`` with one ``simrank_profile_digits`` per
    block and level."""
    lib, bits = load(), _kind(blocks)
    bins = 1 << max(DIGIT_PLAN[bits])
    host = np.empty(bins + 1, dtype=np.uint64)

    def sweep(prefix, pbits, d, want_min):
        host[:] = 0
        host[bins] = 2 ** 64 - 1
        ops.h2d(dev, host)
        for b in blocks:
            stage(ops, timing, "digits_ms", lambda: check(lib.simrank_profile_digits(
                b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], b.get("row_ids"), b.get("col_ids"), prefix, pbits,
                d, dev, dev + 8 * bins if want_min else None, ops.stream), "simrank_profile_digits"))
        ops.d2h(host, dev)
        ops.synchronize()
        return host[:1 << d].copy(), int(host[bins])

    with Scratch(ops) as scratch:
        dev = scratch.malloc(8 * (bins + 1))
        return radix_select(sweep, bits, max_pairs)


# ---- a solver's side ---------------------------------------------------------------------------------------------------------
def _kept_values(ids, vals):
    """A pruned side's lists -> (the kept off-diagonal values, the number of absent +0.0 entries)."""
    kept = ids >= 0
    n = len(ids)
    return vals[kept], n * (n - 1) - int(kept.sum())


def count_pairs(solver, j, ts) -> np.ndarray:
    lists = solver.lists(j)
    if lists is not None:
        vals, zeros = _kept_values(lists[0], lists[1])
        return np.array([int((vals >= t).sum()) + (zeros if 0.0 >= t else 0) for t in ts], dtype=np.int64)
    reader = solver._reader(j)
    if reader.n == 0:
        return np.zeros(len(ts), dtype=np.int64)
    return count_blocks(reader.ops, reader.blocks, ts)


def threshold_for(solver, j, max_pairs: int):
    lists = solver.lists(j)
    if lists is not None:
        return select_values(*_kept_values(lists[0], lists[1]), max_pairs)
    reader = solver._reader(j)
    if reader.n == 0:
        return math.inf, 0
    return threshold_blocks(reader.ops, reader.blocks, max_pairs)
