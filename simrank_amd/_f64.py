"""ctypes binding of libsimrank_f64.so (include/simrank_f64.h): the reference's float64 loop on one GPU.

A companion of libsimrank_hip.so with its own header, version and binding, so that the main library's C ABI stays as it
is; it takes the u8 evidence counts the main library makes (``HipOps.evidence_counts``) as a device pointer.  No CPU
fallback: a missing library or device is an error.
"""
from __future__ import annotations

import ctypes as C

from ._companion import Companion

VERSION = 1              # SIMRANK_F64_VERSION of include/simrank_f64.h
ERR_INVALID, ERR_HIP, ERR_MEMORY = -1, -2, -3

_vp, _i64, _i32, _f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double


class Side(C.Structure):                       # struct simrank_f64_side
    _fields_ = [("n_rows", _i64), ("n_cols", _i64), ("nnz", _i64), ("rowptr", _vp), ("col", _vp), ("rowscale", _vp),
                ("coef", _f64), ("counts", _vp), ("counts_ld", _i64), ("counts_n", _i64), ("prior", _vp), ("lbd", _f64)]


class Options(C.Structure):                    # struct simrank_f64_options
    _fields_ = [("symmetric", _i32)]


# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_f64_version": [],
    "simrank_f64_last_error": [],
    "simrank_f64_plan_bytes": [C.POINTER(Side), _i32, C.POINTER(_i64)],
    "simrank_f64_mem_info": [C.POINTER(_i64), C.POINTER(_i64)],
    "simrank_f64_plan_create": [C.POINTER(Side), _i32, C.POINTER(Options), _vp, C.POINTER(_vp)],
    "simrank_f64_plan_destroy": [_vp],
    "simrank_f64_plan_reset": [_vp],
    "simrank_f64_plan_step": [_vp, _f64, C.POINTER(_i64)],
    "simrank_f64_plan_set_timing": [_vp, _i32],
    "simrank_f64_plan_leg_times": [_vp, C.POINTER(_f64), C.POINTER(_i32)],
    "simrank_f64_plan_result": [_vp, _i32, _vp, _i64],
    "simrank_f64_plan_topk": [_vp, _i32, _i32, _i32, _vp, _vp],
    "simrank_f64_plan_count_above": [_vp, _i32, _f64, _vp],
    "simrank_f64_plan_emit_above": [_vp, _i32, _f64, _i64, _vp, _vp],
    "simrank_f64_plan_trim": [_vp],
    "simrank_f64_plan_get": [_vp, _i32, C.c_char_p, C.POINTER(_i64)],
}
_RESTYPES = {"simrank_f64_last_error": C.c_char_p}


class F64Error(RuntimeError):
    """A call into libsimrank_f64.so failed."""


class F64MemoryError(F64Error, MemoryError):
    """The device has too little free memory for an f64 plan."""


_c = Companion("f64", VERSION, PROTOTYPES, _RESTYPES, F64Error, {ERR_MEMORY: F64MemoryError})
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check
