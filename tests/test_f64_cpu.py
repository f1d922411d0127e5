"""libsimrank_f64.so (include/simrank_f64.h) on a machine without a GPU: header, binding and exports agree, the header is
plain C, argument checks need no device, and ``fit(storage_precision="f64")`` refuses what it does not run before any
device work.  The main library stays at ABI 8 with 117 entry points, the select library at version 1."""
import ctypes
import re

import numpy as np
import pandas as pd
import pytest

from simrank_amd import _f64, _lib, _select
from tests import companion_abi as A


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_f64) == _f64.VERSION == 1


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_f64)


def test_main_library_and_select_library_are_unchanged():
    version, names, exports = A.main_library(_f64)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117
    assert _select.load().simrank_select_version() == _select.VERSION == 1


def test_header_is_c99_and_a_c_program_links(tmp_path):
    assert "f64 1 ok" in A.run_c99(_f64, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_f64.h"
int main(void) {
    int32_t rowptr[3] = {0, 1, 2}, col[2] = {1, 0};
    double rs[2] = {1.0, 1.0};
    simrank_f64_side s;
    simrank_f64_plan* p = NULL;
    int64_t bytes = 0, changed = 0;
    memset(&s, 0, sizeof s);
    s.n_rows = 2; s.n_cols = 2; s.nnz = 2; s.rowptr = rowptr; s.col = col; s.rowscale = rs; s.coef = 0.8;
    if (simrank_f64_version() != SIMRANK_F64_VERSION) return 1;
    if (simrank_f64_plan_bytes(&s, 1, &bytes) != SIMRANK_F64_OK || bytes <= 0) return 2;
    if (simrank_f64_plan_bytes(&s, 3, &bytes) != SIMRANK_F64_ERR_INVALID) return 3;
    if (!strlen(simrank_f64_last_error())) return 4;
    if (simrank_f64_plan_step(NULL, 1e-4, &changed) != SIMRANK_F64_ERR_INVALID) return 5;
    if (simrank_f64_plan_create(&s, 1, NULL, NULL, NULL) != SIMRANK_F64_ERR_INVALID) return 6;
    (void)p;
    printf("f64 %d ok\n", simrank_f64_version());
    return 0;
}
''')


def _side(n_rows=3, n_cols=3, rowptr=(0, 1, 2, 3), col=(1, 2, 0), **kw):
    keep = [np.asarray(rowptr, dtype=np.int32), np.asarray(col, dtype=np.int32), np.ones(n_rows)]
    s = _f64.Side(n_rows=n_rows, n_cols=n_cols, nnz=len(col), rowptr=keep[0].ctypes.data,
                  col=keep[1].ctypes.data if len(col) else None, rowscale=keep[2].ctypes.data, coef=0.8)
    for k, v in kw.items():
        setattr(s, k, v)
    return s, keep


def _fails(rc, pattern):
    assert rc == _f64.ERR_INVALID
    msg = _f64.load().simrank_f64_last_error().decode()
    assert re.search(pattern, msg), msg


def test_null_and_out_of_range_arguments_fail_with_a_message():
    lib = _f64.load()
    b = ctypes.c_int64(0)
    s, keep = _side()
    assert lib.simrank_f64_plan_bytes(ctypes.byref(s), 1, ctypes.byref(b)) == 0 and b.value > 0
    _fails(lib.simrank_f64_plan_bytes(None, 1, ctypes.byref(b)), "sides is NULL")
    _fails(lib.simrank_f64_plan_bytes(ctypes.byref(s), 0, ctypes.byref(b)), "n_sides")
    _fails(lib.simrank_f64_plan_bytes(ctypes.byref(s), 1, None), "bytes is NULL")
    bad, k2 = _side(col=(1, 3, 0))
    _fails(lib.simrank_f64_plan_bytes(ctypes.byref(bad), 1, ctypes.byref(b)), "out of range")
    bad, k3 = _side(rowptr=(0, 2, 1, 3))
    _fails(lib.simrank_f64_plan_bytes(ctypes.byref(bad), 1, ctypes.byref(b)), "decreases")
    bad, k4 = _side(n_rows=3, n_cols=4)
    _fails(lib.simrank_f64_plan_bytes(ctypes.byref(bad), 1, ctypes.byref(b)), "square")
    bad, k5 = _side(n_rows=0)
    _fails(lib.simrank_f64_plan_bytes(ctypes.byref(bad), 1, ctypes.byref(b)), "bad shape")
    bad, k6 = _side(counts=1234, counts_ld=3, counts_n=2)
    _fails(lib.simrank_f64_plan_bytes(ctypes.byref(bad), 1, ctypes.byref(b)), "counts")
    s2, k7 = _side(n_rows=3, n_cols=2, rowptr=(0, 1, 2, 3), col=(1, 0, 1))
    pair = (_f64.Side * 2)(s, s2)
    _fails(lib.simrank_f64_plan_bytes(pair, 2, ctypes.byref(b)), "transpose")
    del s2, k7
    h = ctypes.c_void_p()
    _fails(lib.simrank_f64_plan_create(ctypes.byref(s), 1, None, None, None), "out is NULL")
    _fails(lib.simrank_f64_plan_create(None, 1, None, None, ctypes.byref(h)), "sides is NULL")
    assert not h.value
    changed = (ctypes.c_int64 * 2)()
    _fails(lib.simrank_f64_plan_step(None, 1e-4, changed), "NULL")
    _fails(lib.simrank_f64_plan_result(None, 0, None, 3), "plan is NULL")
    _fails(lib.simrank_f64_plan_topk(None, 0, 3, 1, None, None), "plan is NULL")
    _fails(lib.simrank_f64_plan_count_above(None, 0, 0.5, None), "plan is NULL")
    _fails(lib.simrank_f64_plan_emit_above(None, 0, 0.5, 0, None, None), "plan is NULL")
    _fails(lib.simrank_f64_plan_reset(None), "plan is NULL")
    _fails(lib.simrank_f64_plan_trim(None), "plan is NULL")
    _fails(lib.simrank_f64_plan_leg_times(None, None, None), "NULL")
    assert lib.simrank_f64_plan_destroy(None) == 0
    del keep, k2, k3, k4, k5, k6


def _df():
    return pd.DataFrame({"from": [0, 1, 2, 3], "to": [1, 2, 3, 0], "weight": [1.0, 1.0, 1.0, 1.0]})


def test_fit_refuses_what_f64_does_not_run_before_device_work(monkeypatch):
    import simrank_amd.SimRank as SRA
    from simrank_amd import estimators
    from simrank_amd.driver import LocalWorld

    def no_device(*a, **k):
        raise AssertionError("device work started")
    monkeypatch.setattr(estimators, "_default_ops_factory", no_device)
    with pytest.raises(ValueError, match="dense_precision must be 'f32'"):
        SRA.SimRank().fit(_df(), verbose=False, storage_precision="f64", dense_precision="fp16")
    with pytest.raises(ValueError, match="one GPU"):
        SRA.SimRank().fit(_df(), verbose=False, storage_precision="f64", world=LocalWorld(2))
    with pytest.raises(ValueError, match="one GPU"):
        SRA.SimRankPP().fit(_df(), verbose=False, storage_precision="f64", world=LocalWorld(4))
    with pytest.raises(ValueError, match="mode 'auto' or 'sparse'"):
        SRA.SimRank().fit(_df(), verbose=False, storage_precision="f64", mode="dense")
    with pytest.raises(ValueError, match="^storage_precision must be"):
        SRA.SimRank().fit(_df(), verbose=False, storage_precision="f128")
    with pytest.raises(ValueError, match="^storage_precision must be"):
        SRA.BipartiteSimRank().fit(pd.DataFrame({"user": [1, 2], "item": [3, 3]}), verbose=False,
                                   storage_precision="double")


def test_fit_refuses_f64_on_a_torch_world(monkeypatch):
    from simrank_amd import cdouble
    from simrank_amd.driver import LocalWorld, TorchWorld

    class FakeTorchWorld(TorchWorld):
        def __init__(self):
            self.size, self.rank = 1, 0

    why = cdouble.refusal(FakeTorchWorld.__new__(FakeTorchWorld), [], "auto", None)
    assert why is not None and "one GPU" in why
    assert cdouble.refusal(LocalWorld(1), [], "auto", None) is None
    assert "injected engine" in cdouble.refusal(LocalWorld(1), [], "auto", lambda r: None)
