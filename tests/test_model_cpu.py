"""libsimrank_model.so (include/simrank_model.h), ``compact()`` / ``save()`` / ``load_model()`` on a machine without a
GPU: header, binding and exports agree, the header is plain C99 and stands alone, argument checks need no device, the
file's header round-trips with int, big-int and str labels, every malformed file is a ValueError, and the public calls
refuse what they do not serve before any device work.  The main library's ABI stays at version 8 with 117 entry points."""
import io
import json
import struct

import numpy as np
import pytest

import simrank_amd
import simrank_amd.SimRank as SRA
from simrank_amd import _model
from tests import companion_abi as A

CLASSES = ["SimRank", "SimRankPP", "AprioriSimRank", "BipartiteSimRank", "BipartiteSimRankPP", "BipartitleAprioriSimRank"]


def test_header_binding_and_exports_agree():
    assert A.loaded_version(_model) == _model.VERSION == 1
    A.assert_header_stands_alone(_model)


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_model)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_model)


def test_layout_codes_are_the_shared_ones():
    from simrank_amd import _companion
    want = {"PANEL_F32": 0, "ROWMAJOR_F32": 1, "PANEL_F16": 2, "ROWMAJOR_F64": 3}
    assert A.layout_codes(_model) == want
    for name, value in want.items():
        assert getattr(_model, name) == getattr(_companion, name) == value


def test_main_library_abi_is_unchanged():
    version, names, exports = A.main_library(_model)
    assert version == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_a_c_program_links(tmp_path):
    assert "model 1 ok" in A.run_c99(_model, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_model.h"
int main(void) {
    float src[16], dst[16];
    int64_t count = 0;
    if (simrank_model_version() != SIMRANK_MODEL_VERSION) return 1;
    if (simrank_model_pack(src, 9, 4, 4, 4, NULL, NULL, NULL, 4, dst, SIMRANK_MODEL_ROWMAJOR_F32, 4, 4, 4, NULL, NULL)
        != SIMRANK_MODEL_ERR_INVALID) return 2;                                   /* unknown source layout */
    if (!strstr(simrank_model_last_error(), "layout")) return 3;
    if (simrank_model_pack(src, SIMRANK_MODEL_ROWMAJOR_F32, 4, 4, 4, NULL, NULL, NULL, 4, dst, SIMRANK_MODEL_ROWMAJOR_F64, 4,
                           4, 4, NULL, NULL) != SIMRANK_MODEL_ERR_INVALID) return 4;      /* a pair that is not packed */
    if (simrank_model_pack(src, SIMRANK_MODEL_ROWMAJOR_F32, 4, 4, 4, NULL, NULL, NULL, 4, dst, SIMRANK_MODEL_PANEL_F16, 4,
                           4, 4, NULL, NULL) != SIMRANK_MODEL_ERR_INVALID) return 5;      /* converting without a counter */
    if (simrank_model_pack(src, SIMRANK_MODEL_ROWMAJOR_F32, 2, 4, 4, NULL, NULL, NULL, 4, dst, SIMRANK_MODEL_ROWMAJOR_F32, 4,
                           4, 4, NULL, NULL) != SIMRANK_MODEL_ERR_INVALID) return 6;      /* stride below the columns */
    if (simrank_model_pack(src, SIMRANK_MODEL_ROWMAJOR_F32, 4, 4, 4, NULL, NULL, NULL, 4, dst, SIMRANK_MODEL_ROWMAJOR_F32, 8,
                           8, 8, NULL, NULL) != SIMRANK_MODEL_ERR_INVALID) return 7;      /* more rows than the source, no map */
    if (simrank_model_pack(NULL, SIMRANK_MODEL_PANEL_F16, 0, 0, 0, NULL, NULL, NULL, 0, NULL, SIMRANK_MODEL_PANEL_F16, 0, 0,
                           0, &count, NULL) != SIMRANK_MODEL_OK) return 8;                 /* nothing asked: no device touched */
    printf("model %d ok\n", simrank_model_version());
    return 0;
}
''')


# ---- the file ------------------------------------------------------------------------------------------------------------
def _meta(labels, kind, n=3, storage="f32", cls="SimRank"):
    layout, stride, nbytes = _model.block_shape(storage, n)
    side = dict(n=n, n_src=n, nnz=2, layout=layout, stride=stride, C=0.8, lbd=0.0, evidence=False, prior=False,
                labels=labels, label_kind=kind)
    dtype = _model.STORAGES[storage][1]
    arrays = [("iterate0", dtype.str, [nbytes // dtype.itemsize]), ("rowptr0", "<i4", [n + 1]), ("col0", "<i4", [2]),
              ("rowscale0", "<f8", [n])]
    meta = {"class": cls, "weighted": False, "strict": False, "storage": storage, "sides": [side]}
    return meta, arrays


def _file(meta, arrays, tail=True):
    f = io.BytesIO()
    where = _model.write_header(f, meta, arrays)
    if tail:
        f.write(b"\0" * (max(o + n for o, n in where.values()) - f.tell()))
    return f, where


@pytest.mark.parametrize("labels", [[3, 1, 2], [2 ** 80 + 1, -(2 ** 70), 0], ["b", "a", "ç"], [1, "1", 2],
                                    list(np.array([5, 7, 9], dtype=np.int64)), list(np.array([5, 7, 9], dtype=np.uint32))])
def test_header_round_trips_with_the_labels_types(labels):
    items, kind = _model.encode_labels(labels)
    meta, arrays = _meta(items, kind)
    f, where = _file(meta, arrays)
    f.seek(0)
    got, listed = _model.parse_header(f, len(f.getvalue()))
    _model.check_meta(got, listed)
    assert {k: got[k] for k in meta} == json.loads(json.dumps(meta)) and got["format"] == _model.FORMAT_VERSION
    assert {k: (v["offset"], v["nbytes"]) for k, v in listed.items()} == where
    assert all(o % 64 == 0 for o, _ in where.values())
    back = _model.decode_labels(got["sides"][0]["labels"], got["sides"][0]["label_kind"])
    assert back == labels and [type(x) for x in back] == [type(x) for x in labels]


@pytest.mark.parametrize("bad", [1.5, np.float64(2.0), True, None, (1, 2), b"x"])
def test_a_label_of_another_type_is_refused_by_name(bad):
    with pytest.raises(ValueError, match=type(bad).__name__):
        _model.encode_labels([1, bad] if not isinstance(bad, np.generic) else [bad, bad])


def _load_bytes(tmp_path, data):
    p = tmp_path / "m.simrank"
    p.write_bytes(data)
    return simrank_amd.load_model(p)


def test_malformed_files_are_value_errors_before_any_device_work(tmp_path):
    """No GPU here: anything that got past the checks would fail with another error."""
    meta, arrays = _meta([1, 2, 3], "py")
    good = _file(meta, arrays)[0].getvalue()
    with pytest.raises(ValueError, match="prefix"):
        _load_bytes(tmp_path, good[:10])
    with pytest.raises(ValueError, match="magic"):
        _load_bytes(tmp_path, b"NOTMODEL" + good[8:])
    with pytest.raises(ValueError, match="format version 2"):
        _load_bytes(tmp_path, good[:8] + struct.pack("<I", 2) + good[12:])
    with pytest.raises(ValueError, match="truncated inside its header"):
        _load_bytes(tmp_path, good[:40])
    with pytest.raises(ValueError, match="truncated"):
        _load_bytes(tmp_path, good[:-8])
    with pytest.raises(ValueError, match="truncated"):
        _load_bytes(tmp_path, _file(meta, arrays, tail=False)[0].getvalue())
    # arrays that disagree with the header's sides
    short = [(n, d, [s[0] - 1] if n == "iterate0" else s) for n, d, s in arrays]
    with pytest.raises(ValueError, match="iterate0"):
        _load_bytes(tmp_path, _file(meta, short)[0].getvalue())
    wrong = [(n, "<f8" if n == "iterate0" else d, s) for n, d, s in arrays]
    with pytest.raises(ValueError, match="iterate0"):
        _load_bytes(tmp_path, _file(meta, wrong)[0].getvalue())
    with pytest.raises(ValueError, match="col0"):
        _load_bytes(tmp_path, _file(meta, [a for a in arrays if a[0] != "col0"])[0].getvalue())
    for change in (dict(storage="f16"), {"class": "Nope"}, dict(sides=[]), dict(sides=meta["sides"] * 2)):
        with pytest.raises(ValueError):
            _load_bytes(tmp_path, _file(dict(meta, **change), arrays)[0].getvalue())
    for key, value in (("stride", 3), ("layout", 2), ("labels", [1, 2]), ("label_kind", "<f8"), ("n_src", 4)):
        side = dict(meta["sides"][0], **{key: value})
        with pytest.raises(ValueError):
            _load_bytes(tmp_path, _file(dict(meta, sides=[side]), arrays)[0].getvalue())
    # a header whose length says more than the file holds, and one that is not JSON
    with pytest.raises(ValueError, match="truncated"):
        _load_bytes(tmp_path, good[:12] + struct.pack("<Q", 1 << 40) + good[20:])
    length = struct.unpack("<Q", good[12:20])[0]
    with pytest.raises(ValueError, match="JSON"):
        _load_bytes(tmp_path, good[:20] + b"{" * length + good[20 + length:])
    # the CSR's own offsets are checked too (the arrays are all zeros here: they do not describe 2 entries)
    with pytest.raises(ValueError, match="row offsets"):
        _load_bytes(tmp_path, good)


def test_block_shapes():
    assert _model.block_shape("f32", 33) == (_model.ROWMAJOR_F32, 36, 33 * 36 * 4)
    assert _model.block_shape("f64", 33) == (_model.ROWMAJOR_F64, 34, 33 * 34 * 8)
    assert _model.block_shape("fp16", 65) == (_model.PANEL_F16, 65, 2 * 65 * 64 * 2)
    assert _model.block_shape("f32", 32768)[2] == 4 * 32768 ** 2 and _model.block_shape("fp16", 32768)[2] == 2 * 32768 ** 2


# ---- the public calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_compact_and_save_need_a_kept_model(cls, tmp_path):
    est = getattr(SRA, cls)()
    with pytest.raises(ValueError, match="precision"):
        est.compact(precision="bogus")
    with pytest.raises(ValueError, match="precision"):
        est.compact(precision="f64")
    for call in (est.compact, lambda: est.compact(precision="fp16"), lambda: est.save(tmp_path / "m"),
                 lambda: est.device_bytes):
        with pytest.raises(RuntimeError, match="no kept model"):
            call()
    est.release()
    est._model_released = True                     # what release() of a kept model leaves behind
    for call in (est.compact, lambda: est.save(tmp_path / "m")):
        with pytest.raises(RuntimeError, match="released"):
            call()
    assert not (tmp_path / "m").exists()


class _Stub(_model.DetachedSolver):
    """A detached solver without a device: what ``save`` reads before it touches one."""

    def __init__(self, specs):
        self.specs, self.blocks, self.n, self.storage, self.ops = specs, [], [3], "f32", {0: None}


def test_a_float_label_raises_at_save(tmp_path):
    from simrank_amd.driver import SideSpec
    from simrank_amd.ingest import CSR
    csr = CSR(3, 3, np.array([0, 1, 2, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32), np.ones(3))
    est = SRA.SimRank()
    est._keep(_Stub([SideSpec(csr, csr.rowscale, 0.8)]), [(0, [0.5, 1.5, 2.5])])
    with pytest.raises(ValueError, match="float"):
        est.save(tmp_path / "m")
    assert not (tmp_path / "m").exists()
    est._model = None


def test_load_model_is_exported():
    assert simrank_amd.load_model is simrank_amd.estimators.load_model
