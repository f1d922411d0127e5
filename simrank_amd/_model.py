"""A kept model that is not a plan: ctypes binding of libsimrank_model.so (include/simrank_model.h), the solver that
holds one packed matrix per side (``DetachedSolver``), and the file a model is saved to.

``detach`` packs every side of a kept solver's iterate into one device block in the caller's order (f32 row-major,
fp16-held 64-column panels or float64 row-major) through ``simrank_model_pack``; ``DetachedSolver`` answers every query
of ``_query.SolverQueries`` on that block with identity orders (no column maps), and ``fold_in`` from the few host arrays
of the specs.  ``detach`` is also what ``_query.SolverQueries.one_block`` packs a side held in several column blocks
with, for the one call that needs one block; ``_kept`` calls it for ``compact`` and ``save``.  ``save`` / ``load`` write and read such a solver as one file: a JSON header and raw little-endian arrays,
moved between the device and the file in bands.  No CPU fallback: a missing library or device is an error.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import os
import struct

import numpy as np

from ._companion import PANEL_F16, PANEL_F32, ROWMAJOR_F32, ROWMAJOR_F64, Companion  # noqa: F401 (a block's layouts)
from ._driver import Scratch, bands, stage
from ._query import SolverQueries

VERSION = 1              # SIMRANK_MODEL_VERSION of include/simrank_model.h

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_model_version": [],
    "simrank_model_last_error": [],
    "simrank_model_pack": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _i32, _i64, _i64, _i64, _vp, _vp],
}
_RESTYPES = {"simrank_model_last_error": C.c_char_p}


class ModelError(RuntimeError):
    """A call into libsimrank_model.so failed."""


_c = Companion("model", VERSION, PROTOTYPES, _RESTYPES, ModelError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check

STORAGES = {"f32": (ROWMAJOR_F32, np.dtype("<f4")), "fp16": (PANEL_F16, np.dtype("<f2")), "f64": (ROWMAJOR_F64, np.dtype("<f8"))}
_STORAGE_OF_LAYOUT = {PANEL_F32: "f32", ROWMAJOR_F32: "f32", PANEL_F16: "fp16", ROWMAJOR_F64: "f64"}

BAND_BYTES = 256 << 20   # what crosses between the device and a file at a time


def check_precision(precision):
    """``compact(precision=...)``: None (the model's storage) or "fp16" (ValueError otherwise; nothing touches a device)."""
    if precision not in (None, "fp16"):
        raise ValueError(f"precision must be None (keep the model's storage) or 'fp16', not {precision!r}")
    return precision


def block_shape(storage: str, n: int):
    """(layout, stride, bytes) of the packed block of an n-node side: f32 row-major with 16-byte rows, fp16-held 64-column
    panels of n rows, or float64 row-major."""
    layout, dtype = STORAGES[storage]
    if layout == PANEL_F16:
        return layout, n, -(-n // 64) * n * 64 * 2
    unit = 16 // dtype.itemsize
    stride = -(-n // unit) * unit
    return layout, stride, n * stride * dtype.itemsize


def block_bytes(b: dict) -> int:
    """Bytes of a block as ``engine._iterate_block`` describes it."""
    if b["layout"] == PANEL_F32:
        return -(-b["cols"] // 32) * b["stride"] * 32 * 4
    if b["layout"] == PANEL_F16:
        return -(-b["cols"] // 64) * b["stride"] * 64 * 2
    return b["rows"] * b["stride"] * (8 if b["layout"] == ROWMAJOR_F64 else 4)


# ---- packing -----------------------------------------------------------------------------------------------------------
class Block:
    """One side's packed matrix on the device (the engine's pooled allocator), zeroed, with the identity ids the selection
    library reads the rows' and columns' ids from."""

    def __init__(self, ops, storage: str, n: int):
        from .engine import check as hip_check
        self.ops, self.storage, self.n = ops, storage, int(n)
        self.layout, self.stride, self.nbytes = block_shape(storage, self.n)
        self.ptr = ops._malloc(self.nbytes)
        self.ids = None
        try:
            if self.nbytes:
                hip_check(ops.lib.simrank_memset(C.c_void_p(self.ptr), 0, self.nbytes, ops.stream), "simrank_memset")
            self.ids = ops.put(np.arange(self.n, dtype=np.int32))
            ops.synchronize()
        except Exception:
            self.free()
            raise

    def describe(self) -> dict:
        """The block as ``_query.Reader``, ``engine.Selection`` and ``_foldin.Folder`` take one."""
        return dict(ptr=self.ptr, layout=self.layout, stride=self.stride, rows=self.n, cols=self.n, col_lo=0,
                    row_ids=self.ids, col_ids=self.ids)

    def free(self):
        for name in ("ptr", "ids"):
            p = getattr(self, name, None)
            if p:
                self.ops._free(p)
            setattr(self, name, None)


def pack_reader(reader, dst: Block, overflow_dev=None, timing=None):
    """Queue the packs of every column block of ``reader``'s iterate into ``dst`` (one call per block).  ``timing``: a list
    that receives the kernels' milliseconds (HIP events)."""
    ops, lib, n = reader.ops, load(), reader.n
    identity = np.array_equal(reader.order, np.arange(n, dtype=np.int32))
    with Scratch(ops) as scratch:
        row_map = None if identity else scratch.put(reader.inv)
        for i, b in enumerate(reader.blocks):
            if not b["cols"]:
                continue
            cmap, ids = reader._col_map(i)             # (positions within the block sorted by caller id, those ids)
            whole = b["col_lo"] == 0 and b["cols"] == n
            col_dst = None if whole else scratch.put(np.ascontiguousarray(ids, dtype=np.int32))
            stage(ops, timing, "pack_ms", lambda: check(lib.simrank_model_pack(
                b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], row_map, col_dst, cmap, b["cols"], dst.ptr,
                dst.layout, dst.stride, n, n, overflow_dev, ops.stream), "simrank_model_pack"))


def storage_of(solver, j=0) -> str:
    """"f32" | "fp16" | "f64": what the solver's iterates are held in (from its specs: no device work)."""
    return getattr(solver, "storage", None) or solver.specs[j].storage


def detach(solver, precision=None) -> "DetachedSolver":
    """A ``DetachedSolver`` holding copies of every side of ``solver``'s iterate (a kept plan solver or a detached one);
    ``solver`` is left as it is.  ``precision="fp16"`` narrows f32 sides to the fp16-held form; a value binary16 cannot
    hold is a ValueError that names how many there are, with nothing of ``solver`` changed."""
    check_precision(precision)
    sides = range(len(solver.n))
    have = [storage_of(solver, j) for j in sides]
    if precision == "fp16" and "f64" in have:
        raise ValueError("compact(precision='fp16') narrows f32 models; this one holds float64 (storage_precision='f64'): "
                         "use compact() to keep it")
    ops = next(iter(solver.ops.values()))
    blocks, got = [], np.zeros(1, dtype=np.int64)
    try:
        with Scratch(ops) as scratch:
            count_dev = None                             # (the values binary16 cannot hold, counted over the sides)
            for j in sides:
                want = "fp16" if precision == "fp16" else have[j]
                dst = Block(ops, want, solver.n[j])
                blocks.append(dst)
                if want != have[j]:
                    if count_dev is None:
                        count_dev = scratch.put(got)
                    pack_reader(solver._reader(j), dst, count_dev)
                else:
                    pack_reader(solver._reader(j), dst)
            if count_dev is not None:
                ops.d2h(got, count_dev)
        overflow = int(got[0])
        if overflow:
            raise ValueError(f"compact(precision='fp16'): {overflow} values do not fit the fp16-held form (value x 2^14 in "
                             f"binary16: magnitudes up to 3.998); the model is unchanged")
    except Exception:
        for b in blocks:
            b.free()
        raise
    specs = [dataclasses.replace(s, apriori=None if s.apriori is None else _HAS_PRIOR) for s in solver.specs]
    return DetachedSolver(ops, specs, blocks, mode=getattr(solver, "mode", "sparse"), fitted=solver)


_HAS_PRIOR = np.empty((0, 0))        # stands for a prior matrix the model no longer holds (fold_in asks only whether there was one)


class DetachedSolver(SolverQueries):
    """The queries of a kept model over one packed device block per side, in the caller's order: no plan, no matrices of
    the loop.  ``specs``: per side the CSR, row scale, coefficient, ``lbd``, evidence and prior flags ``fold_in`` reads.
    ``fitted``: the released solver a compacted model came from, which still holds the evidence counts (None for a model
    that was loaded from a file)."""

    def __init__(self, ops, specs, blocks, mode="sparse", fitted=None):
        self.ops = {0: ops}
        self.specs = list(specs)
        self.blocks = list(blocks)
        self.n = [b.n for b in self.blocks]
        self.bipartite = len(self.blocks) == 2
        self.storage = self.blocks[0].storage
        self.mode = mode
        self.fitted = fitted

    @property
    def device_bytes(self) -> int:
        return sum(b.nbytes for b in self.blocks)

    def _block(self, j):
        if j >= len(self.blocks) or not self.blocks[j].ptr and self.blocks[j].nbytes:
            raise ValueError("the model's matrices were released")
        return self.blocks[j]

    def _make_reader(self, j):
        """``_query.Reader`` over side j's own block: identity order, so no column maps."""
        from . import _query
        b = self._block(j)
        return _query.Reader(self.ops[0], [b.describe()], np.arange(b.n, dtype=np.int32))

    def result(self, j=0):
        return self.rows(j, np.arange(self.n[j], dtype=np.int32))

    def topk(self, j, k, exclude_diag=True):
        if not exclude_diag:
            raise ValueError("a detached model selects the k most similar OTHER nodes")
        return self.topk_of(j, np.arange(self.n[j], dtype=np.int32), k)

    def pairs(self, j, t, max_pairs):
        """Side j's pairs at least ``t`` similar in the caller's order: (offsets [n + 1], neighbour ids, values).  f32 and
        fp16-held blocks: ``engine.Selection`` (libsimrank_select.so) in place.  float64 blocks, which that library does
        not read: the rows come back in bands through the query library and are compared in float64 on the host."""
        from .engine import Selection, _pairs_above
        b = self._block(j)
        if b.layout != ROWMAJOR_F64:
            return _pairs_above(Selection(self.ops[0], [b.describe()], t), max_pairs)
        from ._select import too_many
        n, reader = b.n, self._reader(j)
        offsets = np.zeros(n + 1, dtype=np.int64)
        ids, vals, total = [], [], 0
        for r0, m in bands(n, 8 * max(1, n)):
            rows = np.arange(r0, r0 + m, dtype=np.int32)
            got = reader.rows(rows)
            hit = got >= float(t)
            hit[np.arange(rows.size), rows] = False
            offsets[r0 + 1:r0 + 1 + rows.size] = hit.sum(axis=1)
            total += int(hit.sum())
            if max_pairs is None or total <= max_pairs:
                rr, cc = np.nonzero(hit)
                ids.append(cc.astype(np.int32))
                vals.append(got[rr, cc])
        if max_pairs is not None and total > max_pairs:
            raise too_many(total, max_pairs)
        np.cumsum(offsets, out=offsets)
        return (offsets, np.concatenate(ids) if ids else np.empty(0, dtype=np.int32),
                np.concatenate(vals) if vals else np.empty(0, dtype=np.float64))

    def evidence(self, j=0):
        """Evidence matrix of side j from the counts the released solver still keeps."""
        if self.fitted is None or not hasattr(self.fitted, "evidence"):
            raise AttributeError("this model was loaded from a file, not fitted: it holds no evidence counts")
        return self.fitted.evidence(j)

    def release(self):
        self._close_readers()
        for b in self.blocks:
            b.free()


# ---- the file -----------------------------------------------------------------------------------------------------------
# MAGIC, u32 format version, u64 length of the JSON header, the header (UTF-8), zero padding to a multiple of 64, then the
# arrays the header lists, each at its "offset" from the start of the file (multiples of 64), little-endian, C order.
MAGIC = b"SIMRANKM"
FORMAT_VERSION = 1
_PREFIX = struct.Struct("<8sIQ")
_ALIGN = 64
_DTYPES = {"<f2", "<f4", "<f8", "<i4"}
FORMS = ("dense", "neighbors")      # header "form": one packed matrix per side (the default), or per-node neighbour lists
CLASSES = ("SimRank", "SimRankPP", "AprioriSimRank", "BipartiteSimRank", "BipartiteSimRankPP", "BipartitleAprioriSimRank")


def encode_labels(labels):
    """-> (JSON list, kind): Python ``int`` of any size and ``str`` as they are (kind "py"), or the integers of ONE NumPy
    integer type (kind = its dtype string, e.g. "<i8").  Any other type is a ValueError that names it."""
    labels = list(labels)
    kinds = {type(x) for x in labels}
    if kinds <= {int, str}:
        return labels, "py"
    if len(kinds) == 1:
        (t,) = kinds
        if isinstance(t, type) and issubclass(t, np.integer):
            return [int(x) for x in labels], np.dtype(t).newbyteorder("<").str
    bad = sorted(t.__name__ for t in kinds if t not in (int, str) and not (isinstance(t, type) and issubclass(t, np.integer)))
    raise ValueError(f"save() writes labels that are Python int or str (or the integers of one NumPy integer type), not "
                     f"{', '.join(bad) or 'a mix of ' + ', '.join(sorted(t.__name__ for t in kinds))}")


def decode_labels(items, kind):
    if kind == "py":
        for x in items:
            if type(x) not in (int, str):
                raise ValueError(f"the file's labels hold a {type(x).__name__}")
        return list(items)
    try:
        dt = np.dtype(kind)
    except TypeError as e:
        raise ValueError(f"the file names an unknown label type {kind!r}") from e
    if dt.kind not in "iu" or not all(type(x) is int for x in items):
        raise ValueError(f"the file names the label type {kind!r} for labels that are not integers")
    return list(np.asarray(items, dtype=dt.newbyteorder("="))) if items else []


def write_header(f, meta: dict, arrays):
    """Write the prefix and the header for ``arrays`` = [(name, dtype string, shape)] and return {name: (offset, nbytes)}:
    where each array's bytes go."""
    listed, fixed = [], None
    for _ in range(8):               # (the offsets depend on the header's length, which depends on their digits)
        head = json.dumps(dict(meta, format=FORMAT_VERSION, arrays=listed), separators=(",", ":")).encode("utf-8")
        pos = -(-(_PREFIX.size + len(head)) // _ALIGN) * _ALIGN
        if fixed == pos:
            break
        fixed, at, listed = pos, pos, []
        for name, dtype, shape in arrays:
            nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize if len(shape) else np.dtype(dtype).itemsize
            listed.append(dict(name=name, dtype=dtype, shape=[int(s) for s in shape], offset=at, nbytes=nbytes))
            at = -(-(at + nbytes) // _ALIGN) * _ALIGN
    else:
        raise AssertionError("the header's length did not settle")
    f.write(_PREFIX.pack(MAGIC, FORMAT_VERSION, len(head)))
    f.write(head)
    f.write(b"\0" * (fixed - _PREFIX.size - len(head)))
    return {a["name"]: (a["offset"], a["nbytes"]) for a in listed}


def parse_header(f, file_size=None):
    """-> (meta dict, {name: dict(dtype, shape, offset, nbytes)}) of an open file, checked against its size: a truncated
    file, a wrong magic, a newer format or arrays that disagree with the header are a ValueError."""
    if file_size is None:
        file_size = os.fstat(f.fileno()).st_size
    raw = f.read(_PREFIX.size)
    if len(raw) < _PREFIX.size:
        raise ValueError("not a saved model: the file is shorter than its prefix")
    magic, version, length = _PREFIX.unpack(raw)
    if magic != MAGIC:
        raise ValueError("not a saved model: wrong magic")
    if version > FORMAT_VERSION or version < 1:
        raise ValueError(f"the file has format version {version}; this library reads up to {FORMAT_VERSION}")
    if length > file_size - _PREFIX.size:
        raise ValueError("the file is truncated inside its header")
    try:
        meta = json.loads(f.read(length).decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise ValueError(f"the file's header is not JSON: {e}") from e
    if not isinstance(meta, dict) or not isinstance(meta.get("arrays"), list):
        raise ValueError("the file's header lists no arrays")
    if meta.get("format") != version:
        raise ValueError("the header's format version disagrees with the prefix")
    arrays, end = {}, _PREFIX.size + length
    for a in meta["arrays"]:
        try:
            name, dtype, shape, offset, nbytes = a["name"], a["dtype"], [int(s) for s in a["shape"]], int(a["offset"]), int(a["nbytes"])
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError(f"a malformed array entry in the header: {a!r}") from e
        if dtype not in _DTYPES or any(s < 0 for s in shape):
            raise ValueError(f"array {name!r}: bad dtype or shape")
        if nbytes != int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize:
            raise ValueError(f"array {name!r}: {nbytes} bytes disagree with its shape {shape} of {dtype}")
        if offset < end or offset % _ALIGN:
            raise ValueError(f"array {name!r}: bad offset {offset}")
        if offset + nbytes > file_size:
            raise ValueError(f"the file is truncated: array {name!r} ends at byte {offset + nbytes} of {file_size}")
        end = offset + nbytes
        arrays[name] = dict(dtype=dtype, shape=shape, offset=offset, nbytes=nbytes)
    return meta, arrays


def _expect(arrays, name, dtype, shape):
    a = arrays.get(name)
    if a is None:
        raise ValueError(f"the file holds no array {name!r}")
    if a["dtype"] != dtype or a["shape"] != [int(s) for s in shape]:
        raise ValueError(f"array {name!r} is {a['dtype']} {a['shape']}; the header's sides ask for {dtype} {list(shape)}")
    return a


def check_meta(meta, arrays):
    """The header's model description against itself and its arrays (ValueError), before any device allocation."""
    try:
        cls, storage, sides = meta["class"], meta["storage"], meta["sides"]
        bool(meta["weighted"]), bool(meta["strict"])
    except KeyError as e:
        raise ValueError(f"the file's header lacks {e}") from e
    if cls not in CLASSES:
        raise ValueError(f"the file names an unknown class {cls!r}")
    if storage not in STORAGES:
        raise ValueError(f"the file names an unknown storage {storage!r}")
    form = meta.get("form", "dense")                       # (a file from before the neighbour-list form names none)
    if form not in FORMS:
        raise ValueError(f"the file names an unknown form {form!r}")
    if not isinstance(sides, list) or len(sides) != (2 if "ipartit" in cls else 1):
        raise ValueError(f"{cls} has {2 if 'ipartit' in cls else 1} side(s); the file describes {len(sides) if isinstance(sides, list) else sides!r}")
    for j, s in enumerate(sides):
        try:
            n, n_src, nnz = int(s["n"]), int(s["n_src"]), int(s["nnz"])
            float(s["C"]), float(s["lbd"]), bool(s["evidence"]), bool(s["prior"])
            labels, kind = s["labels"], s["label_kind"]
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError(f"side {j} of the header is malformed: {e}") from e
        if n < 0 or n_src < 0 or nnz < 0:
            raise ValueError(f"side {j}: negative sizes")
        if not isinstance(labels, list) or len(labels) != n:
            raise ValueError(f"side {j}: {len(labels) if isinstance(labels, list) else 'no'} labels for {n} nodes")
        decode_labels(labels[:0], kind)
        if form == "neighbors":
            from ._neighbors import MAX_K, clamp_k
            k = s.get("k")
            if type(k) is not int or k < 1 or k > MAX_K or k != clamp_k(k, n):
                raise ValueError(f"side {j}: k = {k!r} kept neighbours disagree with {n} nodes (at most {MAX_K})")
            _expect(arrays, f"nbr_ids{j}", "<i4", [n, k])
            _expect(arrays, f"nbr_vals{j}", "<f8", [n, k])
            _expect(arrays, f"diag{j}", "<f8", [n])
        else:
            layout, stride, nbytes = block_shape(storage, n)
            if s.get("layout") != layout or s.get("stride") != stride:
                raise ValueError(f"side {j}: layout {s.get('layout')} / stride {s.get('stride')} / sizes disagree with {n} "
                                 f"nodes held as {storage}")
            dtype = STORAGES[storage][1].str
            _expect(arrays, f"iterate{j}", dtype, [nbytes // np.dtype(dtype).itemsize])
        _expect(arrays, f"rowptr{j}", "<i4", [n + 1])
        _expect(arrays, f"col{j}", "<i4", [nnz])
        _expect(arrays, f"rowscale{j}", "<f8", [n])
    if len(sides) == 2 and (sides[0]["n_src"] != sides[1]["n"] or sides[1]["n_src"] != sides[0]["n"]):
        raise ValueError("the two sides' patterns are not each other's transpose")
    if len(sides) == 1 and sides[0]["n_src"] != sides[0]["n"]:
        raise ValueError("the side's pattern is not square")


def save(path, solver, meta: dict, labels):
    """Write ``solver`` (a ``DetachedSolver``, or the ``_neighbors.NeighborSolver`` of a pruned model) to ``path``:
    ``meta`` = class, weighted, strict; ``labels`` one list per side.  The blocks come from the device in bands of at most
    ``BAND_BYTES``; a pruned model's tables, which are small, in one copy each."""
    ops = solver.ops[0]
    pruned = not isinstance(solver, DetachedSolver)
    sides, arrays, host = [], [], {}
    for j, s in enumerate(solver.specs):
        items, kind = encode_labels(labels[j])
        csr = s.csr
        side = dict(n=solver.n[j], n_src=int(csr.n_cols), nnz=int(csr.nnz), C=float(s.coef),
                    lbd=float(s.lbd), evidence=s.evidence_from is not None, prior=s.apriori is not None,
                    labels=items, label_kind=kind)
        if pruned:
            t = solver.tables[j]
            side["k"] = t.k
            ids, vals, diag = t.host()
            host[f"nbr_ids{j}"] = np.ascontiguousarray(ids, dtype="<i4")
            host[f"nbr_vals{j}"] = np.ascontiguousarray(vals, dtype="<f8")
            host[f"diag{j}"] = np.ascontiguousarray(diag, dtype="<f8")
            for name in (f"nbr_ids{j}", f"nbr_vals{j}", f"diag{j}"):
                arrays.append((name, host[name].dtype.str, list(host[name].shape)))
        else:
            b = solver.blocks[j]
            side.update(layout=b.layout, stride=b.stride)
            dtype = STORAGES[b.storage][1]
            arrays.append((f"iterate{j}", dtype.str, [b.nbytes // dtype.itemsize]))
        sides.append(side)
        host[f"rowptr{j}"] = np.ascontiguousarray(csr.rowptr, dtype="<i4")
        host[f"col{j}"] = np.ascontiguousarray(csr.col, dtype="<i4")
        host[f"rowscale{j}"] = np.ascontiguousarray(s.rowscale, dtype="<f8")
        for name in (f"rowptr{j}", f"col{j}", f"rowscale{j}"):
            arrays.append((name, host[name].dtype.str, list(host[name].shape)))
    full = dict(meta, storage=solver.storage, sides=sides)
    if pruned:
        full["form"] = "neighbors"
    blocks = [] if pruned else solver.blocks
    tmp = f"{os.fspath(path)}.part"
    stage = np.empty(min(BAND_BYTES, max((b.nbytes for b in blocks), default=0)), dtype=np.uint8)
    try:
        with open(tmp, "wb") as f:
            where = write_header(f, full, arrays)
            for j, b in enumerate(blocks):
                f.seek(where[f"iterate{j}"][0])
                for at in range(0, b.nbytes, BAND_BYTES):
                    m = min(BAND_BYTES, b.nbytes - at)
                    ops.d2h(stage[:m], b.ptr + at, m)
                    ops.synchronize()
                    f.write(memoryview(stage[:m]))
            for name, a in host.items():
                f.seek(where[name][0])
                f.write(memoryview(a).cast("B") if a.size else b"")
            end = max([o + n for o, n in where.values()] or [f.tell()])
            f.truncate(end)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def load_file(path, device=None):
    """-> (meta, DetachedSolver or (a pruned model's) NeighborSolver, [labels per side]) of a saved model.  Everything about the file is checked before the
    first device allocation; the blocks go to the device in bands of at most ``BAND_BYTES``."""
    from .driver import SideSpec
    from .ingest import CSR
    with open(path, "rb") as f:
        meta, arrays = parse_header(f)
        check_meta(meta, arrays)

        def read(name):
            a = arrays[name]
            f.seek(a["offset"])
            out = np.fromfile(f, dtype=a["dtype"], count=a["nbytes"] // np.dtype(a["dtype"]).itemsize)
            if out.nbytes != a["nbytes"]:
                raise ValueError(f"the file is truncated inside array {name!r}")
            return out.astype(np.dtype(a["dtype"]).newbyteorder("="), copy=False)

        labels, csrs, scales = [], [], []
        for j, s in enumerate(meta["sides"]):
            labels.append(decode_labels(s["labels"], s["label_kind"]))
            rowptr, col = read(f"rowptr{j}"), read(f"col{j}")
            n, n_src, nnz = int(s["n"]), int(s["n_src"]), int(s["nnz"])
            if rowptr[0] != 0 or rowptr[-1] != nnz or (np.diff(rowptr) < 0).any():
                raise ValueError(f"side {j}: the row offsets do not describe {nnz} entries")
            if nnz and (int(col.min()) < 0 or int(col.max()) >= n_src):
                raise ValueError(f"side {j}: a column outside the {n_src} source nodes")
            scales.append(read(f"rowscale{j}"))
            csrs.append(CSR(n, n_src, rowptr, col, scales[j]))
        strict = bool(meta["strict"])
        specs = []
        for j, s in enumerate(meta["sides"]):
            evidence_from = None
            if s["evidence"]:
                evidence_from = csrs[0] if (j == 1 and strict) else csrs[j]
            specs.append(SideSpec(csrs[j], scales[j], float(s["C"]), evidence_from=evidence_from,
                                  apriori=_HAS_PRIOR if s["prior"] else None, lbd=float(s["lbd"]), storage=meta["storage"]))
        tables = None
        if meta.get("form", "dense") == "neighbors":
            tables = [tuple(read(f"{name}{j}").reshape(arrays[f"{name}{j}"]["shape"]) for name in ("nbr_ids", "nbr_vals", "diag"))
                      for j in range(len(specs))]
            for j, (ids, _, _) in enumerate(tables):
                if ids.size and (int(ids.min()) < -1 or int(ids.max()) >= int(meta["sides"][j]["n"])):
                    raise ValueError(f"side {j}: a neighbour id outside the {meta['sides'][j]['n']} nodes")
        # ---- the device from here on ----
        from .estimators import _default_ops_factory
        ops = _default_ops_factory(device)(0)
        if tables is not None:
            from ._neighbors import NeighborSolver, Tables
            made = []
            try:
                for ids, vals, diag in tables:
                    made.append(Tables.from_host(ops, ids, vals, diag))
            except BaseException:
                for t in made:
                    t.free()
                raise
            return meta, NeighborSolver(ops, specs, made, storage=meta["storage"]), labels
        blocks = []
        try:
            stage = np.empty(min(BAND_BYTES, max((arrays[f"iterate{j}"]["nbytes"] for j in range(len(specs))), default=0)),
                             dtype=np.uint8)
            for j, s in enumerate(meta["sides"]):
                b = Block(ops, meta["storage"], int(s["n"]))
                blocks.append(b)
                f.seek(arrays[f"iterate{j}"]["offset"])
                for at in range(0, b.nbytes, BAND_BYTES):
                    m = min(BAND_BYTES, b.nbytes - at)
                    if f.readinto(memoryview(stage[:m])) != m:
                        raise ValueError(f"the file is truncated inside array 'iterate{j}'")
                    ops.h2d(b.ptr + at, stage[:m])
                    ops.synchronize()
        except BaseException:
            for b in blocks:
                b.free()
            raise
    return meta, DetachedSolver(ops, specs, blocks), labels
