"""ctypes binding of libsimrank_operator.so (include/simrank_operator.h): a kept model as a linear operator.  The product
of a side's matrix, or of its transpose, with a dense float64 block of vectors,

    out = alpha * S @ X + beta * out          out = alpha * S.T @ X + beta * out

S read in place on the device, once per band of at most ``MAX_D`` columns.  A companion of libsimrank_hip.so with its own
header, version and binding, as ``_diverse.py`` is.  ``check_operand`` and the ``check_embed_*`` functions check the
arguments of ``matmul`` and ``embed`` on the host (no device); ``Session`` holds the operands of one call on the device:
X and the result cross PCIe once, whatever their width.  ``product_lists`` is the host route of a pruned model.  No CPU
fallback for a model held as a matrix: a missing library or device is an error.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._checks import is_int
from ._companion import Companion
from ._driver import Scratch, stage

VERSION = 1              # SIMRANK_OPERATOR_VERSION of include/simrank_operator.h
MAX_D = 64               # SIMRANK_OPERATOR_MAX_D: columns of X in one call
MAX_POWER_ITERATIONS = 16

_vp, _i64, _i32, _f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_operator_version": [],
    "simrank_operator_last_error": [],
    "simrank_operator_parts": [_i64, _i64, _i32, _i32],
    "simrank_operator_workspace_bytes": [_i64, _i64, _i32, _i32],
    "simrank_operator_apply": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _i32, _vp, _i64, _i32, _f64, _f64, _vp, _i64, _vp,
                               _vp],
}
_RESTYPES = {"simrank_operator_last_error": C.c_char_p, "simrank_operator_parts": C.c_int64,
             "simrank_operator_workspace_bytes": C.c_int64}


class OperatorError(RuntimeError):
    """A call into libsimrank_operator.so failed."""


_c = Companion("operator", VERSION, PROTOTYPES, _RESTYPES, OperatorError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- the host half: arguments ----------------------------------------------------------------------------------------
def check_operand(X, index):
    """``X`` of ``matmul`` checked on the host, before any device work -> (float64 [N, d] C-contiguous in the order of
    ``index``, the columns of the result or None for a Series / 1-D input, "series" | "frame" | "vector" | "array", the name of a
    Series).
    A DataFrame or Series is indexed by the fitted labels, in any order, every node exactly once (KeyError for an unknown
    label, ValueError for a repeated or missing one); anything else is an array of shape [N] or [N, d] in the dense
    frame's order.  Real floating or integer data; bool, object and complex dtypes are a ValueError."""
    import pandas as pd
    n = len(index)
    labelled = isinstance(X, (pd.Series, pd.DataFrame))
    if labelled:
        kind = "series" if isinstance(X, pd.Series) else "frame"
        if not X.index.is_unique:
            raise ValueError("X names a node more than once")
        at = index.get_indexer(X.index)
        if (at < 0).any():
            raise KeyError(X.index[int(np.argmax(at < 0))])
        if len(X.index) != n:
            raise ValueError(f"X must name every node exactly once ({len(X.index)} of {n} are there)")
        if kind == "frame":
            bad = [str(t) for t in X.dtypes if t.kind not in "fiu"]
            if bad:
                raise ValueError(f"X must hold real floating or integer data, not {bad[0]}")
        columns = None if kind == "series" else X.columns
        values, name = X.to_numpy(), getattr(X, "name", None)
    else:
        values = np.asarray(X)
        kind = "vector" if values.ndim == 1 else "array"
        columns, name = None, None
    if values.dtype.kind not in "fiu":
        raise ValueError(f"X must hold real floating or integer data, not {values.dtype}")
    if values.ndim not in (1, 2) or values.shape[0] != n:
        raise ValueError(f"X must have shape [{n}] or [{n}, d], not {list(values.shape)}")
    dense = np.array(values if values.ndim == 2 else values[:, None], dtype=np.float64, order="C")
    if labelled:
        placed = np.empty_like(dense)
        placed[at] = dense
        dense = placed
    if kind == "array":
        columns = pd.RangeIndex(dense.shape[1])
    return dense, columns, kind, name


def check_embed_args(dim, oversample, power_iterations, seed, n):
    """The scalars of ``embed`` checked on the host (ValueError) -> (dim, p = min(dim + oversample, n), iterations, seed)."""
    if not is_int(dim) or not 1 <= int(dim) <= n:
        raise ValueError(f"dim must be an integer in 1 .. {n}, not {dim!r}")
    if not is_int(oversample) or int(oversample) < 0:
        raise ValueError(f"oversample must be an integer >= 0, not {oversample!r}")
    if not is_int(power_iterations) or not 0 <= int(power_iterations) <= MAX_POWER_ITERATIONS:
        raise ValueError(f"power_iterations must be an integer in 0 .. {MAX_POWER_ITERATIONS}, not {power_iterations!r}")
    if not is_int(seed) or int(seed) < 0:
        raise ValueError(f"seed must be a non-negative integer, not {seed!r}")
    return int(dim), min(int(dim) + int(oversample), n), int(power_iterations), int(seed)


def signed(V):
    """The columns of V with their signs fixed: the entry of largest magnitude (the first on a tie) is positive."""
    V = np.array(V, dtype=np.float64)
    if V.size:
        at = np.argmax(np.abs(V), axis=0)
        flip = V[at, np.arange(V.shape[1])] < 0
        V[:, flip] = -V[:, flip]
    return V


def embed_host(product, n, dim, p, power_iterations, seed):
    """The randomized subspace iteration of ``embed`` with ``product(Q) = M @ Q`` passed in -> (V [n, dim], w [dim]):

        Q = qr(default_rng(seed).standard_normal((n, p)))[0]
        repeat power_iterations times:  Q = qr(product(Q))[0]
        Y = product(Q);  B = Q.T @ Y;  B = (B + B.T) / 2;  w, Z = eigh(B)
        order = value descending, first dim;  V = Q @ Z[:, order], signs fixed by ``signed``."""
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, p)))[0]
    for _ in range(power_iterations):
        Q = np.linalg.qr(product(Q))[0]
    Y = product(Q)
    B = Q.T @ Y
    B = (B + B.T) / 2
    w, Z = np.linalg.eigh(B)
    order = np.argsort(-w, kind="stable")[:dim]
    return signed(Q @ Z[:, order]), np.ascontiguousarray(w[order])


# ---- the host route of a pruned model --------------------------------------------------------------------------------
def product_lists(ids, vals, diag, X, transpose=False):
    """``P @ X`` (or ``P.T @ X``) for the matrix P of a pruned model's tables (ids int32 [n, kk], -1 = an empty slot; vals
    float64 [n, kk]; diag float64 [n]): a row's kept entries, its diagonal element, +0.0 everywhere else.  Host float64,
    the diagonal term first, then the slots of the lists in their order."""
    n, kk = ids.shape
    X = np.asarray(X, dtype=np.float64)
    out = np.asarray(diag, dtype=np.float64)[:, None] * X
    for e in range(kk):                                      # one slot of every list at a time: n x d doubles in flight
        rows = np.flatnonzero((ids[:, e] >= 0) & (ids[:, e] < n))
        cols = ids[rows, e]
        if transpose:
            np.add.at(out, cols, vals[rows, e, None] * X[rows])
        else:
            out[rows] += vals[rows, e, None] * X[cols]
    return out


# ---- the device half -------------------------------------------------------------------------------------------------
class Session:
    """The operands of one ``matmul`` or ``embed`` on the device of ``reader`` (a ``_query.Reader`` whose one block holds
    every row and column: a solver's ``one_block`` scope): two float64 [n, width] buffers, the workspace of the widest
    band and the maps, allocated once and freed together at the end of the ``with`` block.  ``timing``: a dict that
    receives ``apply_ms`` (HIP events around every product; serialises them), ``h2d_ms`` and ``d2h_ms``."""

    def __init__(self, reader, width, timing=None):
        self.reader, self.ops, self.n, self.width, self.timing = reader, reader.ops, reader.n, int(width), timing
        self.lib = load()
        (self.block,) = reader.blocks
        assert self.block["cols"] == self.n and self.block.get("col_lo", 0) == 0

    def __enter__(self):
        n, b = self.n, self.block
        self.scratch = Scratch(self.ops).__enter__()
        try:
            identity = np.array_equal(self.reader.inv, np.arange(n, dtype=np.int32))
            self.row_pos = None if identity else self.scratch.put(self.reader.inv)
            self.col_pos = self.reader._col_map(0)[0]
            widths = {min(self.width, MAX_D), self.width % MAX_D or MAX_D}      # (the bands' widths: d decides the parts)
            self.work = self.scratch.malloc(max(self.lib.simrank_operator_workspace_bytes(b["rows"], n, t, d)
                                                for t in (0, 1) for d in widths))
            self.x = self.scratch.malloc(8 * n * self.width)
            self.y = self.scratch.malloc(8 * n * self.width)
        except BaseException as e:
            self.scratch.__exit__(type(e), e, e.__traceback__)
            raise
        return self

    def __exit__(self, *exc):
        return self.scratch.__exit__(*exc)

    def _timed(self, name, run):
        if self.timing is None:
            run()
        else:
            stage(self.ops, self.timing, name, run)

    def put(self, X):
        """The host float64 [n, width] block becomes the right-hand side."""
        assert X.shape == (self.n, self.width) and X.dtype == np.float64 and X.flags.c_contiguous
        self._timed("h2d_ms", lambda: self.ops.h2d(self.x, X))

    def apply(self, transpose, alpha, beta):
        """y = alpha * S @ x + beta * y (``transpose``: S.T), in bands of ``MAX_D`` columns."""
        b, n, w = self.block, self.n, self.width
        for q0 in range(0, w, MAX_D):
            d = min(MAX_D, w - q0)
            self._timed("apply_ms", lambda: check(self.lib.simrank_operator_apply(
                b["ptr"], b["layout"], b["stride"], b["rows"], n, self.row_pos, self.col_pos, int(bool(transpose)),
                self.x + 8 * q0, w, d, float(alpha), float(beta), self.y + 8 * q0, w, self.work, self.ops.stream),
                "simrank_operator_apply"))

    def get(self):
        """The result, float64 [n, width] on the host."""
        out = np.empty((self.n, self.width), dtype=np.float64)
        self._timed("d2h_ms", lambda: self.ops.d2h(out, self.y))
        self.ops.synchronize()
        return out


def product(reader, X, transpose=False, timing=None):
    """``S @ X`` (``transpose``: ``S.T @ X``) for the host float64 [n, d] block ``X`` in the caller's order -> float64 [n, d]."""
    n, d = X.shape
    if n == 0 or d == 0:
        return np.zeros((n, d), dtype=np.float64)
    with Session(reader, d, timing) as s:
        s.put(X)
        s.apply(transpose, 1.0, 0.0)
        return s.get()


def embed(reader, dim, p, power_iterations, seed, timing=None):
    """``embed_host`` with ``M @ Q`` on the device: per product Q goes up, two sweeps of S run on it where it lies
    (0.5 S Q, then + 0.5 S.T Q) and Y comes down for the host's QR."""
    import time
    with Session(reader, p, timing) as s:
        def sym(Q):
            s.put(np.ascontiguousarray(Q, dtype=np.float64))
            s.apply(False, 0.5, 0.0)
            s.apply(True, 0.5, 1.0)
            return s.get()
        t0 = time.perf_counter()
        out = embed_host(sym, reader.n, dim, p, power_iterations, seed)
        if timing is not None:
            timing["total_ms"] = (time.perf_counter() - t0) * 1e3
        return out
