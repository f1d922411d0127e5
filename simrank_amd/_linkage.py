"""ctypes binding of libsimrank_linkage.so (include/simrank_linkage.h): the single-linkage dendrogram of a kept model,
found on the device.

``linkage()`` answers the clustering questions that come without a threshold.  Two different nodes a, b fall together at
the height ``w(a, b) = max(S[a, b], S[b, a])`` (NaN is no entry, -0.0 and +0.0 are one height); the dendrogram is a maximum
spanning forest of that graph and every ``components(t)`` a cut of it.  The device finds A forest in at most ceil(log2 n)
Boruvka rounds, each one sweep of the blocks a solver's ``_query.Reader`` describes, in place; ``canonical`` turns any
valid forest into the one table the matrix defines.  A pruned model (a solver with ``lists``) is answered on the
host from its lists.  No CPU fallback for the matrices: a missing library or device is an error.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._checks import finite, is_int
from ._companion import PANEL_F16, PANEL_F32, ROWMAJOR_F32, ROWMAJOR_F64, Companion  # noqa: F401 (a block's layouts)
from ._driver import Scratch, stage
from ._profile import edges_f32

VERSION = 1              # SIMRANK_LINKAGE_VERSION of include/simrank_linkage.h
BAD_COMPONENT, CAP_REACHED = 1, 2      # bits of the device status word

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32

# name -> argtypes (restype is int unless listed in _RESTYPES)
PROTOTYPES = {
    "simrank_linkage_version": [],
    "simrank_linkage_last_error": [],
    "simrank_linkage_phases": [_i32],
    "simrank_linkage_init": [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "simrank_linkage_pick": [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _vp, _vp],
    "simrank_linkage_hook": [_vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "simrank_linkage_flatten": [_vp, _vp, _i64, _vp, _vp],
}
_RESTYPES = {"simrank_linkage_last_error": C.c_char_p}

COLUMNS = ("left", "right", "similarity", "size")


class LinkageError(RuntimeError):
    """A call into libsimrank_linkage.so failed, its kernels reported components out of order, or the rounds did not end
    within their bound."""


_c = Companion("linkage", VERSION, PROTOTYPES, _RESTYPES, LinkageError)
LIB_PATH, HEADER_PATH, load, check = _c.lib_path, _c.header_path, _c.load, _c.check


# ---- argument checks: nothing touches a device ---------------------------------------------------------------------------
def check_floor(min_similarity):
    """``linkage(min_similarity)``: None, or one finite real number as a float.  ValueError otherwise."""
    return None if min_similarity is None else finite(min_similarity, "min_similarity")


def check_cut(t, n_clusters):
    """``cut(Z, t, n_clusters)``: exactly one of the two -> (float | None, int | None).  ValueError otherwise."""
    if (t is None) == (n_clusters is None):
        raise ValueError("cut takes exactly one of t and n_clusters")
    if t is not None:
        return finite(t, "t"), None
    k = n_clusters
    if not is_int(k) or k < 1:
        raise ValueError(f"n_clusters must be an int >= 1, not {k!r}")
    return None, int(k)


def check_table(Z, n: int):
    """The four columns of a ``linkage`` table of ``n`` leaves as arrays, after checking that it is one: at most n - 1
    rows, row i joining two different clusters that exist before it (ids below n + i), sizes that add up.  ValueError
    otherwise."""
    try:
        left, right = (np.asarray(Z[c]) for c in COLUMNS[:2])
        sim, size = np.asarray(Z[COLUMNS[2]], dtype=np.float64), np.asarray(Z[COLUMNS[3]])
    except (KeyError, TypeError, IndexError, ValueError):
        raise ValueError(f"Z must be a table of linkage(): the columns {', '.join(COLUMNS)}") from None
    m = len(left)
    if not (left.ndim == right.ndim == 1 and left.dtype.kind in "iu" and right.dtype.kind in "iu"):
        raise ValueError("Z: left and right must be integer columns")
    if m > max(0, n - 1):
        raise ValueError(f"Z has {m} rows: a model of {n} nodes has at most {max(0, n - 1)}")
    left, right = left.astype(np.int64), right.astype(np.int64)
    upto = n + np.arange(m, dtype=np.int64)
    if ((left < 0) | (right < 0) | (left >= upto) | (right >= upto) | (left == right)).any():
        raise ValueError(f"Z: row i must join two different clusters with ids below {n} + i: not a table of this model")
    if np.isnan(sim).any() or (np.diff(sim) > 0).any():
        raise ValueError("Z: similarity must fall from row to row")
    sizes = np.concatenate([np.ones(n, dtype=np.int64), np.asarray(size, dtype=np.int64)])
    if (sizes[n:] != sizes[left] + sizes[right]).any():
        raise ValueError(f"Z: a size is not the sum of its two clusters' with {n} leaves: not a table of this model")
    return left, right, sim, size


# ---- the device path -----------------------------------------------------------------------------------------------------
def max_rounds(n: int) -> int:
    """ceil(log2 n) + 1.  Every component that has a candidate goes together with at least one other in a round (its
    partner has the same candidate), and one without a candidate never gets one: the components that can still merge at
    least halve per round, so after ceil(log2 n) rounds none is left and one more round hooks nothing."""
    return (max(1, n) - 1).bit_length() + 1


def _plain_pick(lib):
    """Today's pick: ``simrank_linkage_pick`` on a block dict."""
    def pick(b, floor_ref, phase, comp, best, n, status, stream):
        check(lib.simrank_linkage_pick(b["ptr"], b["layout"], b["stride"], b["rows"], b["cols"], b.get("row_ids"),
                                       b.get("col_ids"), floor_ref, phase, comp, best, n, status, stream), "simrank_linkage_pick")
    return pick


def forest_blocks(ops, blocks, n: int, floor, timing=None, pick=None):
    """(a int64, b int64, value float64, rounds): a maximum spanning forest of w(a, b) = max(S[a, b], S[b, a]) over
    ``blocks`` (dicts with ptr, layout, stride, rows, cols and optional device row_ids / col_ids naming ids 0 .. n - 1),
    as edges between node ids with the value they join at, and the number of rounds run.  ``floor``: None or a float;
    entries below it are not used.  One ``simrank_linkage_pick`` per block and round (two for a float64 iterate), all
    into one array of slots.  ``timing``: a list or dict that receives the milliseconds of each stage (HIP events).
    ``pick``: what queues one pick, ``pick(block, floor_ref, phase, comp, best, n, status, stream)``; None is
    ``simrank_linkage_pick`` (``_hdbscan`` passes the pick that clamps every entry by two core similarities).
    LinkageError when the device status word is not 0 or the rounds pass ``max_rounds(n)``."""
    assert n >= 1 and len(blocks) >= 1
    layouts = {b["layout"] for b in blocks}
    wide = ROWMAJOR_F64 in layouts
    assert len({lay == ROWMAJOR_F64 for lay in layouts}) == 1, "the blocks of one iterate hold one type"
    lib = load()
    pick = pick or _plain_pick(lib)
    phases = 2 if wide else 1                                # (float64: the key, then the root; simrank_linkage_phases)
    if floor is None:
        floor_ref = None
    else:
        floor_ref = C.byref(C.c_double(floor) if wide else C.c_float(float(edges_f32([floor])[0])))
    words = np.zeros(2, dtype=np.int32)                      # hooks since the init, the status word
    other, value = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64)
    rounds = total = 0
    with Scratch(ops) as scratch:
        comp, best = scratch.malloc(4 * n), scratch.malloc(16 * n)
        hook_other, hook_value, state = scratch.malloc(4 * n), scratch.malloc(8 * n), scratch.malloc(8)
        status = state + 4
        check(lib.simrank_linkage_init(comp, best, hook_other, hook_value, n, state, status, ops.stream), "simrank_linkage_init")
        while total < n - 1:
            if rounds == max_rounds(n):
                raise LinkageError(f"{rounds} rounds over {n} nodes and components are still merging: the bound is "
                                   f"ceil(log2 n) + 1 = {max_rounds(n)}")
            rounds += 1
            for phase in range(phases):
                for b in blocks:
                    stage(ops, timing, "pick_ms", lambda: pick(b, floor_ref, phase, comp, best, n, status, ops.stream))
            stage(ops, timing, "hook_ms", lambda: check(lib.simrank_linkage_hook(
                best, 64 if wide else 32, comp, hook_other, hook_value, n, state, status, ops.stream), "simrank_linkage_hook"))
            stage(ops, timing, "flatten_ms", lambda: check(lib.simrank_linkage_flatten(comp, best, n, status, ops.stream),
                                                           "simrank_linkage_flatten"))
            ops.d2h(words, state)
            ops.synchronize()
            if words[1] != 0:
                raise LinkageError(f"the linkage kernels reported status {int(words[1])} (1: a component out of range, 2: an "
                                   "iteration cap reached): the forest is not to be trusted")
            if words[0] == total:
                break                                        # a round that hooked nothing: what is apart stays apart
            total = int(words[0])
        ops.d2h(other, hook_other)
        ops.d2h(value, hook_value)
        ops.synchronize()
    a = np.flatnonzero(other >= 0)
    if a.size != total:
        raise LinkageError(f"{a.size} hook records for {total} hooks: the forest is not to be trusted")
    return a.astype(np.int64), other[a].astype(np.int64), value[a], rounds


# ---- the canonical table ---------------------------------------------------------------------------------------------------
def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:
        parent[x], x = root, parent[x]
    return root


def canonical(n: int, a, b, value):
    """The edges (a[i], b[i]) at ``value[i]`` of ANY forest whose cut at every height h is the partition the matrix has
    there -> (left int64, right int64, similarity float64, size int64), the rows the matrix alone defines.  From the
    largest height down: the edges of one height join the classes that exist above it into new classes; a new class
    of m >= 2 old ones c1 .. cm (in the order of their smallest member) gives the m - 1 rows (c1, c2) -> x1, (x1, c3) ->
    x2, ...; the new classes of one height come in the order of their smallest member.  Leaves are 0 .. n - 1, row i
    forms cluster n + i.  -0.0 is reported as +0.0."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    value = np.asarray(value, dtype=np.float64) + 0.0        # (-0.0 + 0.0 = +0.0)
    assert a.shape == b.shape == value.shape and a.ndim == 1 and not np.isnan(value).any()
    order = np.argsort(-value, kind="stable")
    a, b, value = a[order].tolist(), b[order].tolist(), value[order]
    parent = list(range(n))                                  # a class is named by its smallest member
    cluster, members = list(range(n)), [1] * n               # per class name: its cluster id and its size
    left, right, sim, size = [], [], [], []
    starts = np.flatnonzero(np.r_[True, value[1:] != value[:-1]]).tolist() + [len(a)] if len(a) else [0]
    for lo, hi in zip(starts[:-1], starts[1:]):
        h = float(value[lo])
        old = sorted({_find(parent, x) for x in a[lo:hi]} | {_find(parent, x) for x in b[lo:hi]})
        for x, y in zip(a[lo:hi], b[lo:hi]):
            rx, ry = _find(parent, x), _find(parent, y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
        groups = {}
        for c in old:                                        # ascending: every group's list is in member order
            groups.setdefault(_find(parent, c), []).append(c)
        for new in sorted(groups):
            parts = groups[new]
            acc, total = cluster[parts[0]], members[parts[0]]
            for c in parts[1:]:
                left.append(acc)
                right.append(cluster[c])
                total += members[c]
                sim.append(h)
                size.append(total)
                acc = n + len(left) - 1
            cluster[new], members[new] = acc, total
    return (np.array(left, dtype=np.int64), np.array(right, dtype=np.int64), np.array(sim, dtype=np.float64),
            np.array(size, dtype=np.int64))


# ---- the host path of a pruned model ---------------------------------------------------------------------------------------
def forest_of_lists(ids, vals, floor: float):
    """(a, b, value) of a maximum spanning forest of the matrix P of a pruned model above ``floor`` > 0: ``ids`` int
    [n, k] (-1: an empty slot), ``vals`` float64 [n, k] the kept off-diagonal entries of each row.  Every other entry is
    +0.0, below the floor, so the kept entries >= floor are all the edges there are: Kruskal over them, largest first."""
    assert floor > 0
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64)
    n = ids.shape[0]
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], ids.shape)
    with np.errstate(invalid="ignore"):
        use = (ids >= 0) & (ids != rows) & (vals >= floor)   # (NaN passes nothing)
    a, b, v = rows[use], ids[use].astype(np.int64), vals[use]
    order = np.argsort(-v, kind="stable")
    parent, keep = list(range(n)), []
    for i in order.tolist():
        ra, rb = _find(parent, int(a[i])), _find(parent, int(b[i]))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            keep.append(i)
    keep = np.array(keep, dtype=np.int64)
    return a[keep], b[keep], v[keep]


# ---- a solver's side ---------------------------------------------------------------------------------------------------------
def check_solver(solver, floor):
    """What ``linkage`` refuses of a model before any work: a pruned model without a positive floor."""
    if getattr(solver, "kept_k", None) is not None and not (floor is not None and floor > 0):
        raise ValueError("linkage of a pruned model needs min_similarity > 0: the entries a pruned model does not keep are "
                         "+0.0 and tie everything at 0")


def table(solver, j, floor):
    """(n, left, right, similarity, size) of side j: the canonical rows over the caller's ids."""
    lists = solver.lists(j)
    if lists is not None:
        ids, vals, _ = lists
        return (len(ids),) + canonical(len(ids), *forest_of_lists(ids, vals, floor))
    reader = solver._reader(j)
    if reader.n == 0:
        return (0,) + canonical(0, [], [], [])
    a, b, value, _ = forest_blocks(reader.ops, reader.blocks, reader.n, floor)
    return (reader.n,) + canonical(reader.n, a, b, value)


# ---- cutting a table ---------------------------------------------------------------------------------------------------------
def cut_roots(n: int, left, right, n_rows: int) -> np.ndarray:
    """int64 [n]: the smallest leaf of every leaf's cluster once the first ``n_rows`` rows are applied."""
    parent = list(range(n))
    first = list(range(n)) + [0] * n_rows                    # per cluster id: its smallest leaf
    for i in range(n_rows):
        x, y = first[left[i]], first[right[i]]
        lo, hi = (x, y) if x < y else (y, x)
        parent[_find(parent, hi)] = _find(parent, lo)
        first[n + i] = lo
    return np.array([_find(parent, x) for x in range(n)], dtype=np.int64)


def cut_labels(n: int, Z, t, n_clusters) -> np.ndarray:
    """int64 [n]: the components of ``cut``, numbered 0, 1, 2, ... in the order of their first member."""
    left, right, sim, _ = check_table(Z, n)
    if t is not None:
        m = int((sim >= t).sum())                            # (the rows fall in similarity: a prefix)
    else:
        m = n - n_clusters
        if m < 0:
            raise ValueError(f"n_clusters = {n_clusters} is more than the {n} nodes")
        if m > len(left):
            raise ValueError(f"n_clusters = {n_clusters} needs {m} merges and Z has {len(left)} rows: the fewest clusters "
                             f"this table reaches is {n - len(left)}")
    roots = cut_roots(n, left.tolist(), right.tolist(), m)
    return np.unique(roots, return_inverse=True)[1].reshape(-1).astype(np.int64)
