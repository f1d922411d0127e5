"""Exactly summable operands for the two legs, and their references (no GPU).

Let K be an integer matrix, e_c one exponent per operand column and X[j, c] = K[j, c] * 2^e_c; let the pattern's row scales
be powers of two (or 0).  If for every pattern row a and column c

    sum_{j in row a} |K[j, c]|  <  2^(m - h)          (m: mantissa width of the format, h: headroom for the epilogue)

then every partial sum of row a's products — any order, any association, in registers, LDS slabs or MFMA accumulators — is
an integer below 2^m times 2^e_c and therefore representable: a float32 kernel that returns anything but
rowscale[a] * sum has dropped, duplicated, misplaced or mis-split a term.  Signs may be mixed (the bound is on magnitudes).
No tolerance is involved anywhere: the float64 NumPy result cast to float32 is THE result, bit for bit.

`summable_operand` builds such an X for any pattern (and refuses to return one that violates the condition),
`summable_symmetric` builds a symmetric S whose leg-1 AND leg-2 operands satisfy it (so W.(W.S)^T is exactly symmetric and
exactly summable: what the upper-triangle forms need), `exact_epilogue` is the oracle's epilogue expression with a check
that no intermediate of any association rounds in float32, `plant_previous` puts differences of exactly eps, eps + one step
and eps - one step at chosen places, `regular_graph` / `exact_updates` give whole fits whose iterates stay exact;
`short_lengths` / `short_case` / `tie_places_every_row` are the graphs, operands and tie places built for leg 2's short path;
`loop_prior`, `pow2_degree_graph`, `matched_biregular_graph`, `prior_case` / `bi_prior_case` and `count_eps` are the priors,
graphs, cached oracle iterates and counting eps of the whole loops with a prior (tests/test_gpu_exact_priors.py).
"""
from collections import namedtuple

import numpy as np
import pandas as pd
import scipy.sparse as sp

from simrank_amd.ingest import CSR

SENTINEL = np.float32(-7.0e33)          # what padding holds before a launch (no result of these tests is near it)
SENTINEL_U8 = 0xA5


# ---- patterns -------------------------------------------------------------------------------------------------------
def pow2_rowscale(csr, seed):
    """The pattern with row scales 2^-k, k in 0..6, about 5 % of them zero (as tests' random_csr has them)."""
    rng = np.random.default_rng(seed)
    rs = 2.0 ** -rng.integers(0, 7, size=csr.n_rows).astype(np.float64)
    rs[rng.random(csr.n_rows) < 0.05] = 0.0
    return CSR(csr.n_rows, csr.n_cols, csr.rowptr, csr.col, rs)


def pattern(csr):
    """The 0/1 pattern as a scipy int64 CSR matrix."""
    return sp.csr_matrix((np.ones(csr.col.size, dtype=np.int64), csr.col, csr.rowptr), shape=(csr.n_rows, csr.n_cols))


def longest_row(csr):
    return int(np.diff(csr.rowptr).max()) if csr.n_rows else 0


def is_pow2_or_zero(x):
    m, _ = np.frexp(np.asarray(x, dtype=np.float64))
    return bool(np.all((m == 0.5) | (m == 0.0)))


# ---- the operand ----------------------------------------------------------------------------------------------------
Operand = namedtuple("Operand", "X K exp used")        # X float64 (exact in the format), K int64, exp int64 [L], budget share


def _entry_bits(budget_bits, longest):
    """Width w of the ordinary entries: longest * 2^w <= half the budget (the other half is for the wide entry and slack)."""
    w = budget_bits - 1 - int(np.ceil(np.log2(max(1, longest))))
    assert w >= 1, f"a row of {longest} entries leaves no room in 2^{budget_bits}"
    return w


def summable_operand(csr, L, mantissa=24, headroom=0, seed=0, exponents=(-20, 20)):
    """-> Operand for `csr` (K rows = csr.n_cols, L columns).  Both signs; one WIDE entry per column, magnitude in
    [2^(m-h-3), 2^(m-h-2)) with the lowest bit set (so the bf16 hi, mid and lo terms of its split are all non-zero), its row
    rotating with the column so that every 16-row step and every fragment slot carries some; all other entries as wide as the
    longest pattern row allows; e_c drawn from `exponents` (inclusive).  The condition of this module's header is asserted
    in integer arithmetic before anything is returned."""
    assert is_pow2_or_zero(csr.rowscale), "row scales must be powers of two (pow2_rowscale)"
    rng = np.random.default_rng(seed)
    Kr, bits = csr.n_cols, mantissa - headroom
    assert bits >= 5
    w = _entry_bits(bits, longest_row(csr))
    K = rng.integers(1, 2 ** w, size=(Kr, L), dtype=np.int64, endpoint=False)
    K *= rng.choice(np.array([-1, 1], dtype=np.int64), size=(Kr, L))
    wide = rng.integers(2 ** (bits - 3), 2 ** (bits - 2), size=L, dtype=np.int64) | 1
    if bits >= 19:                                       # the bit right below the 8 of hi: mid starts there, lo keeps bit 0
        wide |= 1 << (bits - 3 - 8)
    wide *= rng.choice(np.array([-1, 1], dtype=np.int64), size=L)
    # column c: row c mod 16 of a 16-row step that changes with c, so 16 consecutive columns reach every residue
    c = np.arange(L)
    wide_row = (c % 16 + 16 * ((c // 16 * 5 + c) % max(1, Kr // 16))) % Kr if Kr >= 16 else c % Kr
    K[wide_row, np.arange(L)] = wide
    exp = rng.integers(exponents[0], exponents[1], size=L, endpoint=True).astype(np.int64)
    used = check_summable(csr, K, bits)
    X = np.ldexp(K.astype(np.float64), exp[None, :])
    return Operand(X, K, exp, used)


def check_summable(csr, K, bits):
    """Asserts sum_{j in row a} |K[j, c]| < 2^bits for every row a and column c (int64: no rounding); -> largest share used."""
    tot = pattern(csr) @ np.abs(K)                      # int64
    worst = int(tot.max()) if tot.size else 0
    assert worst < 2 ** bits, f"operand is not exactly summable: a row sums to {worst} >= 2^{bits}"
    return worst / 2.0 ** bits


def product64(csr, X):
    """diag(rowscale) . pattern . X in float64 — exact for a summable X (every partial sum is representable in 53 bits)."""
    rs = np.asarray(csr.rowscale, dtype=np.float64)
    return rs[:, None] * (pattern(csr).astype(np.float64) @ X)


Symmetric = namedtuple("Symmetric", "S Tt KS KT used1 used2")


def summable_symmetric(csr, mantissa=24, headroom=0, seed=0, exponent=0):
    """A symmetric integer S = diag(d) + N (x 2^exponent), K x K for an n x K pattern (K = n: a square one), such that both
    legs of W . S . W^T are exactly summable: leg 1's operand is S, leg 2's is Tt = (W . S)^T — K x n — and the product (n x n)
    is exactly symmetric — what the upper-triangle forms mirror.  d is wide (one odd value of m-h-3 .. m-h-2 bits per column
    after leg 1, as summable_operand has them), N is a symmetric matrix of small integers of both signs, so no element of Tt
    is zero for lack of a term.
    -> (S, Tt, integer S, integer (pattern . S), budget share of leg 1, of leg 2)."""
    assert is_pow2_or_zero(csr.rowscale)
    K, bits = csr.n_cols, mantissa - headroom
    rng = np.random.default_rng(seed)
    longest = longest_row(csr)
    # leg 2 sums |(P S)[a, j]| over j in row b: <= longest * (|d| + longest * nmax)  -> d gets what a row allows, N the rest
    wd = _entry_bits(bits, longest) - 1
    nbits = max(1, min(4, bits - 2 - 2 * int(np.ceil(np.log2(max(1, longest))))))
    d = rng.integers(2 ** (wd - 1), 2 ** wd, size=K, dtype=np.int64) | 1
    d *= rng.choice(np.array([-1, 1], dtype=np.int64), size=K)
    N = rng.integers(-(2 ** nbits) + 1, 2 ** nbits, size=(K, K), dtype=np.int64)
    N = np.triu(N, 1)
    N = N + N.T
    P = pattern(csr)
    # one diagonal entry in 16 as wide as the budget takes (where it reaches 17 bits, the hi, mid and lo terms of its split
    # are all non-zero); rows that hold several of them decide how wide that is
    big = np.arange(K) % 16 == 5
    mag = rng.random(int(big.sum()))
    for wb in range(bits - 2, wd, -1):
        dd = d.copy()
        dd[big] = ((2 ** (wb - 1) * (1 + mag)).astype(np.int64) | 1 | (1 << max(0, wb - 9))) * np.sign(d[big])
        KS = N + np.diag(dd)
        KT = P @ KS                                      # int64 [a, j] = sum_{i in row a} S[i, j]; Tt[j, a] = rs_a * KT[a, j]
        worst2 = int(np.asarray(np.abs(KT) @ P.T).max())  # [a, b] = sum_{j in row b} |KT[a, j]|
        if worst2 < 2 ** bits:
            break
    else:
        KS = N + np.diag(d)
        KT = P @ KS
        worst2 = int(np.asarray(np.abs(KT) @ P.T).max())
    assert worst2 < 2 ** bits, f"leg 2 is not exactly summable: {worst2} >= 2^{bits}"
    used1 = check_summable(csr, KS, bits)
    S = np.ldexp(KS.astype(np.float64), exponent)
    rs = np.asarray(csr.rowscale, dtype=np.float64)
    Tt = (rs[:, None] * np.ldexp(KT.astype(np.float64), exponent)).T.copy()
    assert S.shape == (K, K) and Tt.shape == (K, csr.n_rows)
    return Symmetric(S, Tt, KS, KT, used1, worst2 / 2.0 ** bits)


# ---- the split of fused_dev.h / blockdense.hip, emulated ----------------------------------------------------------
def split3f(x):
    """float32 array -> (hi, mid, lo) float32 arrays as the device's split3f makes them: hi = x truncated to its upper 16
    bits (a bf16), mid = (x - hi) truncated, lo = (x - hi - mid) truncated; hi + mid + lo == x for 24-bit mantissas."""
    x = np.asarray(x, dtype=np.float32)
    trunc = lambda v: (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    hi = trunc(x)
    r = (x - hi).astype(np.float32)
    mid = trunc(r)
    q = (r - mid).astype(np.float32)
    lo = trunc(q)
    return hi, mid, lo


# ---- the epilogue ---------------------------------------------------------------------------------------------------
def _exact32(name, v):
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v), f"{name} rounds in float32"
    return v


def exact_epilogue(prod, coef=0.5, counts=None, prior=None, lbd=None, diag_col0=0, set_diag=True):
    """float64 reference of the fused epilogue in the oracle's expression (oracle.update: (1 - lbd) * E * coef * prod +
    lbd * prior; E * coef * prod; coef * prod), for prod = W . X.  Asserts that every intermediate of every association is
    unchanged by .astype(float32) — coef * s, coef * s * E, s * E, (1 - lbd) * ..., lbd * prior, the result — so neither
    a contraction to FMA nor the order of the factors can matter on the device.  The diagonal (row == diag_col0 + column)
    is 1."""
    prod = _exact32("the product", np.asarray(prod, dtype=np.float64))
    new = _exact32("coef * s", coef * prod)
    if counts is not None:
        E = 1 - 0.5 ** counts.astype(np.float64)
        _exact32("E", E)
        _exact32("s * E", prod * E)
        new = _exact32("coef * s * E", E * coef * prod)
    if prior is not None:
        keep = _exact32("1 - lbd", np.float64(1 - lbd))
        assert float(np.float32(1.0) - np.float32(lbd)) == float(keep)
        a = _exact32("(1 - lbd) * coef * s * E", keep * new)
        if counts is not None:
            _exact32("(1 - lbd) * E", keep * E)
            _exact32("(1 - lbd) * E * coef", keep * E * coef)
            assert np.array_equal((1 - lbd) * E * coef * prod, a)
        b = _exact32("lbd * prior", lbd * np.asarray(prior, dtype=np.float64))
        new = _exact32("the blend", a + b)
    new = new.copy()
    if set_diag:
        c = np.arange(new.shape[1])
        r = diag_col0 + c
        ok = r < new.shape[0]
        new[r[ok], c[ok]] = 1.0
    return new


def epilogue_counts(shape, seed, symmetric=False):
    """Evidence counts from {0, 1, 2, 3, 255} (E = 0, 1/2, 3/4, 7/8 and — 2^-255 is below float32 and float64 alike — 1)."""
    rng = np.random.default_rng(seed)
    c = rng.choice(np.array([0, 1, 2, 3, 255], dtype=np.uint8), size=shape)
    if symmetric:
        c = np.triu(c) + np.triu(c, 1).T
    return c.astype(np.uint8)


def grid_prior(unit, bits, seed, symmetric=False):
    """A prior on the operand's grid: integers of both signs below 2^bits times `unit` (the result grid rowscale_a * 2^e_c)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-(2 ** bits) + 1, 2 ** bits, size=unit.shape, dtype=np.int64)
    if symmetric:
        k = np.triu(k) + np.triu(k, 1).T
    return k.astype(np.float64) * unit


# ---- ties for the convergence count -------------------------------------------------------------------------------
Planted = namedtuple("Planted", "previous count kinds")


def _is32(v):
    return float(np.float32(v)) == float(v) and np.isfinite(np.float32(v))


def plant_previous(want, eps, places, symmetric=False, fmt=np.float32, only=("on", "above", "below")):
    """`previous` = want (float32, from the reference) except at `places` [(r, c), ...], where it differs from want by
    exactly eps ("on"), by eps + one step ("above") or by eps - one step ("below"), the three kinds in turn; a step is the
    smallest power of two at which all three candidates are representable.  -> (previous, the strict-> count over the whole
    matrix, the kinds planted).  `symmetric`: (c, r) gets what (r, c) got.  `only`: the kinds to plant (("on", "below"): nothing
    moved by more than eps, the count is zero)."""
    want = np.asarray(want, dtype=np.float64)
    prev = want.copy()
    m, e = np.frexp(eps)
    assert m == 0.5, "eps must be a power of two"
    kinds = []
    done = set()
    for i, (r, c) in enumerate(places):
        if (r, c) in done:
            continue
        v = want[r, c]
        if symmetric:
            assert want[c, r] == v
        placed = False
        for sign in ((1, -1) if i % 2 == 0 else (-1, 1)):
            step = eps
            best = None
            while step > eps * 2.0 ** -30:
                step /= 2
                cand = [v + sign * eps, v + sign * (eps + step), v + sign * (eps - step)]
                if all(float(fmt(x)) == x for x in cand):
                    best = (step, cand)
                elif best is not None:
                    break
            if best is not None:
                kind = only[len(kinds) % len(only)]
                prev[r, c] = best[1][("on", "above", "below").index(kind)]
                if symmetric:
                    prev[c, r] = prev[r, c]
                    done.add((c, r))
                done.add((r, c))
                kinds.append(kind)
                placed = True
                break
        assert placed, f"no representable tie at {(r, c)}: value {v!r}, eps {eps!r}"
    assert set(only) <= set(kinds)
    count = int((np.abs(want - prev) > eps).sum())
    return Planted(prev.astype(fmt), count, kinds)


def tie_places(rows, cols, panel=32):
    """Places a count can go wrong at: the diagonal, both triangles, the last row and column, the tail behind the last full
    panel, a pair of mirrored tiles, the first and last element of a panel."""
    r_last, c_last = rows - 1, cols - 1
    sq = min(rows, cols)
    p = [(0, 0), (sq // 2, sq // 2), (sq - 1, sq - 1),                    # diagonal
         (1, min(c_last, 5)), (min(r_last, 5), 1),                        # both triangles
         (r_last, 0), (r_last, c_last // 2), (0, c_last), (r_last // 2, c_last), (r_last, c_last),
         (2, (c_last // panel) * panel), (3, c_last - (1 if c_last else 0)),   # the tail panel
         (min(r_last, 3), min(c_last, panel + 2)), (min(r_last, panel + 2), min(c_last, 3)),   # mirrored tiles
         (min(r_last, 7), 0), (min(r_last, 7), min(c_last, panel - 1)),   # first / last element of a panel
         (min(r_last, 9), min(c_last, panel)), (min(r_last, 9), min(c_last, 2 * panel - 1))]
    out = []
    for rc in p:
        if rc not in out and 0 <= rc[0] < rows and 0 <= rc[1] < cols:
            out.append(rc)
    return out


# ---- whole fits -----------------------------------------------------------------------------------------------------
def regular_graph(n, d, seed):
    """Edge list (from, to, weight) in which every node has exactly d in-neighbours (d a power of two, none of them
    itself): every row scale is 1/d, the spread of SimRank++ is exactly 1, and with C = 0.5 the float64 oracle's iterates
    live on a dyadic grid."""
    assert d & (d - 1) == 0 and 0 < d < n
    rng = np.random.default_rng(seed)
    src = np.empty((n, d), dtype=np.int64)
    for v in range(n):
        s = rng.choice(n - 1, size=d, replace=False)
        src[v] = s + (s >= v)
    return pd.DataFrame({"from": src.ravel(), "to": np.repeat(np.arange(n, dtype=np.int64), d), "weight": 1.0})


def biregular_graph(n1, n2, d1, seed):
    """Bipartite edge list (user, item, weight): every user has d1 items and every item d2 = n1 * d1 / n2 users, both
    powers of two (a union of d1 shifted permutations without a repeated pair)."""
    d2 = n1 * d1 // n2
    assert n1 * d1 == n2 * d2 and d1 & (d1 - 1) == 0 and d2 & (d2 - 1) == 0
    rng = np.random.default_rng(seed)
    pu, pi = rng.permutation(n1), rng.permutation(n2)
    # user u's k-th item: slot (u * d1 + k) of n1 * d1 slots dealt to the items in turn
    slots = np.arange(n1 * d1)
    users, items = pu[slots // d1], pi[slots % n2]
    df = pd.DataFrame({"user": users, "item": items, "weight": 1.0})
    assert not df.duplicated(["user", "item"]).any()
    return df


def matched_biregular_graph(n1, n2, d1, seed):
    """Bipartite edge list with the degrees of biregular_graph (every user d1 items, every item d2 = n1 * d1 / n2 users) as a
    union of d1 RANDOM matchings (user u's k-th item: perm_k[u] mod n2): no two nodes need share their whole neighbour list,
    as the nodes of biregular_graph do in pairs — there W S W^T of an asymmetric S is symmetric wherever the evidence is
    not zero, and an asymmetric prior on one side never reaches the other."""
    d2 = n1 * d1 // n2
    assert n1 % n2 == 0 and d1 & (d1 - 1) == 0 and d2 & (d2 - 1) == 0
    rng = np.random.default_rng(seed)
    for _ in range(100):
        items = np.stack([rng.permutation(n1) % n2 for _ in range(d1)], axis=1)
        if all(len(set(row)) == d1 for row in items.tolist()):
            break
    else:
        raise AssertionError("no union of matchings without a repeated pair")
    df = pd.DataFrame({"user": np.repeat(np.arange(n1, dtype=np.int64), d1), "item": items.ravel().astype(np.int64), "weight": 1.0})
    assert set(df.groupby("user").size()) == {d1} and set(df.groupby("item").size()) == {d2}
    return df


def pow2_degree_graph(n, degrees, hubs, share, seed):
    """Edge list (from, to, weight) without self loops or repeated edges in which every node's in-degree is a member of
    `degrees` (powers of two, dealt evenly) and a fraction `share` of all references goes to the first `hubs` nodes, dealt
    to them in turn: hub columns that many rows reference (dense sets for the matrix cores) beside rows of a few entries,
    with row scales that are powers of two."""
    assert all(d & (d - 1) == 0 and 0 < d < hubs for d in degrees) and 0 < hubs < n - max(degrees) and 0 <= share <= 1
    rng = np.random.default_rng(seed)
    deg = np.array([degrees[i % len(degrees)] for i in range(n)], dtype=np.int64)
    rng.shuffle(deg)
    src, dst, acc, taken, turn, waiting = [], [], 0.0, 0, 0, []
    for v in range(n):
        acc += share * deg[v]
        h = int(np.floor(acc + 1e-9)) - taken            # (error diffusion: floor(share * references) go to hubs in all)
        h = min(h, int(deg[v]))
        taken += h
        mine = []
        while len(mine) < h:
            if waiting and waiting[0] != v:
                mine.append(waiting.pop(0))              # (a hub that was passed over as its own row: the next row takes it)
                continue
            u = turn % hubs
            turn += 1
            if u == v:
                waiting.append(u)
            else:
                mine.append(u)
        rest = rng.choice(n - hubs - (1 if v >= hubs else 0), size=int(deg[v]) - h, replace=False) + hubs
        rest = rest + ((rest >= v) if v >= hubs else 0)
        src += mine + rest.tolist()
        dst += [v] * int(deg[v])
    df = pd.DataFrame({"from": np.array(src, dtype=np.int64), "to": np.array(dst, dtype=np.int64), "weight": 1.0})
    assert not df.duplicated(["from", "to"]).any() and not (df["from"] == df["to"]).any()
    assert set(df.groupby("to").size()) <= set(degrees) and df["to"].nunique() == n
    return df


def stable_length_order(lengths):
    """planprep.hip length_order restated: the nodes in ascending row length, equal lengths in the caller's order."""
    return np.argsort(np.asarray(lengths), kind="stable").astype(np.int32)


def pow2_bidegree_graph(deg1, deg2, seed):
    """Bipartite edge list (user, item, weight = 1) with PRESCRIBED degree sequences on both sides (powers of two, equal
    totals; both are shuffled here): a random matching of the stubs, repeated pairs repaired by swapping items between two
    edges.  Every node is present, users are 0 .. n1 - 1 and items 0 .. n2 - 1 (so the sorted label order is the index).
    Asserted: the degree sets, no repeated pair, that the stable length order of EACH side is a real permutation, and — for
    n1 = n2 — that the two orders differ."""
    rng = np.random.default_rng(seed)
    deg1, deg2 = np.array(deg1, dtype=np.int64), np.array(deg2, dtype=np.int64)
    assert deg1.sum() == deg2.sum() and all(d > 0 and d & (d - 1) == 0 for d in set(deg1.tolist()) | set(deg2.tolist()))
    rng.shuffle(deg1)
    rng.shuffle(deg2)
    users = np.repeat(np.arange(deg1.size, dtype=np.int64), deg1)
    items = rng.permutation(np.repeat(np.arange(deg2.size, dtype=np.int64), deg2))
    E = users.size
    for _ in range(200):
        key = users * deg2.size + items
        order = np.argsort(key, kind="stable")
        dup = order[1:][key[order][1:] == key[order][:-1]]
        if dup.size == 0:
            break
        have = set(key.tolist())
        for i in dup.tolist():
            for j in rng.integers(0, E, size=64).tolist():
                a, b = users[i] * deg2.size + items[j], users[j] * deg2.size + items[i]
                if a not in have and b not in have and users[i] != users[j]:
                    items[i], items[j] = items[j], items[i]
                    have.update((int(a), int(b)))
                    break
    else:
        raise AssertionError("repeated pairs could not be repaired")
    df = pd.DataFrame({"user": users, "item": items, "weight": 1.0})
    assert not df.duplicated(["user", "item"]).any()
    got1, got2 = np.bincount(users, minlength=deg1.size), np.bincount(items, minlength=deg2.size)
    assert np.array_equal(got1, deg1) and np.array_equal(got2, deg2)
    o1, o2 = stable_length_order(deg1), stable_length_order(deg2)
    for o in (o1, o2):
        assert not np.array_equal(o, np.arange(o.size)), "the length order is the identity"
    assert deg1.size != deg2.size or not np.array_equal(o1, o2)
    return df


# the graphs of tests/test_gpu_exact_bipartite.py: name -> (degrees of the users, of the items, seed).  Both sides hold
# mixed power-of-two degrees, so both length orders are real permutations; node counts are multiples of 128, so that a
# sharded plan deals its order on 2 and 4 ranks.  "hub": 48 items that 8 users each reference — dense sets for the matrix
# cores in the USERS' pattern (the hub COLUMNS are group 1's).
BI_MIXED = {"mixed384": ([1] * 256 + [2] * 128, [1] * 256 + [2] * 128, 384),
            "mixed512": ([1] * 256 + [2] * 256, [2] * 128 + [4] * 128, 512),
            "hub512": ([1] * 256 + [2] * 256, [8] * 48 + [1] * 128 + [2] * 128, 560)}
_bi_graphs = {}


def bi_graph(name):
    """pow2_bidegree_graph of BI_MIXED[name], once."""
    if name not in _bi_graphs:
        _bi_graphs[name] = pow2_bidegree_graph(*BI_MIXED[name])
    return _bi_graphs[name]


def loop_prior(n, bits, seed, symmetric, density=1.0, half=False):
    """A prior for whole loops: float64 integers in [0, 2^bits) times 2^-bits, dense (`density` < 1: that share non-zero),
    symmetric or — A[r, c] != A[c, r] for more than a quarter of the pairs — not.  The update overwrites the diagonal, so
    it holds values that differ from 1 and from each other (2 + i: a kernel that lets one through shows it; `half`, for
    fp16-held matrices, which take prior values below 4 only: 2 + i / 512, fp16 numbers also when held x 2^14)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 2 ** bits, size=(n, n), dtype=np.int64)
    if density < 1.0:
        k *= rng.random((n, n)) < density
    if symmetric:
        k = np.triu(k) + np.triu(k, 1).T
    A = k.astype(np.float64) * 2.0 ** -bits
    assert not half or n <= 1024
    A[np.arange(n), np.arange(n)] = 2.0 + np.arange(n) * (2.0 ** -9 if half else 1.0)
    assert np.array_equal(A.astype(np.float32).astype(np.float64), A)
    differ = int((np.triu(A != A.T, 1)).sum())
    if symmetric:
        assert differ == 0
    elif density == 1.0:
        assert differ > n * (n - 1) // 2 // 4
    else:
        assert differ > 0
    return A


def lowbit_exp(a):
    """Exponent of the lowest set bit over all non-zero elements (float64 array); None when all are zero."""
    a = np.asarray(a, dtype=np.float64)
    a = np.abs(a[a != 0])
    if a.size == 0:
        return None
    word = np.ascontiguousarray(a).view(np.int64)        # (read off the bits: 53-bit integer mant x 2^(field - 1075))
    field = word >> 52
    assert field.min() > 0 and field.max() < 2047, "subnormal or non-finite"
    mant = (word & ((1 << 52) - 1)) | (1 << 52)
    low = mant & -mant
    tz = (low.astype(np.float64).view(np.int64) >> 52) - 1023          # log2 of a power of two, from its exponent field
    return int((field - 1075 + tz).min())


Exact = namedtuple("Exact", "updates grid_bits bits")


def _one_update(W, S, C, E, mantissa, prior=None, lbd=None):
    """One update new = E * C * W S W^T (diag <- 1) — with a prior (1 - lbd) * E * C * W S W^T + lbd * prior — with the
    bookkeeping of exact_updates: -> (new, -log2 grid, quotient) or None when exactness in float64 itself cannot be vouched
    for.  An iterate that is not symmetric (a prior that is not) is booked on S AND on S^T: the device gathers rows of
    Tt = (W S)^T and then rows of its own product W . Tt, which is the TRANSPOSE of W S W^T (stored transposed); the oracle
    sums W S first and (W S) W^T second.  The update itself is taken as (W (W S)^T)^T."""
    rs = W.max(axis=1)
    assert is_pow2_or_zero(rs) and np.array_equal(W, rs[:, None] * (W != 0))
    P = sp.csr_matrix((W != 0).astype(np.float64))       # (a few entries per row: the products below cost nothing)
    c_exp = lowbit_exp(np.float64(C))
    assert 2.0 ** c_exp == C, "C must be a power of two"
    terms, totals, prod = [], [], None
    for X in ((S,) if np.array_equal(S, S.T) else (S, S.T)):
        sums1 = P @ X                                    # leg 1, unscaled (exact in float64 while the quotient is below 2^53)
        T = rs[:, None] * sums1
        sums2 = P @ T.T
        p = rs[:, None] * sums2                          # W . (W X)^T = (W X W^T)^T
        terms += [X, sums1, T, sums2, p]
        totals += [(P @ np.abs(X)).max(), (P @ np.abs(T.T)).max()]
        if prod is None:
            prod = p.T                                   # from X = S: W S W^T, the transpose of what the device's leg 2 sums
    new = C * prod
    terms.append(new)
    if E is not None:
        terms.append(prod * E)                           # (s * E: the other association of E * C * s)
        new = E * new
        terms.append(new)
    floor = lowbit_exp(S) + 2 * lowbit_exp(rs) + c_exp + (lowbit_exp(E) if E is not None and E.any() else 0)
    if prior is not None:
        keep = np.float64(1 - lbd)
        assert float(np.float32(keep)) == float(keep) and float(np.float32(1.0) - np.float32(lbd)) == float(keep)
        assert float(np.float32(lbd)) == float(lbd)
        # (the diagonal of the update is overwritten with 1: what the blend gives there is read by nobody and is not booked)
        A = np.asarray(prior, dtype=np.float64).copy()
        np.fill_diagonal(A, 0.0)
        off = 1.0 - np.eye(A.shape[0])
        a, b = keep * new, lbd * A
        if E is not None:
            terms += [keep * E, keep * E * C]
            assert np.array_equal((1 - lbd) * E * C * prod, a)
        terms += [keep * C * prod, a * off, b, (a + b) * off]
        new = a + lbd * np.asarray(prior, dtype=np.float64)
        floor += lowbit_exp(keep)
        if b.any():
            floor = min(floor, lowbit_exp(np.float64(lbd)) + lowbit_exp(A))
    np.fill_diagonal(new, 1.0)
    totals += [np.abs(C * prod).max(), np.abs(new).max(), 1.0]
    # (a bound that does not rest on the float64 results themselves: sums stay on their operands' grid, every scale moves it
    # by its own exponent — below 2^53 the numbers above are exact, and the measured grid can be trusted)
    if max(totals) / 2.0 ** floor >= 2.0 ** 53:
        return None
    grid = floor if mantissa >= 53 else min(x for x in (lowbit_exp(t) for t in terms) if x is not None)
    return new, -grid, max(totals) / 2.0 ** grid


def _is_oracle_update(W, S, C, E, prior, lbd, new):
    from oracle import simrank_oracle as O
    want = O.update(W, S, C, E, prior, lbd) if prior is not None else O.update(W, S, C, E)
    assert np.array_equal(new, want), "the booked update is not the oracle's, bit for bit"


def exact_updates(W, C=0.5, E=None, mantissa=24, limit=24, prior=None, lbd=None):
    """How many updates of S' = E * C * W S W^T (diag <- 1) from S = I stay exact in a format of `mantissa` bits: after each
    update the coarsest common grid of the terms of both legs and of the epilogue (the lowest set bit over all non-zero
    terms: the elements of S, of W S unscaled and scaled, of C * prod, E * C * prod) divides the largest total (the largest
    sum of magnitudes a row of either leg can reach, the largest element); the count stops before that quotient reaches
    2^mantissa.  -> (updates, -log2 of the grid at the last exact update, bits of the quotient there).
    `prior`, `lbd`: the update is (1 - lbd) * E * C * W S W^T + lbd * prior (oracle.update; E may be None: a plan without
    evidence); the terms gain (1 - lbd) * E, (1 - lbd) * E * C, (1 - lbd) * x, lbd * prior and the blend, an iterate that is
    not symmetric is booked on itself and on its transpose (_one_update), and every counted update is asserted to be
    oracle.update's result bit for bit."""
    W = np.asarray(W, dtype=np.float64)
    S = np.eye(W.shape[0])
    last = Exact(0, 0, 0)
    for u in range(1, limit + 1):
        r = _one_update(W, S, C, E, mantissa, prior, lbd)
        if r is None or r[2] >= 2.0 ** mantissa:
            break
        if prior is not None:
            _is_oracle_update(W, S, C, E if E is not None else 1.0, prior, lbd, r[0])
        S = r[0]
        last = Exact(u, r[1], int(np.ceil(np.log2(r[2]))))
    return last


def exact_updates_bipartite(W12, W21, C=0.5, E1=None, E2=None, mantissa=24, limit=24, prior1=None, prior2=None,
                            lbd1=None, lbd2=None):
    """The same count for the two-matrix loop (S1 from S2, then S2 from the new S1): both half-updates must stay exact.
    `prior1`, `prior2` (both or neither) with `lbd1`, `lbd2`: the priors of the two groups, as in exact_updates."""
    W12, W21 = np.asarray(W12, dtype=np.float64), np.asarray(W21, dtype=np.float64)
    assert (prior1 is None) == (prior2 is None)
    S2 = np.eye(W21.shape[0])
    last = Exact(0, 0, 0)
    for u in range(1, limit + 1):
        r1 = _one_update(W12, S2, C, E1, mantissa, prior1, lbd1)
        if r1 is None or r1[2] >= 2.0 ** mantissa:
            break
        r2 = _one_update(W21, r1[0], C, E2, mantissa, prior2, lbd2)
        if r2 is None or r2[2] >= 2.0 ** mantissa:
            break
        if prior1 is not None:
            _is_oracle_update(W12, S2, C, E1 if E1 is not None else 1.0, prior1, lbd1, r1[0])
            _is_oracle_update(W21, r1[0], C, E2 if E2 is not None else 1.0, prior2, lbd2, r2[0])
        S2 = r2[0]
        last = Exact(u, max(r1[1], r2[1]), int(np.ceil(np.log2(max(r1[2], r2[2])))))
    return last


def oracle_iterates(W, C, E, updates):
    """[S_0 = I, S_1, ..., S_updates] by the oracle's update."""
    from oracle import simrank_oracle as O
    out = [np.eye(W.shape[0])]
    for _ in range(updates):
        out.append(O.update(W, out[-1], C, E))
    return out


class PriorCase:
    """A directed graph with a prior: the oracle's matrices and (lazily, once) the exact update count and the oracle's
    iterates of (1 - lbd) * E * C * W S W^T + lbd * A with C = 0.5 (tests/test_exact_cpu.py, tests/test_gpu_exact_priors.py).
    `evidence=False`: the plan-level loop without the evidence factor (simrank_plan_options allows it).  Nobody writes to
    what this holds."""

    def __init__(self, name, df, symmetric, lbd, bits=2, evidence=True, mantissa=24, limit=8):
        from oracle import simrank_oracle as O
        self.name, self.df, self.symmetric, self.lbd, self.bits = name, df, symmetric, lbd, bits
        self.mantissa, self.limit = mantissa, limit
        self.labels, self.G = O.directed_graph(df)
        self.n = len(self.labels)
        assert self.labels == list(range(self.n))
        assert np.array_equal(O.weight(self.G), self.G)   # spread exactly 1, or 0 and 1 entries in a row: W is G
        self.E = O.evidence(self.G) if evidence else None
        self.A = loop_prior(self.n, bits, seed=self.n + bits + (0 if symmetric else 1), symmetric=symmetric,
                            half=mantissa == 11)
        self._exact, self._its = None, [np.eye(self.n)]

    def exact(self):
        if self._exact is None:
            self._exact = exact_updates(self.G, 0.5, self.E, mantissa=self.mantissa, limit=self.limit, prior=self.A,
                                        lbd=self.lbd)
            print(f"{self.name} {'symmetric' if self.symmetric else 'asymmetric'} {self.bits}-bit prior, lbd {self.lbd}, "
                  f"mantissa {self.mantissa}{'' if self.E is not None else ', no evidence'}: {self._exact}")
        return self._exact

    updates = property(lambda self: self.exact().updates)

    def iterates(self, updates=None):
        from oracle import simrank_oracle as O
        updates = self.updates if updates is None else updates
        while len(self._its) <= updates:
            self._its.append(O.update(self.G, self._its[-1], 0.5, 1.0 if self.E is None else self.E, self.A, self.lbd))
        return self._its[:updates + 1]

    def oracle(self, iterations, eps):
        """(S, k) of oracle.iterate_directed with the prior, from the cached iterates."""
        from oracle import simrank_oracle as O
        its = self.iterates(iterations)
        old = np.zeros((self.n, self.n))
        for k in range(iterations):
            if O.converged(old, its[k], eps):
                return its[k], k
            old = its[k]
        return its[iterations], None


# the cases of tests/test_gpu_exact_priors.py (here, so that tests/test_exact_cpu.py pins every one of them)
PRIOR_GRAPHS = [("regular", 300, 2), ("regular", 1031, 4), ("regular", 2100, 2), ("regular", 2100, 4)]
PRIOR_RANK_GRAPHS = [("regular", 512, 4), ("regular", 1031, 4)]     # 512: the half form of a sharded leg 2 at 2, 4, 8 ranks
PRIOR_LBD = (0.5, 0.25)
HUB_GRAPHS = [("hubs", 1031, (1, 2, 4, 8)), ("hubs", 1031, (2, 4))]
# rows of 2 and of 4 entries in a shuffled order, WITH evidence (2 exact updates; 1 with degrees up to 8): the graph on which
# the solver's ascending-length order is a real permutation, so that a plan's upload permutes the prior
MIXED_GRAPH = ("hubs", 1031, (2, 4))
PRIOR_F64 = [("regular", 300, 2), ("regular", 1031, 4)]
PRIOR_FP16 = [("regular", 300, 2), ("regular", 512, 2)]            # (a 1-bit prior; (1031, 4) has ONE exact update at 11 bits)
# (n1, n2, d1, lbd, matched): biregular_graph(384, 192, 2) has 1 exact update with priors, and so has every graph here at
# lbd 0.25 but the one with d1 = 1; matched_biregular_graph: the one in which an asymmetric prior reaches the other side
BI_PRIOR = [(256, 256, 2, 0.5, False), (384, 192, 1, 0.5, False), (384, 192, 1, 0.25, False), (384, 384, 2, 0.5, True)]
BI_PRIOR_KINDS = [(True, True), (False, True), (True, False)]     # both symmetric, prior 1 asymmetric alone, prior 2 alone
_graphs, _prior_cases = {}, {}


def loop_graph(key):
    """("regular", n, d) -> regular_graph(n, d, n + d); ("hubs", n, degrees) -> pow2_degree_graph(n, degrees, 48, 0.5, n); once."""
    if key not in _graphs:
        kind, n, d = key
        _graphs[key] = regular_graph(n, d, seed=n + d) if kind == "regular" else pow2_degree_graph(n, d, 48, 0.5, seed=n)
    return _graphs[key]


def prior_case(graph, symmetric, lbd, bits=2, evidence=True, mantissa=24):
    """The PriorCase of loop_graph(graph), built once per argument list and shared."""
    key = (graph, symmetric, lbd, bits, evidence, mantissa)
    if key not in _prior_cases:
        name = f"{graph[0]}_graph{graph[1:]}"
        # (the loop limit: 8 updates, 10 in float64; 4 from 2000 nodes on, where the oracle's dense update is the slowest
        # part of every test that leans on it)
        limit = 4 if graph[1] >= 2000 else 8 if mantissa < 53 else 10
        _prior_cases[key] = PriorCase(name, loop_graph(graph), symmetric, lbd, bits, evidence, mantissa, limit=limit)
    return _prior_cases[key]


class BiPriorCase:
    """biregular_graph(n1, n2, d1) with one prior per group (sorted label order, the corrected evidence of
    strict_reference=False): the oracle's matrices, the exact update count and the half-update iterates
    [(S1_1, S2_1), (S1_2, S2_2), ...] of oracle.iterate_bipartite with C1 = C2 = 0.5."""

    def __init__(self, n1, n2, d1, symmetric1, symmetric2, lbd, bits=2, mantissa=24, matched=False):
        from oracle import simrank_oracle as O
        self.n1, self.n2, self.lbd = n1, n2, lbd
        self.df = (matched_biregular_graph if matched else biregular_graph)(n1, n2, d1, seed=n1 + n2)
        base = O.fit_bipartite_pp(self.df, C1=0.5, C2=0.5, iterations=0, verbose=False, strict_reference=False)
        assert np.array_equal(base["W1"], base["G12"]) and np.array_equal(base["W2"], base["G21"])
        self.base = base
        self.A1 = loop_prior(n1, bits, seed=n1 + 10, symmetric=symmetric1)
        self.A2 = loop_prior(n2, bits, seed=n2 + 20, symmetric=symmetric2)
        self.exact = exact_updates_bipartite(base["G12"], base["G21"], 0.5, base["E1"], base["E2"], mantissa=mantissa, limit=4,
                                             prior1=self.A1, prior2=self.A2, lbd1=lbd, lbd2=lbd)
        print(f"{'matched_' if matched else ''}biregular_graph({n1}, {n2}, {d1}) priors {'sym' if symmetric1 else 'asym'} / {'sym' if symmetric2 else 'asym'}, "
              f"lbd {lbd}: {self.exact}")
        self.updates = self.exact.updates
        self.pairs = []
        s2 = np.eye(n2)
        for _ in range(self.updates):
            s1 = O.update(base["G12"], s2, 0.5, base["E1"], self.A1, lbd)
            s2 = O.update(base["G21"], s1, 0.5, base["E2"], self.A2, lbd)
            self.pairs.append((s1, s2))

    def oracle(self, iterations, eps):
        from oracle import simrank_oracle as O
        return O.fit_bipartite_pp(self.df, C1=0.5, C2=0.5, iterations=iterations, eps=eps, verbose=False, strict_reference=False,
                                  apriori1=self.A1, apriori2=self.A2, lbd1=self.lbd, lbd2=self.lbd)


_bi_cases = {}


def bi_prior_case(n1, n2, d1, lbd, matched, symmetric1, symmetric2):
    """The BiPriorCase of one entry of BI_PRIOR and one of BI_PRIOR_KINDS, built once and shared."""
    key = (n1, n2, d1, lbd, matched, symmetric1, symmetric2)
    if key not in _bi_cases:
        _bi_cases[key] = BiPriorCase(n1, n2, d1, symmetric1, symmetric2, lbd, matched=matched)
    return _bi_cases[key]


class BiLoop:
    """One two-matrix loop on bi_graph(name), C1 = C2 = 0.5: `pp` (the evidence factors; E2 = E1 position by position when
    `strict`), priors (`kinds` = (symmetric1, symmetric2) of 2-bit loop_priors, or None) with `lbd`.  The oracle's matrices,
    the exact update count (exact_updates_bipartite on the oracle's G12, G21, E1, E2) and the half-update iterates
    [(S1_1, S2_1), ...] of oracle.iterate_bipartite.  Built once per argument list (bi_loop); nobody writes to it."""

    def __init__(self, name, pp=False, strict=False, kinds=None, lbd=0.5, mantissa=24):
        from oracle import simrank_oracle as O
        self.O = O                                       # (imported here, as everywhere in this module: once per loop)
        self.name, self.pp, self.strict, self.kinds, self.lbd, self.mantissa = name, pp, strict, kinds, lbd, mantissa
        self.df = bi_graph(name)
        base = O.fit_bipartite_pp(self.df, C1=0.5, C2=0.5, iterations=0, verbose=False, strict_reference=False)
        assert np.array_equal(base["W1"], base["G12"]) and np.array_equal(base["W2"], base["G21"])
        self.G12, self.G21 = base["G12"], base["G21"]
        self.n1, self.n2 = self.G12.shape
        self.lab1, self.lab2 = list(base["sorted1"]), list(base["sorted2"])
        assert self.lab1 == list(range(self.n1)) and self.lab2 == list(range(self.n2))
        assert not strict or (pp and self.n1 == self.n2)
        self.E1 = base["E1"] if pp else None
        self.E2 = (base["E1"] if strict else base["E2"]) if pp else None
        self.A1 = self.A2 = None
        if kinds is not None:
            self.A1 = loop_prior(self.n1, 2, seed=self.n1 + 10, symmetric=kinds[0])
            self.A2 = loop_prior(self.n2, 2, seed=self.n2 + 20, symmetric=kinds[1])
        self.exact = exact_updates_bipartite(self.G12, self.G21, 0.5, self.E1, self.E2, mantissa=mantissa,
                                             limit=4 if mantissa < 53 else 6, prior1=self.A1, prior2=self.A2,
                                             lbd1=lbd if kinds else None, lbd2=lbd if kinds else None)
        print(f"bi_graph({name!r}) {'++' if pp else 'plain'}{' strict' if strict else ''} priors {kinds} lbd {lbd} "
              f"mantissa {mantissa}: {self.exact}")
        self.updates = self.exact.updates
        self.pairs = []
        s2 = np.eye(self.n2)
        for _ in range(self.updates):
            s1 = self.update(1, s2)
            s2 = self.update(2, s1)
            self.pairs.append((s1, s2))

    def update(self, group, S_other):
        O = self.O
        W, E, A = (self.G12, self.E1, self.A1) if group == 1 else (self.G21, self.E2, self.A2)
        if A is not None:
            return O.update(W, S_other, 0.5, 1.0 if E is None else E, A, self.lbd)
        return O.update(W, S_other, 0.5, E)

    def oracle(self, iterations, eps):
        """(S1, S2, k) of oracle.iterate_bipartite, from the cached half-updates."""
        O = self.O
        assert iterations <= self.updates
        old, new = (np.zeros((self.n1, self.n1)), np.zeros((self.n2, self.n2))), (np.eye(self.n1), np.eye(self.n2))
        for k in range(iterations):
            if O.converged(old[0], new[0], eps) and O.converged(old[1], new[1], eps):
                return new[0], new[1], k
            old, new = new, self.pairs[k]
        return new[0], new[1], None

    def lengths(self, group):
        """Row lengths of the group's pattern in the caller's order."""
        return ((self.G12 if group == 1 else self.G21) != 0).sum(axis=1)

    def tie_eps(self):
        """-> (U, eps, step): eps = the largest difference of either group between the states the loop compares at index
        U - 1 (the half-updates U - 1 and U - 2; state 0 is the identity pair) — the test there passes only under strict > —
        and the grid step of those states; asserted: the oracle's loop stops at U - 1 with eps and runs on with eps - step."""
        fmt = np.float64 if self.mantissa == 53 else np.float32
        U = self.updates
        states = [(np.eye(self.n1), np.eye(self.n2))] + self.pairs
        while U > 2 and all(np.array_equal(states[U - 1][j], states[U - 2][j]) for j in (0, 1)):
            U -= 1
        assert U >= 2
        new, old = states[U - 1], states[U - 2]
        eps = max(float(np.abs(new[j] - old[j]).max()) for j in (0, 1))
        step = 2.0 ** min(lowbit_exp(m) for m in new + old)
        assert eps >= step > 0 and float(fmt(eps)) == eps and float(fmt(eps - step)) == eps - step
        assert self.oracle(U, eps)[2] == U - 1 and self.oracle(U, eps - step)[2] is None
        return U, eps, step


def dealt_order(order, deal):
    """planprep.hip deal_order restated: the ascending order dealt to `deal` shards in runs of 128 (32) nodes, where the node
    count divides evenly; else the order itself."""
    order = np.asarray(order)
    n = order.size
    if deal <= 1 or n % (32 * deal):
        return order
    unit = 128 if n % (128 * deal) == 0 else 32
    per = n // (unit * deal)
    return order.reshape(per, deal, unit).transpose(1, 0, 2).reshape(n)


_bi_loops = {}


def bi_loop(name, pp=False, strict=False, kinds=None, lbd=0.5, mantissa=24):
    key = (name, pp, strict, kinds, lbd, mantissa)
    if key not in _bi_loops:
        _bi_loops[key] = BiLoop(*key)
    return _bi_loops[key]


def count_eps(new, old):
    """The three eps of a stepped count, each with NumPy's count under strict >: [0] an eps below every difference but
    zero, [1] a difference that occurs in the update — the largest but one where there are two, so that the elements that
    moved by exactly eps do not count and the ones above do —, [2] that minus one grid step (0.0 where that is all there
    is): the elements of [1]'s tie count again.  Differences of two iterates on a common grid are representable."""
    diff = np.abs(new - old)
    top = float(diff.max())
    below = diff[(diff < top) & (diff > 0)]
    tie = float(below.max()) if below.size else top
    step = 2.0 ** min(lowbit_exp(new), lowbit_exp(old))
    less = max(tie - step, 0.0)
    assert float(np.float32(tie)) == tie and float(np.float32(less)) == less
    return [(eps, int((diff > eps).sum())) for eps in (1e-30, tie, less)]


def tie_eps(iterates, fmt=np.float32):
    """-> (U, eps, step) for a loop that is to stop on a tie: U = the last update (of those given) that still moved an
    element (SimRank++ on a small regular graph reaches its fixed point exactly), eps = max |S_{U-1} - S_{U-2}|, a difference
    that occurs in the run — the test at loop index U - 1 of `iterations=U` passes only under strict > — and the grid step
    of those two iterates (eps - step may be 0: then every difference counts)."""
    U = len(iterates) - 1
    while U > 2 and not np.any(iterates[U - 1] != iterates[U - 2]):
        U -= 1
    a, b = iterates[U - 1], iterates[U - 2]
    eps = float(np.abs(a - b).max())
    step = 2.0 ** min(lowbit_exp(a), lowbit_exp(b))
    assert eps >= step > 0 and float(fmt(eps)) == eps and float(fmt(eps - step)) == eps - step
    return U, eps, step


# ---- the cases of tests/test_gpu_exact_kernels.py (here, so that tests/test_exact_cpu.py can build every operand) --------
LEG1_FUSED = [(520, 400, 333), (129, 77, 33), (130, 200, 2), (64, 1000, 96), (2100, 2100, 160)]
LEG1_GATHER = [(300, 257, 100), (64, 64, 64), (5, 5, 5)]
LEG1_SHARD = [((1024, 1024, 256), 256, 4), ((1024, 1024, 200), 128, 0), ((640, 900, 96), 0, 0), ((2048, 2048, 512), 256, 8),
              ((1000, 1000, 64), 384, 4)]
LEG1_UNITS = (300, 6000, 100)
LEG2_N = [64, 129, 1031, 2100]
HEADROOM = {"plain": 0, "evidence": 3, "all": 5}        # bits the epilogue needs: x 7/8 takes 3, the blend 2 more


def corner_case(M, K, seed, **kw):
    from tests.test_gpu_kernels import corner_csr
    return pow2_rowscale(corner_csr(M, K, seed=seed, **kw), seed)


def gather_case(M, K, seed):
    from tests.test_gpu_kernels import random_csr
    csr = random_csr(M, K, 9, seed=seed, heavy={1: min(K, 200), 3: min(K, 70)} if M > 3 else {})
    return pow2_rowscale(csr, seed)


def star_case():
    """The star of test_fused_long_rows_go_to_the_matrix_cores_whole: one row references every column."""
    M = K = 1500
    rng = np.random.default_rng(4)
    rows = [np.sort(rng.choice(K, size=3, replace=False)).astype(np.int32) for _ in range(M)]
    rows[700] = np.arange(K, dtype=np.int32)
    rows[701] = np.arange(0, K, 3, dtype=np.int32)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return pow2_rowscale(CSR(M, K, rowptr, np.concatenate(rows), np.ones(M)), 4)


def wide_ids_case(K=65537):
    """More than 65536 operand rows (32-bit ids whatever the knob says), the last columns referenced."""
    M = 420
    rng = np.random.default_rng(K)
    hubs = rng.choice(K - 8, size=60, replace=False)
    rows = []
    for a in range(M):
        c = set(rng.choice(K - 8, size=5, replace=False).tolist())
        if a < 300:
            c |= set(hubs[rng.random(60) < 0.3].tolist())
        if a % 7 == 3:
            c |= {K - 1}
        if a % 11 == 2:
            c |= {K - 2, K - 1}
        rows.append(np.array(sorted(c), dtype=np.int32))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return pow2_rowscale(CSR(M, K, rowptr, np.concatenate(rows), np.ones(M)), K)


def leg2_case(n, variant, mantissa=24, seed=None, exponent=0):
    """-> (csr, Symmetric, counts or None, prior or None, lbd, want float64) of a symmetric leg 2 with the epilogue."""
    seed = n if seed is None else seed
    csr = corner_case(n, n, seed, hubs=min(n, 150))
    return leg2_on(csr, variant, mantissa, seed, exponent)


def leg2_on(csr, variant, mantissa=24, seed=0, exponent=0):
    """leg2_case on a given pattern, n x K (row scales powers of two): the operand Tt is K x n, the counts, the prior and the
    result n x n."""
    n = csr.n_rows
    h = HEADROOM[variant] if mantissa == 24 else 0
    sym = summable_symmetric(csr, mantissa=mantissa, headroom=h, seed=seed, exponent=exponent)
    counts = epilogue_counts((n, n), seed, symmetric=True) if variant != "plain" else None
    prior = lbd = None
    if variant == "all":
        rs = np.where(csr.rowscale > 0, csr.rowscale, 1.0)
        bits = (mantissa - h - 1) if mantissa == 24 else 8
        prior = grid_prior(rs[:, None] * rs[None, :] * 2.0 ** exponent, bits, seed + 1, symmetric=True)
        lbd = 0.25
    want = exact_epilogue(product64(csr, sym.Tt), 0.5, counts, prior, lbd)
    assert np.array_equal(want, want.T)
    return csr, sym, counts, prior, lbd, want


# leg 2 on RECTANGULAR patterns (tests/test_gpu_exact_rect.py): (rows n, operand rows K) — K < n and K > n, the operand's
# rows_pad above and below the result's, and K = 20: fewer operand rows than a panel has columns
LEG2_RECT = [(129, 77), (520, 333), (64, 1000), (1031, 2100), (2100, 700), (660, 20)]
LEG2_RECT_BELOW = (63, 200)                             # fewer than 64 rows: no upper-triangle form


def rect_case(M, K, variant, mantissa=24, exponent=0):
    """leg2_case on corner_case(M, K, M + K, hubs=min(K, 150)): a symmetric leg 2 whose pattern is M x K."""
    seed = M + K
    return leg2_on(corner_case(M, K, seed, hubs=min(K, 150)), variant, mantissa, seed, exponent)


# ---- graphs built for leg 2's short path (tests/test_gpu_exact_short.py; the rule: tests/leg2_rule.py) -------------------
SHORT_WIDTHS = (0, 8, 16)
SHORT_EPS = 1.0                                          # as EPS of tests/test_gpu_exact_kernels.py
# The longest row of the heavy-row graph.  400 (tests/leg2_short_worker.py) holds summable_symmetric's integer assertion
# with the 19 bits that the "all" variant leaves; were it to fail there, this is the number to lower.
HEAVY_ROW = 400


def short_lengths():
    """name -> (row lengths in the caller's order, seed of the columns): the smallest shapes at which each new thing of
    short_group3 / build_short_image can go wrong.
    boundary   660 rows: groups short at both widths, at 16 only, never; rows of exactly 0, 8, 9, 16, 17 entries, a wholly
               empty tile, a ragged last tile of 20 rows (a multiple of 4: the vector mirror store with r4 < nrows) and a
               last panel of 20 columns (the scalar mirror store)
    ragged21   the same with 21 rows in the last tile (the scalar mirror store in whole panels too); ragged1: with 1 row
    n64        the smallest graph with an image: ONE group of two tiles, tiles 2 and 3 of the image are padding
    n63        no image (and no upper-triangle form): everything the rule counts is 0
    n129       a general group (one row of 17 entries) and a second group that is one tile of one row, short
    heavy_row  700 rows, one of HEAVY_ROW entries whose block is cut: cut tiles beside short groups, groups off the 128-row grid
    equal8 / equal16   150 rows of exactly 8 / 16 entries: within a tile the image's order is the reverse row order."""
    from tests import leg2_rule as R
    rng = np.random.default_rng(31)
    one = R.boundary_lengths(1)
    one[-1] = 5                                          # (a last row with entries: the 1-row tile does something)
    n64 = rng.integers(0, 9, 64)
    n64[[3, 40]] = 8
    n63 = rng.integers(0, 9, 63)
    n129 = rng.integers(0, 9, 129)
    n129[70], n129[128] = 17, 7
    return {"boundary": (R.boundary_lengths(20), 22), "ragged21": (R.boundary_lengths(21), 22), "ragged1": (one, 22),
            "n64": (n64.tolist(), 64), "n63": (n63.tolist(), 63), "n129": (n129.tolist(), 129),
            "heavy_row": (R.heavy_row_lengths(HEAVY_ROW), 24), "equal8": ([8] * 150, 41), "equal16": ([16] * 150, 42)}


SHORT_GRAPHS = ("boundary", "ragged21", "ragged1", "n64", "n63", "n129", "heavy_row", "equal8", "equal16")
SHORT_EQUAL = ("equal8", "equal16")
_short = {}


def short_case(name, variant, K=None):
    """leg2_case on short_lengths()[name]: -> (csr, Symmetric, counts, prior, lbd, want float64, row lengths).  Built once
    per (name, variant, K) and shared: nobody writes to what this returns.  `K`: the pattern's columns (None: as many as
    rows) — the same row lengths on a rectangular pattern."""
    key = (name, variant) if K is None else (name, variant, K)
    if key not in _short:
        from tests import leg2_rule as R
        lengths, seed = short_lengths()[name]
        csr = pow2_rowscale(R.from_lengths(lengths, seed, K), seed)
        assert np.array_equal(np.diff(csr.rowptr), lengths) and csr.n_cols == (len(lengths) if K is None else K)
        _short[key] = leg2_on(csr, variant, seed=seed) + (list(lengths),)
    return _short[key]


def tie_places_every_row(n, panel=32):
    """For EVERY row a: the diagonal, the first and the last column of a's own 32-column block, column n - 1 and one column
    of another panel, (7 a + 3) % n — about 5 n places, so every slot of every pass of every lane group of every tile
    holds a tie, on both sides of the diagonal (the upper-triangle forms compute (a, c) at row min(a, c))."""
    out, seen = [], set()
    for a in range(n):
        b0 = a // panel * panel
        for c in (a, b0, min(n - 1, b0 + panel - 1), n - 1, (7 * a + 3) % n):
            if (a, c) not in seen:
                seen.add((a, c))
                out.append((a, c))
    return out


_planted = {}


def short_planted(name, variant, K=None):
    """-> (want float32, Planted with all three kinds, Planted with "on" and "below" only) at tie_places_every_row; once."""
    key = (name, variant) if K is None else (name, variant, K)
    if key not in _planted:
        want = short_case(name, variant, K)[5]
        want32 = want.astype(np.float32)
        assert np.array_equal(want32.astype(np.float64), want)
        places = tie_places_every_row(want.shape[0])
        p = plant_previous(want32, SHORT_EPS, places, symmetric=True)
        q = plant_previous(want32, SHORT_EPS, places, symmetric=True, only=("on", "below"))
        _planted[key] = (want32, p, q)
    return _planted[key]


# ---- the count on fp16-held matrices (half.hip's header) ------------------------------------------------------------
def half_spacing(stored):
    """Half the fp16 spacing at the stored values (float64 array of fp16 numbers): 2^(max(exponent field, 1) - 26)."""
    bits = np.asarray(stored, dtype=np.float16).view(np.uint16)
    field = np.maximum((bits >> 10) & 31, 1).astype(np.int64)
    return np.ldexp(1.0, field - 26)


def half_moved(new_stored, old_stored, eps_stored):
    """The rule of half.hip: an element moved when |new (before rounding) - old (stored)| > eps + half the spacing at old."""
    return np.abs(new_stored - old_stored) > eps_stored + half_spacing(old_stored)


def plant_previous_half(want_stored, eps_stored, places, symmetric=False):
    """fp16 `previous` (stored units) = want rounded, except at `places`: differences a whole fp16 spacing and more ABOVE
    the widened eps, a whole spacing and more BELOW it, in turn; the caller plants the tie itself (it needs a new value
    that lies half a spacing off the fp16 grid: the diagonal).  -> (previous as float64 of fp16 values, kinds)."""
    want = np.asarray(want_stored, dtype=np.float64)
    prev = want.astype(np.float16).astype(np.float64)
    kinds = []
    for i, (r, c) in enumerate(places):
        v = want[r, c]
        kind = ("above", "below")[i % 2]
        sign = 1.0 if (i // 2) % 2 == 0 else -1.0
        sp = 2 * float(half_spacing(np.float16(abs(v) + 2 * eps_stored)))       # the spacing where the old value will lie
        cand = np.float16(v + sign * (eps_stored + 4 * sp if kind == "above" else max(0.0, eps_stored - 4 * sp)))
        old = float(cand)
        widened = eps_stored + float(half_spacing(cand))
        gap = abs(v - old) - widened
        spo = 2 * float(half_spacing(cand))
        # (where the spacing exceeds eps, "below" is the rounded value itself: inside the bound by eps at least)
        assert np.isfinite(old) and (gap >= spo if kind == "above" else gap <= -min(spo, eps_stored)), (r, c, v, old, kind)
        prev[r, c] = old
        if symmetric:
            assert want[c, r] == v
            prev[c, r] = old
        kinds.append(kind)
    return prev, kinds
