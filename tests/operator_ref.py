"""The NumPy statement of ``matmul`` and ``embed`` (include/simrank_operator.h, simrank_amd/_operator.py), the bounds their
GPU tests hold the device to, and the operands on which a product is exact in any order.  Written for reading.

The bounds are derived, not measured (DESIGN.md 4.29 has the derivation), with u = 2^-52, which is twice the unit
roundoff of a double and so covers every "1 + O(u)" factor dropped at first order:

    product      |computed - reference| <= K u sum_k |S[m][k]| |X[k][q]|, K the length of the contraction: a sum of K
                 products in any order, fused or not, is within K u / 2 of the exact one at first order (gamma_K with the
                 unit roundoff u / 2), the device's and the NumPy reference's alike, so the two are within K u
    c1(p)        max |V.T V - I| <= c1 u:   c1 = 4 N p^1.5 + 8 p^2
                 Householder QR of an N x p matrix leaves ||Q.T Q - I||_F <= 2 sqrt(p) gamma_{N p} (Higham, Accuracy and
                 Stability of Numerical Algorithms, 2nd ed., eq. 19.13), written 4 N p^1.5 u with the constant of gamma
                 doubled; the eigenvectors of ``eigh`` lose at most p^2 u of their orthogonality in norm (LAPACK Users'
                 Guide 4.7, p(n) taken as n^2, once for the backward error and once for Z itself), and the product
                 Q @ Z adds gamma_p |Q| |Z| on either side of V.T V, 2 p^2 u each at most
    c2(p)        |eigenvalue_i - v_i.T M v_i| <= (N + c2) u || |M| ||_2:
                 c2 = N (sqrt(p) + p + 1) + c1(p) + 2 p^2 + 2 p^1.5 + 2 sqrt(p)
                 the two device products carry (N + 2) u |M| |Q| into Y, seen through v and |Q| |z| (norm sqrt(p));
                 B = Q.T @ Y carries N u |Q.T| |Y|, at most N p u ||M||; ``eigh`` returns eigenvalues of B + E with
                 ||E|| <= p^2 u ||B|| and a Rayleigh quotient within the same of them; V = Q @ Z is p^1.5 u off, twice;
                 v is c1 u off unit length; and the reference v.T (M v) is itself 2 N u |v|.T |M| |v| off, of which one
                 N stands in front of the bracket.  || |M| ||_2 >= ||M||_2 bounds every norm of M used on the way.
"""
import numpy as np

U = 2.0 ** -52


def matmul_ref(S, X, transpose=False):
    S, X = np.asarray(S, dtype=np.float64), np.asarray(X, dtype=np.float64)
    return (S.T if transpose else S) @ X


def product_bound(S, X, transpose=False, factor=1):
    """float64 [n_out, d]: ``factor`` x K x u x (|S| @ |X|)."""
    A = np.abs(np.asarray(S, dtype=np.float64))
    A = A.T if transpose else A
    return factor * A.shape[1] * U * (A @ np.abs(np.asarray(X, dtype=np.float64)))


def sym(S):
    S = np.asarray(S, dtype=np.float64)
    return (S + S.T) / 2


def embed_ref(product, N, dim, oversample=8, power_iterations=2, seed=0):
    """The statement of ``embed`` with ``product(Q) = M @ Q`` passed in -> (V float64 [N, dim], w float64 [dim])."""
    p = min(dim + oversample, N)
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((N, p)))[0]
    for _ in range(power_iterations):
        Q = np.linalg.qr(product(Q))[0]
    Y = product(Q)
    B = Q.T @ Y
    B = (B + B.T) / 2
    w, Z = np.linalg.eigh(B)
    order = np.argsort(-w, kind="stable")[:dim]
    V = Q @ Z[:, order]
    for c in range(V.shape[1]):
        if V[np.argmax(np.abs(V[:, c])), c] < 0:
            V[:, c] = -V[:, c]
    return V, w[order]


def c1(p, N):
    return 4.0 * N * p ** 1.5 + 8.0 * p ** 2


def c2(p, N):
    return N * (np.sqrt(p) + p + 1.0) + c1(p, N) + 2.0 * p ** 2 + 2.0 * p ** 1.5 + 2.0 * np.sqrt(p)


def check_embedding(V, w, M, p, what=""):
    """The invariants of an embedding (V [N, dim], w [dim]) of the symmetric matrix M: orthonormal columns, eigenvalues
    that are the Rayleigh quotients, descending, and the sign rule.  Prints each figure before it asserts."""
    V, w, M = np.asarray(V, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(M, dtype=np.float64)
    N, dim = V.shape
    gram = np.abs(V.T @ V - np.eye(dim)).max()
    print(what, "max |V.T V - I| =", gram, "bound", c1(p, N) * U)
    assert gram <= c1(p, N) * U, what
    norm = np.linalg.norm(np.abs(M), 2)
    rayleigh = np.einsum("ic,ic->c", V, M @ V)
    off = np.abs(w - rayleigh).max()
    print(what, "max |w - v.T M v| =", off, "bound", (N + c2(p, N)) * U * norm)
    assert off <= (N + c2(p, N)) * U * norm, what
    assert (np.diff(w) <= 0).all(), what
    at = np.argmax(np.abs(V), axis=0)
    assert (V[at, np.arange(dim)] > 0).all(), what


def planted(N=257, values=(4.0, 3.0, 2.0, 1.0)):
    """A symmetric matrix of EXACT rank len(values) with those non-zero eigenvalues, every entry a multiple of 2^-8: the
    sum of value_i / 256 x h_i h_i.T over Walsh vectors h_i (+-1 on the first 256 nodes, mutually orthogonal, of squared
    length 256) and 0 on the rest.  No entry is rounded, so the rank is exact in float64."""
    H = np.array([[1.0]])
    while H.shape[0] < 256:
        H = np.block([[H, H], [H, -H]])
    assert N >= 256 and np.array_equal(H @ H.T, 256 * np.eye(256))
    M = np.zeros((N, N))
    for i, v in enumerate(values):
        h = np.zeros(N)
        h[:256] = H[3 + 5 * i]
        M += (v / 256.0) * np.outer(h, h)
    assert np.array_equal(M, M.T) and np.array_equal(M * 256, np.round(M * 256))
    return M


# ---- operands on which every product and every partial sum is exact ----------------------------------------------------
def exact_operand(rng, n, d, layout):
    """float64 [n, d]: small integers times powers of two, sized for the dyadic blocks of tests/blocks.py: integers of
    magnitude <= 15 times 2^e with e in {-2, -1, 0, 1} (2^-2 steps, magnitude < 2^5)."""
    return rng.integers(-15, 16, size=(n, d)) * 2.0 ** rng.integers(-2, 2, size=(n, d))


def assert_exact(A, X, alpha=1.0, beta=0.0, out0=None):
    """Integer arithmetic on the host: with A in steps of 2^-10 and X in steps of 2^-2, every product is an integer of
    2^-12 steps and the sum of the magnitudes of a whole row of products stays below 2^53 steps, so every partial sum in
    any order, fused or not, is exact in a double; so are the scaled result and the epilogue."""
    a = np.asarray(A, dtype=np.float64) * 1024.0
    x = np.asarray(X, dtype=np.float64) * 4.0
    assert np.array_equal(a, np.round(a)) and np.array_equal(x, np.round(x))
    assert np.abs(a).max(initial=0) * np.abs(x).max(initial=0) * max(1, a.shape[1]) < 2.0 ** 62    # (int64 holds the sums)
    steps = np.abs(a).astype(np.int64) @ np.abs(x).astype(np.int64)
    assert steps.max(initial=0) < 2 ** 52
    if out0 is not None and beta != 0.0:
        o = np.abs(np.asarray(out0, dtype=np.float64)) * 4096.0
        assert np.array_equal(o, np.round(o))
        assert (abs(alpha) * steps.astype(np.float64) + abs(beta) * o).max() * 4 < 2.0 ** 52


# ---- shapes at which one workgroup walks SEVERAL tiles of the contraction -------------------------------------------------
# operator.hip cuts the contraction into parts = min(ceil(1536 / strips), tiles, 64) and gives a workgroup
# tiles_per_part = ceil(tiles / parts) tiles: one, unless tiles > 64.  These are the smallest shapes past that, per kernel:
# (kernel, n_rows, n_cols, transpose, the d's it is run at, output rows per strip, contraction steps per tile).
LONG_CASES = [
    ("product, TQ = 4", 131, 2130, 0, (9, 32), 128, 32),
    ("product, TQ = 8", 131, 2130, 0, (33, 64), 128, 32),
    ("product, TQ = 8", 5, 4200, 0, (33, 64), 128, 32),
    ("product, transposed", 2130, 131, 1, (9, 64), 128, 32),
    ("product, transposed", 4200, 5, 1, (9, 64), 128, 32),
    ("rows", 20, 16700, 0, (1, 8), 16, 256),
    ("rows", 20, 33000, 0, (1, 8), 16, 256),
    ("rows", 20, 16400, 0, (1, 8), 16, 256),            # 65 tiles in parts of 2: the one rows shape with a short last part
    ("cols", 4200, 9, 1, (1, 8), 1024, 64),
    ("cols", 8300, 40, 1, (1, 8), 1024, 64),
]
LONG_IDS = ["%s %dx%d" % (c[0].replace(",", "").replace(" ", "_").replace("=", ""), c[1], c[2]) for c in LONG_CASES]


def split_of(lib, case, d):
    """(tiles, parts, tiles per part, tiles of the last part) of a LONG_CASES entry at d: the parts from the library, the
    tiles from the mirrored depth."""
    _, n_rows, n_cols, transpose, _, _, depth = case
    n_in = n_rows if transpose else n_cols
    tiles = -(-n_in // depth)
    parts = lib.simrank_operator_parts(n_rows, n_cols, transpose, d)
    assert 1 <= parts <= tiles
    per = -(-tiles // parts)
    return tiles, parts, per, tiles - (parts - 1) * per


def assert_long_cases_walk_several_tiles(lib):
    """Every case has a workgroup that takes at least two tiles, its last part is not empty, and every kernel has one case
    whose last part is shorter than the others: a change to the split makes this fail instead of quietly going back to
    one tile per part."""
    short = {}
    for case in LONG_CASES:
        for d in case[4]:
            tiles, parts, per, last = split_of(lib, case, d)
            assert per >= 2 and 1 <= last <= per, (case, d, tiles, parts, per, last)
            short[case[0]] = short.get(case[0], False) or last < per
    assert short and all(short.values()), short
