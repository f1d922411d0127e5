// Density clusters of an iterate that stays on the device (include/simrank_density.h, libsimrank_density.so): how many
// neighbours every node has under "S[a][b] >= t or S[b][a] >= t", and DBSCAN's clusters grown through the core nodes.
//
// The degrees sweep is the one kernel of this project that pairs entry (a, b) with entry (b, a).  The square block is cut
// into 64 x 64 tiles and one workgroup takes a PAIR of tiles (I, J), I <= J: tile (I, J) holds S[a][b] for a in I, b in
// J and tile (J, I) holds S[b][a] for the same nodes.  A wave reads a tile's row with one element per lane (the 64
// columns of a row are 128 to 512 contiguous bytes in every layout, and the tile's lines are used whole; the binary16
// panels take two rows per load, 4 bytes per lane, and keep their masks in the bit order of slot()), and the
// compare of a level IS the ballot: a 64-bit pass mask per row and level, parked in LDS (2 tiles x 8 levels x 64 rows x
// 8 bytes = 8 KiB, and one word of padding per level).  Then, per level, lane a of a wave owns row a of the first tile:
// its own mask, ORed with column a of the second tile's bit matrix (64 reads of one LDS word that the whole wave shares: a broadcast, no bank conflict),
// minus padding and the node itself, is the set of a's neighbours in J; its popcount goes to deg with an integer atomic
// add.  The same with the tiles' roles swapped counts the neighbours in I of every node of J.  Every element is read
// once, a pair that passes both ways is one bit, and the sums are exact in any order.
//
// The union sweep is cluster.hip's walk and forest (this library's own copy of them), for one level, with DBSCAN's rule
// on top: an entry unites only two core nodes; between a core node and another it lowers the other's `attach` to the
// core node (an atomic minimum, tried only when a read says it would change something); between two others it does
// nothing.  Every read of `parent` and `attach` is a relaxed device-scope load, as in cluster.hip, and nothing waits:
// walks and retries are capped, a cap reached or a value out of order sets a bit of *status and drops the edge.
#include <algorithm>
#include <type_traits>

#include "simrank_density.h"

#define COMPANION_ERR_INVALID SIMRANK_DENSITY_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_DENSITY_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_DENSITY_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_DENSITY_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_DENSITY_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_DENSITY_, ROWMAJOR_F64);

constexpr int kMaxLevels = SIMRANK_DENSITY_MAX_LEVELS;
constexpr int kTile = SIMRANK_DENSITY_TILE;
constexpr int kThreads = kSweepThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxGrid = kSweepMaxGrid;
constexpr unsigned kCapSlack = 8;
constexpr int32_t kNone = SIMRANK_DENSITY_NONE;
// A level's 64 masks and one word of padding: lane l stores level l's mask of a row, and 65 words of 8 bytes put the
// lanes' stores 2 banks apart where 64 words would put all of them into the same two banks.
constexpr int kMaskRow = kTile + 1;
static_assert(kTile == 64, "a row's pass mask is one wave's ballot");
static_assert(kTile % kWaves == 0, "the waves share a tile's rows evenly");

// ---- the degrees sweep ---------------------------------------------------------------------------------------------------
// Which bit of a 64-bit pass mask stands for column c (0 .. 63) of a tile.  One element per lane leaves the columns in
// their order.  The binary16 panels are loaded as 4 bytes per lane, two rows per wave load, and a lane's two columns
// come out 32 bits apart: the even columns fill the low half of a mask and the odd ones the high half.  Every mask of a
// sweep uses the one order, so ORs and popcounts never notice; only the transposed read and the valid masks name bits.
template <int LAYOUT>
__device__ inline int slot(int c) {
    if constexpr (LAYOUT == PANEL_F16) return (c >> 1) + 32 * (c & 1);
    else return c;
}

// The pass masks of the tile whose rows start at position r0 and columns at c0: mask[l][row] bit slot(j) =
// v(r0 + row, c0 + j) >= edge[l].  Rows past n read nothing and pass nothing (columns past n: the valid mask of
// degrees_kernel takes them out).  A wave takes kTile / kWaves rows, all of their loads in flight together; lane l keeps
// level l's ballot and stores it, one LDS store per row.
template <int LAYOUT>
__device__ inline void tile_masks(const void* __restrict__ S, int64_t stride, int64_t n, int64_t r0, int64_t c0,
                                  const typename Elem<LAYOUT>::Cmp (&edge)[kMaxLevels], int n_levels,
                                  uint64_t (*mask)[kMaskRow], int wave, int lane) {
    using Cmp = typename Elem<LAYOUT>::Cmp;
    constexpr int kRows = kTile / kWaves;
    const int row0 = wave * kRows;
    if constexpr (LAYOUT == PANEL_F16) {
        // A row of the tile is the 128 contiguous bytes of its panel's row (c0 is a multiple of 64; the panel's tail past
        // n is stored): lanes 0 .. 31 take one row and lanes 32 .. 63 the next, 4 bytes each, 256 contiguous bytes a load.
        using E = Elem<LAYOUT>;
        const uint32_t* words = static_cast<const uint32_t*>(S);
        const int64_t panel = c0 >> 6;
        uint32_t x[kRows / 2];
#pragma unroll
        for (int u = 0; u < kRows / 2; ++u) {
            const int64_t r = r0 + row0 + 2 * u + (lane >> 5);
            x[u] = 0x7e007e00u;                                          // (two NaN: they pass nothing)
            if (r < n) x[u] = words[(panel * stride + r) * 32 + (lane & 31)];
        }
#pragma unroll
        for (int u = 0; u < kRows / 2; ++u) {
            const Cmp even = E::value(x[u] & 0xffffu), odd = E::value(x[u] >> 16);
            uint64_t first = 0, second = 0;
#pragma unroll
            for (int l = 0; l < kMaxLevels; ++l) {
                if (l >= n_levels) break;                                // (wave-uniform)
                const uint64_t e = __ballot(even >= edge[l]), o = __ballot(odd >= edge[l]);
                if (lane == l) {
                    first = (e & 0xffffffffull) | (o << 32);             // the row of lanes 0 .. 31
                    second = (e >> 32) | (o & 0xffffffff00000000ull);    // the row of lanes 32 .. 63
                }
            }
            if (lane < n_levels) {
                mask[lane][row0 + 2 * u] = first;
                mask[lane][row0 + 2 * u + 1] = second;
            }
        }
        return;
    }
    const int64_t c = c0 + lane;
    Cmp v[kRows];                                                        // (the loads of all of the wave's rows in flight together)
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
        const int64_t r = r0 + row0 + u;
        v[u] = Cmp(__builtin_nanf(""));                                  // (NaN passes nothing)
        if (r < n && c < n) v[u] = load<LAYOUT>(S, stride, r, c);
    }
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
        uint64_t mine = 0;
#pragma unroll
        for (int l = 0; l < kMaxLevels; ++l) {
            if (l >= n_levels) break;                                    // (wave-uniform)
            const uint64_t m = __ballot(v[u] >= edge[l]);                // (-0.0 >= +0.0 passes)
            if (lane == l) mine = m;
        }
        if (lane < n_levels) mask[lane][row0 + u] = mine;
    }
}

// (I, J), I <= J, of pair p = J (J + 1) / 2 + I.  The square root is a first guess that two steps either way correct
// (8 p + 1 < 2^53 is exact in a double; the root is off by less than one).
__device__ inline void tiles_of_pair(int64_t p, int64_t& I, int64_t& J) {
    int64_t j = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    if (j * (j + 1) / 2 > p) --j;
    if (j * (j + 1) / 2 > p) --j;
    if ((j + 1) * (j + 2) / 2 <= p) ++j;
    if ((j + 1) * (j + 2) / 2 <= p) ++j;
    J = j;
    I = p - j * (j + 1) / 2;
}

template <int LAYOUT>
__global__ __launch_bounds__(kThreads) void degrees_kernel(const void* __restrict__ S, int64_t stride, int64_t n,
                                                           const int32_t* __restrict__ ids,
                                                           const typename Elem<LAYOUT>::Cmp* __restrict__ edges_dev,
                                                           int n_levels, int32_t* __restrict__ deg, int64_t n_pairs) {
    using Cmp = typename Elem<LAYOUT>::Cmp;
    __shared__ uint64_t mask[2][kMaxLevels][kMaskRow];   // [tile (I, J) | tile (J, I)][level][row (+ 1 of padding)]
    __shared__ uint64_t valid[2];                        // bit slot(j): position 64 I + j (64 J + j) is a node
    __shared__ int32_t node[2][kTile];                   // its id
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    Cmp edge[kMaxLevels];
#pragma unroll
    for (int l = 0; l < kMaxLevels; ++l) edge[l] = edges_dev[l < n_levels ? l : 0];

    for (int64_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        int64_t I, J;
        tiles_of_pair(p, I, J);
        const bool diag = I == J;
        if (wave < 2) {                                                  // wave 0: the nodes of I; wave 1: of J
            const int local = LAYOUT == PANEL_F16 ? 2 * (lane & 31) + (lane >> 5) : lane;     // slot(local) == lane
            const int64_t pos = (wave == 0 ? I : J) * kTile + local;
            int32_t id = -1;
            if (pos < n) id = ids ? ids[pos] : int32_t(pos);
            const bool ok = id >= 0 && id < n;                           // (an id outside the nodes is padding)
            node[wave][local] = id;
            const uint64_t m = __ballot(ok);
            if (lane == 0) valid[wave] = m;
        }
        tile_masks<LAYOUT>(S, stride, n, I * kTile, J * kTile, edge, n_levels, mask[0], wave, lane);
        if (!diag) tile_masks<LAYOUT>(S, stride, n, J * kTile, I * kTile, edge, n_levels, mask[1], wave, lane);
        __syncthreads();

        // item (level, side): side 0 counts, for the nodes of I, their neighbours in J; side 1 the other way round
        const int sides = diag ? 1 : 2;
        for (int it = wave; it < n_levels * sides; it += kWaves) {
            const int l = it / sides, side = it - l * sides;
            const uint64_t* rows = mask[side][l];
            const uint64_t* other = mask[diag ? 0 : 1 - side][l];
            uint64_t w = rows[lane];
            const int own = slot<LAYOUT>(lane);
#pragma unroll 8
            for (int j = 0; j < kTile; ++j) w |= ((other[j] >> own) & 1ull) << slot<LAYOUT>(j);   // column `lane`, transposed
            w &= valid[diag ? 0 : 1 - side];
            if (diag) w &= ~(1ull << own);                               // (a node is not its own neighbour)
            const int count = __popcll(w);
            if (((valid[side] >> own) & 1ull) && count)
                atomicAdd(reinterpret_cast<int*>(deg + int64_t(l) * n + node[side][lane]), count);
        }
        __syncthreads();                                                 // (the next pair overwrites the masks)
    }
}

// ---- the forest (cluster.hip's, for one level) ------------------------------------------------------------------------------
__device__ inline int32_t ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a parent p read at node x is in order when 0 <= p <= x (x itself is in 0 .. n - 1)
__device__ inline bool in_order(int32_t p, int32_t x) { return uint32_t(p) <= uint32_t(x); }

// The root above x (0 <= x < n), or -1 with a bit of `bad` set.  WRITE: path halving, parent[x] = its grandparent as just
// read.  x is no root then and never becomes one again, so the store meets no compare-and-swap that could succeed.
template <bool WRITE>
__device__ inline int32_t find(typename std::conditional<WRITE, int32_t, const int32_t>::type* P, int32_t x, unsigned cap,
                               unsigned& bad) {
    for (unsigned it = 0; it < cap; ++it) {
        const int32_t p = ld(P + x);
        if (p == x) return x;
        if (!in_order(p, x)) {
            bad |= SIMRANK_DENSITY_BAD_PARENT;
            return -1;
        }
        const int32_t gp = ld(P + p);
        if (gp == p) return p;
        if (!in_order(gp, p)) {
            bad |= SIMRANK_DENSITY_BAD_PARENT;
            return -1;
        }
        if constexpr (WRITE) st(P + x, gp);
        x = gp;
    }
    bad |= SIMRANK_DENSITY_CAP_REACHED;
    return -1;
}

// Hook the larger of the roots a != b under the smaller.  A swap that finds the larger one hooked already goes on from
// the parent it found there: below the node it was tried on, so the larger side falls with every turn.  Returns the
// smaller root the pair ended under, or -1 with a bit of `bad` set.
__device__ inline int32_t unite(int32_t* P, int32_t a, int32_t b, unsigned cap, unsigned& bad) {
    for (unsigned it = 0; it < cap; ++it) {
        if (a == b) return a;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = (int32_t)atomicCAS(reinterpret_cast<int*>(P + hi), (int)hi, (int)lo);
        if (old == hi) return lo;
        if (!in_order(old, hi)) {
            bad |= SIMRANK_DENSITY_BAD_PARENT;
            return -1;
        }
        a = find<true>(P, old, cap, bad);
        b = find<true>(P, lo, cap, bad);
        if (a < 0 || b < 0) return -1;
    }
    bad |= SIMRANK_DENSITY_CAP_REACHED;
    return -1;
}

// attach[x] = min(attach[x], core): the atomic only where a read says it would lower the value (a value read late is
// only larger than the current one: the atomic then changes nothing)
__device__ inline void claim(int32_t* attach, int32_t x, int32_t core) {
    if (ld(attach + x) > core) atomicMin(reinterpret_cast<int*>(attach + x), (int)core);
}

// ---- the union sweep -------------------------------------------------------------------------------------------------------
template <int LAYOUT>
__global__ __launch_bounds__(kThreads) void union_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                         int64_t n_cols, const int32_t* __restrict__ row_ids,
                                                         const int32_t* __restrict__ col_ids,
                                                         const typename Elem<LAYOUT>::Cmp* __restrict__ edge_dev,
                                                         const int32_t* __restrict__ deg, int32_t min_neighbors,
                                                         int32_t* parent, int32_t* attach, int64_t n, int32_t* status,
                                                         int vec) {
    using E = Elem<LAYOUT>;
    using Cmp = typename E::Cmp;
    WALK_GEOMETRY(LAYOUT, n_cols);
    const unsigned cap = unsigned(n) + kCapSlack;
    unsigned bad = 0;
    const Cmp edge = edge_dev[0];
    int32_t* const P = parent;

    // `mine`: a member of the (core) row node's cluster, its root as of this lane's last walk.
    int32_t mine = -1;

    // The slow path of one entry between two core nodes, called by every lane of the wave together (`act`: this lane's
    // entry is an edge whose column parent differed from `mine`).
    auto join = [&](bool act, int32_t cid) {
        int32_t a = -1, b = -1;
        if (act) act = ld(P + cid) != mine;                              // (an earlier entry of the piece may have settled it)
        if (act) {
            a = find<true>(P, mine, cap, bad);
            b = find<true>(P, cid, cap, bad);
            act = a >= 0 && b >= 0;
            if (act) {
                mine = a;
                if (b != cid && ld(P + cid) != b) st(P + cid, b);        // the next read of this column ends at once
                act = a != b;
            }
        }
        // one lane per distinct pair of roots goes on to the swap
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        bool rep = act;
        uint64_t pending = __ballot(act);
        while (pending) {                                                // (wave-uniform; one turn per distinct pair)
            const int lead = __ffsll((unsigned long long)pending) - 1;
            const int32_t hi0 = __builtin_amdgcn_readlane(hi, lead), lo0 = __builtin_amdgcn_readlane(lo, lead);
            const bool same = act && hi == hi0 && lo == lo0;
            if (same && lane != lead) rep = false;
            pending &= ~__ballot(same);
        }
        if (rep) {
            const int32_t root = unite(P, a, b, cap, bad);
            if (root >= 0) mine = root;
        }
    };

    for (int64_t r0 = wave * R; r0 < n_rows; r0 += nwaves * R) {
        const int64_t r = r0 + g;
        const bool live = r < n_rows;
        const int32_t rid = live ? (row_ids ? row_ids[r] : int32_t(r)) : -1;
        const bool row_ok = live && rid >= 0 && rid < n;                 // (an id outside the nodes is padding)
        const bool row_core = row_ok && deg[rid] >= min_neighbors;
        mine = rid;
        int32_t best = kNone;                                            // a non-core row: its smallest core column so far
        for (int64_t k0 = 0; k0 < n_chunks; k0 += U) {
            WALK_LOAD(LAYOUT, x, S, stride, r, live, k0, n_cols, vec)
#pragma unroll 1
            for (int u = 0; u < U; ++u) {
                if (k0 + u >= n_chunks) break;                           // (wave-uniform)
                const v4u32 xu = u == 0 ? x[0] : u == 1 ? x[1] : u == 2 ? x[2] : x[3];
                const int64_t c0 = (k0 + u) * W + int64_t(q) * V;
                int32_t cid[V];
                unsigned hit = 0;                                        // bit i: value i is a passing entry between two nodes
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const Cmp v = E::value(E::raw(xu, i));
                    cid[i] = 0;
                    if (row_ok && c0 + i < n_cols && v >= edge) {        // (NaN passes nothing; -0.0 >= +0.0 passes)
                        cid[i] = col_ids ? col_ids[c0 + i] : int32_t(c0 + i);
                        if (cid[i] != rid && cid[i] >= 0 && cid[i] < n) hit |= 1u << i;
                    }
                }
                if (!__ballot(hit != 0)) continue;                       // (wave-uniform)
                unsigned open = 0;                                       // bit i: two core nodes whose clusters may differ
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if (!((hit >> i) & 1)) continue;
                    const bool col_core = deg[cid[i]] >= min_neighbors;
                    if (row_core && col_core) {
                        if (ld(P + cid[i]) != mine) open |= 1u << i;
                    } else if (row_core) {
                        claim(attach, cid[i], rid);
                    } else if (col_core) {
                        best = cid[i] < best ? cid[i] : best;
                    }
                }
                if (!__ballot(open != 0)) continue;                      // (wave-uniform)
#pragma unroll 1
                for (int i = 0; i < V; ++i) {
                    const bool act = (open >> i) & 1;
                    if (!__ballot(act)) continue;                        // (wave-uniform)
                    join(act, act ? (col_ids ? col_ids[c0 + i] : int32_t(c0 + i)) : 0);
                }
            }
        }
        if (best != kNone) claim(attach, rid, best);
    }
    if (bad) atomicOr(reinterpret_cast<int*>(status), (int)bad);
}

__global__ __launch_bounds__(kThreads) void init_kernel(int32_t* __restrict__ deg, int32_t* __restrict__ parent,
                                                        int32_t* __restrict__ attach, int64_t n, int64_t total,
                                                        int32_t* __restrict__ status) {
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < total; i += step) {
        deg[i] = 0;
        if (parent && i < n) {
            parent[i] = int32_t(i);
            attach[i] = kNone;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = 0;
}

__global__ __launch_bounds__(kThreads) void labels_kernel(const int32_t* parent, const int32_t* attach,
                                                          const int32_t* __restrict__ deg, int32_t min_neighbors, int64_t n,
                                                          int32_t* __restrict__ labels, int32_t* status) {
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    const unsigned cap = unsigned(n) + kCapSlack;
    unsigned bad = 0;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += step) {
        int32_t from = int32_t(i);
        if (deg[i] < min_neighbors) {
            from = ld(attach + i);
            if (from == kNone) {
                labels[i] = -1;                                          // noise
                continue;
            }
            if (from < 0 || from >= n) {
                bad |= SIMRANK_DENSITY_BAD_PARENT;
                labels[i] = -1;
                continue;
            }
        }
        labels[i] = find<false>(parent, from, cap, bad);
    }
    if (bad) atomicOr(reinterpret_cast<int*>(status), (int)bad);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int check_nodes(int64_t n, const void* status) {
    REQUIRE(n >= 0 && n < (int64_t(1) << 31) - kCapSlack, "bad node count %lld", (long long)n);
    REQUIRE(status, "status is NULL");
    return SIMRANK_DENSITY_OK;
}

int check_levels(int32_t n_levels) {
    REQUIRE(n_levels >= 1 && n_levels <= kMaxLevels, "n_levels must be 1 .. %d (got %d)", kMaxLevels, (int)n_levels);
    return SIMRANK_DENSITY_OK;
}

int check_forest(const void* parent, const void* attach, const void* deg, int32_t min_neighbors, int64_t n,
                 const void* status) {
    const int rc = check_nodes(n, status);
    if (rc) return rc;
    REQUIRE(min_neighbors >= 0, "min_neighbors must be >= 0 (got %d)", (int)min_neighbors);
    REQUIRE(n == 0 || parent, "parent is NULL");
    REQUIRE(n == 0 || attach, "attach is NULL");
    REQUIRE(n == 0 || deg, "deg is NULL");
    return SIMRANK_DENSITY_OK;
}

int flat_grid(int64_t total) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((total + kThreads - 1) / kThreads, kMaxGrid));
}

}  // namespace

extern "C" {

int simrank_density_version(void) { return SIMRANK_DENSITY_VERSION; }

const char* simrank_density_last_error(void) { return g_error.c_str(); }

int simrank_density_init(int32_t* deg, int32_t* parent, int32_t* attach, int64_t n, int32_t n_levels, int32_t* status,
                         void* stream) {
    int rc = check_nodes(n, status);
    if (rc) return rc;
    rc = check_levels(n_levels);
    if (rc) return rc;
    REQUIRE(n == 0 || deg, "deg is NULL");
    REQUIRE((parent == nullptr) == (attach == nullptr), "parent and attach are given together, or both NULL");
    const int64_t total = n * n_levels;
    hipLaunchKernelGGL(init_kernel, dim3(flat_grid(total)), dim3(kThreads), 0, as_stream(stream), deg, parent, attach, n,
                       total, status);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_DENSITY_OK;
}

int simrank_density_degrees(const void* S, int32_t layout, int64_t stride, int64_t n, const int32_t* ids, const void* edges,
                            int32_t n_levels, int32_t* deg, void* stream) {
    Launch l;                                                            // (the checks of a swept block; its launch is not used)
    int rc = plan_launch(S, layout, stride, n, n, true, &l);
    if (rc) return rc;
    REQUIRE(n < (int64_t(1) << 31) - kCapSlack, "bad node count %lld", (long long)n);
    rc = check_levels(n_levels);
    if (rc) return rc;
    REQUIRE(edges, "edges is NULL");
    REQUIRE(n == 0 || deg, "deg is NULL");
    if (n == 0) return SIMRANK_DENSITY_OK;
    const int64_t tiles = (n + kTile - 1) / kTile, n_pairs = tiles * (tiles + 1) / 2;
    const unsigned grid = (unsigned)std::min<int64_t>(n_pairs, (int64_t(1) << 31) - 1);
    hipStream_t st = as_stream(stream);
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL((degrees_kernel<L>), dim3(grid), dim3(kThreads), 0, st, S, stride, n, ids,
                           static_cast<const typename Elem<L>::Cmp*>(edges), (int)n_levels, deg, n_pairs);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_DENSITY_OK;
}

int simrank_density_union(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                          const int32_t* row_ids, const int32_t* col_ids, const void* edge, const int32_t* deg,
                          int32_t min_neighbors, int32_t* parent, int32_t* attach, int64_t n, int32_t* status, void* stream) {
    Launch l;
    int rc = plan_launch(S, layout, stride, n_rows, n_cols, true, &l);
    if (rc) return rc;
    rc = check_forest(parent, attach, deg, min_neighbors, n, status);
    if (rc) return rc;
    REQUIRE(edge, "edge is NULL");
    if (n_rows == 0 || n_cols == 0 || n == 0) return SIMRANK_DENSITY_OK;
    hipStream_t st = as_stream(stream);
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL((union_kernel<L>), dim3(l.grid), dim3(kThreads), 0, st, S, stride, n_rows, n_cols, row_ids,
                           col_ids, static_cast<const typename Elem<L>::Cmp*>(edge), deg, min_neighbors, parent, attach, n,
                           status, l.vec);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_DENSITY_OK;
}

int simrank_density_labels(const int32_t* parent, const int32_t* attach, const int32_t* deg, int32_t min_neighbors, int64_t n,
                           int32_t* labels, int32_t* status, void* stream) {
    const int rc = check_forest(parent, attach, deg, min_neighbors, n, status);
    if (rc) return rc;
    REQUIRE(n == 0 || labels, "labels is NULL");
    REQUIRE(n == 0 || (labels != parent && labels != attach && labels != deg), "labels must be an array of its own");
    if (n == 0) return SIMRANK_DENSITY_OK;
    hipLaunchKernelGGL(labels_kernel, dim3(flat_grid(n)), dim3(kThreads), 0, as_stream(stream), parent, attach, deg,
                       min_neighbors, n, labels, status);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_DENSITY_OK;
}

}  // extern "C"
