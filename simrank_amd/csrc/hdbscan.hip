// Core similarities and mutual-reachability picks of an iterate that stays on the device (include/simrank_hdbscan.h,
// libsimrank_hdbscan.so): the symmetric per-node k-th-largest select over w(a, b) = max(S[a][b], S[b][a]), and
// linkage.hip's Boruvka pick with every entry clamped by the two nodes' core similarities.
//
// The count sweep has density.hip's shape: the square block is cut into 64 x 64 tiles and one workgroup takes a PAIR of
// tiles (I, J), I <= J.  Both tiles go into LDS as order-preserving keys (NaN: the key 0, which no value has), element
// (r, c) of a tile at word r * 64 + (c ^ r): the wave that stores row r and the wave that reads column a (lane b at row
// b, word a ^ b) both touch 64 different words, 32 different banks per half wave.  Then a wave owns 16 rows of each
// side: for row a of tile (I, J) lane b holds the key of S[a][b] from its own tile and of S[b][a], transposed, from the
// other; the larger is the key of w(a, b).  A key takes part when both positions are nodes, the pair exists, b is not a
// itself and the key agrees with the node's prefix above this pass' digit (the prefixes of the 2 x 64 positions are
// loaded once per pair of tiles, next to their ids, and a row's comes out of its lane).  A row in which no lane takes
// part ends there: most rows, once a few digits are fixed.  Otherwise one ballot and a popcount per digit VALUE THAT IS
// PRESENT count the lanes (the first pending lane names the value, the lanes that hold it leave `pending`: at most 16
// turns, one or two in a matrix of ties and zeros), lane d keeps the count of value d, and those lanes add theirs to
// the node's counters, one 64-byte line, with an integer atomic.  One atomic per element would all land on the counter
// of the one value that such a matrix holds; a ballot for each of the 16 values, present or not, with the prefix loaded
// per row took twice the time of this loop.
//
// The pick is linkage.hip's, word for word but for the clamp (this library's own copy: the companions link nothing of
// each other): the row's core similarity is read once per row, the column's with the column's component.
#include <algorithm>
#include <type_traits>

#include "simrank_hdbscan.h"

#define COMPANION_ERR_INVALID SIMRANK_HDBSCAN_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_HDBSCAN_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_HDBSCAN_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_HDBSCAN_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_HDBSCAN_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_HDBSCAN_, ROWMAJOR_F64);

constexpr int kTile = SIMRANK_HDBSCAN_TILE;
constexpr int kDigit = SIMRANK_HDBSCAN_DIGIT_BITS;
constexpr int kBins = SIMRANK_HDBSCAN_BINS;
constexpr int kThreads = kSweepThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxGrid = kSweepMaxGrid;
constexpr unsigned kCapSlack = 8;
static_assert(kTile == 64, "a row of a tile is one wave");
static_assert(kBins == 1 << kDigit && kBins <= 64, "lane d keeps the count of digit value d");
static_assert(kTile % kWaves == 0, "the waves share a tile's rows evenly");

typedef unsigned long long u64;

// ---- keys ------------------------------------------------------------------------------------------------------------------
// An unsigned integer that orders as the value does; -0.0 takes the key of +0.0; NaN takes 0, which no value has (the
// bits that would give it are a NaN's).  binary16 is keyed on its stored bits: x 2^-14 keeps the order.
__device__ inline uint32_t key16(uint32_t h) {
    if ((h & 0x7fffu) > 0x7c00u) return 0;
    if (h == 0x8000u) h = 0;
    return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}
__device__ inline uint32_t key_of(float v) {
    if (v != v) return 0;
    uint32_t b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline u64 key_of(double v) {
    if (v != v) return 0;
    u64 b = (u64)__double_as_longlong(v);
    if (b == 0x8000000000000000ull) b = 0;
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline float value_of_key16(uint32_t k) {
    const uint32_t h = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
    return float(__builtin_bit_cast(_Float16, (unsigned short)h)) * kHalfScale;
}
__device__ inline float value_of_key32(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ inline double value_of_key64(u64 k) {
    return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k));
}

template <int LAYOUT> struct Keyed {
    using Key = typename std::conditional<LAYOUT == ROWMAJOR_F64, u64, uint32_t>::type;
    static constexpr int BITS = LAYOUT == ROWMAJOR_F64 ? 64 : LAYOUT == PANEL_F16 ? 16 : 32;
    static constexpr int PASSES = BITS / kDigit;
};

inline int passes_of(int32_t layout) { return layout == ROWMAJOR_F64 ? 16 : layout == PANEL_F16 ? 4 : 8; }

// ---- the count sweep -------------------------------------------------------------------------------------------------------
// The key of element (r, c) of the block; 0 (no entry) outside it.
template <int LAYOUT>
__device__ inline typename Keyed<LAYOUT>::Key key_at(const void* __restrict__ S, int64_t stride, int64_t n, int64_t r,
                                                     int64_t c) {
    if (r >= n || c >= n) return 0;
    if constexpr (LAYOUT == PANEL_F16) {
        return key16(static_cast<const unsigned short*>(S)[offset_of<LAYOUT>(stride, r, c)]);
    } else {
        return key_of(load<LAYOUT>(S, stride, r, c));
    }
}

// The tile whose rows start at position r0 and columns at c0, as keys: a wave takes kTile / kWaves rows, one element per
// lane (the 64 columns of a row are 128 to 512 contiguous bytes in every layout), all of their loads in flight together.
template <int LAYOUT>
__device__ inline void tile_keys(const void* __restrict__ S, int64_t stride, int64_t n, int64_t r0, int64_t c0,
                                 typename Keyed<LAYOUT>::Key* tile, int wave, int lane) {
    using Key = typename Keyed<LAYOUT>::Key;
    constexpr int kRows = kTile / kWaves;
    const int row0 = wave * kRows;
    Key k[kRows];
#pragma unroll
    for (int u = 0; u < kRows; ++u) k[u] = key_at<LAYOUT>(S, stride, n, r0 + row0 + u, c0 + lane);
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
        const int r = row0 + u;
        tile[r * kTile + (lane ^ r)] = k[u];
    }
}

// (I, J), I <= J, of pair p = J (J + 1) / 2 + I: density.hip's.  The square root is a first guess that two steps either
// way correct (8 p + 1 < 2^53 is exact in a double; the root is off by less than one).
__device__ inline void tiles_of_pair(int64_t p, int64_t& I, int64_t& J) {
    int64_t j = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    if (j * (j + 1) / 2 > p) --j;
    if (j * (j + 1) / 2 > p) --j;
    if ((j + 1) * (j + 2) / 2 <= p) ++j;
    if ((j + 1) * (j + 2) / 2 <= p) ++j;
    J = j;
    I = p - j * (j + 1) / 2;
}

// lane `a`'s value of x, for a lane number that is the same in every lane: a scalar
__device__ inline uint32_t lane_value(uint32_t x, int a) { return (uint32_t)__builtin_amdgcn_readlane((int)x, a); }
__device__ inline u64 lane_value(u64 x, int a) {
    return ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), a) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, a);
}

// `shift`: the bit this pass' digit starts at; `first`: pass 0, where every key agrees with the (empty) prefix.
template <int LAYOUT>
__global__ __launch_bounds__(kThreads) void count_kernel(const void* __restrict__ S, int64_t stride, int64_t n,
                                                         const int32_t* __restrict__ ids, int shift, int first,
                                                         const u64* __restrict__ prefix, int32_t* __restrict__ hist,
                                                         int64_t n_pairs) {
    using Key = typename Keyed<LAYOUT>::Key;
    __shared__ Key tile[2][kTile * kTile];               // [tile (I, J) | tile (J, I)], word r * 64 + (c ^ r)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (in a scalar register: it names lanes to read below)
    constexpr int kRows = kTile / kWaves;

    for (int64_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        int64_t I, J;
        tiles_of_pair(p, I, J);
        const bool diag = I == J;
        // lane l keeps the ids of positions 64 I + l and 64 J + l (-1: no node) and, after the first pass, their prefixes
        int32_t node[2];
        Key pre[2] = {0, 0};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int64_t pos = (s == 0 ? I : J) * kTile + lane;
            int32_t id = -1;
            if (pos < n) id = ids ? ids[pos] : int32_t(pos);
            node[s] = (id >= 0 && id < n) ? id : -1;                     // (an id outside the nodes is padding)
            if (!first && node[s] >= 0) pre[s] = Key(prefix[node[s]]);
        }
        tile_keys<LAYOUT>(S, stride, n, I * kTile, J * kTile, tile[0], wave, lane);
        if (!diag) tile_keys<LAYOUT>(S, stride, n, J * kTile, I * kTile, tile[1], wave, lane);
        __syncthreads();

        // side 0: the rows of I against the columns of J; side 1: the rows of J against the columns of I
        const int sides = diag ? 1 : 2;
        for (int side = 0; side < sides; ++side) {
            const Key* own = tile[side];
            const Key* other = tile[diag ? 0 : 1 - side];
            const int32_t row_node = side == 0 ? node[0] : node[1], col_node = side == 0 ? node[1] : node[0];
            const Key row_pre = side == 0 ? pre[0] : pre[1];
            const bool col_ok = col_node >= 0;                           // (diag: node[0] == node[1])
#pragma unroll 4
            for (int u = 0; u < kRows; ++u) {
                const int a = wave * kRows + u;                          // (scalar)
                const int32_t rid = __builtin_amdgcn_readlane(row_node, a);
                if (rid < 0) continue;
                const Key k1 = own[a * kTile + (lane ^ a)], k2 = other[lane * kTile + (a ^ lane)];
                const Key k = k1 > k2 ? k1 : k2;
                bool use = col_ok && k != 0 && !(diag && lane == a);
                if (!first) use = use && ((k ^ lane_value(row_pre, a)) >> (shift + kDigit)) == 0;
                u64 pending = __ballot(use);
                if (!pending) continue;                                  // (most rows of a tile, once a few digits are fixed)
                // One ballot and popcount per digit value PRESENT in the row: a matrix of ties and zeros has one or two
                // of the 16, and every turn takes at least one lane out of `pending`.
                const int d = int((k >> shift) & Key(kBins - 1));
                int mine = 0;
                for (int turn = 0; turn < kBins && pending; ++turn) {
                    const int dv = __builtin_amdgcn_readlane(d, __ffsll((unsigned long long)pending) - 1);
                    const u64 same = __ballot(use && d == dv);
                    if (lane == dv) mine = __popcll(same);
                    pending &= ~same;
                }
                if (lane < kBins && mine) atomicAdd(reinterpret_cast<int*>(hist + int64_t(rid) * kBins + lane), mine);
            }
        }
        __syncthreads();                                                 // (the next pair overwrites the tiles)
    }
}

__global__ __launch_bounds__(kThreads) void select_init_kernel(u64* __restrict__ prefix, int32_t* __restrict__ remaining,
                                                               int32_t* __restrict__ hist, int64_t n, int32_t rank) {
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n * kBins; i += step) {
        hist[i] = 0;
        if (i < n) {
            prefix[i] = 0;
            remaining[i] = rank;
        }
    }
}

__global__ __launch_bounds__(kThreads) void step_kernel(int shift, u64* __restrict__ prefix, int32_t* __restrict__ remaining,
                                                        int32_t* __restrict__ hist, int64_t n) {
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += step) {
        int32_t* bins = hist + i * kBins;
        int64_t r = remaining[i];
        int found = -1;
#pragma unroll
        for (int d = kBins - 1; d >= 0; --d) {
            const int64_t c = bins[d];
            bins[d] = 0;
            if (r > 0 && found < 0) {
                if (r <= c) found = d;
                else r -= c;
            }
        }
        if (remaining[i] > 0) {
            if (found >= 0) {
                prefix[i] |= u64(found) << shift;
                remaining[i] = int32_t(r);
            } else {
                remaining[i] = -1;                                       // fewer pairs than the rank
            }
        }
    }
}

template <int LAYOUT>
__global__ __launch_bounds__(kThreads) void finish_kernel(const u64* __restrict__ prefix, const int32_t* __restrict__ remaining,
                                                          int64_t n, double* __restrict__ core64,
                                                          typename Elem<LAYOUT>::Cmp* __restrict__ core_cmp) {
    using Cmp = typename Elem<LAYOUT>::Cmp;
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += step) {
        const int32_t r = remaining[i];
        Cmp v;
        if (r == 0) v = Cmp(__builtin_inff());
        else if (r < 0) v = -Cmp(__builtin_inff());
        else if constexpr (LAYOUT == ROWMAJOR_F64) v = value_of_key64(prefix[i]);
        else if constexpr (LAYOUT == PANEL_F16) v = value_of_key16(uint32_t(prefix[i]));
        else v = value_of_key32(uint32_t(prefix[i]));
        if (core64) core64[i] = double(v);
        if (core_cmp) core_cmp[i] = v;
    }
}

// ---- the clamped pick (linkage.hip's sweep) ----------------------------------------------------------------------------------
__device__ inline u64 ld(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a slot as the compute unit's own cache has it: never above what the slot holds now (a slot only grows within a round,
// and the cache starts every kernel empty)
__device__ inline u64 ld_near(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ inline u64 other_code(int32_t root) { return 0xffffffffull - (u64)(uint32_t)root; }

__device__ inline u64 max_over_lanes(u64 x, int width) {
    for (int off = width >> 1; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), off);
        const u64 y = ((u64)hi << 32) | lo;
        x = y > x ? y : x;
    }
    return x;
}

// PHASE 0: the largest candidate (f32, binary16: key and other root in one word; float64: the key) into best[0].
// PHASE 1 (float64): among the entries whose clamped key is the component's best[0], the largest other_code into best[1].
template <int LAYOUT, int PHASE>
__global__ __launch_bounds__(kThreads) void pick_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                        int64_t n_cols, const int32_t* __restrict__ row_ids,
                                                        const int32_t* __restrict__ col_ids,
                                                        typename Elem<LAYOUT>::Cmp floor, int has_floor,
                                                        const typename Elem<LAYOUT>::Cmp* __restrict__ core,
                                                        const int32_t* __restrict__ comp, u64* best, int64_t n,
                                                        int32_t* status, int vec) {
    using E = Elem<LAYOUT>;
    using Cmp = typename E::Cmp;
    constexpr bool WIDE = LAYOUT == ROWMAJOR_F64;
    static_assert(PHASE == 0 || WIDE, "only a float64 key needs a second sweep");
    WALK_GEOMETRY(LAYOUT, n_cols);
    unsigned bad = 0;
    u64* const slots = best + (PHASE ? n : 0);                           // where this phase's maxima go
    const int64_t n_turns = (n_chunks + U - 1) / U;                      // (>= 1: the host launches nothing for no columns)
    const Cmp none = -Cmp(__builtin_inff());

    for (int64_t r0 = wave * R; r0 < n_rows; r0 += nwaves * R) {
        const int64_t r = r0 + g;
        const bool live = r < n_rows;
        const int32_t rid = live ? (row_ids ? row_ids[r] : int32_t(r)) : -1;
        bool row_ok = live && rid >= 0 && rid < n;                       // (an id outside the nodes is padding)
        int32_t rc = 0;
        Cmp row_core = none;
        if (row_ok) {
            rc = comp[rid];
            row_core = core[rid];
            if (uint32_t(rc) >= uint64_t(n)) {
                bad |= SIMRANK_HDBSCAN_BAD_COMPONENT;
                row_ok = false;
                rc = 0;
            }
        }
        const u64 row_code = other_code(rc);
        u64 row_key = 0;                                                 // PHASE 1: the key the row's component settled on
        if (PHASE == 1 && row_ok) row_key = ld(best + rc);
        u64 mine = 0;                                                    // the row's best candidate so far
        // every turn of U chunks once, starting at a turn of the wave's own (linkage.hip says why)
        const int64_t first = int64_t(((uint64_t(r0 / R) * 2654435761ull) >> 7) % uint64_t(n_turns));
        for (int64_t t = 0; t < n_turns; ++t) {
            const int64_t k0 = (first + t < n_turns ? first + t : first + t - n_turns) * U;
            WALK_LOAD(LAYOUT, x, S, stride, r, live, k0, n_cols, vec)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!row_ok || k0 + u >= n_chunks) continue;
                const int64_t c0 = (k0 + u) * W + int64_t(q) * V;
                // the piece in three steps: the components and core similarities of its columns, then the slots of those
                // that lie in another component, then the maxima
                int32_t cc[V];
                Cmp cv[V];                                               // the clamped values
                unsigned open = 0;                                       // bit i: entry i lies between two components
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    cc[i] = rc;
                    cv[i] = none;
                    const Cmp v = E::value(E::raw(x[u], i));
                    if (c0 + i >= n_cols || v != v) continue;            // (NaN is no entry)
                    const int32_t cid = col_ids ? col_ids[c0 + i] : int32_t(c0 + i);
                    if (cid != rid && cid >= 0 && cid < n) {
                        const Cmp col_core = core[cid];
                        Cmp m = v < row_core ? v : row_core;
                        m = m < col_core ? m : col_core;
                        if (m == none || (has_floor && !(m >= floor))) continue;       // (-inf is no candidate)
                        cv[i] = m;
                        cc[i] = comp[cid];
                        open |= 1u << i;
                    }
                }
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if (uint32_t(cc[i]) >= uint64_t(n)) {
                        bad |= SIMRANK_HDBSCAN_BAD_COMPONENT;
                        cc[i] = rc;
                    }
                    if (cc[i] == rc) open &= ~(1u << i);                 // the usual end of an entry
                }
                if (!open) continue;
                // the column's slot, a near read: too small a value only costs an atomic.  PHASE 1 reads the settled key
                // here, which must be exact: no kernel of that phase writes it, and this one started with the cache
                // invalidated (the note at the head of linkage.hip)
                u64 cur[V];
#pragma unroll
                for (int i = 0; i < V; ++i) cur[i] = ((open >> i) & 1) ? ld_near(best + cc[i]) : ~0ull;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if (!((open >> i) & 1)) continue;
                    const auto key = key_of(cv[i]);
                    if constexpr (!WIDE) {
                        const u64 to_row = ((u64)key << 32) | other_code(cc[i]), to_col = ((u64)key << 32) | row_code;
                        mine = to_row > mine ? to_row : mine;
                        if (to_col > cur[i]) atomicMax(best + cc[i], to_col);
                    } else if constexpr (PHASE == 0) {
                        mine = key > mine ? key : mine;
                        if (key > cur[i]) atomicMax(best + cc[i], key);
                    } else {
                        if (key == row_key) mine = other_code(cc[i]) > mine ? other_code(cc[i]) : mine;
                        if (key == cur[i] && row_code > ld(slots + cc[i])) atomicMax(slots + cc[i], row_code);
                    }
                }
            }
        }
        mine = max_over_lanes(mine, L);                                  // (every lane of the wave takes part)
        if (q == 0 && mine != 0 && mine > ld(slots + rc)) atomicMax(slots + rc, mine);
    }
    if (bad) atomicOr(reinterpret_cast<int*>(status), (int)bad);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
int check_nodes(int64_t n) {
    REQUIRE(n >= 0 && n < (int64_t(1) << 31) - kCapSlack, "bad node count %lld", (long long)n);
    return SIMRANK_HDBSCAN_OK;
}

int check_pass(int32_t layout, int32_t pass) {
    REQUIRE(known_layout(layout), "unknown layout %d", (int)layout);
    REQUIRE(pass >= 0 && pass < passes_of(layout), "pass %d of layout %d: its select has passes 0 .. %d", (int)pass, (int)layout,
            passes_of(layout) - 1);
    return SIMRANK_HDBSCAN_OK;
}

int check_select_state(const void* prefix, const void* remaining, int64_t n) {
    const int rc = check_nodes(n);
    if (rc) return rc;
    REQUIRE(n == 0 || prefix, "prefix is NULL");
    REQUIRE(n == 0 || remaining, "remaining is NULL");
    return SIMRANK_HDBSCAN_OK;
}

int shift_of(int32_t layout, int32_t pass) { return (passes_of(layout) - 1 - pass) * kDigit; }

int flat_grid(int64_t total) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((total + kThreads - 1) / kThreads, kMaxGrid));
}

}  // namespace

extern "C" {

int simrank_hdbscan_version(void) { return SIMRANK_HDBSCAN_VERSION; }

const char* simrank_hdbscan_last_error(void) { return g_error.c_str(); }

int simrank_hdbscan_select_passes(int32_t layout) {
    REQUIRE(known_layout(layout), "unknown layout %d", (int)layout);
    return passes_of(layout);
}

int simrank_hdbscan_select_init(uint64_t* prefix, int32_t* remaining, int32_t* hist, int64_t n, int64_t rank, void* stream) {
    const int rc = check_select_state(prefix, remaining, n);
    if (rc) return rc;
    REQUIRE(n == 0 || hist, "hist is NULL");
    REQUIRE(rank >= 0, "rank must be >= 0 (got %lld)", (long long)rank);
    if (n == 0) return SIMRANK_HDBSCAN_OK;
    const int32_t r = (int32_t)std::min<int64_t>(rank, (int64_t(1) << 31) - 1);
    hipLaunchKernelGGL(select_init_kernel, dim3(flat_grid(n * kBins)), dim3(kThreads), 0, as_stream(stream),
                       reinterpret_cast<u64*>(prefix), remaining, hist, n, r);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_HDBSCAN_OK;
}

int simrank_hdbscan_select_count(const void* S, int32_t layout, int64_t stride, int64_t n, const int32_t* ids, int32_t pass,
                                 const uint64_t* prefix, int32_t* hist, void* stream) {
    Launch l;                                                            // (the checks of a swept block; its launch is not used)
    int rc = plan_launch(S, layout, stride, n, n, true, &l);
    if (rc) return rc;
    rc = check_nodes(n);
    if (rc) return rc;
    rc = check_pass(layout, pass);
    if (rc) return rc;
    REQUIRE(n == 0 || prefix, "prefix is NULL");
    REQUIRE(n == 0 || hist, "hist is NULL");
    if (n == 0) return SIMRANK_HDBSCAN_OK;
    const int64_t tiles = (n + kTile - 1) / kTile, n_pairs = tiles * (tiles + 1) / 2;
    const unsigned grid = (unsigned)std::min<int64_t>(n_pairs, (int64_t(1) << 31) - 1);
    const int shift = shift_of(layout, pass);
    hipStream_t st = as_stream(stream);
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL((count_kernel<L>), dim3(grid), dim3(kThreads), 0, st, S, stride, n, ids, shift, pass == 0 ? 1 : 0,
                           reinterpret_cast<const u64*>(prefix), hist, n_pairs);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_HDBSCAN_OK;
}

int simrank_hdbscan_select_step(int32_t layout, int32_t pass, uint64_t* prefix, int32_t* remaining, int32_t* hist, int64_t n,
                                void* stream) {
    int rc = check_pass(layout, pass);
    if (rc) return rc;
    rc = check_select_state(prefix, remaining, n);
    if (rc) return rc;
    REQUIRE(n == 0 || hist, "hist is NULL");
    if (n == 0) return SIMRANK_HDBSCAN_OK;
    hipLaunchKernelGGL(step_kernel, dim3(flat_grid(n)), dim3(kThreads), 0, as_stream(stream), shift_of(layout, pass),
                       reinterpret_cast<u64*>(prefix), remaining, hist, n);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_HDBSCAN_OK;
}

int simrank_hdbscan_select_finish(int32_t layout, const uint64_t* prefix, const int32_t* remaining, int64_t n, double* core64,
                                  void* core_cmp, void* stream) {
    REQUIRE(known_layout(layout), "unknown layout %d", (int)layout);
    const int rc = check_select_state(prefix, remaining, n);
    if (rc) return rc;
    REQUIRE(n == 0 || core64 || core_cmp, "core64 and core_cmp are both NULL");
    if (n == 0) return SIMRANK_HDBSCAN_OK;
    hipStream_t st = as_stream(stream);
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL((finish_kernel<L>), dim3(flat_grid(n)), dim3(kThreads), 0, st, reinterpret_cast<const u64*>(prefix),
                           remaining, n, core64, static_cast<typename Elem<L>::Cmp*>(core_cmp));
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_HDBSCAN_OK;
}

int simrank_hdbscan_select(const void* S, int32_t layout, int64_t stride, int64_t n, const int32_t* ids, int64_t rank,
                           uint64_t* prefix, int32_t* remaining, int32_t* hist, double* core64, void* core_cmp, void* stream) {
    // every argument check before the first launch
    Launch l;
    int rc = plan_launch(S, layout, stride, n, n, true, &l);
    if (rc) return rc;
    rc = check_select_state(prefix, remaining, n);
    if (rc) return rc;
    REQUIRE(n == 0 || hist, "hist is NULL");
    REQUIRE(rank >= 0, "rank must be >= 0 (got %lld)", (long long)rank);
    REQUIRE(n == 0 || core64 || core_cmp, "core64 and core_cmp are both NULL");
    rc = simrank_hdbscan_select_init(prefix, remaining, hist, n, rank, stream);
    if (rc) return rc;
    for (int32_t pass = 0; pass < passes_of(layout) && rank > 0; ++pass) {      // (rank 0: +inf for everybody, no sweep)
        rc = simrank_hdbscan_select_count(S, layout, stride, n, ids, pass, prefix, hist, stream);
        if (rc) return rc;
        rc = simrank_hdbscan_select_step(layout, pass, prefix, remaining, hist, n, stream);
        if (rc) return rc;
    }
    return simrank_hdbscan_select_finish(layout, prefix, remaining, n, core64, core_cmp, stream);
}

int simrank_hdbscan_pick(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols, const int32_t* row_ids,
                         const int32_t* col_ids, const void* floor, int32_t phase, const void* core, const int32_t* comp,
                         uint64_t* best, int64_t n, int32_t* status, void* stream) {
    Launch l;
    int rc = plan_launch(S, layout, stride, n_rows, n_cols, true, &l);
    if (rc) return rc;
    rc = check_nodes(n);
    if (rc) return rc;
    REQUIRE(status, "status is NULL");
    REQUIRE(n == 0 || comp, "comp is NULL");
    REQUIRE(n == 0 || best, "best is NULL");
    REQUIRE(n == 0 || core, "core is NULL");
    REQUIRE(phase == 0 || (phase == 1 && layout == ROWMAJOR_F64), "phase %d of layout %d: a float64 block has phases 0 and 1, "
            "the others phase 0", (int)phase, (int)layout);
    if (n_rows == 0 || n_cols == 0 || n == 0) return SIMRANK_HDBSCAN_OK;
    hipStream_t st = as_stream(stream);
    u64* slots = reinterpret_cast<u64*>(best);
    with_layout(layout, [&](auto L) {
        using Cmp = typename Elem<L>::Cmp;
        const Cmp f = floor ? *static_cast<const Cmp*>(floor) : Cmp(0);
        const Cmp* cs = static_cast<const Cmp*>(core);
        if constexpr (L == ROWMAJOR_F64) {
            if (phase == 1) {
                hipLaunchKernelGGL((pick_kernel<L, 1>), dim3(l.grid), dim3(kThreads), 0, st, S, stride, n_rows, n_cols, row_ids,
                                   col_ids, f, floor ? 1 : 0, cs, comp, slots, n, status, l.vec);
                return;
            }
        }
        hipLaunchKernelGGL((pick_kernel<L, 0>), dim3(l.grid), dim3(kThreads), 0, st, S, stride, n_rows, n_cols, row_ids,
                           col_ids, f, floor ? 1 : 0, cs, comp, slots, n, status, l.vec);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_HDBSCAN_OK;
}

}  // extern "C"
