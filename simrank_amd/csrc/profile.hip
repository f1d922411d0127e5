// The distribution of an iterate that stays on the device (include/simrank_profile.h, libsimrank_profile.so): how many
// off-diagonal entries lie between sorted thresholds, and one pass of a global radix select on an order-preserving key.
//
// Both are one sweep of a block in the layout the plan stores it, on the walk that select.hip and cluster.hip share
// (companion.h: eight rows per wave on panels, one on a row-major block, 16-byte loads).  Every entry becomes a bin
// number; a workgroup counts bins in 32-bit words of local memory and adds them to the caller's 64-bit counters once, at
// its end.  A fitted S is mostly exact zeros plus a few repeated values: before the local-memory atomics, up to two
// rounds of (first pending lane's bin, ballot of the lanes that share it, one add of the popcount by that lane) take the
// dominant bins out of the way; what is left adds 1 per lane.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

#include "simrank_profile.h"

#define COMPANION_ERR_INVALID SIMRANK_PROFILE_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_PROFILE_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_PROFILE_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_PROFILE_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_PROFILE_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_PROFILE_, ROWMAJOR_F64);

constexpr int kMaxEdges = SIMRANK_PROFILE_MAX_EDGES;
constexpr int kMaxBins = 1 << SIMRANK_PROFILE_MAX_DIGIT_BITS;
constexpr int kThreads = kSweepThreads;

// ---- keys (host and device) ---------------------------------------------------------------------------------------------
// sign set: every bit flipped (larger magnitude = smaller key); sign clear: the sign bit set.  -0.0 is keyed as +0.0.
__host__ __device__ inline uint32_t key32(uint32_t b) {
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline uint32_t unkey32(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }
__host__ __device__ inline uint64_t key64(uint64_t b) {
    if (b == 0x8000000000000000ull) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline uint64_t unkey64(uint64_t k) { return (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k; }
__host__ __device__ inline uint32_t key16(uint32_t b) {
    if (b == 0x8000u) b = 0;
    return ((b & 0x8000u) ? ~b : (b | 0x8000u)) & 0xffffu;
}
__host__ __device__ inline uint32_t unkey16(uint32_t k) { return ((k & 0x8000u) ? (k & 0x7fffu) : ~k) & 0xffffu; }

// ---- a layout's element (companion.h) as a key -----------------------------------------------------------------------------
template <int LAYOUT>
struct Keyed : Elem<LAYOUT> {
    using Raw = typename Elem<LAYOUT>::Raw;
    static constexpr int KEY_BITS = LAYOUT == PANEL_F16 ? 16 : LAYOUT == ROWMAJOR_F64 ? 64 : 32;

    __device__ static bool is_nan(Raw b) {
        if constexpr (LAYOUT == ROWMAJOR_F64) return (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
        else if constexpr (LAYOUT == PANEL_F16) return (b & 0x7fffu) > 0x7c00u;
        else return (b & 0x7fffffffu) > 0x7f800000u;
    }
    __device__ static uint64_t key(Raw b) {
        if constexpr (LAYOUT == ROWMAJOR_F64) return key64(b);
        else if constexpr (LAYOUT == PANEL_F16) return key16(b);
        else return key32(b);
    }
};

// One entry's bin into the workgroup's bins.  Called by every lane of the wave together (`in` = this lane has an entry).
template <bool AGG>
__device__ inline void bump(uint32_t* bins, bool in, uint32_t j, int lane) {
    if (AGG) {
        uint64_t pending = __ballot(in);
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            if (!pending) break;                                         // (wave-uniform)
            const int lead = __ffsll((unsigned long long)pending) - 1;
            const uint32_t j0 = (uint32_t)__builtin_amdgcn_readlane((int)j, lead);
            const uint64_t same = __ballot(in && j == j0);
            if (lane == lead) atomicAdd(&bins[j0], (uint32_t)__popcll(same));
            pending &= ~same;
            in = in && j != j0;
        }
    }
    if (in) atomicAdd(&bins[j], 1u);
}

// The sweep both kernels share: op(in, raw bits) for every element slot, called wave-uniformly; `in` only for entries of
// the block proper (live row, column below n_cols) whose ids differ.
template <int LAYOUT, class Op>
__device__ inline void sweep(const void* __restrict__ S, int64_t stride, int64_t n_rows, int64_t n_cols,
                             const int32_t* __restrict__ row_ids, const int32_t* __restrict__ col_ids, int vec, Op& op) {
    WALK_GEOMETRY(LAYOUT, n_cols);
    for (int64_t r0 = wave * R; r0 < n_rows; r0 += nwaves * R) {
        const int64_t r = r0 + g;
        const bool live = r < n_rows;
        const int32_t rid = live ? (row_ids ? row_ids[r] : int32_t(r)) : 0;
        for (int64_t k0 = 0; k0 < n_chunks; k0 += U) {
            WALK_LOAD(LAYOUT, x, S, stride, r, live, k0, n_cols, vec)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (k0 + u >= n_chunks) break;                           // (wave-uniform)
                const int64_t c0 = (k0 + u) * W + int64_t(q) * V;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    bool in = live && c0 + i < n_cols;
                    if (in) in = (col_ids ? col_ids[c0 + i] : int32_t(c0 + i)) != rid;
                    op(in, Elem<LAYOUT>::raw(x[u], i));
                }
            }
        }
    }
}

__device__ inline void flush(const uint32_t* bins, int n_bins, unsigned long long* out) {
    __syncthreads();
    for (int b = threadIdx.x; b < n_bins; b += blockDim.x)
        if (bins[b]) atomicAdd(&out[b], (unsigned long long)bins[b]);
}

// ---- count ---------------------------------------------------------------------------------------------------------------
// bin of v = the number of edges <= v: a branch-free upper bound over the sorted edges in local memory, skipped while a
// lane meets the same bits again (most of a fitted S is one value).
template <int LAYOUT, bool AGG>
__global__ __launch_bounds__(kThreads) void count_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                         int64_t n_cols, const int32_t* __restrict__ row_ids,
                                                         const int32_t* __restrict__ col_ids,
                                                         const typename Elem<LAYOUT>::Cmp* __restrict__ edges_dev,
                                                         int n_edges, int top, unsigned long long* __restrict__ counts,
                                                         int vec) {
    using E = Keyed<LAYOUT>;
    using Cmp = typename E::Cmp;
    using Raw = typename E::Raw;
    __shared__ Cmp edges[kMaxEdges];
    __shared__ uint32_t bins[kMaxEdges + 1];
    for (int i = threadIdx.x; i < n_edges; i += blockDim.x) edges[i] = edges_dev[i];
    for (int i = threadIdx.x; i <= n_edges; i += blockDim.x) bins[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    auto search = [&](Cmp v) {
        uint32_t j = 0;
        for (uint32_t s = (uint32_t)top; s; s >>= 1) {
            const uint32_t k = j + s;
            if (k <= (uint32_t)n_edges && edges[k - 1] <= v) j = k;
        }
        return j;
    };
    Raw last = 0;                                // the bits of +0.0 in every stored type
    uint32_t last_j = search(Cmp(0));
    auto op = [&](bool in, Raw b) {
        uint32_t j = 0;
        if (in) {
            if (b != last) {
                last = b;
                last_j = search(E::value(b));
            }
            j = last_j;
        }
        bump<AGG>(bins, in, j, lane);
    };
    sweep<LAYOUT>(S, stride, n_rows, n_cols, row_ids, col_ids, vec, op);
    flush(bins, n_edges + 1, counts);
}

// ---- digits --------------------------------------------------------------------------------------------------------------
template <int LAYOUT, bool AGG>
__global__ __launch_bounds__(kThreads) void digits_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                          int64_t n_cols, const int32_t* __restrict__ row_ids,
                                                          const int32_t* __restrict__ col_ids, uint64_t prefix,
                                                          int prefix_bits, int digit_bits,
                                                          unsigned long long* __restrict__ hist,
                                                          unsigned long long* __restrict__ min_above, int vec) {
    using E = Keyed<LAYOUT>;
    using Raw = typename E::Raw;
    __shared__ uint32_t bins[kMaxBins];
    const int n_bins = 1 << digit_bits;
    for (int i = threadIdx.x; i < n_bins; i += blockDim.x) bins[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int shift = E::KEY_BITS - prefix_bits - digit_bits;
    const int pshift = E::KEY_BITS - prefix_bits;                        // (prefix_bits == 0: every key is under the prefix)
    const uint32_t mask = uint32_t(n_bins - 1);
    uint64_t lane_min = ~0ull;
    auto op = [&](bool in, Raw b) {
        uint32_t d = 0;
        bool here = false;
        if (in && !E::is_nan(b)) {
            const uint64_t key = E::key(b);
            const uint64_t head = prefix_bits ? key >> pshift : 0;
            here = head == prefix;
            d = uint32_t(key >> shift) & mask;
            if (head > prefix && key < lane_min) lane_min = key;
        }
        bump<AGG>(bins, here, d, lane);
    };
    sweep<LAYOUT>(S, stride, n_rows, n_cols, row_ids, col_ids, vec, op);
    if (min_above) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t other = __shfl_xor((unsigned long long)lane_min, off);
            if (other < lane_min) lane_min = other;
        }
        if (lane == 0 && lane_min != ~0ull) atomicMin(min_above, (unsigned long long)lane_min);
    }
    flush(bins, n_bins, hist);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// a swept block (companion.h) of which no workgroup sees 2^32 entries: its bins are 32-bit
int plan_profile(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols, Launch* l) {
    const int rc = plan_launch(S, layout, stride, n_rows, n_cols, true, l);
    if (rc) return rc;
    REQUIRE((double)l->rows * (double)n_cols < 4294967296.0,
            "a block of %lld x %lld gives one workgroup 2^32 entries or more: sweep it in pieces of fewer rows",
            (long long)n_rows, (long long)n_cols);
    return SIMRANK_PROFILE_OK;
}

// SIMRANK_PROFILE_PLAIN=1 (read at every call; documented in the header): the kernels without the ballot rounds, for
// measuring what they buy.  TODO: once tools/bench_profile.py has decided, remove the slower form, the AGG template
// parameter and this switch.
bool plain_bins() {
    const char* s = std::getenv("SIMRANK_PROFILE_PLAIN");
    return s && *s && std::strcmp(s, "0") != 0;
}

float half_value(uint32_t h) {                   // (float)h * 2^-14 of binary16 bits, without a host binary16 type
    const int e = (h >> 10) & 31, m = h & 1023;
    float mag;
    if (e == 0) mag = std::ldexp((float)m, -24);
    else if (e == 31) mag = m ? NAN : INFINITY;
    else mag = std::ldexp((float)(m + 1024), e - 25);
    return ((h & 0x8000u) ? -mag : mag) * kHalfScale;
}

}  // namespace

extern "C" {

int simrank_profile_version(void) { return SIMRANK_PROFILE_VERSION; }

const char* simrank_profile_last_error(void) { return g_error.c_str(); }

int simrank_profile_key_bits(int32_t layout) {
    REQUIRE(known_layout(layout), "unknown layout %d", (int)layout);
    return layout == PANEL_F16 ? 16 : layout == ROWMAJOR_F64 ? 64 : 32;
}

int simrank_profile_count(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                          const int32_t* row_ids, const int32_t* col_ids, const void* edges, int32_t n_edges,
                          uint64_t* counts, void* stream) {
    Launch l;
    const int rc = plan_profile(S, layout, stride, n_rows, n_cols, &l);
    if (rc) return rc;
    REQUIRE(n_edges >= 1 && n_edges <= kMaxEdges, "n_edges must be 1 .. %d (got %d)", kMaxEdges, (int)n_edges);
    REQUIRE(edges && counts, "edges or counts is NULL");
    if (n_rows == 0 || n_cols == 0) return SIMRANK_PROFILE_OK;
    int top = 1;
    while (top * 2 <= n_edges) top *= 2;
    hipStream_t st = as_stream(stream);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
    const bool agg = !plain_bins();
    with_layout(layout, [&](auto L) {
        const auto* e = static_cast<const typename Elem<L>::Cmp*>(edges);
        if (agg)
            hipLaunchKernelGGL((count_kernel<L, true>), dim3(l.grid), dim3(kThreads), 0, st, S, stride, n_rows, n_cols,
                               row_ids, col_ids, e, (int)n_edges, top, out, l.vec);
        else
            hipLaunchKernelGGL((count_kernel<L, false>), dim3(l.grid), dim3(kThreads), 0, st, S, stride, n_rows, n_cols,
                               row_ids, col_ids, e, (int)n_edges, top, out, l.vec);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_PROFILE_OK;
}

int simrank_profile_digits(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                           const int32_t* row_ids, const int32_t* col_ids, uint64_t prefix, int32_t prefix_bits,
                           int32_t digit_bits, uint64_t* hist, uint64_t* min_above, void* stream) {
    Launch l;
    const int rc = plan_profile(S, layout, stride, n_rows, n_cols, &l);
    if (rc) return rc;
    const int key_bits = layout == PANEL_F16 ? 16 : layout == ROWMAJOR_F64 ? 64 : 32;
    REQUIRE(digit_bits >= 1 && digit_bits <= SIMRANK_PROFILE_MAX_DIGIT_BITS, "digit_bits must be 1 .. %d (got %d)",
            SIMRANK_PROFILE_MAX_DIGIT_BITS, (int)digit_bits);
    REQUIRE(prefix_bits >= 0 && prefix_bits + digit_bits <= key_bits, "prefix_bits %d + digit_bits %d pass the %d bits of the key",
            (int)prefix_bits, (int)digit_bits, key_bits);
    REQUIRE(prefix_bits == 64 || (prefix >> prefix_bits) == 0, "the prefix has more than prefix_bits = %d bits", (int)prefix_bits);
    REQUIRE(hist, "hist is NULL");
    if (n_rows == 0 || n_cols == 0) return SIMRANK_PROFILE_OK;
    hipStream_t st = as_stream(stream);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(hist);
    unsigned long long* mn = reinterpret_cast<unsigned long long*>(min_above);
    const bool agg = !plain_bins();
    with_layout(layout, [&](auto L) {
        if (agg)
            hipLaunchKernelGGL((digits_kernel<L, true>), dim3(l.grid), dim3(kThreads), 0, st, S, stride, n_rows, n_cols,
                               row_ids, col_ids, prefix, (int)prefix_bits, (int)digit_bits, out, mn, l.vec);
        else
            hipLaunchKernelGGL((digits_kernel<L, false>), dim3(l.grid), dim3(kThreads), 0, st, S, stride, n_rows, n_cols,
                               row_ids, col_ids, prefix, (int)prefix_bits, (int)digit_bits, out, mn, l.vec);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_PROFILE_OK;
}

uint32_t simrank_profile_key_f32(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return key32(b);
}

float simrank_profile_unkey_f32(uint32_t key) {
    const uint32_t b = unkey32(key);
    float v;
    std::memcpy(&v, &b, 4);
    return v;
}

uint64_t simrank_profile_key_f64(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return key64(b);
}

double simrank_profile_unkey_f64(uint64_t key) {
    const uint64_t b = unkey64(key);
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

uint32_t simrank_profile_key_f16(uint16_t half_bits) { return key16(half_bits); }

double simrank_profile_unkey_f16(uint32_t key) { return (double)half_value(unkey16(key & 0xffffu)); }

int simrank_profile_pick(const uint64_t* hist, int32_t bins, uint64_t above, uint64_t max_pairs, int32_t* bin,
                         uint64_t* above_out) {
    REQUIRE(hist && bin && above_out && bins >= 1, "bad pick arguments");
    uint64_t cum = above;
    int32_t lowest = -1;
    for (int32_t b = bins - 1; b >= 0; --b) {
        if (!hist[b]) continue;
        if (cum > max_pairs || hist[b] > max_pairs - cum) {              // (no overflow: cum <= max_pairs on the right)
            *bin = b;
            *above_out = cum;
            return 1;
        }
        cum += hist[b];
        lowest = b;
    }
    *bin = lowest;
    *above_out = lowest < 0 ? above : cum - hist[lowest];
    return 0;
}

}  // extern "C"
