// A kept model as per-node neighbour lists (include/simrank_neighbors.h, libsimrank_neighbors.so): the selection that
// builds the lists from a block of an iterate read IN PLACE, and the queries that read them.
//
//     select  one workgroup per query row.  The k-th best element in the total order (value descending, id ascending) is
//             found by a radix select: every element has the composite key (order-preserving integer of the widened
//             value, INT32_MAX - id), larger = better; a pass histograms one 11-bit digit of the elements that still share
//             the k-th's prefix (2048 counters in LDS), finds the bin that holds the k-th by a suffix scan, and stops as
//             soon as that bin is needed whole.  f32 and binary16 values have a 32-bit value key (3 passes), float64 a
//             64-bit one (6); the 31 id bits (3 passes) are only walked when the k-th value ties.  One more sweep collects
//             everything at or above the threshold into LDS, where a bitonic sort puts the at most k survivors into the
//             total order.  So a row is swept at most 7 (10) times whatever k is; after the first sweep it comes from L2.
//             -0.0 is canonicalised in the KEY only and NaN has the key 0, below -inf, and is never a candidate.
//             A row that is mostly one value (the zeros of a sparse model) would serialise its LDS atomics on one counter:
//             the lanes that share the first active lane's digit are counted with one ballot.
//     rows    one workgroup per (query row, 2048 columns): zeros in LDS, the list's entries and the diagonal that fall
//             into the chunk, then coalesced 8-byte stores.
//     pairs   one thread per pair walks a's list.
//     score   one workgroup per (basket, 2048 columns) keeps the chunk's float64 sums in LDS and applies the members
//             strictly in list order, one barrier per member: a member's ids are distinct, so its adds touch distinct
//             sums; a repeated member is a later step.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>

#include "simrank_neighbors.h"

#define COMPANION_ERR_INVALID SIMRANK_NEIGHBORS_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_NEIGHBORS_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_NEIGHBORS_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_NEIGHBORS_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_NEIGHBORS_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_NEIGHBORS_, ROWMAJOR_F64);

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kDigitBits = 11;
constexpr int kBins = 1 << kDigitBits;                     // counters of one pass
constexpr int kBinsPerThread = kBins / kThreads;
constexpr int kSweepUnroll = 4;                            // elements of one lane in flight in a sweep
constexpr int kChunk = SIMRANK_NEIGHBORS_CHUNK;
constexpr int kChunkPerThread = kChunk / kThreads;
constexpr int kIdBits = 31;

// ---- keys ----------------------------------------------------------------------------------------------------------
// Order-preserving integer of a value: larger key = larger value; -0.0 and +0.0 share a key; NaN -> 0, below -inf.
__device__ __forceinline__ uint64_t key_of(double v) {
    if (v != v) return 0;
    if (v == 0.0) v = 0.0;                                  // (-0.0 -> +0.0 in the key only)
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | (uint64_t(1) << 63));
}

__device__ __forceinline__ uint64_t key_of(float v) {      // the same order in the upper 32 bits; the lower ones are 0
    if (v != v) return 0;
    if (v == 0.0f) v = 0.0f;
    const uint32_t b = __float_as_uint(v);
    return uint64_t((b >> 31) ? ~b : (b | 0x80000000u)) << 32;
}

// The width of a layout's value key and the type load<L> (companion.h) hands an element back in.  The f32 and binary16
// layouts widen exactly and monotonically, so the key of the float orders as the key of the double would.
template <int L>
struct Value {
    static constexpr int kKeyBits = (L == ROWMAJOR_F64) ? 64 : 32;
    using Held = typename std::conditional<L == ROWMAJOR_F64, double, float>::type;
};

// The passes of the radix select: (which key, shift, bits), from the most significant digit down.
struct Pass {
    int on_id, shift, bits;
};

template <int KEY_BITS>
__device__ __forceinline__ Pass pass_of(int p) {
    constexpr int value_passes = KEY_BITS == 32 ? 3 : 6;
    if (p < value_passes) {
        const int lowest = KEY_BITS == 32 ? 32 : 0;        // (a 32-bit key lies in the upper half)
        const int shift = 64 - kDigitBits * (p + 1);
        return shift >= lowest ? Pass{0, shift, kDigitBits} : Pass{0, lowest, shift + kDigitBits - lowest};
    }
    const int shift = kIdBits - kDigitBits * (p - value_passes + 1);
    return shift >= 0 ? Pass{1, shift, kDigitBits} : Pass{1, 0, shift + kDigitBits};
}

template <int KEY_BITS>
constexpr int n_passes() {
    return (KEY_BITS == 32 ? 3 : 6) + 3;
}

// What the workgroup agrees on between the passes (LDS).
struct SelectState {
    uint64_t tv;           // threshold: value key (the digits found so far, zeros below)
    uint32_t ti;           // threshold: id key among the elements whose value key is tv
    int need;              // how many of the current bin's elements are wanted
    int done;              // the threshold is final
    int count;             // survivors collected
    int wave_sum[kWaves];
};
static_assert(sizeof(SelectState) % 8 == 0, "the survivors' doubles follow the state and the histogram");

// Add 1 to hist[d] for every active lane; the lanes that share the first active lane's digit go in one add.
__device__ __forceinline__ void count_digit(uint32_t* hist, bool active, uint32_t d, int lane) {
    const uint64_t any = __ballot(active);
    if (!any) return;
    const int leader = __ffsll((unsigned long long)any) - 1;
    const uint32_t d0 = __shfl(d, leader);
    const uint64_t same = __ballot(active && d == d0);
    if (lane == leader) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
    if (active && d != d0) atomicAdd(&hist[d], 1u);
}

// After a pass: the bin (from the top) in which the cumulative count reaches st.need, or "take everything" when the
// candidates are fewer.  Thread t owns the bins kBins - 1 - t * kBinsPerThread downwards.
__device__ __forceinline__ void find_bin(const uint32_t* hist, SelectState& st, Pass ps, bool first_pass) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int top = kBins - 1 - tid * kBinsPerThread;
    int mine = 0;
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) mine += (int)hist[top - i];
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) st.wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) before += st.wave_sum[w];
        total += st.wave_sum[w];
    }
    incl += before;
    const int need = st.need;                               // (read by all before anyone writes: the barrier below)
    __syncthreads();
    if (total <= need) {
        // fewer candidates than wanted (only the first pass can see this): every candidate survives
        if (tid == 0 && first_pass) { st.tv = 0; st.ti = 0; st.done = 1; }
    } else if (incl >= need && incl - mine < need) {
        int above = incl - mine;
        for (int i = 0; i < kBinsPerThread; ++i) {
            const int c = (int)hist[top - i];
            if (above + c >= need) {
                const uint64_t digit = uint64_t(top - i);
                if (ps.on_id) st.ti |= uint32_t(digit << ps.shift);
                else st.tv |= digit << ps.shift;
                st.need = need - above;
                if (need - above == c) st.done = 1;         // the bin is wanted whole: no digit below matters
                break;
            }
            above += c;
        }
    }
    __syncthreads();
}

template <int L>
__global__ __launch_bounds__(kThreads) void neighbors_select_kernel(const void* __restrict__ S, int64_t stride,
                                                                    int64_t n_rows, int64_t n_cols,
                                                                    const int32_t* __restrict__ row_pos,
                                                                    const int32_t* __restrict__ row_ids, int64_t n_q,
                                                                    const int32_t* __restrict__ col_ids, int k, int cap,
                                                                    int32_t* __restrict__ idx_out,
                                                                    double* __restrict__ val_out) {
    using V = Value<L>;
    extern __shared__ __align__(16) unsigned char lds[];
    // the state, the histogram, cap doubles, cap ints (cap: a power of two >= k)
    SelectState& st = *reinterpret_cast<SelectState*>(lds);
    uint32_t* hist = reinterpret_cast<uint32_t*>(lds + sizeof(SelectState));
    double* sv = reinterpret_cast<double*>(hist + kBins);
    int32_t* si = reinterpret_cast<int32_t*>(sv + cap);
    const int tid = threadIdx.x, lane = tid & 63;

    for (int64_t q = blockIdx.x; q < n_q; q += gridDim.x) {
        const int64_t r = row_pos[q];
        const int self = row_ids[q];
        const int64_t cols = (r >= 0 && r < n_rows) ? n_cols : 0;       // (a row outside the block: no candidates)
        if (tid == 0) { st.tv = 0; st.ti = 0; st.need = k; st.done = 0; st.count = 0; }
        __syncthreads();

        // ---- the threshold: the composite key of the k-th best ----
        for (int p = 0; p < n_passes<V::kKeyBits>(); ++p) {
            if (st.done) break;                              // (uniform: written before the last barrier of find_bin)
            const Pass ps = pass_of<V::kKeyBits>(p);
            for (int i = tid; i < kBins; i += kThreads) hist[i] = 0;
            const uint64_t tv = st.tv;
            const uint32_t ti = st.ti;
            __syncthreads();
            // the digits above this one, as a mask of the key the pass works on
            const int upto = ps.shift + ps.bits;
            const uint64_t vmask = ps.on_id ? ~uint64_t(0) : (upto >= 64 ? 0 : ~uint64_t(0) << upto);
            const uint32_t imask = ps.on_id ? (upto >= 32 ? 0u : ~0u << upto) : 0u;
            for (int64_t c0 = 0; c0 < cols; c0 += kThreads * kSweepUnroll) {
                typename V::Held v[kSweepUnroll];
                int id[kSweepUnroll];
#pragma unroll
                for (int u = 0; u < kSweepUnroll; ++u) {
                    const int64_t c = c0 + u * kThreads + tid;
                    v[u] = typename V::Held(0);
                    id[u] = self;
                    if (c < cols) {
                        v[u] = load<L>(S, stride, r, c);
                        id[u] = col_ids ? col_ids[c] : int(c);
                    }
                }
#pragma unroll
                for (int u = 0; u < kSweepUnroll; ++u) {
                    const uint64_t kv = key_of(v[u]);
                    const uint32_t ki = uint32_t(0x7fffffff - id[u]);
                    const bool active = id[u] != self && kv != 0 && ((kv ^ tv) & vmask) == 0 && ((ki ^ ti) & imask) == 0;
                    const uint32_t d = ps.on_id ? (ki >> ps.shift) & ((1u << ps.bits) - 1)
                                                : uint32_t(kv >> ps.shift) & ((1u << ps.bits) - 1);
                    count_digit(hist, active, d, lane);
                }
            }
            __syncthreads();
            find_bin(hist, st, ps, p == 0);
        }

        // ---- collect: everything at or above the threshold ----
        {
            const uint64_t tv = st.tv;
            const uint32_t ti = st.ti;
            for (int64_t c0 = 0; c0 < cols; c0 += kThreads * kSweepUnroll) {
                typename V::Held v[kSweepUnroll];
                int id[kSweepUnroll];
#pragma unroll
                for (int u = 0; u < kSweepUnroll; ++u) {
                    const int64_t c = c0 + u * kThreads + tid;
                    v[u] = typename V::Held(0);
                    id[u] = self;
                    if (c < cols) {
                        v[u] = load<L>(S, stride, r, c);
                        id[u] = col_ids ? col_ids[c] : int(c);
                    }
                }
#pragma unroll
                for (int u = 0; u < kSweepUnroll; ++u) {
                    const uint64_t kv = key_of(v[u]);
                    const uint32_t ki = uint32_t(0x7fffffff - id[u]);
                    if (id[u] != self && kv != 0 && (kv > tv || (kv == tv && ki >= ti))) {
                        const int at = atomicAdd(&st.count, 1);
                        if (at < cap) {                      // (always, for distinct ids: at most k survive)
                            sv[at] = (double)v[u];
                            si[at] = id[u];
                        }
                    }
                }
            }
        }
        __syncthreads();
        const int count = min(st.count, k);
        int size = 1;
        while (size < count) size <<= 1;                     // (<= cap)
        for (int i = min(st.count, cap) + tid; i < size; i += kThreads) {
            sv[i] = __builtin_nan("");                       // padding: key 0, last in the order
            si[i] = 0x7fffffff;
        }
        __syncthreads();

        // ---- sort the survivors: best first ----
        for (int span = 2; span <= size; span <<= 1) {
            for (int step = span >> 1; step > 0; step >>= 1) {
                for (int i = tid; i < (size >> 1); i += kThreads) {
                    const int lo = ((i & ~(step - 1)) << 1) | (i & (step - 1));
                    const int hi = lo | step;
                    const bool forward = (lo & span) == 0;
                    const double a = sv[lo], b = sv[hi];
                    const int ia = si[lo], ib = si[hi];
                    const uint64_t ka = key_of(a), kb = key_of(b);
                    const bool b_first = kb > ka || (kb == ka && ib < ia);       // b is better than a
                    if (b_first == forward) {
                        sv[lo] = b, sv[hi] = a;
                        si[lo] = ib, si[hi] = ia;
                    }
                }
                __syncthreads();
            }
        }
        for (int j = tid; j < k; j += kThreads) {
            idx_out[q * k + j] = j < count ? si[j] : -1;
            val_out[q * k + j] = j < count ? sv[j] : 0.0;
        }
        __syncthreads();                                     // (the next row reuses the LDS)
    }
}

// ---- the queries on the lists --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void neighbors_rows_kernel(const int32_t* __restrict__ nbr_ids,
                                                                  const double* __restrict__ nbr_vals,
                                                                  const double* __restrict__ diag, int64_t n, int k,
                                                                  const int32_t* __restrict__ row_pos, int64_t n_q,
                                                                  int64_t chunks, double* __restrict__ out, int64_t ld_out) {
    __shared__ double row[kChunk];
    const int64_t q = blockIdx.x / chunks;
    const int64_t lo = (blockIdx.x % chunks) * kChunk;
    const int tid = threadIdx.x;
    const int64_t r = row_pos[q];
    const bool ok = r >= 0 && r < n;
    const double fill = ok ? 0.0 : __builtin_nan("");
#pragma unroll
    for (int i = 0; i < kChunkPerThread; ++i) row[tid + i * kThreads] = fill;
    __syncthreads();
    if (ok) {
        for (int j = tid; j < k; j += kThreads) {
            const int64_t id = nbr_ids[r * k + j];
            if (id >= lo && id < lo + kChunk && id < n) row[id - lo] = nbr_vals[r * k + j];
        }
    }
    __syncthreads();
    if (ok && tid == 0 && r >= lo && r < lo + kChunk) row[r - lo] = diag[r];
    __syncthreads();
    double* o = out + q * ld_out + lo;
#pragma unroll
    for (int i = 0; i < kChunkPerThread; ++i) {
        const int j = tid + i * kThreads;
        if (lo + j < n) o[j] = row[j];
    }
}

__global__ __launch_bounds__(256) void neighbors_pairs_kernel(const int32_t* __restrict__ nbr_ids,
                                                              const double* __restrict__ nbr_vals,
                                                              const double* __restrict__ diag, int64_t n, int k,
                                                              const int32_t* __restrict__ a_pos,
                                                              const int32_t* __restrict__ b_pos, int64_t n_pairs,
                                                              double* __restrict__ out) {
    const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (i >= n_pairs) return;
    const int64_t a = a_pos[i], b = b_pos[i];
    double v = __builtin_nan("");
    if (a >= 0 && a < n && b >= 0 && b < n) {
        if (a == b) {
            v = diag[a];
        } else {
            v = 0.0;
            for (int j = 0; j < k; ++j)
                if (nbr_ids[a * k + j] == b) {
                    v = nbr_vals[a * k + j];
                    break;
                }
        }
    }
    out[i] = v;
}

// acc + (w * s) with both roundings: the compiler may not contract the two into a fused multiply-add
__device__ __forceinline__ double add_product(double acc, double w, double s) {
#pragma clang fp contract(off)
    const double p = w * s;
    return acc + p;
}

// An absent entry of P is +0.0: it would add w * (+0.0) = +-0.0 to its sum.  The sum starts at +0.0; x + (+-0.0) is x for
// every x but -0.0, and a sum is never -0.0: (+0.0) + (-0.0) is +0.0 in round-to-nearest, and so is every exact
// cancellation.  So skipping the absent entries leaves every bit as it is (weights are finite: w * 0 is no NaN).
__global__ __launch_bounds__(kThreads) void neighbors_score_kernel(const int32_t* __restrict__ nbr_ids,
                                                                   const double* __restrict__ nbr_vals,
                                                                   const double* __restrict__ diag, int64_t n, int k,
                                                                   const int64_t* __restrict__ set_ptr,
                                                                   const int32_t* __restrict__ set_pos,
                                                                   const double* __restrict__ set_w, int64_t n_sets,
                                                                   const int64_t* __restrict__ excl_ptr,
                                                                   const int32_t* __restrict__ excl_cols, int64_t chunks,
                                                                   double* __restrict__ out, int64_t ld_out) {
    __shared__ double acc[kChunk];
    const int64_t q = blockIdx.x / chunks;
    const int64_t lo = (blockIdx.x % chunks) * kChunk;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < kChunkPerThread; ++i) acc[tid + i * kThreads] = 0.0;
    __syncthreads();
    bool poisoned = false;
    const int64_t e1 = set_ptr[q + 1];
    for (int64_t e = set_ptr[q]; e < e1; ++e) {              // (uniform over the workgroup)
        const int64_t r = set_pos[e];
        if (r < 0 || r >= n) {
            poisoned = true;
            continue;
        }
        const double w = set_w[e];
        for (int j = tid; j <= k; j += kThreads) {           // (j == k: the diagonal)
            const int64_t id = j < k ? int64_t(nbr_ids[r * k + j]) : r;
            if (id >= lo && id < lo + kChunk && id < n) {
                const double s = j < k ? nbr_vals[r * k + j] : diag[r];
                acc[id - lo] = add_product(acc[id - lo], w, s);
            }
        }
        __syncthreads();
    }
    if (poisoned) {
#pragma unroll
        for (int i = 0; i < kChunkPerThread; ++i) acc[tid + i * kThreads] = __builtin_nan("");
        __syncthreads();
    }
    if (excl_ptr) {
        const int64_t x0 = excl_ptr[q], x1 = excl_ptr[q + 1];
        for (int64_t x = x0 + tid; x < x1; x += kThreads) {
            const int64_t c = excl_cols[x];
            if (c >= lo && c < lo + kChunk) acc[c - lo] = -__builtin_inf();
        }
        __syncthreads();
    }
    double* o = out + q * ld_out + lo;
#pragma unroll
    for (int i = 0; i < kChunkPerThread; ++i) {
        const int j = tid + i * kThreads;
        if (lo + j < n) o[j] = acc[j];
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
int check_k(int32_t k) {
    REQUIRE(k >= 1 && k <= SIMRANK_NEIGHBORS_MAX_K, "k must be in [1, %d] (got %d)", SIMRANK_NEIGHBORS_MAX_K, (int)k);
    return SIMRANK_NEIGHBORS_OK;
}

int check_tables(const int32_t* nbr_ids, const double* nbr_vals, const double* diag, int64_t n, int32_t k) {
    const int rc = check_k(k);
    if (rc) return rc;
    REQUIRE(n >= 0 && n < (int64_t(1) << 31), "bad number of nodes %lld", (long long)n);
    REQUIRE(n == 0 || (nbr_ids && nbr_vals && diag), "nbr_ids, nbr_vals or diag is NULL");
    return SIMRANK_NEIGHBORS_OK;
}

int check_grid(int64_t rows, int64_t n, int64_t& chunks) {
    chunks = (n + kChunk - 1) / kChunk;
    REQUIRE(rows * chunks <= SIMRANK_NEIGHBORS_MAX_BLOCKS, "%lld rows x %lld columns are too many for one call (%lld "
            "workgroups): cut the rows into bands", (long long)rows, (long long)n, (long long)(rows * chunks));
    return SIMRANK_NEIGHBORS_OK;
}

}  // namespace

extern "C" {

int simrank_neighbors_version(void) { return SIMRANK_NEIGHBORS_VERSION; }

const char* simrank_neighbors_last_error(void) { return g_error.c_str(); }

int simrank_neighbors_select(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                             const int32_t* row_pos, const int32_t* row_ids, int64_t n_q, const int32_t* col_ids, int32_t k,
                             int32_t* idx_out, double* val_out, void* stream) {
    int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    rc = check_k(k);
    if (rc) return rc;
    REQUIRE(n_q >= 0 && n_q < (int64_t(1) << 31), "bad number of query rows %lld", (long long)n_q);
    if (n_q == 0) return SIMRANK_NEIGHBORS_OK;
    REQUIRE(row_pos && row_ids && idx_out && val_out, "row_pos, row_ids, idx_out or val_out is NULL");
    int cap = 1;
    while (cap < k) cap <<= 1;
    const size_t lds = size_t(cap) * 12 + kBins * sizeof(uint32_t) + sizeof(SelectState);
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)std::min<int64_t>(n_q, int64_t(1) << 20));
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL(neighbors_select_kernel<L>, grid, dim3(kThreads), lds, st, S, stride, n_rows, n_cols, row_pos,
                           row_ids, n_q, col_ids, (int)k, cap, idx_out, val_out);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_NEIGHBORS_OK;
}

int simrank_neighbors_rows(const int32_t* nbr_ids, const double* nbr_vals, const double* diag, int64_t n, int32_t k,
                           const int32_t* row_pos, int64_t n_q, double* out, int64_t ld_out, void* stream) {
    const int rc = check_tables(nbr_ids, nbr_vals, diag, n, k);
    if (rc) return rc;
    REQUIRE(n_q >= 0 && n_q < (int64_t(1) << 31) && ld_out >= n, "bad output shape %lld x %lld (ld %lld)", (long long)n_q,
            (long long)n, (long long)ld_out);
    if (n_q == 0 || n == 0) return SIMRANK_NEIGHBORS_OK;
    REQUIRE(row_pos && out, "row_pos or out is NULL");
    int64_t chunks;
    const int rg = check_grid(n_q, n, chunks);
    if (rg) return rg;
    hipLaunchKernelGGL(neighbors_rows_kernel, dim3((unsigned)(n_q * chunks)), dim3(kThreads), 0, as_stream(stream), nbr_ids,
                       nbr_vals, diag, n, (int)k, row_pos, n_q, chunks, out, ld_out);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_NEIGHBORS_OK;
}

int simrank_neighbors_pairs(const int32_t* nbr_ids, const double* nbr_vals, const double* diag, int64_t n, int32_t k,
                            const int32_t* a_pos, const int32_t* b_pos, int64_t n_pairs, double* out, void* stream) {
    const int rc = check_tables(nbr_ids, nbr_vals, diag, n, k);
    if (rc) return rc;
    REQUIRE(n_pairs >= 0 && n_pairs < (int64_t(1) << 38), "bad number of pairs %lld", (long long)n_pairs);
    if (n_pairs == 0) return SIMRANK_NEIGHBORS_OK;
    REQUIRE(a_pos && b_pos && out, "a_pos, b_pos or out is NULL");
    hipLaunchKernelGGL(neighbors_pairs_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, as_stream(stream),
                       nbr_ids, nbr_vals, diag, n, (int)k, a_pos, b_pos, n_pairs, out);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_NEIGHBORS_OK;
}

int simrank_neighbors_score(const int32_t* nbr_ids, const double* nbr_vals, const double* diag, int64_t n, int32_t k,
                            const int64_t* set_ptr, const int32_t* set_pos, const double* set_w, int64_t n_sets,
                            const int64_t* excl_ptr, const int32_t* excl_cols, double* out, int64_t ld_out, void* stream) {
    const int rc = check_tables(nbr_ids, nbr_vals, diag, n, k);
    if (rc) return rc;
    REQUIRE(n_sets >= 0 && n_sets < (int64_t(1) << 31) && ld_out >= n, "bad output shape %lld x %lld (ld %lld)",
            (long long)n_sets, (long long)n, (long long)ld_out);
    REQUIRE((excl_ptr == nullptr) == (excl_cols == nullptr), "excl_ptr and excl_cols go together");
    if (n_sets == 0 || n == 0) return SIMRANK_NEIGHBORS_OK;
    REQUIRE(set_ptr && out, "set_ptr or out is NULL");
    // (set_pos and set_w may be NULL when every basket is empty: they are then never read)
    int64_t chunks;
    const int rg = check_grid(n_sets, n, chunks);
    if (rg) return rg;
    hipLaunchKernelGGL(neighbors_score_kernel, dim3((unsigned)(n_sets * chunks)), dim3(kThreads), 0, as_stream(stream),
                       nbr_ids, nbr_vals, diag, n, (int)k, set_ptr, set_pos, set_w, n_sets, excl_ptr, excl_cols, chunks, out,
                       ld_out);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_NEIGHBORS_OK;
}

}  // extern "C"
