// The k best of chosen rows of a kept model among a list of candidate columns (include/simrank_candidates.h,
// libsimrank_candidates.so).
//
//     topk    one workgroup of 256 per query row; the candidate list (block positions and ids) is the same for every row
//             and read with coalesced 4-byte loads, the elements are gathered from the block in place.  Every candidate
//             has the composite key (order-preserving integer of its widened value, n_cand - 1 - list index), larger =
//             better; the k-th best is found by the radix select of neighbors.hip: a pass histograms one 11-bit digit of
//             the candidates that still share the k-th's prefix (2048 counters in LDS), finds the bin that holds the
//             k-th by a suffix scan and stops as soon as that bin is wanted whole.  f32 and binary16 values have a 32-bit
//             key (3 passes), float64 a 64-bit one (6); the bits of the list index (at most 3 passes, fewer for a short
//             list) are only walked when the k-th value ties.
//             STAGED (n_cand <= the layout's cap): one gathering sweep writes the row's keys to LDS, key 0 for what is no
//             candidate (NaN, the row's own id, a position outside the block); every pass and the collecting sweep read
//             the keys there.  So an element is fetched once per query, and once more if it survives: a key folds the
//             two zeros, the value written out is the element's own.
//             Not STAGED: every pass and the collecting sweep gather again; after the first the row comes from L2.
//             The at most k survivors (key, list index) are sorted in LDS by a bitonic sort and written best first.
//             The dynamic LDS of a launch is the state, the histogram, cap (key, index) pairs with cap the power of two
//             >= min(k, n_cand), and, STAGED, n_cand keys: a short list at a small k leaves the CU to many workgroups,
//             whose gathers hide each other's latency.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>

#include "simrank_candidates.h"

#define COMPANION_ERR_INVALID SIMRANK_CANDIDATES_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_CANDIDATES_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_CANDIDATES_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_CANDIDATES_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_CANDIDATES_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_CANDIDATES_, ROWMAJOR_F64);

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kDigitBits = 11;
constexpr int kBins = 1 << kDigitBits;                     // counters of one pass
constexpr int kBinsPerThread = kBins / kThreads;
constexpr int kSweepUnroll = 4;                            // candidates of one lane in flight in a sweep
constexpr int64_t kStaged32 = 16384;                       // 64 KiB of 32-bit keys
constexpr int64_t kStaged64 = 8192;                        // 64 KiB of 64-bit keys
constexpr size_t kDefaultLds = 48 * 1024;                  // more dynamic LDS than this is asked for by attribute

// ---- keys ----------------------------------------------------------------------------------------------------------
// Order-preserving integer of a value: larger key = larger value; -0.0 and +0.0 share a key; NaN -> 0, below -inf (whose
// key is not 0).  Key 0 is "no candidate".
__device__ __forceinline__ uint64_t key_of(double v) {
    if (v != v) return 0;
    if (v == 0.0) v = 0.0;                                  // (-0.0 -> +0.0 in the key only)
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | (uint64_t(1) << 63));
}

__device__ __forceinline__ uint32_t key_of(float v) {
    if (v != v) return 0;
    if (v == 0.0f) v = 0.0f;
    const uint32_t b = __float_as_uint(v);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}

// The key of a layout's values.  The f32 and binary16 layouts widen exactly and monotonically, so the key of the float
// load<L> (companion.h) hands back orders as the key of the double would.
template <int L>
struct Value {
    using Key = typename std::conditional<L == ROWMAJOR_F64, uint64_t, uint32_t>::type;
    static constexpr int kKeyBits = 8 * sizeof(Key);
    static constexpr int kValuePasses = (kKeyBits + kDigitBits - 1) / kDigitBits;
};

// The passes of the radix select: (which key, shift, bits), from the most significant digit down.
struct Pass {
    int on_index, shift, bits;
};

__device__ __forceinline__ Pass pass_of(int p, int key_bits, int value_passes, int index_bits) {
    const bool on_index = p >= value_passes;
    const int width = on_index ? index_bits : key_bits;
    const int shift = width - kDigitBits * ((on_index ? p - value_passes : p) + 1);
    return shift >= 0 ? Pass{on_index, shift, kDigitBits} : Pass{on_index, 0, shift + kDigitBits};
}

// What the workgroup agrees on between the passes (LDS).
struct SelectState {
    uint64_t tv;           // threshold: value key (the digits found so far, zeros below)
    uint32_t ti;           // threshold: index key among the candidates whose value key is tv
    int need;              // how many of the current bin's candidates are wanted
    int done;              // the threshold is final
    int count;             // survivors collected
    int wave_sum[kWaves];
};
static_assert(sizeof(SelectState) % 8 == 0, "the 64-bit keys follow the state and the histogram");

// Add 1 to hist[d] for every active lane; the lanes that share the first active lane's digit go in one add (a row that
// is mostly one value would serialise its LDS atomics on one counter).
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
        // no more candidates than wanted (only the first pass can see this): every candidate survives
        if (tid == 0 && first_pass) { st.tv = 0; st.ti = 0; st.done = 1; }
    } else if (incl >= need && incl - mine < need) {
        int above = incl - mine;
        for (int i = 0; i < kBinsPerThread; ++i) {
            const int c = (int)hist[top - i];
            if (above + c >= need) {
                const uint64_t digit = uint64_t(top - i);
                if (ps.on_index) st.ti |= uint32_t(digit << ps.shift);
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

// The keys of this lane's kSweepUnroll candidates of the sweep turn that starts at list index i0 (lane t takes i0 + t,
// i0 + 256 + t, ...): gathered from the block, all loads in flight before the first is used; 0 past the list and for
// what is no candidate.
template <int L>
__device__ __forceinline__ void gather_keys(const void* __restrict__ S, int64_t stride, int64_t r, int64_t n_cols,
                                            const int32_t* __restrict__ cand_pos, const int32_t* __restrict__ cand_ids,
                                            int64_t n, int self, int64_t i0, typename Value<L>::Key (&key)[kSweepUnroll]) {
    decltype(load<L>(S, stride, r, 0)) v[kSweepUnroll];
    bool ok[kSweepUnroll];
#pragma unroll
    for (int u = 0; u < kSweepUnroll; ++u) {
        const int64_t i = i0 + u * kThreads + threadIdx.x;
        ok[u] = false;
        v[u] = 0;
        if (i < n) {
            const int64_t p = cand_pos[i];
            const int id = cand_ids ? cand_ids[i] : int(p);
            ok[u] = p >= 0 && p < n_cols && id != self;
            if (ok[u]) v[u] = load<L>(S, stride, r, p);
        }
    }
#pragma unroll
    for (int u = 0; u < kSweepUnroll; ++u) key[u] = ok[u] ? key_of(v[u]) : typename Value<L>::Key(0);
}

template <int L, bool STAGED>
__global__ __launch_bounds__(kThreads) void candidates_topk_kernel(const void* __restrict__ S, int64_t stride,
                                                                   int64_t n_rows, int64_t n_cols,
                                                                   const int32_t* __restrict__ row_pos,
                                                                   const int32_t* __restrict__ row_ids, int64_t n_q,
                                                                   const int32_t* __restrict__ cand_pos,
                                                                   const int32_t* __restrict__ cand_ids, int64_t n_cand,
                                                                   int k, int cap, int index_bits,
                                                                   int32_t* __restrict__ idx_out,
                                                                   double* __restrict__ val_out) {
    using V = Value<L>;
    using Key = typename V::Key;
    extern __shared__ __align__(16) unsigned char lds[];
    // the state, the histogram, cap survivor keys, (STAGED) n_cand keys, cap survivor list indices
    SelectState& st = *reinterpret_cast<SelectState*>(lds);
    uint32_t* hist = reinterpret_cast<uint32_t*>(lds + sizeof(SelectState));
    Key* skey = reinterpret_cast<Key*>(hist + kBins);
    Key* keys = skey + cap;
    int32_t* sidx = reinterpret_cast<int32_t*>(keys + (STAGED ? n_cand : 0));
    const int tid = threadIdx.x, lane = tid & 63;

    for (int64_t q = blockIdx.x; q < n_q; q += gridDim.x) {
        const int64_t r = row_pos[q];
        const int self = row_ids[q];
        const int64_t n = (r >= 0 && r < n_rows) ? n_cand : 0;          // (a row outside the block: no candidates)
        if (tid == 0) { st.tv = 0; st.ti = 0; st.need = k; st.done = 0; st.count = 0; }
        if constexpr (STAGED) {
            // ---- the one gather of this row ----
            for (int64_t i0 = 0; i0 < n; i0 += kThreads * kSweepUnroll) {
                Key key[kSweepUnroll];
                gather_keys<L>(S, stride, r, n_cols, cand_pos, cand_ids, n, self, i0, key);
#pragma unroll
                for (int u = 0; u < kSweepUnroll; ++u) {
                    const int64_t i = i0 + u * kThreads + tid;
                    if (i < n) keys[i] = key[u];
                }
            }
        }
        __syncthreads();

        // this lane's keys of a sweep turn: from LDS, or gathered again
        auto keys_of_turn = [&](int64_t i0, Key(&key)[kSweepUnroll]) {
            if constexpr (STAGED) {
#pragma unroll
                for (int u = 0; u < kSweepUnroll; ++u) {
                    const int64_t i = i0 + u * kThreads + tid;
                    key[u] = i < n ? keys[i] : Key(0);
                }
            } else {
                gather_keys<L>(S, stride, r, n_cols, cand_pos, cand_ids, n, self, i0, key);
            }
        };

        // ---- the threshold: the composite key of the k-th best ----
        for (int p = 0; p < V::kValuePasses + (index_bits + kDigitBits - 1) / kDigitBits; ++p) {
            if (st.done) break;                              // (uniform: written before the last barrier of find_bin)
            const Pass ps = pass_of(p, V::kKeyBits, V::kValuePasses, index_bits);
            for (int i = tid; i < kBins; i += kThreads) hist[i] = 0;
            const uint64_t tv = st.tv;
            const uint32_t ti = st.ti;
            __syncthreads();
            // the digits above this one, as a mask of the key the pass works on
            const int upto = ps.shift + ps.bits;
            const uint64_t vmask = ps.on_index ? ~uint64_t(0) : (upto >= 64 ? 0 : ~uint64_t(0) << upto);
            const uint32_t imask = ps.on_index ? (upto >= 32 ? 0u : ~0u << upto) : 0u;
            for (int64_t i0 = 0; i0 < n; i0 += kThreads * kSweepUnroll) {
                Key key[kSweepUnroll];
                keys_of_turn(i0, key);
#pragma unroll
                for (int u = 0; u < kSweepUnroll; ++u) {
                    const uint64_t kv = key[u];
                    const uint32_t ki = uint32_t(n - 1 - (i0 + u * kThreads + tid));      // (only used where kv != 0)
                    const bool active = kv != 0 && ((kv ^ tv) & vmask) == 0 && ((ki ^ ti) & imask) == 0;
                    const uint32_t d = ps.on_index ? (ki >> ps.shift) & ((1u << ps.bits) - 1)
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
            for (int64_t i0 = 0; i0 < n; i0 += kThreads * kSweepUnroll) {
                Key key[kSweepUnroll];
                keys_of_turn(i0, key);
#pragma unroll
                for (int u = 0; u < kSweepUnroll; ++u) {
                    const uint64_t kv = key[u];
                    const int64_t i = i0 + u * kThreads + tid;
                    const uint32_t ki = uint32_t(n - 1 - i);
                    if (kv != 0 && (kv > tv || (kv == tv && ki >= ti))) {
                        const int at = atomicAdd(&st.count, 1);
                        if (at < cap) {                      // (always: list indices are distinct, at most k survive)
                            skey[at] = key[u];
                            sidx[at] = int32_t(i);
                        }
                    }
                }
            }
        }
        __syncthreads();
        const int count = min(min(st.count, k), cap);
        int size = 1;
        while (size < count) size <<= 1;                     // (<= cap)
        for (int i = count + tid; i < size; i += kThreads) {
            skey[i] = 0;                                     // padding: last in the order
            sidx[i] = 0x7fffffff;
        }
        __syncthreads();

        // ---- sort the survivors: best first ----
        for (int span = 2; span <= size; span <<= 1) {
            for (int step = span >> 1; step > 0; step >>= 1) {
                for (int i = tid; i < (size >> 1); i += kThreads) {
                    const int lo = ((i & ~(step - 1)) << 1) | (i & (step - 1));
                    const int hi = lo | step;
                    const bool forward = (lo & span) == 0;
                    const Key ka = skey[lo], kb = skey[hi];
                    const int ia = sidx[lo], ib = sidx[hi];
                    const bool b_first = kb > ka || (kb == ka && ib < ia);       // b is better than a
                    if (b_first == forward) {
                        skey[lo] = kb, skey[hi] = ka;
                        sidx[lo] = ib, sidx[hi] = ia;
                    }
                }
                __syncthreads();
            }
        }
        // ---- write them out: the survivor's own element (the key folded its zero's sign) ----
        for (int j = tid; j < k; j += kThreads) {
            int id = -1;
            double v = 0.0;
            if (j < count) {
                const int64_t i = sidx[j];
                const int64_t p = cand_pos[i];               // (inside the block: it became a candidate)
                id = cand_ids ? cand_ids[i] : int(p);
                v = (double)load<L>(S, stride, r, p);
            }
            idx_out[q * k + j] = id;
            val_out[q * k + j] = v;
        }
        __syncthreads();                                     // (the next row reuses the LDS)
    }
}

int64_t staged_of(int32_t layout) { return layout == ROWMAJOR_F64 ? kStaged64 : kStaged32; }

template <int L, bool STAGED, class... Args>
int launch(dim3 grid, size_t lds, hipStream_t st, Args... args) {
    auto kern = candidates_topk_kernel<L, STAGED>;
    if (lds > kDefaultLds)
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, st, args...);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_CANDIDATES_OK;
}

}  // namespace

extern "C" {

int simrank_candidates_version(void) { return SIMRANK_CANDIDATES_VERSION; }

const char* simrank_candidates_last_error(void) { return g_error.c_str(); }

int64_t simrank_candidates_staged(int32_t layout) { return known_layout(layout) ? staged_of(layout) : -1; }

int simrank_candidates_topk(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                            const int32_t* row_pos, const int32_t* row_ids, int64_t n_q, const int32_t* cand_pos,
                            const int32_t* cand_ids, int64_t n_cand, int32_t k, int32_t* idx_out, double* val_out,
                            void* stream) {
    int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    REQUIRE(k >= 1 && k <= SIMRANK_CANDIDATES_MAX_K, "k must be in [1, %d] (got %d)", SIMRANK_CANDIDATES_MAX_K, (int)k);
    REQUIRE(n_q >= 0 && n_q < (int64_t(1) << 31), "bad number of query rows %lld", (long long)n_q);
    REQUIRE(n_cand >= 0 && n_cand < (int64_t(1) << 31), "bad number of candidates %lld", (long long)n_cand);
    REQUIRE(n_cand == 0 || cand_pos, "cand_pos is NULL with %lld candidates", (long long)n_cand);
    if (n_q == 0) return SIMRANK_CANDIDATES_OK;
    REQUIRE(row_pos && row_ids && idx_out && val_out, "row_pos, row_ids, idx_out or val_out is NULL");
    // a row of an empty block has no element to read: its rows are "outside" for the kernel as well (n_rows = 0), and
    // n_cols = 0 leaves every position outside
    int cap = 1;
    while (cap < std::min<int64_t>(k, n_cand)) cap <<= 1;
    int index_bits = 1;
    while (index_bits < 31 && (int64_t(1) << index_bits) < n_cand) ++index_bits;
    const bool staged = n_cand <= staged_of(layout);
    const size_t key_bytes = layout == ROWMAJOR_F64 ? 8 : 4;
    const size_t lds = sizeof(SelectState) + kBins * sizeof(uint32_t) + size_t(cap) * (key_bytes + 4) +
                       (staged ? size_t(n_cand) * key_bytes : 0);
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)std::min<int64_t>(n_q, SIMRANK_CANDIDATES_MAX_BLOCKS));
    with_layout(layout, [&](auto L) {
        rc = staged ? launch<L, true>(grid, lds, st, S, stride, n_rows, n_cols, row_pos, row_ids, n_q, cand_pos, cand_ids,
                                      n_cand, (int)k, cap, index_bits, idx_out, val_out)
                    : launch<L, false>(grid, lds, st, S, stride, n_rows, n_cols, row_pos, row_ids, n_q, cand_pos, cand_ids,
                                       n_cand, (int)k, cap, index_bits, idx_out, val_out);
    });
    return rc;
}

}  // extern "C"
