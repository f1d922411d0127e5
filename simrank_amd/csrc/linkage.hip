// The single-linkage dendrogram of an iterate that stays on the device (include/simrank_linkage.h,
// libsimrank_linkage.so): a maximum spanning forest of w(a, b) = max(S[a][b], S[b][a]) by Boruvka's rounds.
//
// The sweep is the walk that select.hip, profile.hip and cluster.hip share (companion.h: eight rows per wave on panels,
// one on a row-major block, 16-byte loads; only what is done with a loaded piece is written here).  An entry between two
// components is a candidate of both.  The row's component is one for the whole row: its best candidate is kept in a
// register, reduced over the lanes of the row and offered with one atomic.  The column's component changes with every
// value: its slot is read first and the atomic issued only for a candidate that beats it.
//
// A candidate is a 64-bit integer whose order is the order of the picks: the order-preserving key of the value, then
// 0xffffffff - other root (the smaller root wins a tie).  A 32-bit key and the root share a word; a float64 key fills
// one, and the root goes into a second array in a second sweep, among the entries whose key won the first.
//
// What the column's side costs.  A piece is handled in three steps (the components of its columns, the slots of those in
// another component, the maxima) so that the loads of a step are in flight together.  `comp` is only read by the sweep,
// so plain loads serve it.  The slot check before an atomic reads through the compute unit's own cache: the four or eight
// values of a lane lie in the same few lines, and a stale value is only ever too small, which costs an atomic and never a
// pick.  Every wave starts its row at a turn of its own: waves that began together would otherwise all offer to the
// same columns at the same time, each having read the empty slot before any of the others wrote, which matters most
// in the first round, where every node is a component of its own and every entry a candidate.  The row's side reads its
// slot at device scope, in the L2 the atomics work in.
//
// What the plain and the near reads rest on.  "Too small only costs an atomic" covers PHASE 0.  The plain loads of `comp`
// and PHASE 1's near read of the settled key in best[0] must be exact: they read what an EARLIER kernel wrote (init,
// hook, flatten, the picks of phase 0), and are right because a kernel starts with the caches it reads through
// invalidated.  So a pick must stay a launch of its own: never fused with init, hook, flatten or a pick of the other
// phase into one kernel, nor replayed from a graph whose nodes skip the acquire at their start.
//
// hook_kernel writes comp[c] and the record of root c alone and reads nothing another thread of it writes;
// flatten_kernel overwrites comp[i] with an ancestor of i while other threads walk, so every value a walk reads is an
// ancestor of where it stands, and it ends at the root.  Nothing waits: walks are capped, and a cap reached or an id
// out of range sets a bit of *status.
#include <algorithm>
#include <type_traits>

#include "simrank_linkage.h"

#define COMPANION_ERR_INVALID SIMRANK_LINKAGE_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_LINKAGE_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_LINKAGE_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_LINKAGE_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_LINKAGE_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_LINKAGE_, ROWMAJOR_F64);

constexpr int kThreads = kSweepThreads;
constexpr int kMaxGrid = kSweepMaxGrid;
constexpr unsigned kCapSlack = 8;

typedef unsigned long long u64;

__device__ inline int32_t ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline u64 ld(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a slot as the compute unit's own cache has it: never above what the slot holds now (a slot only grows within a round,
// and the cache starts every kernel empty)
__device__ inline u64 ld_near(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// ---- keys ------------------------------------------------------------------------------------------------------------------
// An unsigned integer that orders as the value does (no NaN comes here); -0.0 takes the key of +0.0.  No key is 0.
__device__ inline uint32_t key_of(float v) {
    uint32_t b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline u64 key_of(double v) {
    u64 b = (u64)__double_as_longlong(v);
    if (b == 0x8000000000000000ull) b = 0;
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double value_of_key32(uint32_t k) {
    return (double)__uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ inline double value_of_key64(u64 k) {
    return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ inline u64 other_code(int32_t root) { return 0xffffffffull - (u64)(uint32_t)root; }

__device__ inline u64 max_over_lanes(u64 x, int width) {
    for (int off = width >> 1; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), off);
        const u64 y = ((u64)hi << 32) | lo;
        x = y > x ? y : x;
    }
    return x;
}

// ---- the sweep -------------------------------------------------------------------------------------------------------------
// PHASE 0: the largest candidate (f32, binary16: key and other root in one word; float64: the key) into best[0].
// PHASE 1 (float64): among the entries whose key is the component's best[0], the largest other_code into best[1].
template <int LAYOUT, int PHASE>
__global__ __launch_bounds__(kThreads) void pick_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                        int64_t n_cols, const int32_t* __restrict__ row_ids,
                                                        const int32_t* __restrict__ col_ids,
                                                        typename Elem<LAYOUT>::Cmp floor, int has_floor,
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

    for (int64_t r0 = wave * R; r0 < n_rows; r0 += nwaves * R) {
        const int64_t r = r0 + g;
        const bool live = r < n_rows;
        const int32_t rid = live ? (row_ids ? row_ids[r] : int32_t(r)) : -1;
        bool row_ok = live && rid >= 0 && rid < n;                       // (an id outside the nodes is padding)
        int32_t rc = 0;
        if (row_ok) {
            rc = comp[rid];
            if (uint32_t(rc) >= uint64_t(n)) {
                bad |= SIMRANK_LINKAGE_BAD_COMPONENT;
                row_ok = false;
                rc = 0;
            }
        }
        const u64 row_code = other_code(rc);
        u64 row_key = 0;                                                 // PHASE 1: the key the row's component settled on
        if (PHASE == 1 && row_ok) row_key = ld(best + rc);
        u64 mine = 0;                                                    // the row's best candidate so far
        // Every turn of U chunks once, starting at a turn of the wave's own: waves that began together would otherwise
        // all offer to the same columns' slots at the same time, each having read them before any of the others wrote.
        const int64_t first = int64_t(((uint64_t(r0 / R) * 2654435761ull) >> 7) % uint64_t(n_turns));
        for (int64_t t = 0; t < n_turns; ++t) {
            const int64_t k0 = (first + t < n_turns ? first + t : first + t - n_turns) * U;
            WALK_LOAD(LAYOUT, x, S, stride, r, live, k0, n_cols, vec)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!row_ok || k0 + u >= n_chunks) continue;
                const int64_t c0 = (k0 + u) * W + int64_t(q) * V;
                // The piece in three steps, so that the loads of each step are in flight together: the components of its
                // columns, then the slots of those that lie in another component, then the maxima.
                int32_t cc[V];
                unsigned open = 0;                                       // bit i: entry i lies between two components
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    cc[i] = rc;
                    const Cmp v = E::value(E::raw(x[u], i));
                    if (c0 + i >= n_cols || v != v || (has_floor && !(v >= floor))) continue;      // (NaN is no entry)
                    const int32_t cid = col_ids ? col_ids[c0 + i] : int32_t(c0 + i);
                    if (cid != rid && cid >= 0 && cid < n) {
                        cc[i] = comp[cid];
                        open |= 1u << i;
                    }
                }
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if (uint32_t(cc[i]) >= uint64_t(n)) {
                        bad |= SIMRANK_LINKAGE_BAD_COMPONENT;
                        cc[i] = rc;
                    }
                    if (cc[i] == rc) open &= ~(1u << i);                 // the usual end of an entry
                }
                if (!open) continue;
                // the column's slot, a near read: too small a value only costs an atomic.  PHASE 1 reads the settled key
                // here, which must be exact: no kernel of that phase writes it, and this one started with the cache
                // invalidated (the note at the head of the file).
                u64 cur[V];
#pragma unroll
                for (int i = 0; i < V; ++i) cur[i] = ((open >> i) & 1) ? ld_near(best + cc[i]) : ~0ull;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if (!((open >> i) & 1)) continue;
                    const auto key = key_of(E::value(E::raw(x[u], i)));
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

__global__ __launch_bounds__(kThreads) void init_kernel(int32_t* __restrict__ comp, u64* __restrict__ best,
                                                        int32_t* __restrict__ hook_other, double* __restrict__ hook_value,
                                                        int64_t n, int32_t* __restrict__ n_hooked,
                                                        int32_t* __restrict__ status) {
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += step) {
        comp[i] = int32_t(i);
        best[i] = 0;
        best[n + i] = 0;
        hook_other[i] = -1;
        hook_value[i] = 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *status = 0;
        *n_hooked = 0;
    }
}

template <bool WIDE>
__global__ __launch_bounds__(kThreads) void hook_kernel(const u64* __restrict__ best, int32_t* __restrict__ comp,
                                                        int32_t* __restrict__ hook_other, double* __restrict__ hook_value,
                                                        int64_t n, int32_t* n_hooked, int32_t* status) {
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    unsigned bad = 0;
    int hooked = 0;
    for (int64_t c = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; c < n; c += step) {
        const u64 pick = best[c];
        if (pick == 0) continue;                                         // no candidate, or no root
        const u64 code = WIDE ? best[n + c] : (pick & 0xffffffffull);
        const int64_t other = int64_t(0xffffffffull - (code & 0xffffffffull));
        if (other >= n || other == c || (WIDE && code == 0)) {
            bad |= SIMRANK_LINKAGE_BAD_COMPONENT;
            continue;
        }
        // the other root's pick: mutual when it names c (its value is then this one)
        const u64 theirs = best[other];
        const u64 their_code = WIDE ? best[n + other] : (theirs & 0xffffffffull);
        const bool mutual = theirs != 0 && int64_t(0xffffffffull - (their_code & 0xffffffffull)) == c;
        if (mutual && c < other) continue;                               // the smaller root of a mutual pick stays
        comp[c] = int32_t(other);
        hook_other[c] = int32_t(other);
        hook_value[c] = WIDE ? value_of_key64(pick) : value_of_key32(uint32_t(pick >> 32));
        ++hooked;
    }
    if (hooked) atomicAdd(reinterpret_cast<int*>(n_hooked), hooked);
    if (bad) atomicOr(reinterpret_cast<int*>(status), (int)bad);
}

__global__ __launch_bounds__(kThreads) void flatten_kernel(int32_t* comp, u64* __restrict__ best, int64_t n, int32_t* status) {
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    const unsigned cap = unsigned(n) + kCapSlack;
    unsigned bad = 0;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += step) {
        best[i] = 0;
        best[n + i] = 0;
        // comp[i] climbs to its own parent until that is a root.  Every node does so at once, each storing to its own
        // word alone, so a step usually skips what the parent has climbed already: a chain of m hooks takes about log2 m
        // steps where the nodes move together and at most m where they do not.
        int32_t p = ld(comp + i);
        unsigned it = 0;
        for (; it < cap; ++it) {
            if (uint32_t(p) >= uint64_t(n)) {
                bad |= SIMRANK_LINKAGE_BAD_COMPONENT;
                break;
            }
            const int32_t up = ld(comp + p);
            if (up == p) break;                                          // p is the root
            p = up;
            if (uint32_t(p) < uint64_t(n)) st(comp + i, p);
        }
        if (it == cap) bad |= SIMRANK_LINKAGE_CAP_REACHED;
    }
    if (bad) atomicOr(reinterpret_cast<int*>(status), (int)bad);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
int check_state(const void* comp, const void* best, int64_t n, const void* status) {
    REQUIRE(n >= 0 && n < (int64_t(1) << 31) - kCapSlack, "bad node count %lld", (long long)n);
    REQUIRE(status, "status is NULL");
    REQUIRE(n == 0 || comp, "comp is NULL");
    REQUIRE(n == 0 || best, "best is NULL");
    return SIMRANK_LINKAGE_OK;
}

int flat_grid(int64_t total) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((total + kThreads - 1) / kThreads, kMaxGrid));
}

}  // namespace

extern "C" {

int simrank_linkage_version(void) { return SIMRANK_LINKAGE_VERSION; }

const char* simrank_linkage_last_error(void) { return g_error.c_str(); }

int simrank_linkage_phases(int32_t layout) {
    REQUIRE(known_layout(layout), "unknown layout %d", (int)layout);
    return layout == ROWMAJOR_F64 ? 2 : 1;
}

int simrank_linkage_init(int32_t* comp, uint64_t* best, int32_t* hook_other, double* hook_value, int64_t n,
                         int32_t* n_hooked, int32_t* status, void* stream) {
    const int rc = check_state(comp, best, n, status);
    if (rc) return rc;
    REQUIRE(n_hooked, "n_hooked is NULL");
    REQUIRE(n == 0 || (hook_other && hook_value), "a hook array is NULL");
    hipLaunchKernelGGL(init_kernel, dim3(flat_grid(n)), dim3(kThreads), 0, as_stream(stream), comp,
                       reinterpret_cast<u64*>(best), hook_other, hook_value, n, n_hooked, status);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_LINKAGE_OK;
}

int simrank_linkage_pick(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols, const int32_t* row_ids,
                         const int32_t* col_ids, const void* floor, int32_t phase, const int32_t* comp, uint64_t* best,
                         int64_t n, int32_t* status, void* stream) {
    Launch l;
    int rc = plan_launch(S, layout, stride, n_rows, n_cols, true, &l);
    if (rc) return rc;
    rc = check_state(comp, best, n, status);
    if (rc) return rc;
    REQUIRE(phase == 0 || (phase == 1 && layout == ROWMAJOR_F64), "phase %d of layout %d: a float64 block has phases 0 and 1, "
            "the others phase 0", (int)phase, (int)layout);
    if (n_rows == 0 || n_cols == 0 || n == 0) return SIMRANK_LINKAGE_OK;
    hipStream_t st = as_stream(stream);
    u64* slots = reinterpret_cast<u64*>(best);
    with_layout(layout, [&](auto L) {
        using Cmp = typename Elem<L>::Cmp;
        const Cmp f = floor ? *static_cast<const Cmp*>(floor) : Cmp(0);
        if constexpr (L == ROWMAJOR_F64) {
            if (phase == 1) {
                hipLaunchKernelGGL((pick_kernel<L, 1>), dim3(l.grid), dim3(kThreads), 0, st, S, stride, n_rows, n_cols, row_ids,
                                   col_ids, f, floor ? 1 : 0, comp, slots, n, status, l.vec);
                return;
            }
        }
        hipLaunchKernelGGL((pick_kernel<L, 0>), dim3(l.grid), dim3(kThreads), 0, st, S, stride, n_rows, n_cols, row_ids,
                           col_ids, f, floor ? 1 : 0, comp, slots, n, status, l.vec);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_LINKAGE_OK;
}

int simrank_linkage_hook(const uint64_t* best, int32_t key_bits, int32_t* comp, int32_t* hook_other, double* hook_value,
                         int64_t n, int32_t* n_hooked, int32_t* status, void* stream) {
    const int rc = check_state(comp, best, n, status);
    if (rc) return rc;
    REQUIRE(key_bits == 32 || key_bits == 64, "key_bits must be 32 or 64 (got %d)", (int)key_bits);
    REQUIRE(n_hooked, "n_hooked is NULL");
    REQUIRE(n == 0 || (hook_other && hook_value), "a hook array is NULL");
    if (n == 0) return SIMRANK_LINKAGE_OK;
    const u64* slots = reinterpret_cast<const u64*>(best);
    if (key_bits == 64)
        hipLaunchKernelGGL(hook_kernel<true>, dim3(flat_grid(n)), dim3(kThreads), 0, as_stream(stream), slots, comp, hook_other,
                           hook_value, n, n_hooked, status);
    else
        hipLaunchKernelGGL(hook_kernel<false>, dim3(flat_grid(n)), dim3(kThreads), 0, as_stream(stream), slots, comp, hook_other,
                           hook_value, n, n_hooked, status);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_LINKAGE_OK;
}

int simrank_linkage_flatten(int32_t* comp, uint64_t* best, int64_t n, int32_t* status, void* stream) {
    const int rc = check_state(comp, best, n, status);
    if (rc) return rc;
    if (n == 0) return SIMRANK_LINKAGE_OK;
    hipLaunchKernelGGL(flatten_kernel, dim3(flat_grid(n)), dim3(kThreads), 0, as_stream(stream), comp,
                       reinterpret_cast<u64*>(best), n, status);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_LINKAGE_OK;
}

}  // extern "C"
