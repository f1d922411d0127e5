// Single-linkage clusters of an iterate that stays on the device (include/simrank_cluster.h, libsimrank_cluster.so): the
// connected components of "S[a][b] >= t or S[b][a] >= t" for up to 8 thresholds in one sweep of the matrix.
//
// The sweep is the walk that select.hip and profile.hip share (companion.h: eight rows per wave on panels, one on a
// row-major block, 16-byte loads; only what is done with a loaded piece is written here).  Every entry that passes a
// level's threshold is an edge (row node, column node) of that level's graph; the graph lives in a forest
// parent[level][node] with parent[x] <= x always.
//
// What an edge costs.  At a low threshold nearly every entry is an edge and at most n - 1 of them change anything, so an
// entry first reads its column node's parent and compares it with a member of the row's component that the lane keeps in
// a register per level (the root, as of its last walk): equal means the same component and nothing more is done.  Only
// a lane whose two values differ walks to both roots, shortens the column's path, and, if the roots still differ,
// offers the pair to the wave: one lane per distinct (larger root, smaller root) goes on to the compare-and-swap that
// hooks the larger root under the smaller.  A failed swap returns the parent that was there, which is below the root it
// was tried on: the retry starts lower, so the loop ends after at most n turns whatever other threads do.
//
// Every read of `parent` is a relaxed device-scope load and every shortening store a relaxed device-scope store: vector
// memory operations that go to the L2 the atomics work in, past a compute unit's own cache, whose stale lines would
// otherwise send lanes down the slow path for the rest of the kernel.  A value read late is still an ancestor or a
// former root of the node, in its component and not above it: equal values prove one component, different ones only
// cost the walk.  Nothing waits: walks and retries are capped, and a cap reached or a parent out of order sets a bit of
// *status and drops the edge.
#include <algorithm>
#include <type_traits>

#include "simrank_cluster.h"

#define COMPANION_ERR_INVALID SIMRANK_CLUSTER_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_CLUSTER_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_CLUSTER_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_CLUSTER_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_CLUSTER_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_CLUSTER_, ROWMAJOR_F64);

constexpr int kMaxLevels = SIMRANK_CLUSTER_MAX_LEVELS;
constexpr int kThreads = kSweepThreads;
constexpr int kMaxGrid = kSweepMaxGrid;
constexpr unsigned kCapSlack = 8;

// ---- the forest ----------------------------------------------------------------------------------------------------------
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
            bad |= SIMRANK_CLUSTER_BAD_PARENT;
            return -1;
        }
        const int32_t gp = ld(P + p);
        if (gp == p) return p;
        if (!in_order(gp, p)) {
            bad |= SIMRANK_CLUSTER_BAD_PARENT;
            return -1;
        }
        if constexpr (WRITE) st(P + x, gp);
        x = gp;
    }
    bad |= SIMRANK_CLUSTER_CAP_REACHED;
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
            bad |= SIMRANK_CLUSTER_BAD_PARENT;
            return -1;
        }
        a = find<true>(P, old, cap, bad);
        b = find<true>(P, lo, cap, bad);
        if (a < 0 || b < 0) return -1;
    }
    bad |= SIMRANK_CLUSTER_CAP_REACHED;
    return -1;
}

// ---- the sweep -----------------------------------------------------------------------------------------------------------
template <int LAYOUT>
__global__ __launch_bounds__(kThreads) void union_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                         int64_t n_cols, const int32_t* __restrict__ row_ids,
                                                         const int32_t* __restrict__ col_ids,
                                                         const typename Elem<LAYOUT>::Cmp* __restrict__ edges_dev,
                                                         int n_levels, int32_t* parent, int64_t n, int32_t* status,
                                                         int vec) {
    using E = Elem<LAYOUT>;
    using Cmp = typename E::Cmp;
    WALK_GEOMETRY(LAYOUT, n_cols);
    const unsigned cap = unsigned(n) + kCapSlack;
    unsigned bad = 0;

    Cmp edge[kMaxLevels];
#pragma unroll
    for (int l = 0; l < kMaxLevels; ++l) edge[l] = edges_dev[l < n_levels ? l : 0];

    // `mine[l]`: a member of the row node's component in level l, its root as of this lane's last walk.
    int32_t mine[kMaxLevels];

    // The slow path of one entry in one level, called by every lane of the wave together (`act`: this lane's entry is an
    // edge whose column parent differed from `mine_l`).
    auto join = [&](int32_t* P, bool act, int32_t cid, int32_t& mine_l) {
        int32_t a = -1, b = -1;
        if (act) act = ld(P + cid) != mine_l;                            // (an earlier entry of the piece may have settled it)
        if (act) {
            a = find<true>(P, mine_l, cap, bad);
            b = find<true>(P, cid, cap, bad);
            act = a >= 0 && b >= 0;
            if (act) {
                mine_l = a;
                if (b != cid && ld(P + cid) != b) st(P + cid, b);        // the next read of this column ends the level at once
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
            if (root >= 0) mine_l = root;
        }
    };

    for (int64_t r0 = wave * R; r0 < n_rows; r0 += nwaves * R) {
        const int64_t r = r0 + g;
        const bool live = r < n_rows;
        const int32_t rid = live ? (row_ids ? row_ids[r] : int32_t(r)) : -1;
        const bool row_ok = live && rid >= 0 && rid < n;                 // (an id outside the nodes is padding)
#pragma unroll
        for (int l = 0; l < kMaxLevels; ++l) mine[l] = rid;
        for (int64_t k0 = 0; k0 < n_chunks; k0 += U) {
            WALK_LOAD(LAYOUT, x, S, stride, r, live, k0, n_cols, vec)
            // One 16-byte piece at a time, as a loop: the slow path below then exists once per level, not once per value
            // in flight.
#pragma unroll 1
            for (int u = 0; u < U; ++u) {
                if (k0 + u >= n_chunks) break;                           // (wave-uniform)
                const v4u32 xu = u == 0 ? x[0] : u == 1 ? x[1] : u == 2 ? x[2] : x[3];
                const int64_t c0 = (k0 + u) * W + int64_t(q) * V;
                int32_t cid[V];
                Cmp v[V];
                unsigned ok = 0;                                         // bit i: value i is an entry between two nodes
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    v[i] = E::value(E::raw(xu, i));
                    cid[i] = 0;
                    if (row_ok && c0 + i < n_cols) {
                        cid[i] = col_ids ? col_ids[c0 + i] : int32_t(c0 + i);
                        if (cid[i] != rid && cid[i] >= 0 && cid[i] < n) ok |= 1u << i;
                    }
                }
#pragma unroll
                for (int l = 0; l < kMaxLevels; ++l) {
                    if (l >= n_levels) break;                            // (wave-uniform)
                    int32_t* P = parent + int64_t(l) * n;
                    // an edge whose column node's parent is the row's member is settled: the usual end of an entry
                    unsigned open = 0;
#pragma unroll
                    for (int i = 0; i < V; ++i)                          // (NaN passes nothing; -0.0 >= +0.0 passes)
                        if (((ok >> i) & 1) && v[i] >= edge[l] && ld(P + cid[i]) != mine[l]) open |= 1u << i;
                    if (!__ballot(open != 0)) continue;                  // (wave-uniform)
#pragma unroll 1
                    for (int i = 0; i < V; ++i) {
                        const bool act = (open >> i) & 1;
                        if (!__ballot(act)) continue;                    // (wave-uniform)
                        join(P, act, act ? (col_ids ? col_ids[c0 + i] : int32_t(c0 + i)) : 0, mine[l]);
                    }
                }
            }
        }
    }
    if (bad) atomicOr(reinterpret_cast<int*>(status), (int)bad);
}

__global__ __launch_bounds__(kThreads) void init_kernel(int32_t* __restrict__ parent, int64_t n, int64_t total,
                                                        int32_t* __restrict__ status) {
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < total; i += step) parent[i] = int32_t(i % n);
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = 0;
}

__global__ __launch_bounds__(kThreads) void labels_kernel(const int32_t* parent, int64_t n, int64_t total,
                                                          int32_t* __restrict__ labels, int32_t* status) {
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    const unsigned cap = unsigned(n) + kCapSlack;
    unsigned bad = 0;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < total; i += step) {
        const int64_t l = i / n;
        labels[i] = find<false>(parent + l * n, int32_t(i - l * n), cap, bad);
    }
    if (bad) atomicOr(reinterpret_cast<int*>(status), (int)bad);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int check_forest(const void* parent, int64_t n, int32_t n_levels, const void* status) {
    REQUIRE(n >= 0 && n < (int64_t(1) << 31) - kCapSlack, "bad node count %lld", (long long)n);
    REQUIRE(n_levels >= 1 && n_levels <= kMaxLevels, "n_levels must be 1 .. %d (got %d)", kMaxLevels, (int)n_levels);
    REQUIRE(status, "status is NULL");
    REQUIRE(n == 0 || parent, "parent is NULL");
    return SIMRANK_CLUSTER_OK;
}

int flat_grid(int64_t total) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((total + kThreads - 1) / kThreads, kMaxGrid));
}

}  // namespace

extern "C" {

int simrank_cluster_version(void) { return SIMRANK_CLUSTER_VERSION; }

const char* simrank_cluster_last_error(void) { return g_error.c_str(); }

int simrank_cluster_init(int32_t* parent, int64_t n, int32_t n_levels, int32_t* status, void* stream) {
    const int rc = check_forest(parent, n, n_levels, status);
    if (rc) return rc;
    const int64_t total = n * n_levels;
    hipLaunchKernelGGL(init_kernel, dim3(flat_grid(total)), dim3(kThreads), 0, as_stream(stream), parent, n, total, status);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_CLUSTER_OK;
}

int simrank_cluster_union(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                          const int32_t* row_ids, const int32_t* col_ids, const void* edges, int32_t n_levels,
                          int32_t* parent, int64_t n, int32_t* status, void* stream) {
    Launch l;
    int rc = plan_launch(S, layout, stride, n_rows, n_cols, true, &l);
    if (rc) return rc;
    rc = check_forest(parent, n, n_levels, status);
    if (rc) return rc;
    REQUIRE(edges, "edges is NULL");
    if (n_rows == 0 || n_cols == 0 || n == 0) return SIMRANK_CLUSTER_OK;
    hipStream_t st = as_stream(stream);
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL((union_kernel<L>), dim3(l.grid), dim3(kThreads), 0, st, S, stride, n_rows, n_cols, row_ids,
                           col_ids, static_cast<const typename Elem<L>::Cmp*>(edges), (int)n_levels, parent, n, status,
                           l.vec);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_CLUSTER_OK;
}

int simrank_cluster_labels(const int32_t* parent, int64_t n, int32_t n_levels, int32_t* labels, int32_t* status,
                           void* stream) {
    const int rc = check_forest(parent, n, n_levels, status);
    if (rc) return rc;
    REQUIRE(n == 0 || labels, "labels is NULL");
    REQUIRE(n == 0 || labels != parent, "labels must not be the parent array");
    if (n == 0) return SIMRANK_CLUSTER_OK;
    const int64_t total = n * n_levels;
    hipLaunchKernelGGL(labels_kernel, dim3(flat_grid(total)), dim3(kThreads), 0, as_stream(stream), parent, n, total, labels,
                       status);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_CLUSTER_OK;
}

}  // extern "C"
